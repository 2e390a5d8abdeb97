// nsk_compile_segments.cpp -- graph compiler: homogeneous segments and what rides on them.  Decides: the segment and
// rest lists and the draw tables (plan_segments), implicit adjacency (build_segment_adjacency), wide quads
// (build_segment_wide) and the learning launch plan (plan_learning_launches).
// Fills: phase_gen_bin_tile, dyn_tiles, phase_dyn_base, segments, zprogs, nztab, rest_tiles, phase_rest_base; seg_aff;
// seg_wide, wide_exc, ntab_quads, nwide_quads; learn_seg, learn_rest_tiles, phase_learn_rest_base.
#include <cstring>
#include <map>

#include "nsk_compile_ctx.h"

namespace nsk {

// Homogeneous segments: runs of uniform tiles with one program (and one evidence flag) become segment launches,
// with a draw table when their members are binary; the other uniform / shape tiles of a colour form its rest
// list.  Also the colour's all-binary general tiles and its tiles with per-lane headers.  lane_words(v, out) is
// the compiler's per-variable word list of the fast path (nsk_compile_words.cpp).
void CompileCtx::plan_segments() {
    const int64_t nvar = c.nvar;
    c.phase_gen_bin_tile.assign((size_t)ncolors, 0);
    for (int32_t k = 0; k < ncolors; k++) {
        int64_t t = c.phase_wb_base[k + 1] - c.phase_wb_base[k];
        while (t > c.phase_gen_tile[k] && ((c.tiles[4 * (c.phase_wb_base[k] + t - 1) + 3] >> 12) & 15u) <= 2u) t--;
        c.phase_gen_bin_tile[k] = t;
    }
    c.phase_dyn_base.assign((size_t)ncolors + 1, 0);
    for (int32_t k = 0; k < ncolors; k++) {
        for (int64_t b = 0; b < c.phase_wb_base[k + 1] - c.phase_wb_base[k]; b++)
            if (c.tiles[4 * (c.phase_wb_base[k] + b) + 2] == 0xFFFFFFFFu)
                c.dyn_tiles.push_back((uint32_t)(c.phase_start[k] + 64 * b));
        c.phase_dyn_base[k + 1] = (int64_t)c.dyn_tiles.size();
    }
    if (c.dyn_tiles.empty()) c.dyn_tiles.push_back(0);
    // homogeneous segments and the rest list
    const int64_t SEG_MIN = 1;
    std::map<uint32_t, int64_t> ztab_of;                        // program -> first table entry
    c.phase_rest_base.assign((size_t)ncolors + 1, 0);
    for (int32_t k = 0; k < ncolors; k++) {
        const int64_t nt = c.phase_wb_base[k + 1] - c.phase_wb_base[k];
        auto tile_ev = [&](int64_t b, bool &full) -> int {     // common isEvidence of a tile or -999
            const int64_t p0 = c.phase_start[k] + 64 * b, p1 = std::min(p0 + 64, c.phase_fast_end[k]);
            full = true;                                       // padding lanes are masked in-kernel
            int ev = -999;
            bool any = false;
            for (int64_t p = p0; p < p1; p++) {
                if (c.p_vid[p] < 0) continue;
                const int e2 = d->variable[c.p_vid[p]].isEvidence;
                any = true;
                if (ev == -999) ev = e2;
                else if (e2 != ev) return -999;
            }
            // (a tile of padding positions only -- run padding, place_variables -- goes with the tiles in front of it)
            if (!any)
                for (int64_t q = p0 - 1; q >= c.phase_start[k]; q--)
                    if (c.p_vid[q] >= 0) return (int)d->variable[c.p_vid[q]].isEvidence;
            return ev;
        };
        int64_t b = 0;
        while (b < nt) {
            const uint32_t *td = &c.tiles[4 * (c.phase_wb_base[k] + b)];
            bool full;
            const int ev = tile_ev(b, full);
            int64_t e = b + 1;
            const bool seg_ok = td[2] != 0xFFFFFFFFu && ((td[3] >> 8) & 7u) < 6u && full && ev != -999 &&
                                (td[3] & 0xFFu) > 0;
            if (seg_ok) {
                while (e < nt) {
                    const uint32_t *te = &c.tiles[4 * (c.phase_wb_base[k] + e)];
                    bool f2;
                    if (te[2] != td[2] || te[3] != td[3] || te[1] != td[1] || tile_ev(e, f2) != ev || !f2) break;
                    e++;
                }
            }
            if (e - b >= SEG_MIN && seg_ok) {
                Compiled::Segment sg;
                sg.phase = k; sg.pos0 = c.phase_start[k] + 64 * b; sg.ntiles = (int32_t)(e - b);
                sg.adj_off = td[0]; sg.prog = td[2]; sg.nslots = td[3] & 0xFFu; sg.kind = (td[3] >> 8) & 7u;
                sg.ev = ev;
                sg.ztab = -1;
                if ((td[3] >> 11) & 1u) {                      // draw table of the program (shared)
                    auto zi = ztab_of.find(sg.prog);
                    if (zi == ztab_of.end() && c.nztab + ((int64_t)1 << sg.nslots) <= ((int64_t)1 << 20)) {
                        zi = ztab_of.emplace(sg.prog, c.nztab).first;
                        c.zprogs.push_back({sg.prog, sg.nslots, (uint32_t)c.nztab, 0u});
                        c.nztab += (int64_t)1 << sg.nslots;
                    }
                    if (zi != ztab_of.end()) sg.ztab = zi->second;
                }
                c.segments.push_back(sg);
            } else if (td[2] == 0xFFFFFFFFu || ((td[3] >> 8) & 7u) != 6u) {      // general tiles: own kernel
                for (int64_t t = b; t < e; t++) c.rest_tiles.push_back((uint32_t)t);
            }
            b = e;
        }
        c.phase_rest_base[k + 1] = (int64_t)c.rest_tiles.size();
    }
    if (c.rest_tiles.empty()) c.rest_tiles.push_back(0);
    if (knobs.verbose) {                 // layout report: tiles by kind, per colour
        for (int32_t k = 0; k < ncolors; k++) {
            int64_t kinds[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int64_t b = 0; b < c.phase_wb_base[k + 1] - c.phase_wb_base[k]; b++) {
                const uint32_t *td = &c.tiles[4 * (c.phase_wb_base[k] + b)];
                kinds[td[2] == 0xFFFFFFFFu ? 8 : (td[3] >> 8) & 7u]++;
            }
            if (knobs.debug_tiles)
                for (int64_t b = 0, shown = 0; b < c.phase_wb_base[k + 1] - c.phase_wb_base[k] && shown < 3; b++) {
                    const uint32_t *td = &c.tiles[4 * (c.phase_wb_base[k] + b)];
                    if (td[2] != 0xFFFFFFFFu) continue;
                    shown++;
                    fprintf(stderr, "  per-lane tile %lld (gen tiles start %lld):", (long long)b, (long long)c.phase_gen_tile[k]);
                    for (int64_t p = c.phase_start[k] + 64 * b; p < c.phase_start[k] + 64 * b + 64; p += 9) {
                        const int64_t v = c.p_vid[p];
                        if (v < 0) { fprintf(stderr, " pad"); continue; }
                        std::vector<uint32_t> ww;
                        lane_words(v, ww);
                        fprintf(stderr, " v%lld f%d ev%d [", (long long)v, (int)fast[v], (int)d->variable[v].isEvidence);
                        for (size_t j = 0; j < ww.size(); j += 1 + ((ww[j] >> 24) & 7u))
                            fprintf(stderr, "%u:%u:%u ", ww[j] >> 27, (ww[j] >> 24) & 7u, ww[j] & 0xFFFFFFu);
                        fprintf(stderr, "]");
                    }
                    fprintf(stderr, "\n");
                }
            fprintf(stderr, "[nsk] colour %d: %lld positions, tiles uniform %lld pair %lld general %lld shape %lld "
                            "per-lane %lld; generic %lld (hub-style %lld)\n", (int)k,
                    (long long)(c.phase_start[k + 1] - c.phase_start[k]),
                    (long long)kinds[0], (long long)(kinds[2] + kinds[3] + kinds[4]), (long long)kinds[6],
                    (long long)kinds[7], (long long)kinds[8],
                    (long long)(c.phase_start[k + 1] - c.phase_fast_end[k]),
                    (long long)(c.phase_heavy_end[k] - c.phase_fast_end[k]));
        }
    }
    if (const char *dv = knobs.debug_var) {       // (diagnostic: where a variable landed)
        for (const char *q = dv; *q;) {
            const int64_t v = atoll(q);
            while (*q && *q != ',') q++;
            if (*q == ',') q++;
            if (v < 0 || v >= nvar || c.color[v] < 0) continue;
            const int64_t p = c.iid[v];
            const int32_t k = c.color[v];
            const int64_t b = (p - c.phase_start[k]) / 64;
            const uint32_t *td = &c.tiles[4 * (c.phase_wb_base[k] + b)];
            fprintf(stderr, "[nsk] var %lld: colour %d position %lld tile %lld td {%u, %u, %u, %#x} kind %u slots %u",
                    (long long)v, (int)k, (long long)p, (long long)b, td[0], td[1], td[2], td[3], (td[3] >> 8) & 7u, td[3] & 0xFFu);
            for (const Compiled::Segment &sg : c.segments)
                if (p >= sg.pos0 && p < sg.pos0 + 64 * (int64_t)sg.ntiles)
                    fprintf(stderr, " | segment pos0 %lld ntiles %d prog %u nslots %u kind %u ev %d ztab %lld", (long long)sg.pos0,
                            sg.ntiles, sg.prog, sg.nslots, sg.kind, sg.ev, (long long)sg.ztab);
            if (td[2] != 0xFFFFFFFFu && ((td[3] >> 8) & 7u) < 6u) {
                fprintf(stderr, " | program:");
                for (uint32_t j = 0; j < 8; j++) {
                    const uint32_t w_ = c.tile_hdr[td[2] + j];
                    fprintf(stderr, " [w%u c%u F%u cl%u ig%u fx%u]", w_ & 0xFFFFFFu, (w_ >> 24) & 7u, (w_ >> 27) & 1u, (w_ >> 28) & 1u,
                            (w_ >> 29) & 1u, (w_ >> 30) & 1u);
                }
            }
            fprintf(stderr, "\n");
        }
    }
}

// Implicit adjacency of table segments (nsk_compile.h seg_aff): per tile the base ids of its member runs when the
// lanes' members are consecutive (a regular grid), so the sweep kernels need no stream there.
int CompileCtx::build_segment_adjacency() {
    uint64_t ntile4 = 0;
    const bool no_aff = knobs.no_affine;
    for (Compiled::Segment &sg : c.segments) {
        sg.aff = -1;
        if (sg.ztab < 0 || no_aff) continue;
        sg.aff = (int64_t)ntile4;
        ntile4 += (uint64_t)sg.ntiles * (sg.nslots > 4 ? 2 : 1);
    }
    if (ntile4 >= ((uint64_t)1 << 30)) { err = "implicit adjacency table too large"; return NSK_E_RANGE; }
    c.seg_aff.assign((size_t)ntile4 * 4 + 4, 0xFFFFFFFFu);
    for (const Compiled::Segment &sg : c.segments) {
        if (sg.aff < 0) continue;
        const int nch = sg.nslots > 4 ? 2 : 1;
        parallel_for(sg.ntiles, [&](int64_t tb0, int64_t tb1, int) {
            for (int64_t t = tb0; t < tb1; t++) {
                const uint64_t wbase = ((uint64_t)sg.adj_off + (uint64_t)t * 64 * nch) * 4;
                int64_t first = -1;                         // first live lane
                for (int64_t i = 0; i < 64 && first < 0; i++) if (c.p_vid[sg.pos0 + 64 * t + i] >= 0) first = i;
                if (first < 0) continue;
                bool ok = true;
                uint32_t base[8];
                for (uint32_t j = 0; j < (uint32_t)(4 * nch) && ok; j++) {
                    const uint64_t wj = wbase + 256 * (j / 4) + (j % 4);
                    const int64_t b0 = (int64_t)c.adj[wj + 4 * first] - first;
                    if (b0 < 0 || b0 + 63 >= c.nid) { ok = false; break; }       // every lane reads a valid id
                    for (int64_t i = 0; i < 64 && ok; i++)
                        if (c.p_vid[sg.pos0 + 64 * t + i] >= 0 && (int64_t)c.adj[wj + 4 * i] != b0 + i) ok = false;
                    base[j] = (uint32_t)b0;
                }
                if (!ok || base[0] == 0xFFFFFFFFu) continue;
                for (int cidx = 0; cidx < nch; cidx++)
                    for (int q = 0; q < 4; q++) c.seg_aff[((size_t)sg.aff + (size_t)t * nch + cidx) * 4 + q] = base[4 * cidx + q];
            }
        }, 64);
    }
    return NSK_OK;
}

// Wide quads of table segments (nsk_compile.h seg_wide): per quad the slot bases when one lane can take four
// consecutive positions, plus the few positions whose member lies elsewhere (exceptions).
int CompileCtx::build_segment_wide() {
    c.seg_wide.clear();
    c.wide_exc.clear();
    c.ntab_quads = c.nwide_quads = 0;
    for (Compiled::Segment &sg : c.segments) sg.wide = -1;
    if (c.vbytes != 1 || knobs.no_wide || c.nsampled < knobs.wide_min) {
        c.seg_wide.assign(4, 0xFFFFFFFFu); c.wide_exc.assign(2, 0u); return NSK_OK;
    }
    uint64_t ndw = 0;
    for (Compiled::Segment &sg : c.segments) {
        if (sg.ztab < 0) continue;
        const int nch = sg.nslots > 4 ? 2 : 1;
        const int64_t nq = ((sg.pos0 + 64 * (int64_t)sg.ntiles + 255) >> 8) - (sg.pos0 >> 8);
        sg.wide = (int64_t)ndw;
        ndw += (uint64_t)nq * NSK_WIDE_STRIDE(nch);
        c.ntab_quads += nq;
    }
    if (ndw >= ((uint64_t)1 << 31)) { err = "wide-quad table too large"; return NSK_E_RANGE; }
    c.seg_wide.assign((size_t)ndw + 4, 0xFFFFFFFFu);
    const int T = compile_threads();
    std::vector<std::vector<uint32_t>> exc_of((size_t)T);              // per thread: {descriptor dword, count, pairs ...}
    std::vector<int64_t> nwide_of((size_t)T, 0);
    for (const Compiled::Segment &sg : c.segments) {
        if (sg.wide < 0) continue;
        const int nch = sg.nslots > 4 ? 2 : 1, stride = NSK_WIDE_STRIDE(nch);
        const int64_t q0 = sg.pos0 >> 8;
        const int64_t nq = ((sg.pos0 + 64 * (int64_t)sg.ntiles + 255) >> 8) - q0;
        parallel_for(nq, [&](int64_t qb0, int64_t qb1, int th) {
            std::vector<uint32_t> &exo = exc_of[(size_t)th];
            for (int64_t qi = qb0; qi < qb1; qi++) {
                const int64_t P = (q0 + qi) << 8;                       // the quad's first position
                if (P < sg.pos0 || P + 256 > sg.pos0 + 64 * (int64_t)sg.ntiles) continue;     // not wholly inside the segment
                const int64_t t0 = (P - sg.pos0) >> 6;
                // member id of slot j at offset o of the quad
                auto member = [&](int64_t o, uint32_t j) -> int64_t {
                    const uint64_t wbase = ((uint64_t)sg.adj_off + (uint64_t)(t0 + (o >> 6)) * 64 * nch) * 4;
                    return (int64_t)c.adj[wbase + 256 * (j / 4) + (j % 4) + 4 * (uint64_t)(o & 63)];
                };
                int64_t first = -1, last = -1;
                for (int64_t o = 0; o < 256; o++)
                    if (c.p_vid[P + o] >= 0) { if (first < 0) first = o; last = o; }
                if (first < 0) continue;
                uint32_t base[8], smask = 0, nexc = 0, exc[2 * NSK_WIDE_MAXEXC];
                bool ok = true;
                for (uint32_t j = 0; j < sg.nslots && ok; j++) {
                    // a slot that names the always-zero id in every lane is no member at all
                    bool zero = true;
                    for (int64_t o = first; o <= last && zero; o++)
                        if (c.p_vid[P + o] >= 0 && member(o, j) != c.zero_id) zero = false;
                    if (zero) { base[j] = 0xFFFFFFFFu; continue; }
                    // the base most live positions agree on: the first's or the last's (an odd cell sits at a run's end)
                    int64_t best = -1, best_miss = 1 << 30;
                    const int64_t cand[3] = {member(first, j) - first, member(last, j) - last,
                                             member((first + last) / 2, j) - (first + last) / 2};
                    for (int k = 0; k < 3; k++) {
                        const int64_t b = cand[k];
                        if (b < 0 || b + 255 >= c.nid || (k > 0 && b == cand[0]) || (k > 1 && b == cand[1])) continue;
                        int64_t miss = 0;
                        for (int64_t o = first; o <= last && miss <= NSK_WIDE_MAXEXC; o++)
                            if (c.p_vid[P + o] >= 0 && member(o, j) != b + o) miss++;
                        if (miss < best_miss) { best_miss = miss; best = b; }
                    }
                    if (best < 0 || nexc + best_miss > NSK_WIDE_MAXEXC) {
                        if (knobs.debug_wide)
                            fprintf(stderr, "[nsk] quad at %lld (segment pos0 %lld): slot %u best %lld misses %lld (first %lld last %lld cand %lld %lld %lld)\n",
                                    (long long)P, (long long)sg.pos0, j, (long long)best, (long long)best_miss, (long long)first, (long long)last,
                                    (long long)cand[0], (long long)cand[1], (long long)cand[2]);
                        if (knobs.debug_wide) {
                            for (int64_t o = first; o <= last; o++)
                                if (c.p_vid[P + o] >= 0 && member(o, j) != best + o) fprintf(stderr, " [o %lld vid %d member %lld]", (long long)o, c.p_vid[P + o], (long long)member(o, j));
                            fprintf(stderr, "\n");
                        }
                        ok = false; break; }
                    base[j] = (uint32_t)best;
                    smask |= 1u << j;
                    for (int64_t o = first; o <= last; o++)
                        if (c.p_vid[P + o] >= 0 && member(o, j) != best + o) {
                            exc[2 * nexc] = (uint32_t)o | (j << 8);
                            exc[2 * nexc + 1] = (uint32_t)member(o, j);
                            nexc++;
                        }
                }
                if (!ok || smask == 0) continue;
                uint32_t any = 0;
                for (uint32_t j = 0; j < sg.nslots; j++) if ((smask >> j) & 1u) { any = base[j]; break; }
                uint32_t *dq = &c.seg_wide[(size_t)sg.wide + (size_t)qi * stride];
                for (uint32_t j = 0; j < (uint32_t)(4 * nch); j++) dq[j] = (j < sg.nslots && ((smask >> j) & 1u)) ? base[j] : any;
                if (dq[0] == 0xFFFFFFFFu) { for (uint32_t j = 0; j < (uint32_t)(4 * nch); j++) dq[j] = 0xFFFFFFFFu; continue; }   // (cannot happen: ids < 2^31)
                dq[4 * nch] = 0; dq[4 * nch + 1] = nexc; dq[4 * nch + 2] = smask; dq[4 * nch + 3] = 0;
                nwide_of[(size_t)th]++;
                if (nexc) {
                    exo.push_back((uint32_t)(sg.wide + qi * stride));
                    exo.push_back(nexc);
                    exo.insert(exo.end(), exc, exc + 2 * nexc);
                }
            }
        }, 16);
        // the segment's exception lists: the threads hold ascending ranges of its quads, so thread order is quad
        // order whatever the thread count
        for (int th = 0; th < T; th++) {
            std::vector<uint32_t> &exo = exc_of[(size_t)th];
            for (size_t i = 0; i < exo.size();) {
                const uint32_t dq = exo[i], n = exo[i + 1];
                c.seg_wide[(size_t)dq + 4 * nch] = (uint32_t)(c.wide_exc.size() / 2);
                c.wide_exc.insert(c.wide_exc.end(), exo.begin() + (long)i + 2, exo.begin() + (long)i + 2 + 2 * (long)n);
                i += 2 + 2 * (size_t)n;
            }
            exo.clear();
        }
    }
    c.nwide_quads = 0;
    for (int th = 0; th < T; th++) c.nwide_quads += nwide_of[(size_t)th];
    c.wide_exc.resize(c.wide_exc.size() + 2, 0u);
    return NSK_OK;
}

// Learning launches over homogeneous segments: segments grouped by (kind, chunks) into tables of <= 8, the
// NSK_LEARN_SEG_LAUNCHES largest tables of a colour become launches, the tiles of the others join the colour's
// learning rest list.
void CompileCtx::plan_learning_launches() {
    // learning launches: segments grouped by (kind, chunks) into tables of <= 8, the
    // NSK_LEARN_SEG_LAUNCHES largest tables of a colour become launches, the tiles of the
    // others join the colour's rest list
    c.phase_learn_rest_base.assign((size_t)ncolors + 1, 0);
    for (int32_t k = 0; k < ncolors; k++) {
        std::vector<Compiled::SegLaunch> tabs;
        for (int tab = 0; tab <= 1; tab++)                  // 0 no draw table, 1 table (compact stream or not)
        for (int kind = 0; kind <= 4; kind++)
            for (int nch = 1; nch <= 2; nch++) {
                Compiled::SegLaunch t;
                memset(&t, 0, sizeof(t));
                t.phase = k; t.kind = tab ? 8 : kind; t.nch = nch; t.tab = tab;
                std::vector<const Compiled::Segment *> mine;       // largest first (seg_of_tile's first probe)
                for (const Compiled::Segment &sg : c.segments) {
                    // table segments of any function share a launch (the table encodes the function)
                    if (sg.phase != k || (sg.nslots > 4 ? 2 : 1) != nch || (sg.ztab < 0 ? 0 : 1) != tab ||
                        (tab ? kind != 0 : (int)(sg.kind == 1 ? 3 : sg.kind) != kind))
                        continue;
                    mine.push_back(&sg);
                }
                std::stable_sort(mine.begin(), mine.end(), [](const Compiled::Segment *a, const Compiled::Segment *b) {
                    return a->ntiles > b->ntiles; });
                for (const Compiled::Segment *sgp : mine) {
                    const Compiled::Segment &sg = *sgp;
                    t.pos0[t.n] = (int32_t)sg.pos0; t.adj_off[t.n] = sg.adj_off; t.prog[t.n] = sg.prog;
                    t.aff[t.n] = sg.aff >= 0 ? (uint32_t)sg.aff : 0xFFFFFFFFu;
                    t.zoff[t.n] = sg.ztab >= 0 ? (uint32_t)sg.ztab : 0u;
                    t.zmask[t.n] = (1u << sg.nslots) - 1u;
                    t.ev[t.n] = sg.ev;
                    t.wide[t.n] = sg.wide;
                    t.tile_start[t.n + 1] = t.tile_start[t.n] + sg.ntiles;
                    if (++t.n == 8) { tabs.push_back(t); t.n = 0; t.tile_start[0] = 0; }
                }
                if (t.n) tabs.push_back(t);
            }
        std::stable_sort(tabs.begin(), tabs.end(), [](const Compiled::SegLaunch &a, const Compiled::SegLaunch &b) {
            return a.tile_start[a.n] > b.tile_start[b.n]; });
        std::vector<uint32_t> extra;
        for (size_t i = 0; i < tabs.size(); i++) {
            if (i < NSK_LEARN_SEG_LAUNCHES && !knobs.no_learn_seg) { c.learn_seg.push_back(tabs[i]); continue; }
            for (int j = 0; j < tabs[i].n; j++)
                for (int32_t t = 0; t < tabs[i].tile_start[j + 1] - tabs[i].tile_start[j]; t++)
                    extra.push_back((uint32_t)((tabs[i].pos0[j] - c.phase_start[k]) / 64 + t));
        }
        for (int64_t i = c.phase_rest_base[k]; i < c.phase_rest_base[k + 1]; i++) extra.push_back(c.rest_tiles[i]);
        std::sort(extra.begin(), extra.end());
        c.learn_rest_tiles.insert(c.learn_rest_tiles.end(), extra.begin(), extra.end());
        c.phase_learn_rest_base[k + 1] = (int64_t)c.learn_rest_tiles.size();
    }
    if (c.learn_rest_tiles.empty()) c.learn_rest_tiles.push_back(0);
}

}  // namespace nsk
