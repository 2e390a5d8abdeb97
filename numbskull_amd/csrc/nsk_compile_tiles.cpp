// nsk_compile_tiles.cpp -- graph compiler, tile stage: what every 64-position tile looks like and what its stream holds.
// Decides: uniform / shape / general / per-lane tiles and their pooled programs, stream offsets and weight rows
// (shape_tiles), which weights are updated in place and their device numbering (find_direct_weights,
// number_direct_weights), the stream contents (fill_tiles) and the gradient format (choose_gradient_format).
// Fills: phase_wb_base, tiles, tile_wrow, nwrows, tile_hdr, adj, nfast; w_direct, multi_wids, ndirect, wmap, wuser
// (and renumbers w_init, f_rec); packed_grad, grad_bound, grad_shift.
#include <cmath>
#include <cstring>
#include <map>

#include "nsk_compile_ctx.h"

namespace nsk {

// Pass 1 over the tiles: the shape of every tile.  Uniform tile = all its lanes have the same header sequence
// (slot program, draw-table candidate); shape tile = same word layout, per-lane functions and weights; general tile =
// E entries x (2 + M) words.  Phase A (parallel over tiles) classifies the tile and reduces its program to a short
// key; phase B (sequential) pools the programs, assigns stream offsets and weight rows.  Sets nwb, tile_colour[t] and
// total4 (the stream's size in 16-byte units) of the context.
int CompileCtx::shape_tiles() {
    const int64_t nw = c.nweight;
    // ---- inlined adjacency streams of the fast variables, one column-major tile per 64 positions
    c.phase_wb_base.assign((size_t)ncolors + 1, 0);
    for (int32_t k = 0; k < ncolors; k++)
        c.phase_wb_base[k + 1] = c.phase_wb_base[k] + (c.phase_fast_end[k] - c.phase_start[k] + 63) / 64;
    nwb = c.phase_wb_base[ncolors];
    c.tiles.assign((size_t)nwb * 4 + 4, 0);
    c.tile_wrow.assign((size_t)nwb + 1, 0);
    auto headers_of = [&](const std::vector<uint32_t> &w, std::vector<uint32_t> &h) {
        h.clear();
        for (size_t j = 0; j < w.size(); j += 1 + ((w[j] >> 24) & 7u)) h.push_back(w[j]);
    };
    // pass 1: shape of every tile.  Uniform tile = all its lanes have the same header sequence.
    // Phase A (parallel over tiles): classify the tile and reduce its program to a short key;
    // phase B (sequential): pool the programs, assign stream offsets and weight rows.
    struct TileShape {
        uint8_t cls;            // 0 per-lane headers, 1 general, 2 uniform, 3 shape
        uint8_t nkey;
        uint8_t empty;          // no variable at all (run padding, place_variables): takes the shape of the tile in front
        int32_t len;            // words per lane before rounding to chunks
        uint32_t flags;         // td[3]
        uint32_t nrows;         // materialised weight rows the tile needs
        uint32_t key[32];       // uniform / shape: the program words (NSK_SHAPE_WORDS); general: {E, M}
    };
    std::vector<TileShape> shapes_of((size_t)nwb);
    tile_colour.assign((size_t)nwb, 0);
    for (int32_t k = 0; k < ncolors; k++)
        for (int64_t t = c.phase_wb_base[k]; t < c.phase_wb_base[k + 1]; t++) tile_colour[t] = k;
    const bool no_shape = knobs.no_shape, no_ztab = knobs.no_ztab;
    parallel_for(nwb, [&](int64_t tb0, int64_t tb1, int) {
        std::vector<uint32_t> words, hdrs, hdrs0;
        for (int64_t t = tb0; t < tb1; t++) {
            const int32_t k = tile_colour[t];
            const int64_t b = t - c.phase_wb_base[k];
            const int64_t p0 = c.phase_start[k] + 64 * b, p1 = std::min(p0 + 64, c.phase_fast_end[k]);
            TileShape &ts = shapes_of[t];
            memset(&ts, 0, sizeof(ts));
            bool gen_tile = false;                             // general tile (kind 6)
            for (int64_t p = p0; p < p1 && !gen_tile; p++)
                if (c.p_vid[p] >= 0 && fast[c.p_vid[p]] == 2) gen_tile = true;
            if (gen_tile) {
                // layout shared by the 64 lanes: E entries of 2 + M words, E and M the maxima over
                // the lanes
                uint32_t E = 0, M = 0, maxcard = 2;
                for (int64_t p = p0; p < p1; p++) {
                    if (c.p_vid[p] < 0) continue;
                    general_words(c.p_vid[p], &words);
                    uint32_t ne = 0;
                    for (size_t j = 0; j < words.size(); j += 2 + ((words[j + 1] >> 4) & 7u)) {
                        ne++;
                        M = std::max(M, (words[j + 1] >> 4) & 7u);
                    }
                    E = std::max(E, ne);
                    maxcard = std::max(maxcard, (uint32_t)d->variable[c.p_vid[p]].cardinality);
                }
                // the walk is specialised on M and eats whole 16-byte chunks: E is a multiple of
                // the entries per super-group (general_walk_m, nsk_kernels_gibbs.h)
                const uint32_t EG = ((2 + M) % 4 == 0) ? 1u : ((2 + M) % 2 == 0) ? 2u : 4u;
                E = (E + EG - 1) / EG * EG;
                if (c.phase_ep[k]) {            // entry-parallel group layout: no per-tile stream
                    ts.cls = 1; ts.nkey = 2; ts.key[0] = 0; ts.key[1] = M;
                    ts.len = 0;
                    ts.flags = (6u << 8) | (maxcard << 12) | (M << 16);
                    continue;
                }
                ts.cls = 1; ts.nkey = 2; ts.key[0] = E; ts.key[1] = M;
                ts.len = (int32_t)(E * (2 + M));
                ts.flags = (uint32_t)ts.len | (6u << 8) | (maxcard << 12) | (M << 16);
                if (nw * 8 > (4 << 20) && E > 0) { ts.flags |= 1u << 19; ts.nrows = E; }
                continue;
            }
            int64_t len = 0;
            bool uniform = true, have0 = false, same_shape = true;
            bool binmem = true;                // every member the lanes read is a binary variable
            // same shape: the lanes have the same number of entries and agree on which entries have members
            // at all; an entry's member slots are the most any lane has there (lanes with fewer leave null
            // words, NSK_SHAPE_NULL).  The classes of the position stage keep that padding small: exact
            // shapes first, member counts rounded up to even for the rest.
            uint32_t slots[32];
            size_t nent = 0;
            for (int64_t p = p0; p < p1; p++) {
                if (c.p_vid[p] < 0) continue;                  // padding position
                lane_words(c.p_vid[p], words);
                for (size_t j = 0; j < words.size(); j += 1 + ((words[j] >> 24) & 7u))
                    for (uint32_t m = 1; m <= ((words[j] >> 24) & 7u); m++)
                        if (d->variable[words[j + m]].cardinality != 2) binmem = false;
                len = std::max<int64_t>(len, (int64_t)words.size());
                headers_of(words, have0 ? hdrs : hdrs0);
                if (have0 && hdrs != hdrs0) {
                    uniform = false;
                    if (hdrs.size() != hdrs0.size()) same_shape = false;
                }
                {
                    const std::vector<uint32_t> &hh = have0 ? hdrs : hdrs0;
                    if (!have0) { nent = std::min<size_t>(hh.size(), 32); if (hh.size() > 32) same_shape = false; }
                    for (size_t j = 0; j < nent && j < hh.size() && same_shape; j++) {
                        const uint32_t no = (hh[j] >> 24) & 7u;
                        if (!have0) slots[j] = no;
                        else if ((no == 0) != (slots[j] == 0)) same_shape = false;
                        else slots[j] = std::max(slots[j], no);
                    }
                }
                have0 = true;
            }
            if (!have0) { hdrs0.clear(); uniform = false; same_shape = false; ts.empty = 1; }
            // (the last tile of a shape class, left with one or two lanes, is no uniform tile: a segment
            //  launch of its own per such tile costs more than the shape walk of its lanes)
            if (p0 >= shape_at[k] && p0 < shape_end[k] && same_shape) uniform = false;
            // slot program of a uniform tile: one word per member slot (an entry without other
            // members still gets one, ignored, slot):
            //   weightId | code << 24 | first << 27 | last << 28 | ignore << 29 | weight fixed << 30
            //   code: 0 NOOP, 1 IMPLY_NATURAL, 2 OR, 3 AND/ISTRUE, 4 EQUAL
            int64_t nslots = 0;
            for (uint32_t h : hdrs0) nslots += std::max<int64_t>(1, (h >> 24) & 7u);
            ts.cls = 0; ts.len = (int32_t)len;
            if (uniform && nslots <= 8 && p1 > p0) {
                uint32_t n = 0;
                for (uint32_t h : hdrs0) {
                    const int fn = (int)(h >> 27) - 1;
                    const uint32_t code = fn == 3 ? 4u : (fn == 2 || fn == 4) ? 3u : fn == 1 ? 2u : fn == 0 ? 1u : 0u;
                    const uint32_t no = (h >> 24) & 7u, wid = h & 0xFFFFFFu;
                    for (uint32_t m = 0; m < std::max(1u, no); m++)
                        ts.key[n++] = wid | (code << 24) | ((m == 0 ? 1u : 0u) << 27) |
                                      ((m + 1 >= no ? 1u : 0u) << 28) | ((no == 0 ? 1u : 0u) << 29) |
                                      ((c.w_fixed[wid] ? 1u : 0u) << 30);
                }
                ts.nkey = (uint8_t)n;
                // kind: every entry has exactly one other member and the same function code ->
                // the kernel runs a specialised, table-free step (code in bits 8..10)
                uint32_t kind = n == 0 ? 0u : (ts.key[0] >> 24) & 7u;
                for (uint32_t j = 0; j < n; j++)
                    if (((ts.key[j] >> 24) & 7u) != kind || ((ts.key[j] >> 27) & 7u) != 3u) kind = 0;   // first+last, not ignored
                // bit 11: draw-table candidate (padding slots read the always-zero id and are masked off by nslots)
                ts.cls = 2;
                ts.flags = (uint32_t)nslots | (kind << 8) | ((binmem && !no_ztab) ? 1u << 11 : 0u);
                ts.len = (int32_t)nslots;
            } else if (same_shape && len > 0 && !no_shape && [&] {
                           int64_t pl = 0;
                           for (size_t j = 0; j < nent; j++) pl += 1 + (int64_t)slots[j];
                           len = pl;                                   // (the padded length from here on)
                           return pl <= knobs.shape_words; }()) {
                // shape tile: per-lane headers (own function and weight) but one word layout for the
                // 64 lanes.  Role program, one word per stream word: 1 header | 8 header of an
                // entry without other members | 16 member | 2 first member | 4 last member; kind 7.
                uint32_t n = 0;
                for (size_t e = 0; e < nent; e++) {
                    const uint32_t no = slots[e];
                    ts.key[n++] = 1u | (no == 0 ? 8u : 0u) | 0x80000000u;   // bit 31 marks role words
                    for (uint32_t m = 0; m < no; m++)
                        ts.key[n++] = 16u | (m == 0 ? 2u : 0u) | (m + 1 == no ? 4u : 0u) | 0x80000000u;
                }
                ts.nkey = (uint8_t)n;
                ts.cls = 3;
                ts.len = (int32_t)len;
                ts.flags = (uint32_t)len | (7u << 8);
                ts.nrows = (uint32_t)hdrs0.size();
            }
        }
    }, 64);
    // a tile of padding positions only (in front of a run that starts on a quad boundary) continues the uniform tiles
    // in front of it: the segment stays one segment, its lanes sample into their own never-read positions
    for (int64_t t = 1; t < nwb; t++)
        if (shapes_of[t].empty && tile_colour[t - 1] == tile_colour[t] && shapes_of[t - 1].cls == 2) {
            shapes_of[t] = shapes_of[t - 1];
            shapes_of[t].empty = 1;
        }
    std::map<std::vector<uint32_t>, uint32_t> hdr_pool;
    std::vector<uint32_t> words, prog;
    total4 = 0;                      // stream size in 16-byte units
    const TileShape *last_ts = nullptr;
    uint32_t last_prog = 0;
    for (int64_t t = 0; t < nwb; t++) {
        const TileShape &ts = shapes_of[t];
        uint32_t *td = &c.tiles[4 * t];
        int64_t len = ts.len;
        td[2] = 0xFFFFFFFFu;
        if (ts.cls != 0) {
            if (last_ts && last_ts->cls == ts.cls && last_ts->nkey == ts.nkey &&
                !memcmp(last_ts->key, ts.key, sizeof(uint32_t) * ts.nkey)) {
                td[2] = last_prog;                              // same program as the previous tile
            } else {
                prog.clear();
                if (ts.cls == 1) {
                    // role program: 1 weight word | 32 descriptor word (8: no member slots) | 16 member
                    // slot | 2 first slot | 4 last slot
                    const uint32_t E = ts.key[0], M = ts.key[1];
                    for (uint32_t e = 0; e < E; e++) {
                        prog.push_back(1u | 0x80000000u);
                        prog.push_back(32u | (M == 0 ? 8u : 0u) | 0x80000000u);
                        for (uint32_t m = 0; m < M; m++)
                            prog.push_back(16u | (m == 0 ? 2u : 0u) | (m + 1 == M ? 4u : 0u) | 0x80000000u);
                    }
                } else {
                    prog.assign(ts.key, ts.key + ts.nkey);
                }
                auto it = hdr_pool.find(prog);
                if (it == hdr_pool.end()) {
                    it = hdr_pool.emplace(prog, (uint32_t)c.tile_hdr.size()).first;
                    c.tile_hdr.insert(c.tile_hdr.end(), prog.begin(), prog.end());
                    c.tile_hdr.resize((c.tile_hdr.size() + 7) / 8 * 8, 0u);   // pad: NOOP, weight 0
                }
                td[2] = it->second;
                last_ts = &ts; last_prog = td[2];
            }
            td[3] = ts.flags;
            if (ts.nrows) {
                // a weight table beyond the L2 (general tiles) / per-lane weights (shape tiles):
                // inference reads materialised weight rows, one coalesced row per entry
                c.tile_wrow[t] = (uint32_t)c.nwrows;
                c.nwrows += (int64_t)ts.nrows;
                if (c.nwrows >= ((int64_t)1 << 31)) { err = "weight stream too large"; return NSK_E_RANGE; }
            }
        }
        len = (len + 3) / 4 * 4;
        td[0] = (uint32_t)total4;
        td[1] = (uint32_t)len;
        total4 += (uint64_t)(len / 4) * 64;
        if (total4 >= ((uint64_t)1 << 31)) { err = "adjacency stream too large"; return NSK_E_RANGE; }
    }
    c.tile_hdr.resize(c.tile_hdr.size() + 8, 0u);
    return NSK_OK;
}

// Direct weights (nsk_compile.h w_direct): the weights with one factor, when at least half of all weights are of
// that kind.  nwb = number of tiles (weights a uniform tile's program names stay with the accumulators).
void CompileCtx::find_direct_weights() {
    const int64_t nw = c.nweight, nfac = c.nfactor;
    c.w_direct.clear(); c.multi_wids.clear(); c.ndirect = 0;
    if (nw > 256 && !knobs.no_direct) {
        std::vector<uint8_t> nfac_of((size_t)nw, 0);                 // factors per weight, saturating at 2
        for (int64_t f = 0; f < nfac; f++) {
            const int64_t wid = d->factor[f].weightId;
            if (wid >= 0 && wid < nw && nfac_of[(size_t)wid] < 2) nfac_of[(size_t)wid]++;
        }
        for (int64_t f : c.repeated_factors) {                       // a factor listed twice by one variable: two visits per class
            const int64_t wid = d->factor[f].weightId;
            if (wid >= 0 && wid < nw) nfac_of[(size_t)wid] = 2;
        }
        // a NOOP factor reads no member, so the colouring may put two of its members into one class: two visits
        // of its weight in that class, which only the accumulators take.  (Its member list is not validated: it is
        // read here only where it lies inside fmap.)
        std::vector<std::pair<int32_t, int64_t>> seen;                // (colour, variable) of a NOOP factor's members
        for (int64_t f = 0; f < nfac; f++) {
            const nsk_factor &fa = d->factor[f];
            if (fa.factorFunction != -1 || fa.arity < 2 || fa.weightId < 0 || fa.weightId >= nw) continue;
            if (fa.ftv_offset < 0 || fa.arity > c.nedge || fa.ftv_offset > c.nedge - fa.arity) continue;
            seen.clear();
            for (int64_t l = fa.ftv_offset; l < fa.ftv_offset + fa.arity; l++) {
                const int64_t v = d->fmap[l].vid;
                if (v >= 0 && v < c.nvar && c.color[(size_t)v] >= 0) seen.push_back({c.color[(size_t)v], v});
            }
            std::sort(seen.begin(), seen.end());
            for (size_t a = 1; a < seen.size(); a++)
                if (seen[a].first == seen[a - 1].first && seen[a].second != seen[a - 1].second) { nfac_of[(size_t)fa.weightId] = 2; break; }
        }
        for (int64_t t = 0; t < nwb; t++) {                          // weights named by uniform tiles' programs
            const uint32_t *td = &c.tiles[4 * t];
            if (td[2] == 0xFFFFFFFFu || ((td[3] >> 8) & 7u) >= 6u) continue;
            for (uint32_t j = 0; j < (td[3] & 0xFFu); j++) {
                const uint32_t wid = c.tile_hdr[td[2] + j] & 0xFFFFFFu;
                if ((int64_t)wid < nw) nfac_of[wid] = 2;
            }
        }
        int64_t nd = 0;
        for (int64_t w = 0; w < nw; w++) nd += (nfac_of[(size_t)w] == 1 && !c.w_fixed[(size_t)w]) ? 1 : 0;
        if (2 * nd >= nw) {
            c.w_direct.assign((size_t)(nw + 31) / 32, 0u);
            for (int64_t w = 0; w < nw; w++) {
                if (nfac_of[(size_t)w] == 1 && !c.w_fixed[(size_t)w]) c.w_direct[(size_t)w >> 5] |= 1u << (w & 31);
                else c.multi_wids.push_back((int32_t)w);
            }
            c.ndirect = nd;
        }
        if (knobs.verbose) fprintf(stderr, "[nsk] weights with one factor %lld of %lld: %s\n", (long long)nd, (long long)nw,
                             c.ndirect ? "updated in place" : "too few, accumulators for all");
    }
}

// Internal numbering of the direct weights (nsk_compile.h wmap): the order in which the layout's positions, each
// walking its lists, first meet them; a weight no position names keeps the tail.  Returns false (and leaves the
// caller's numbering) on a handle that samples a range of a larger graph: the ranks of a distributed run add their
// weight tables element by element.
bool CompileCtx::number_direct_weights() {
    const int64_t nw = c.nweight, nvar = c.nvar, nfac = c.nfactor;
    c.wmap.clear(); c.wuser.clear();
    if (!(c.ndirect && c.own_begin == 0 && c.own_end == nvar && !(d->flags & NSK_FLAG_PARTITION) && !knobs.no_worder))
        return false;
    auto is_direct = [&](int64_t w) { return (c.w_direct[(size_t)w >> 5] >> (w & 31)) & 1u; };
    std::vector<uint32_t> seen((size_t)(nw + 31) / 32, 0u);
    // (bands of 2^24 ids are numbered separately: a slot then has the bits of the id it replaces, and the
    // 24-bit weight field of the uniform-tile words holds whatever held before)
    std::vector<std::vector<int32_t>> order((size_t)((nw - 1) >> 24) + 1);
    for (int64_t p = 0; p < (int64_t)c.p_vid.size(); p++) {
        const int64_t v = c.p_vid[p];
        if (v < 0) continue;
        const nsk_variable &var = d->variable[v];
        const int64_t nslots = var.dataType == 0 ? 1 : var.cardinality;
        for (int64_t k = 0; k < nslots; k++) {
            const nsk_vtf &vt = d->vmap[var.vtf_offset + k];
            for (int64_t j = 0; j < vt.factor_index_length; j++) {
                const int64_t w = d->factor[d->factor_index[vt.factor_index_offset + j]].weightId;
                if (w < 0 || w >= nw || !is_direct(w) || ((seen[(size_t)w >> 5] >> (w & 31)) & 1u)) continue;
                seen[(size_t)w >> 5] |= 1u << (w & 31);
                order[(size_t)w >> 24].push_back((int32_t)w);
            }
        }
    }
    for (int64_t w = 0; w < nw; w++)
        if (is_direct(w) && !((seen[(size_t)w >> 5] >> (w & 31)) & 1u)) order[(size_t)w >> 24].push_back((int32_t)w);
    c.wmap.resize((size_t)nw); c.wuser.resize((size_t)nw);
    std::vector<size_t> taken(order.size(), 0);
    for (int64_t w = 0; w < nw; w++) {
        if (!is_direct(w)) { c.wmap[(size_t)w] = (int32_t)w; c.wuser[(size_t)w] = (int32_t)w; continue; }
        const int32_t met = order[(size_t)w >> 24][taken[(size_t)w >> 24]++];
        c.wmap[(size_t)met] = (int32_t)w;               // the k-th weight of the band met takes its k-th direct slot
        c.wuser[(size_t)w] = met;
    }
    for (int64_t w = 0; w < nw; w++) c.w_init[(size_t)w] = d->weight[c.wuser[(size_t)w]].initialValue;
    for (int64_t f = 0; f < nfac; f++) {
        const int64_t w = d->factor[f].weightId;
        if (w >= 0 && w < nw) c.f_rec[4 * f + 2] = (uint32_t)c.wmap[(size_t)w];
    }
    return true;
}

// Pass 2 over the tiles: the lanes' words into the stream `adj` (total4 = its size in 16-byte units), chunk-major
// per tile.  general_words / lane_words (nsk_compile_words.cpp) are the per-variable word lists (general tiles / fast path).
void CompileCtx::fill_tiles() {
    // pass 2: fill the tiles.  Padding: member slots read the always-zero id (c.zero_id) in uniform
    // tiles, 0xFFFFFFFF in tiles with per-lane headers.
    c.adj.assign((size_t)total4 * 4 + 4, 0xFFFFFFFFu);
    std::vector<int64_t> nfast_part((size_t)compile_threads() + 1, 0);
    parallel_for(nwb, [&](int64_t tb0, int64_t tb1, int tix) {
        std::vector<uint32_t> words;
        int64_t nfast_here = 0;
        for (int64_t t = tb0; t < tb1; t++) {
            const int32_t k = tile_colour[t];
            const int64_t b = t - c.phase_wb_base[k];
            const int64_t p0 = c.phase_start[k] + 64 * b, p1 = std::min(p0 + 64, c.phase_fast_end[k]);
            const uint32_t *td = &c.tiles[4 * t];
            const uint64_t base = (uint64_t)td[0] * 4;
            const bool uniform = td[2] != 0xFFFFFFFFu && ((td[3] >> 8) & 7u) < 6u;
            const bool general = td[2] != 0xFFFFFFFFu && ((td[3] >> 8) & 7u) == 6u;
            const bool shape = td[2] != 0xFFFFFFFFu && ((td[3] >> 8) & 7u) == 7u;
            if (td[2] != 0xFFFFFFFFu) {     // padding: uniform tiles read the always-zero id, shape tiles variable / weight 0
                const uint32_t padw = uniform ? (uint32_t)c.zero_id : 0u;
                for (uint64_t j = 0; j < (uint64_t)td[1] * 64; j++) c.adj[base + j] = padw;
            }
            for (int64_t p = p0; p < p1; p++) {
                if (c.p_vid[p] < 0) continue;
                size_t out = 0;
                auto put = [&](uint32_t word) {
                    c.adj[base + 256 * (out / 4) + 4 * (uint64_t)(p - p0) + (out % 4)] = word;
                    out++;
                };
                if (general && c.phase_ep[k]) { nfast_here++; continue; }     // laid out by groups, below
                if (general) {               // entries padded to M member slots, then E entries
                    general_words(c.p_vid[p], &words);
                    const uint32_t M = (td[3] >> 16) & 7u, E = (td[3] & 0xFFu) / (2 + M);
                    uint32_t ne = 0;
                    for (size_t j = 0; j < words.size(); ne++) {
                        const uint32_t no = (words[j + 1] >> 4) & 7u;
                        put(words[j]); put(words[j + 1]);
                        for (uint32_t m = 2; m < 2 + no; m++)        // member: internal id | deo << 27
                            put((uint32_t)c.iid[words[j + m] & NSK_GEN_NULL] | (words[j + m] & ~NSK_GEN_NULL));
                        for (uint32_t m = no; m < M; m++) put(NSK_GEN_NULL);
                        j += 2 + no;
                    }
                    for (; ne < E; ne++) {                        // an entry no candidate value owns
                        put(0u);
                        put(14u << 14);
                        for (uint32_t m = 0; m < M; m++) put(NSK_GEN_NULL);
                    }
                    nfast_here++;
                    continue;
                }
                lane_words(c.p_vid[p], words);
                for (size_t j = 0; j < words.size();) {
                    const uint32_t nother = (words[j] >> 24) & 7u;
                    if (!uniform) put(words[j]);
                    else if (nother == 0) put((uint32_t)c.zero_id);      // the ignored slot of a member-less entry
                    for (uint32_t m = 1; m <= nother; m++) put((uint32_t)c.iid[words[j + m]]);
                    // shape tile: the member slots of the tile's layout that this lane's entry lacks
                    while (shape && out < (size_t)td[1] && (c.tile_hdr[td[2] + out] & 0x80000010u) == 0x80000010u)
                        put(NSK_SHAPE_NULL);
                    j += 1 + nother;
                }
                nfast_here++;
            }
        }
        nfast_part[tix] = nfast_here;
    }, 64);
    for (int64_t x : nfast_part) c.nfast += x;
}

// Gradient format of the learning accumulators.  Integer gradients?  (p1 - p0) * featureValue is an integer of
// magnitude <= 2 when featureValue is -1, 0 or 1 and no function returns counts or logarithms; visits per weight and
// class are bounded by the weight's member edges: the 32 fraction bits of G then carry the visit count (packed_grad).
// And the fixed-point range (grad_bound, grad_shift).
void CompileCtx::choose_gradient_format() {
    const int64_t nw = c.nweight, nfac = c.nfactor;
    bool ok = true;
    std::vector<int64_t> edges_of((size_t)nw, 0);
    for (int64_t f = 0; f < nfac && ok; f++) {
        const nsk_factor &fa = d->factor[f];
        const int fn = fa.factorFunction;
        if (!(fa.featureValue == 1.0 || fa.featureValue == 0.0 || fa.featureValue == -1.0)) ok = false;
        if (fn == 7 || fn == 8 || fn == 30) ok = false;            // LINEAR, RATIO, UFO
        if (fa.weightId >= 0 && fa.weightId < nw) edges_of[fa.weightId] += std::max<int64_t>(fa.arity, 1);
    }
    for (int64_t i = 0; i < nw && ok; i++) if (edges_of[i] >= ((int64_t)1 << 28)) ok = false;
    c.packed_grad = ok && !knobs.no_packed;
    // Q31.32 range: a class's gradient sum for weight w is at most sum over its factors of
    // |featureValue| * (largest |value difference| of the function) * (member edges)
    std::vector<double> gbound((size_t)nw, 0.0);
    for (int64_t f = 0; f < nfac; f++) {
        const nsk_factor &fa = d->factor[f];
        if (fa.weightId < 0 || fa.weightId >= nw) continue;
        const double ar = (double)std::max<int64_t>(fa.arity, 1);
        const int fn = fa.factorFunction;
        const double span = fn == 7 ? ar : fn == 8 ? std::log(ar + 1.0) : fn == 30 ? 1e6 : 2.0;
        gbound[fa.weightId] += std::fabs(fa.featureValue) * span * ar;
    }
    c.grad_bound = 0.0;
    for (int64_t i = 0; i < nw; i++) c.grad_bound = std::max(c.grad_bound, gbound[i]);
    // Q31.32 holds sums below 2^31; a larger bound trades fraction bits for range (the reference
    // sums float64 gradients, learning.py:109): Q(31+s).(32-s), gradients below 2^-(33-s) vanish
    c.grad_shift = 0;
    while (c.grad_shift < 32 && c.grad_bound >= 1073741824.0 * std::ldexp(1.0, c.grad_shift)) c.grad_shift++;
    if (c.grad_shift > 0) c.packed_grad = false;       // the fraction bits are no longer free for visit counts
}

}  // namespace nsk
