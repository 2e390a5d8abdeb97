// nsk_compile_place.cpp -- graph compiler, position stage: where every sampled variable sits.  Decides: the classes of
// the fast variables, which variables move to general tiles or the generic path, the order inside a colour, run
// padding for wide quads (find_run_padding) and the internal ids (assign_internal_ids).
// Fills: phase_start, phase_end, phase_fast_end, phase_heavy_end, phase_gen_tile, phase_ep, phase_ep_emax, npos,
// nsampled, p_vid, v_pos (p_info, p_slot, p_cnt, p_init sized); iid, zero_id, nid, v_card_i, m_rec (to internal ids).
#include <map>
#include <thread>
#include <unordered_map>

#include "nsk_compile_ctx.h"

namespace nsk {

// run padding of one exact class: (rank in the class, empty positions in front of it) pairs and their sum
struct ClassPad { std::vector<std::pair<int64_t, int64_t>> at; int64_t total = 0; };

// Affine runs of one exact class in a first layout (place_variables): the class holds `count` variables at positions
// [start, start + count), id order, all with the same slot program.  B_j(r) = (position of member j of the r-th
// variable) - r is constant along a run.  A position whose members disagree with the run's bases in some slot is an
// EXCEPTION when its successors agree again (the end cell of a grid row: its neighbour lives in the border class), a
// BREAK when they settle on other bases (the next grid row).  Out: the empty positions to put in front of ranks so
// that every long run starts on a multiple of 256 (the class itself will start on one); false: nothing worth padding.
static bool find_run_padding(const CompileCtx &x, int64_t start, int64_t count, ClassPad &pd) {
    const nsk_graph_desc *d = x.d;
    const Compiled &c = x.c;
    std::vector<std::pair<int64_t, int64_t>> &at = pd.at;
    int64_t &total = pd.total;
    at.clear();
    total = 0;
    // member slots of the class (its variables share one program: same factor functions and member counts)
    int ns = 0;
    {
        const int64_t v = c.p_vid[start];
        const nsk_vtf &vt = d->vmap[d->variable[v].vtf_offset];
        for (int64_t j = 0; j < vt.factor_index_length; j++) {
            const nsk_factor &fa = d->factor[d->factor_index[vt.factor_index_offset + j]];
            if (fa.factorFunction == -1) continue;
            for (int64_t l = fa.ftv_offset; l < fa.ftv_offset + fa.arity; l++) if (d->fmap[l].vid != v) ns++;
        }
    }
    if (ns == 0 || ns > 8) return false;
    // provisional ids: a sampled variable's position, the ghosts this handle reads behind them in id order
    std::vector<int64_t> B((size_t)count * (size_t)ns);
    const int64_t NONE = INT64_MIN / 2;
    parallel_for(count, [&](int64_t rb0, int64_t rb1, int) {
        for (int64_t r = rb0; r < rb1; r++) {
            const int64_t v = c.p_vid[start + r];
            const nsk_vtf &vt = d->vmap[d->variable[v].vtf_offset];
            int s = 0;
            for (int64_t j = 0; j < vt.factor_index_length && s <= ns; j++) {
                const nsk_factor &fa = d->factor[d->factor_index[vt.factor_index_offset + j]];
                if (fa.factorFunction == -1) continue;
                for (int64_t l = fa.ftv_offset; l < fa.ftv_offset + fa.arity; l++) {
                    const int64_t m = d->fmap[l].vid;
                    if (m == v) continue;
                    int64_t id = c.v_pos[m];
                    if (id < 0) {
                        const auto it = std::lower_bound(c.ghost_needs.begin(), c.ghost_needs.end(), (int32_t)m);
                        id = (it != c.ghost_needs.end() && *it == m) ? c.npos + (it - c.ghost_needs.begin()) : NONE;
                    }
                    if (s < ns) B[(size_t)r * ns + s] = id == NONE ? NONE + r : id - r;     // (NONE + r: equal to nothing)
                    s++;
                }
            }
            for (; s < ns; s++) B[(size_t)r * ns + s] = NONE + r;
        }
    });
    auto miss = [&](int64_t r, const int64_t *base) { int m = 0; for (int j = 0; j < ns; j++) m += B[(size_t)r * ns + j] != base[j]; return m; };
    // per-slot mode over a short window ahead of r
    auto settle = [&](int64_t r, int64_t *out) {
        for (int j = 0; j < ns; j++) {
            int64_t best = B[(size_t)r * ns + j];
            int bestn = 0;
            for (int64_t a = r; a < std::min(count, r + 5); a++) {
                int n = 0;
                for (int64_t b2 = r; b2 < std::min(count, r + 5); b2++) n += B[(size_t)b2 * ns + j] == B[(size_t)a * ns + j];
                if (n > bestn) { bestn = n; best = B[(size_t)a * ns + j]; }
            }
            out[j] = best;
        }
    };
    std::vector<int64_t> run_start;          // ranks
    int64_t cur[8], nxt[8];
    settle(0, cur);
    run_start.push_back(0);
    for (int64_t r = 1; r < count; r++) {
        if (miss(r, cur) == 0) continue;
        settle(r, nxt);
        bool same = true;
        for (int j = 0; j < ns; j++) same = same && nxt[j] == cur[j];
        if (same) continue;                                           // an exception: its successors agree with the run
        // a break: the new run starts at the first position that fits the new bases better than the old ones
        int64_t rb = r;
        while (rb < std::min(count, r + 4) && miss(rb, nxt) >= miss(rb, cur)) rb++;
        if (rb >= std::min(count, r + 4)) rb = r;
        if (rb > run_start.back()) run_start.push_back(rb);
        for (int j = 0; j < ns; j++) cur[j] = nxt[j];
        r = rb;
    }
    run_start.push_back(count);
    // long runs start on multiples of 256 when that wastes little
    int64_t posn = 0;                         // position relative to the class start (a multiple of 256)
    int64_t padded = 0, covered = 0;
    for (size_t i = 0; i + 1 < run_start.size(); i++) {
        const int64_t len = run_start[i + 1] - run_start[i];
        const int64_t waste = (256 - len % 256) % 256;
        const bool good = len >= 384 && waste * 12 <= len;
        if (good && posn % 256 != 0) {
            const int64_t pad = 256 - posn % 256;
            at.push_back({run_start[i], pad});
            total += pad;
            posn += pad;
        }
        if (good) { padded++; covered += len; }
        posn += len;
    }
    if (x.knobs.debug_wide) {
        fprintf(stderr, "[nsk] class at %lld (%lld variables, %d slots): %zu runs, %lld padded, %lld empty positions; runs start at", (long long)start,
                (long long)count, ns, run_start.size() - 1, (long long)padded, (long long)total);
        for (size_t i = 0; i + 1 < run_start.size() && i < 12; i++) fprintf(stderr, " %lld", (long long)run_start[i]);
        fprintf(stderr, "\n");
    }
    if (padded == 0 || total * 10 > count || covered * 2 < count) { at.clear(); total = 0; return false; }
    return true;
}

// Positions: colour-major.  Inside a colour the fast variables grouped by class -- exact program, exact shape, padded
// shape (per id range) -- so that the 64 lanes of a tile share one slot program / word layout; every class with at
// least 64 members starts on a tile boundary (the gap is padded with empty positions, p_vid = -1); smaller classes
// share a tail in id order; then the general tiles' variables (sorted), then the generic-path variables (binned by
// work).  fast[v]: 1 fast path, 2 general tile, 0 generic (variables that fit no class move from 1 to 2 or 0 here).
// [shape_at[k], shape_end[k]) = the positions of colour k's shape classes (tile shapes, pass 1).
int CompileCtx::place_variables() {
    const int64_t nvar = c.nvar, nw = c.nweight;
    const int64_t LIM = (int64_t)1 << 31;
    // ---- positions: colour-major.  Inside a colour: the fast variables grouped by "shape class"
    // -- the sequence of (function, member count, weight id) of their factor lists plus their
    // evidence flag -- so that the 64 lanes of a tile share one slot program; every class with at
    // least 64 members starts on a tile boundary (the gap is padded with empty positions,
    // p_vid = -1); smaller classes share a tail in id order; then the generic-path variables.
    // Order inside a class: variable id.
    c.phase_start.assign((size_t)ncolors + 1, 0);
    c.phase_end.assign((size_t)ncolors, 0);
    c.phase_fast_end.assign((size_t)ncolors, 0);
    c.phase_gen_tile.assign((size_t)ncolors, 0);
    c.v_pos.assign(nvar, -1);
    shape_at.assign((size_t)ncolors, 0);
    shape_end.assign((size_t)ncolors, 0);
    // id blocks of the general tiles' sort order (per-lane walk / entry-parallel groups)
    const int64_t gen_block = knobs.gen_block;
    const int64_t ep_block = knobs.ep_block;
    // sig: exact program (function, member count, weight id per entry, evidence flag);
    // shp: shape only (member count per entry, evidence flag), 0 when the stream would exceed
    //      16 words.  General-tile variables are not classed: they are sorted (below).
    // pshp: the shape with every entry's member count rounded up to even ("padded" shape): variables whose
    //      exact shape is rare share tiles with near shapes, the missing member slots filled with null
    //      words (NSK_SHAPE_NULL) -- with individual weights and lists of 7+ entries the exact shapes
    //      (2^(entries-1) of them on the weighted boolean graph) no longer fill tiles
    std::vector<uint64_t> sig, shp, pshp;           // (sized below, when the graph has such variables at all)
    // Shape classes are formed per id range ("part") of the graph: the lanes of a shape tile then come from
    // one part, and the values and weights they gather -- mostly those of id neighbours -- from a
    // correspondingly narrow stretch of every colour's positions (the kernels hand an XCD a contiguous
    // eighth of the colour's tiles, so one L2 serves those gathers).  One class over the whole id range
    // put 64 unrelated variables into a tile: the learning sweep of the 4M-variable weighted boolean
    // graph missed the L2 11 times per variable.  Parts of >= 2^18 ids keep the leftovers (< 64 members
    // of a shape in a part, general tiles) few: that graph's learning sweep, 8 / 16 / 32 parts: 3.71 / 4.07 /
    // 4.06e9 updates/s (tools/sessions/history/r4_s26.sh).
    const bool no_pshape = knobs.no_pad_shape || knobs.no_shape;
    const int64_t shape_parts = knobs.shape_parts ? knobs.shape_parts             // (0: not set)
                                                  : std::max<int64_t>(1, std::min<int64_t>(64, (nvar + (1 << 18) - 1) >> 18));
    std::vector<int64_t> nfast_of((size_t)ncolors, 0), ngen_of((size_t)ncolors, 0), ngt_of((size_t)ncolors, 0);
    for (int64_t v = 0; v < nvar; v++) {
        if (c.color[v] < 0) continue;
        if (fast[v] == 2) ngt_of[c.color[v]]++;
        else if (!fast[v]) ngen_of[c.color[v]]++;
        else nfast_of[c.color[v]]++;
    }
    {
        int64_t nclassed = 0;
        for (int32_t k = 0; k < ncolors; k++) nclassed += nfast_of[k];
        if (nclassed > 0) { sig.assign((size_t)nvar, 0); shp.assign((size_t)nvar, 0); pshp.assign((size_t)nvar, 0); }
    }
    parallel_for(nvar, [&](int64_t vb0, int64_t vb1, int) {
    for (int64_t v = vb0; v < vb1; v++) {
        if (c.color[v] < 0 || fast[v] != 1) continue;
        const nsk_variable &var = d->variable[v];
        const nsk_vtf &vt = d->vmap[var.vtf_offset];
        // (the evidence flag is multiplied in before the first word: a plain xor would cancel
        // against the low bit of the first weight id / member count)
        uint64_t h = (0xcbf29ce484222325ull ^ (uint64_t)(uint8_t)var.isEvidence) * 0x100000001b3ull;
        uint64_t h2 = (h ^ 0x9e3779b97f4a7c15ull ^ ((uint64_t)(v * shape_parts / std::max<int64_t>(nvar, 1)) << 40)) * 0x100000001b3ull;
        uint64_t h3 = (h2 ^ 0xd6e8feb86659fd93ull) * 0x100000001b3ull;
        int64_t nwords = 0, pwords = 0;
        uint64_t maxo = 0;
        for (int64_t j = 0; j < vt.factor_index_length; j++) {
            const nsk_factor &fa = d->factor[d->factor_index[vt.factor_index_offset + j]];
            uint64_t others = 0;
            if (fa.factorFunction != -1)
                for (int64_t l = fa.ftv_offset; l < fa.ftv_offset + fa.arity; l++)
                    if (d->fmap[l].vid != v) others++;
            const uint64_t word = ((uint64_t)(fa.factorFunction + 1) << 27) | (others << 24) | (uint64_t)fa.weightId;
            h = (h ^ word) * 0x100000001b3ull;
            h ^= h >> 29;
            h2 = (h2 ^ (others + 1)) * 0x100000001b3ull;
            h2 ^= h2 >> 31;
            const uint64_t padded = (others + 1) & ~(uint64_t)1;
            maxo = std::max(maxo, others);
            h3 = (h3 ^ (padded + 1)) * 0x100000001b3ull;
            h3 ^= h3 >> 31;
            nwords += 1 + (int64_t)others;
            pwords += 1 + (int64_t)padded;
        }
        sig[v] = h | 1;
        // (a variable the entry-parallel groups can take -- <= 3 other members per entry, <= 16 entries -- joins a
        //  shape class only with a list of a few words, shape_words_ep)
        const int64_t lim = (maxo <= 3 && vt.factor_index_length <= 16) ? knobs.shape_words_ep : knobs.shape_words;
        shp[v] = nwords <= lim ? (h2 | 1) : 0;
        pshp[v] = (pwords <= lim && !no_pshape) ? (h3 | 1) : 0;
    }
    });
    lap("positions: signatures");
    // (hash maps: with one weight per factor every variable is a class of its own -- millions of keys;
    //  nothing below depends on their iteration order.  The colours are independent: one thread each.)
    typedef std::unordered_map<uint64_t, std::pair<int64_t, int64_t>> ClassMap;        // key -> (count, first vid)
    std::vector<ClassMap> classes((size_t)ncolors), shapes((size_t)ncolors), pshapes((size_t)ncolors);
    // a class gets tiles of its own when it fills at least one (64 members) -- or whatever its
    // size when the colour has only a few small classes (then padding them costs nothing
    // and no tile is left with mixed programs, e.g. the corner cells of a grid)
    std::vector<int64_t> min_class((size_t)ncolors, 64);
    parallel_for(ncolors, [&](int64_t kb0, int64_t kb1, int) {
    for (int32_t k = (int32_t)kb0; k < (int32_t)kb1; k++) {
        if (nfast_of[k] == 0) continue;                 // (nothing to class: four scans of the variables saved)
        ClassMap &cls = classes[k], &shs = shapes[k], &pss = pshapes[k];
        cls.reserve((size_t)nfast_of[k]);
        for (int64_t v = 0; v < nvar; v++) {
            if (c.color[v] != k || fast[v] != 1) continue;
            auto &e = cls[sig[v]];
            if (e.first++ == 0) e.second = v;
        }
        int64_t nsmall = 0;
        for (auto &kv : cls) if (kv.second.first < 64) nsmall++;
        if (nsmall <= 16) min_class[k] = 1;
        // variables outside the big exact classes are grouped by shape
        for (int64_t v = 0; v < nvar; v++) {
            if (c.color[v] != k || fast[v] != 1 || shp[v] == 0 || cls[sig[v]].first >= min_class[k]) continue;
            auto &e = shs[shp[v]];
            if (e.first++ == 0) e.second = v;
        }
        // ... and the ones whose exact shape fills no tile by padded shape
        for (int64_t v = 0; v < nvar; v++) {
            if (c.color[v] != k || fast[v] != 1 || pshp[v] == 0 || cls[sig[v]].first >= min_class[k]) continue;
            if (shp[v] != 0 && shs[shp[v]].first >= 64) continue;
            auto &e = pss[pshp[v]];
            if (e.first++ == 0) e.second = v;
        }
        // what neither an exact nor a shape class can take would end in mixed tiles with per-lane
        // parsing: the general tiles' sorted layout serves those variables better
        for (int64_t v = 0; v < nvar && !no_general; v++) {
            if (c.color[v] != k || fast[v] != 1 || cls[sig[v]].first >= min_class[k]) continue;
            if (shp[v] != 0 && shs[shp[v]].first >= 64) continue;
            if (pshp[v] != 0 && pss[pshp[v]].first >= 64) continue;
            if (shp[v] != 0) shs[shp[v]].first--;
            if (pshp[v] != 0) pss[pshp[v]].first--;
            nfast_of[k]--;
            if (general_words(v, nullptr)) { fast[v] = 2; ngt_of[k]++; }
            else { fast[v] = 0; ngen_of[k]++; }          // long lists: wave-per-variable / generic kernels
        }
    }
    }, 1);
    // a colour whose exact / shape classes are a sliver next to its general tiles gives them up:
    // their few tiles would cost two or three extra launches per class and sweep
    for (int32_t k = 0; k < ncolors && !no_general; k++) {
        if (nfast_of[k] == 0 || nfast_of[k] * 20 >= ngt_of[k]) continue;
        for (int64_t v = 0; v < nvar; v++) {
            if (c.color[v] != k || fast[v] != 1) continue;
            nfast_of[k]--;
            if (general_words(v, nullptr)) { fast[v] = 2; ngt_of[k]++; }
            else { fast[v] = 0; ngen_of[k]++; }
        }
        classes[k].clear();
        shapes[k].clear();
        pshapes[k].clear();
    }
    if (knobs.verbose) { int64_t ng = 0, nf = 0; for (int32_t k = 0; k < ncolors; k++) { ng += ngt_of[k]; nf += nfast_of[k]; } fprintf(stderr, "[nsk] after the classes: %lld general-tile variables, %lld classed\n", (long long)ng, (long long)nf); }
    lap("positions: classes");
    // ---- what does not depend on the positions: work bins of the generic-path variables, the general tiles' order ----
    // generic-path variables of a colour are ordered by the work of one update (factor-list
    // lengths x arities over all candidate values, binned) so that the 64 lanes of a wave finish
    // together; inside a bin: variable id.
    std::vector<uint32_t> gw;
    std::vector<uint8_t> work_bin(nvar, 0);
    for (int64_t v = 0; v < nvar; v++) {
        if (c.color[v] < 0 || fast[v]) continue;
        const nsk_variable &var = d->variable[v];
        const int64_t nslots = var.dataType == 0 ? 1 : var.cardinality;
        int64_t work = 0, listlen = 0;
        for (int64_t kk = 0; kk < nslots; kk++) {
            const nsk_vtf &vt = d->vmap[var.vtf_offset + kk];
            listlen += vt.factor_index_length;
            for (int64_t j = 0; j < vt.factor_index_length; j++)
                work += 2 + std::max<int64_t>(d->factor[d->factor_index[vt.factor_index_offset + j]].arity, 0);
        }
        if (var.dataType == 0) work *= var.cardinality;
        int bin = 0;
        while (work > 8 && bin < 39) { work = work * 3 / 4; bin++; }     // ~log_{4/3} bins
        work_bin[v] = (uint8_t)(40 - bin);                               // heavier variables first
        // hubs: a whole wave works on one such variable (heavy_update in k_gibbs_general / k_learn_heavy)
        if (listlen >= NSK_HEAVY_LIST && !knobs.no_heavy) work_bin[v] = 0;
    }
    // a colour with few generic-path variables gives every one of them a wave: the one-lane
    // kernel's run time is the latency of its longest serial walk however few lanes are busy
    if (!knobs.no_heavy)
        for (int64_t v = 0; v < nvar; v++)
            if (c.color[v] >= 0 && !fast[v] && ngen_of[c.color[v]] <= NSK_FEW_GENERIC) work_bin[v] = 0;
    std::vector<std::vector<int64_t>> bin_count((size_t)ncolors, std::vector<int64_t>(42, 0));
    for (int64_t v = 0; v < nvar; v++)
        if (c.color[v] >= 0 && !fast[v]) bin_count[c.color[v]][work_bin[v] + 1]++;
    lap("positions: work bins");
    // general-tile variables of a colour: sorted by (entries, most other members of an entry),
    // largest first, and cut into tiles of 64 -- a tile's layout is the maximum over its lanes,
    // so neighbours in this order waste the least padding (SELL-C-sigma)
    std::vector<std::vector<std::pair<int64_t, int64_t>>> order((size_t)ncolors);   // (key, vid)
    std::vector<uint8_t> g_ne(nvar, 0), g_mo(nvar, 0);      // entries / widest entry of a general lane
    parallel_for(nvar, [&](int64_t vb0, int64_t vb1, int) {
        std::vector<uint32_t> w;
        for (int64_t v = vb0; v < vb1; v++) {
            if (c.color[v] < 0 || fast[v] != 2) continue;
            general_words(v, &w);
            int64_t ne = 0, mo = 0;
            for (size_t j = 0; j < w.size(); j += 2 + ((w[j + 1] >> 4) & 7u)) {
                ne++;
                mo = std::max<int64_t>(mo, (w[j + 1] >> 4) & 7u);
            }
            g_ne[v] = (uint8_t)ne; g_mo[v] = (uint8_t)mo;
        }
    });
    lap("positions: lane sizes");
    // entry-parallel groups (nsk_compile.h ep_desc) serve a colour whose general variables all
    // have entries of at most 3 other members and at most 16 entries (ordinal: 5 bits, LDS slots).  (With the default
    // gen_max_entries of 16 the second half never decides: a variable of 17 entries is no general-tile variable at all,
    // it takes a wave of its own and its colour keeps its groups; only NSK_GEN_MAX_ENTRIES above 16 lets it count.)
    c.phase_ep.assign((size_t)ncolors, 0);
    c.phase_ep_emax.assign((size_t)ncolors, 0);
    if (!knobs.no_ep && nw < ((int64_t)1 << 27)) {
        for (int32_t k = 0; k < ncolors; k++) c.phase_ep[k] = ngt_of[k] > 0 ? 1 : 0;
        for (int64_t v = 0; v < nvar; v++) {
            if (c.color[v] < 0 || fast[v] != 2) continue;
            if (g_mo[v] > 3 || g_ne[v] > 16) c.phase_ep[c.color[v]] = 0;
            c.phase_ep_emax[c.color[v]] = std::max<int32_t>(c.phase_ep_emax[c.color[v]], g_ne[v]);
        }
    }
    // key: categorical lanes first (their tiles form a launch of their own), then blocks
    // of gen_block consecutive ids (sigma of SELL-C-sigma: each XCD walks a contiguous
    // run of tiles, so its L2 then sees one slice of the value array instead of all of
    // it), largest layouts first inside a block.  Entry-parallel groups carry no padding to the
    // widest lane, so their colours are cut into small id blocks -- a group's member values then
    // share cache lines --, with the variables of more than 8 entries (two LDS passes per group)
    // in front of the others.  One colour per thread: collect its variables, sort them.
    auto collect = [&](int32_t k) {
        std::vector<std::pair<int64_t, int64_t>> &ord = order[(size_t)k];
        ord.reserve((size_t)ngt_of[k]);
        const bool epk = c.phase_ep[k] != 0;
        const int64_t gb = epk ? ep_block : gen_block;
        for (int64_t v = 0; v < nvar; v++) {
            if (c.color[v] != k || fast[v] != 2) continue;
            const int64_t ne = g_ne[v], mo = g_mo[v];
            const int64_t catv = c.v_card[v] > 2 ? 0 : 1;
            const int64_t small = (epk && ne <= 8) ? 1 : 0;
            ord.push_back({(small << 51) | (catv << 50) | ((v / gb) << 20) | (0xFFFFF - (ne * 8 + mo)), v});
        }
        std::sort(ord.begin(), ord.end());
    };
    {
        std::vector<std::thread> sorters;             // (few colours only)
        for (int32_t k = 0; k < ncolors; k++) {
            if (ncolors <= 64 && compile_threads() > 1) sorters.emplace_back([&, k] { collect(k); });
            else collect(k);
        }
        for (auto &t : sorters) t.join();
    }
    lap("positions: lane order");

    // ---- positions.  Run padding (ClassPad): inside an exact class -- id order -- the members of consecutive variables
    // are, on regular graphs, consecutive positions of another class (a grid row's neighbours are the rows above,
    // below and beside it): an AFFINE RUN.  The table kernels take such positions four to a lane (nsk_compile.h
    // seg_wide) when a run starts on a multiple of 256, so the positions are laid out twice when that pays: the
    // first layout finds the runs (find_run_padding), the second starts every long run on a quad boundary, with
    // empty positions (p_vid = -1) in front.
    struct ClassAt { int32_t k; uint64_t key; int64_t start, count; };
    struct Cursor { int64_t next, rank; size_t bi; const ClassPad *pad; };
    std::vector<std::unordered_map<uint64_t, ClassPad>> pads((size_t)ncolors);
    std::vector<ClassAt> exact_at;
    auto lay = [&]() -> int {
        std::vector<int64_t> next_gen((size_t)ncolors, 0), tail_at((size_t)ncolors, 0), gt_at((size_t)ncolors, 0);
        std::vector<std::vector<int64_t>> gen_bin_start;
        std::vector<std::unordered_map<uint64_t, Cursor>> start((size_t)ncolors);
        std::vector<std::map<uint64_t, int64_t>> start2((size_t)ncolors), start3((size_t)ncolors);
        exact_at.clear();
        c.nsampled = 0;
        int64_t pos = 0;
        for (int32_t k = 0; k < ncolors; k++) {
            pos = (pos + 127) / 128 * 128;      // tiles sit on multiples of 64, tile pairs on multiples of
            if (!pads[k].empty()) pos = (pos + 255) / 256 * 256;
            c.phase_start[k] = pos;             // 128: a lane's position & 63 is its lane (generator ids)
            int64_t nbig = 0;
            for (int level = 0; level < 3; level++) {
                if (level == 1) shape_at[k] = pos;
                ClassMap &cm = level == 0 ? classes[k] : level == 1 ? shapes[k] : pshapes[k];
                std::vector<std::pair<int64_t, uint64_t>> big;        // (first vid, key)
                const int64_t need = level == 0 ? min_class[k] : 64;
                for (auto &kv : cm)
                    if (kv.second.first >= need) { big.push_back({kv.second.second, kv.first}); nbig += kv.second.first; }
                std::sort(big.begin(), big.end());
                for (auto &bc : big) {
                    const int64_t count = cm[bc.second].first;
                    if (level == 0) {
                        const auto pit = pads[k].find(bc.second);
                        const ClassPad *pd = pit == pads[k].end() ? nullptr : &pit->second;
                        if (pd) pos = (pos + 255) / 256 * 256;          // a padded class owns whole quads
                        Cursor cu{pos, 0, 0, pd};
                        if (pd && !pd->at.empty() && pd->at[0].first == 0) { cu.next += pd->at[0].second; cu.bi = 1; }
                        start[k][bc.second] = cu;
                        exact_at.push_back(ClassAt{k, bc.second, pos, count});
                        pos += count + (pd ? pd->total : 0);
                        if (pd) pos = (pos + 255) / 256 * 256;
                    } else {
                        (level == 1 ? start2[k] : start3[k])[bc.second] = pos;
                        pos += count;
                    }
                    pos = c.phase_start[k] + (pos - c.phase_start[k] + 63) / 64 * 64;
                }
            }
            tail_at[k] = pos;
            shape_end[k] = pos;
            pos += nfast_of[k] - nbig;
            pos = c.phase_start[k] + (pos - c.phase_start[k] + 63) / 64 * 64;   // tiles own all 64 positions
            gt_at[k] = pos;                                                     // general tiles
            c.phase_gen_tile[k] = (pos - c.phase_start[k]) / 64;
            pos += ngt_of[k];
            pos = c.phase_start[k] + (pos - c.phase_start[k] + 63) / 64 * 64;
            c.phase_fast_end[k] = pos;
            next_gen[k] = pos;
            pos += ngen_of[k];
            c.phase_end[k] = pos;               // (the next colour starts at the next multiple of 128)
        }
        c.phase_start[ncolors] = pos;
        c.npos = pos;
        if (c.npos >= LIM - 1) { err = "too many positions"; return NSK_E_RANGE; }
        c.p_vid.assign(c.npos, -1); c.p_info.assign(c.npos, 0); c.p_slot.assign(c.npos, 0);
        c.p_cnt.assign(c.npos, 0); c.p_init.assign(c.npos, 0);
        gen_bin_start.assign((size_t)ncolors, std::vector<int64_t>(42, 0));
        c.phase_heavy_end.assign((size_t)ncolors, 0);
        for (int32_t k = 0; k < ncolors; k++) {
            gen_bin_start[k][0] = next_gen[k];
            for (int b = 0; b < 41; b++) gen_bin_start[k][b + 1] = gen_bin_start[k][b] + bin_count[k][b + 1];
            c.phase_heavy_end[k] = gen_bin_start[k][1];              // bin 0 = the hubs
        }
        for (int32_t k = 0; k < ncolors; k++) {
            for (auto &o : order[k]) {
                const int64_t p = gt_at[k]++;
                c.p_vid[p] = (int32_t)o.second;
                c.v_pos[o.second] = (int32_t)p;
                c.nsampled++;
            }
        }
        for (int64_t v = 0; v < nvar; v++) {
            const int32_t k = c.color[v];
            if (k < 0 || fast[v] == 2) continue;
            int64_t p;
            if (!fast[v]) p = gen_bin_start[k][work_bin[v]]++;
            else {
                auto it = start[k].find(sig[v]);
                if (it != start[k].end()) {
                    Cursor &cu = it->second;
                    p = cu.next++;
                    cu.rank++;
                    if (cu.pad && cu.bi < cu.pad->at.size() && cu.pad->at[cu.bi].first == cu.rank) cu.next += cu.pad->at[cu.bi++].second;
                } else {
                    auto it2 = shp[v] ? start2[k].find(shp[v]) : start2[k].end();
                    if (it2 != start2[k].end()) p = it2->second++;
                    else {
                        auto it3 = pshp[v] ? start3[k].find(pshp[v]) : start3[k].end();
                        p = (it3 != start3[k].end()) ? it3->second++ : tail_at[k]++;
                    }
                }
            }
            c.p_vid[p] = (int32_t)v;
            c.v_pos[v] = (int32_t)p;
            c.nsampled++;
        }
        return NSK_OK;
    };
    if (int rc = lay()) return rc;
    lap("positions: arrays");
    if (c.vbytes == 1 && !knobs.no_wide && !knobs.no_run_pad && c.nsampled >= knobs.wide_min) {
        // the runs of the big exact classes in the layout just made
        bool any = false;
        for (const ClassAt &ca : exact_at) {
            if (ca.count < 1024) continue;
            ClassPad pd;
            if (find_run_padding(*this, ca.start, ca.count, pd)) { pads[(size_t)ca.k][ca.key] = std::move(pd); any = true; }
        }
        lap("positions: runs");
        if (any) {
            if (int rc = lay()) return rc;
            lap("positions: padded arrays");
        }
    }
    return NSK_OK;
}

// Internal ids: a positioned variable's id is its position; the others (ghosts, isEvidence
// == 4 -- read but never sampled here) follow.  Every variable id stored for the device from
// here on is internal (m_rec, tiles, gstream, v_card): values are kept in this order, so the
// stores of a colour class are contiguous and its gathers run through the other classes' ranges
// in step with the lanes (DESIGN.md "internal numbering").
int CompileCtx::assign_internal_ids() {
    const int64_t nvar = c.nvar, nedge = c.nedge;
    const int64_t LIM = (int64_t)1 << 31;
    c.iid.assign(nvar, -1);
    {
        // (the ghosts the sampled variables READ come first among the others, in id order: the receive list of
        // a peer-to-peer exchange -- all of them, ascending -- is then one contiguous run of internal ids, which
        // lets a shard's kernels read ghost values straight from the exchange buffer, nsk_exchange.hip)
        int64_t next = c.npos;
        for (int32_t v : c.ghost_needs) if (c.v_pos[v] < 0) c.iid[v] = (int32_t)next++;
        for (int64_t v = 0; v < nvar; v++)
            if (c.v_pos[v] >= 0) c.iid[v] = c.v_pos[v];
            else if (c.iid[v] < 0) c.iid[v] = (int32_t)next++;
        // one more id that belongs to no variable and always holds 0: where the ignored member slots and the
        // padding of uniform tiles point.  The draw-table kernels take a member's value as its bit (values
        // are regular, members binary), so such a slot must not read a categorical variable's value --
        // position 0 may hold one (a 2 there set the NEXT slot's bit: wrong table entry, wrong gradient).
        c.zero_id = next++;
        c.nid = next;
        if (c.nid >= LIM - 1) { err = "too many internal ids"; return NSK_E_RANGE; }
        parallel_for(nedge, [&](int64_t lb0, int64_t lb1, int) {
            for (int64_t l = lb0; l < lb1; l++)
                if (c.m_rec[2 * l] >= 0) c.m_rec[2 * l] = c.iid[c.m_rec[2 * l]];
        });
        std::vector<int32_t> card_i((size_t)c.nid, 2);
        for (int64_t v = 0; v < nvar; v++) card_i[c.iid[v]] = c.v_card[v];
        c.v_card_i.swap(card_i);
    }
    return NSK_OK;
}

}  // namespace nsk
