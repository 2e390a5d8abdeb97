// nsk_seg_plan.h -- the segment launches of a sweep: which segments share a launch, how its tiles are numbered, which
// kernel takes it and on what grid.  Like nsk_class_plan.h, host only and pure: no HIP type, no environment variable,
// nothing of the handle.  The sweep drivers (nsk_gibbs.hip, nsk_learn.hip) fill a SegPlanOpts once per call -- the
// diagnostic switches and the addresses are read there --, keep the plans while the options stay the same, and launch
// from the plans' tables and grids (tests/test_seg_plan_cpu.py pins the plans down without a GPU).
// Invariant: every tile of every sampled segment lies in exactly one entry of exactly one launch of its class; the
// virtual tile ranges of a launch's entries are disjoint and add up to SegTable.ntiles; in a wide launch with a listed
// rest, the whole wide quads and the listed quads together are all its quads, each once.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nsk_compile.h"
#include "nsk_seg_table.h"

namespace nsk {

// The kernels' own constants (NSK_LEARN_TPW of nsk_learn.hip, NSK_LEARN_SEG_BLOCKS and NSK_SERVICE_BLOCKS of the kernel
// headers, which this one cannot include); the drivers assert that the copies agree.
constexpr int SEG_LEARN_TPW = 2, SEG_LEARN_SEG_BLOCKS = 2048, SEG_SERVICE_BLOCKS = 8;
#ifndef NSK_TABW_PER_CU
#define NSK_TABW_PER_CU 6           // workgroups per CU of the wide-quad inference grid (no kernel reads it)
#endif
// On the 4M grid the tile-by-tile learning kernel wins (24.3 against 27.5 us per sweep): wide learning launches from
// this many quads on (NSK_WIDE_LEARN_MIN)
constexpr int NSK_WIDE_LEARN_MIN_QUADS = 12000;

// What the plans read besides the layout.  A driver fills the common group and its own; two that differ give other
// plans (operator==: the drivers' cache key).
struct SegPlanOpts {
    bool sample_evidence = false;   // evidence segments are sampled too (inference.py:24)
    bool use_tab = true;            // the values lie in their domains: the draw tables are usable
    bool byte_values = true;        // int8 values (only they have wide quads in learning)
    bool offsets_fit = true;        // cnt_pos, seg_wide and ztab lie whole 256-byte units from val that fit 32 bits (NSK_TABW_HOT)
    // inference
    bool fused = false;             // the boundary exchange rides in the table launches: runs of border / interior tiles
    const std::vector<int32_t> *border_tiles = nullptr;     // sorted (NskP2PSetup::border_tiles); null: none
    bool no_wide_kernel = false;    // NSK_NO_WIDE_KERNEL
    bool no_tabw_rest = false;      // NSK_NO_TABW_REST: no rest quad listed, the waves sample them in line (learning too)
    int tab_grid_cap = 0, tabw_grid_cap = 0;                // NSK_TAB_GRID_CAP, NSK_TABW_GRID_CAP (seg_cap_rounds), 0: none
    // learning
    int nweight = 0;
    bool smallw = false;            // gradients accumulate in LDS
    int wide_learn_min_quads = NSK_WIDE_LEARN_MIN_QUADS;    // NSK_WIDE_LEARN_MIN
    bool no_wide_learn = false;     // NSK_NO_WIDE_LEARN
    int learn_grid_cap = 0, learn_tabw_grid_cap = 0;        // NSK_LEARN_GRID_CAP (seg_cap_blocks), NSK_LEARN_TABW_GRID_CAP (seg_cap_rounds)
    bool operator==(const SegPlanOpts &b) const {
        return sample_evidence == b.sample_evidence && use_tab == b.use_tab && byte_values == b.byte_values && offsets_fit == b.offsets_fit &&
               fused == b.fused && border_tiles == b.border_tiles && no_wide_kernel == b.no_wide_kernel && no_tabw_rest == b.no_tabw_rest &&
               tab_grid_cap == b.tab_grid_cap && tabw_grid_cap == b.tabw_grid_cap && nweight == b.nweight && smallw == b.smallw &&
               wide_learn_min_quads == b.wide_learn_min_quads && no_wide_learn == b.no_wide_learn &&
               learn_grid_cap == b.learn_grid_cap && learn_tabw_grid_cap == b.learn_tabw_grid_cap;
    }
};
// a diagnostic grid cap as the drivers pass it in: whole rounds of XCDs, at least one / blocks, at least one; unset: 0
static inline int seg_cap_rounds(const char *env) { return env ? std::max(8, std::abs(atoi(env)) & ~7) : 0; }
static inline int seg_cap_blocks(const char *env) { return env ? std::max(1, atoi(env)) : 0; }

// ---- grids ----
// Grid of a table-driven inference segment launch (k_gibbs_seg_tab) over `vtiles` virtual tiles (a multiple
// of 4): one wave per tile PAIR while that fits the resident grid, else the resident grid -- 6 blocks per CU,
// whole rounds of XCDs -- whose waves loop over QUADS (the kernel deals whole rounds of quads, then pairs).
// Six, not the seven the compiler's occupancy and the occupancy API report: the kernel holds 106 scalar
// registers and the hardware admits min(8, 800 / (ceil(sgpr / 16) * 16 + 16)) blocks of 256 threads per CU
// (MI355X_MICROARCH.md); capping the registers for a seventh or eighth block was slower.  A grid beyond the resident one runs a tail round as long as
// the first: per 10M-grid class 1024 blocks 15.2 us, 1280 14.3, 1536 12.7, 1632 16.2, 1792 14.1, 2048 14.3
// (NSK_TAB_GRID_CAP); the 1M grid (1954 blocks of pairs) is indifferent (4.2 us).
static inline int nsk_tab_grid(int vtiles, int cap) {
    const int npairs = vtiles / 2;
    const int need = std::max(8, 8 * ((((npairs + 3) / 4) + 7) / 8));
    return std::min(cap ? cap : (need <= 2048 ? 2048 : 1536), need);   // (a launch that needs fewer blocks than 2048 runs in pairs: one trip per wave)
}
// Grid of a wide-quad table launch (k_gibbs_seg_tabw) over `vtiles` virtual tiles: a wave per quad while that fits the
// resident grid (NSK_TABW_PER_CU blocks per CU), else the resident grid, whole rounds of XCDs
static inline int nsk_tabw_grid(int vtiles, int cap) {
    const int nquads = vtiles / 4, ntrips = nquads + 8;                     // (+ 8: every XCD's share rounds up)
    const int need = std::max(8, 8 * ((((ntrips + 3) / 4) + 7) / 8));
    return std::min(cap ? cap : 256 * NSK_TABW_PER_CU, need);
}
// a workgroup in front of a wide launch's grid for each listed rest quad, whole rounds of XCDs
static inline int nsk_tabw_front_blocks(uint32_t nrest) { return (int)((nrest + 7u) & ~7u); }
// Grid of a table-driven learning segment launch: resident -- the waves loop over their XCD's trips
// with the next trip's loads in flight (k_learn_seg_tab) -- and smaller when a block's flush of its
// LDS sums (a few atomics per weight) would rival its tile traffic
static inline int nsk_learn_tab_grid(int ntiles, int nweight, bool smallw, int cap) {
    const int blocks = (ntiles + 7) / 8;                            // 4 waves x 2 tiles
    const int trips = smallw ? std::max(1, (nweight * 16 * 16 + 14847) / 14848) : 1;
    // Six blocks per CU.  The kernel holds 7 waves per SIMD (112 scalar registers), so 2048 blocks are
    // not all resident, and whole blocks per CU beat fractions (measured on the 10M grid, per class with
    // the update launch: 1024 blocks 31.2 us, 1280 30.1, 1408 31.1, 1536 29.6, 1664 31.2, 1792 32.2,
    // 1920 32.5, 2048 31.4, 3072 31.3, 4096 31.7; the 1M grid is indifferent: 14.1-14.3)
    // (SMALLW launches carry the service blocks in front, k_learn_seg_tab: they count towards the six per CU)
    const int limit = cap ? cap : 1536 - (smallw ? SEG_SERVICE_BLOCKS : 0);
    return 8 * ((std::max(1, std::min(limit, (blocks + trips - 1) / trips)) + 7) / 8);     // whole rounds of XCDs
}
// Grid of a wide-quad learning launch (k_learn_seg_tabw) over `vtiles` virtual tiles, whole rounds of XCDs (the service
// and front blocks come on top).  One MI355X, us per learning sweep: 10M grid 45.6 / 45.6 / 40.3 / 42.6 / 41.8 / 43.7 /
// 43.3 at 512 / 640 / 768 / 896 / 1024 / 1152 / 1280 blocks (45.5 tile by tile; 41.0 at 1024 and 43.0 at 1536 in another
// pass); 40M grid 120.8 / 117.7 / 117.4 / 111.6 at 768 / 1024 / 1536 / 2048 (146.6 tile by tile).  (While the waves whose
// turn they were sampled the launch's few quads that are not wide in line, these figures jumped by a quarter from one
// grid size to the next -- whichever waves drew those quads ended the launch.)
static inline int nsk_learn_tabw_grid(int vtiles, int cap) {
    const int nquads = vtiles / 4 + 8;
    const int need = std::max(8, 8 * ((((nquads + 3) / 4) + 7) / 8));
    return std::min(cap ? cap : (nquads >= 40000 ? 2048 : 1024), need);
}
// grid of a learning segment launch over `ntiles` real tiles that is not wide: the table kernel's, or a wave per tile
static inline int nsk_learn_seg_grid(int ntiles, bool table, const SegPlanOpts &o) {
    if (table) return nsk_learn_tab_grid(ntiles, o.nweight, o.smallw, o.learn_grid_cap);
    return std::min(SEG_LEARN_SEG_BLOCKS, (ntiles + 3) / 4);
}

// ---- the pieces both sweeps share ----
// Table launches number their tiles virtually: a segment starts on a quad boundary (positions 256 m), with up to three
// dead tiles in front (lead), and ends on one
static inline int seg_lead(int64_t pos0) { return (int)((pos0 / 64) & 3); }
static inline int seg_quad_tiles(int nt, int lead) { return (nt + lead + 3) & ~3; }

// entry of `nt` tiles from position pos0 on, at launch tile `tile_start`
static inline void seg_entry(SegEntry &en, int tile_start, int nt, int lead, int64_t pos0, uint32_t adj_off, uint32_t prog,
                             uint32_t zoff, uint32_t zmask_ev, uint32_t aff_off, uint32_t push_off, uint32_t wide_off) {
    en.tile_start = tile_start;
    en.ntiles_lead = (uint32_t)nt | ((uint32_t)lead << 30);
    en.pos0 = (int)pos0; en.adj_off = adj_off; en.prog = prog; en.zoff = zoff; en.zmask_ev = zmask_ev;
    en.aff_off = aff_off; en.push_off = push_off; en.wide_off = wide_off;
}

// The wide quads (nsk_compile.h seg_wide: first dword not 0xFFFFFFFF) among the quads that `nt` tiles from pos0 on
// touch, and those of them the tiles hold whole; wide_off = the descriptor of the quad of pos0
struct WideQuads { int touched = 0, whole = 0; };
static inline WideQuads seg_wide_quads(const Compiled &c, uint32_t wide_off, int nch, int64_t pos0, int nt) {
    WideQuads w;
    const int64_t end = pos0 + 64 * (int64_t)nt;
    for (int64_t P = pos0 & ~(int64_t)255; P < end; P += 256)
        if (c.seg_wide[(size_t)wide_off + (size_t)((P >> 8) - (pos0 >> 8)) * NSK_WIDE_STRIDE(nch)] != 0xFFFFFFFFu) {
            w.touched++;
            if (P >= pos0 && P + 256 <= end) w.whole++;
        }
    return w;
}

// The quads of a wide launch that are not wide ones (TabwCold.rest / TabwRest; the kernels' own tests of a quad, mirrored):
// each gets a workgroup in front of the grid.  More than NSK_TABW_REST_MAX of them: none listed, the waves sample them in
// line (`listed` false, NSK_NO_TABW_REST: likewise).  Bit 31: the quad is flagged wide all the same (it draws from the wide scheme).
static inline uint32_t seg_rest_list(const Compiled &c, const SegTable &tab, int nch, bool listed, uint32_t *out) {
    const int ST = NSK_WIDE_STRIDE(nch);
    std::vector<uint32_t> rest;
    for (int i = 0; i < tab.n; i++) {
        const SegEntry &en = tab.e[i];
        const int tend = i + 1 < NSK_SEG_MAX ? tab.e[i + 1].tile_start : tab.ntiles;
        const int lead = (int)(en.ntiles_lead >> 30), nt = (int)(en.ntiles_lead & 0x3FFFFFFFu);
        const int qs = en.tile_start >> 2, qin_lo = qs + (lead ? 1 : 0);
        const uint32_t qin_n = (uint32_t)(qs + ((lead + nt) >> 2) - qin_lo);
        const bool hasw = en.wide_off != NSK_NO_STREAM;
        for (int Q = qs; Q < (tend >> 2); Q++) {
            const bool flagged = hasw && c.seg_wide[(size_t)en.wide_off + (size_t)(Q - qs) * ST] != 0xFFFFFFFFu;
            if (flagged && (uint32_t)(Q - qin_lo) < qin_n) continue;     // a wide quad
            rest.push_back((uint32_t)Q | (flagged ? 0x80000000u : 0u));
        }
    }
    if (rest.size() > NSK_TABW_REST_MAX || !listed) return 0;
    std::copy(rest.begin(), rest.end(), out);
    return (uint32_t)rest.size();
}

// ---- inference ----
// One prepared segment launch: the table, the rest quads of a wide launch, and its grids
struct SegLaunchPlan {
    int kind = 0, nch = 1;          // kind 8: a table launch (segments with draw tables, any function); else k_gibbs_seg<kind>
    SegTable tab = {};
    uint32_t nrest = 0, rest[NSK_TABW_REST_MAX] = {};       // wide launches: the quads that are not wide (TabwCold.rest)
    int grid = 0;                   // kind 8: the tile-pair grid (nsk_tab_grid); else the segment kernel's, a wave per tile
    int wide_grid = 0, front = 0;   // tab.wide: the wide-quad grid (nsk_tabw_grid) and the blocks for the rest quads in front of it
};
struct SegPlans {
    std::vector<std::vector<SegLaunchPlan>> by_class;
    int first_phase = -1;           // the first class with sampled segments -- with border tiles, when the exchange is fused
    uint32_t border_total = 0;      // border tiles one sweep of these plans samples
    bool border_all = true;         // ... and that is every border tile
    bool all_tab = true, all_wide = true;       // every launch is a table launch; ... a wide one
};

// The segment launches of every colour: segments batched by (kind, chunks) into tables of <= NSK_SEG_MAX; kind 8 =
// segments with draw tables.  With a fused exchange the table segments are split into runs of border tiles
// (SegEntry.push_off = their first row in the push map: a tile's rank among the border tiles) and runs of interior tiles.
static inline SegPlans plan_segments(const Compiled &c, const SegPlanOpts &o) {
    static const std::vector<int32_t> none;
    const std::vector<int32_t> &bt = o.border_tiles ? *o.border_tiles : none;
    const size_t nphase = c.phase_start.size() - 1;
    const auto sampled = [&](const Compiled::Segment &sg) { return sg.ev == 0 || o.sample_evidence; };      // inference.py:24
    SegPlans r;
    r.by_class.assign(nphase, std::vector<SegLaunchPlan>());
    struct Run { const Compiled::Segment *sg; int t0, nt; uint32_t push_off; };
    for (const Compiled::Segment &sg : c.segments) {
        if (sampled(sg)) { if (r.first_phase < 0 || sg.phase < r.first_phase) r.first_phase = sg.phase; }
        else if (o.fused) {         // border tiles of segments this call does not sample: the fused exchange cannot run
            const int32_t f = (int32_t)(sg.pos0 / 64);
            const auto it = std::lower_bound(bt.begin(), bt.end(), f);
            if (it != bt.end() && *it < f + sg.ntiles) r.border_all = false;
        }
    }
    for (size_t ph = 0; ph < nphase; ph++)
        for (int kind = 0; kind <= 8; kind++) {
            if (kind == 1 || (kind > 4 && kind < 8)) continue;   // IMPLY_NATURAL shares the AND step (3)
            for (int nch = 1; nch <= 2; nch++) {
                SegLaunchPlan pl;
                SegTable &tab = pl.tab;
                auto flush = [&]() {
                    if (tab.n == 0) return;
                    for (int i = tab.n; i < NSK_SEG_MAX; i++) tab.e[i].tile_start = tab.ntiles;
                    // the wide-quad kernel takes the launch when at least half of its quads are wide ones (the others:
                    // its front workgroups, or tile by tile in line)
                    tab.wide = (kind >= 8 && 8 * tab.wide >= tab.ntiles && tab.ntiles < (1 << 28) && o.offsets_fit && !o.no_wide_kernel) ? 1 : 0;
                    pl.kind = kind; pl.nch = nch;
                    if (kind >= 8) pl.grid = nsk_tab_grid(tab.ntiles, o.tab_grid_cap);
                    else pl.grid = 8 * (((tab.ntiles + 3) / 4 + 7) / 8);
                    if (tab.wide) {
                        pl.nrest = seg_rest_list(c, tab, nch, !o.no_tabw_rest, pl.rest);
                        pl.wide_grid = nsk_tabw_grid(tab.ntiles, o.tabw_grid_cap);
                        pl.front = nsk_tabw_front_blocks(pl.nrest);
                    }
                    r.by_class[ph].push_back(pl);
                    pl = SegLaunchPlan();
                };
                std::vector<Run> mine;
                for (const Compiled::Segment &sg : c.segments) {
                    if (sg.phase != (int)ph) continue;
                    const int k3 = (o.use_tab && sg.ztab >= 0) ? 8 : sg.kind == 1 ? 3 : (int)sg.kind;
                    if (k3 != kind || (sg.nslots > 4 ? 2 : 1) != nch || !sampled(sg)) continue;
                    if (!o.fused || kind < 8) { mine.push_back(Run{&sg, 0, sg.ntiles, NSK_NO_STREAM}); continue; }
                    // runs of border / interior tiles
                    const int32_t f = (int32_t)(sg.pos0 / 64);
                    size_t bi = (size_t)(std::lower_bound(bt.begin(), bt.end(), f) - bt.begin());
                    for (int t = 0; t < sg.ntiles;) {
                        const bool isb = bi < bt.size() && bt[bi] == f + t;
                        int e = t + 1;
                        if (isb) { while (e < sg.ntiles && bi + (size_t)(e - t) < bt.size() && bt[bi + (size_t)(e - t)] == f + e) e++; }
                        else e = (bi < bt.size() && bt[bi] < f + sg.ntiles) ? bt[bi] - f : sg.ntiles;
                        mine.push_back(Run{&sg, t, e - t, isb ? (uint32_t)bi : NSK_NO_STREAM});
                        if (isb) { bi += (size_t)(e - t); r.border_total += (uint32_t)(e - t); }
                        t = e;
                    }
                }
                // Largest first: the kernels find a tile's segment with a scan whose first probe is the table's first
                // entry -- but, for a shard that exchanges inside its launches, the border runs in front: their
                // chain (flag, system-coherent ghost loads, pushes, acknowledgement, counter) is twice a trip long and
                // overlaps the interior trips when it starts first; behind them it was a tail of every launch (a
                // border wave that waits for a peer holds one of 6144 wave slots, nothing else)
                std::stable_sort(mine.begin(), mine.end(), [](const Run &a, const Run &b) {
                    const bool ba = a.push_off != NSK_NO_STREAM, bb = b.push_off != NSK_NO_STREAM;
                    if (ba != bb) return ba;
                    return a.nt > b.nt; });
                for (const Run &rn : mine) {
                    const Compiled::Segment &sg = *rn.sg;
                    const int64_t pos0 = sg.pos0 + 64 * (int64_t)rn.t0;
                    const int lead = kind >= 8 ? seg_lead(pos0) : 0;
                    // quad descriptors from the quad of the run's first position on; NCH of the descriptors = the
                    // segment's own chunk count = this launch's.  (bit 16 of zmask_ev: the positions of a segment with a
                    // draw table draw from the quad scheme whichever kernel samples them, nsk_device.h quad_block)
                    uint32_t wide_off = (sg.ztab >= 0 && sg.wide >= 0)
                        ? (uint32_t)(sg.wide + ((pos0 >> 8) - (sg.pos0 >> 8)) * NSK_WIDE_STRIDE(nch)) : NSK_NO_STREAM;
                    if (wide_off != NSK_NO_STREAM) {      // the wide quads the run touches; those it holds whole (SegTable.wide, flush)
                        const WideQuads w = seg_wide_quads(c, wide_off, nch, pos0, rn.nt);
                        if (kind >= 8) tab.wide += w.whole;
                        if (!w.touched) wide_off = NSK_NO_STREAM;        // (none: the kernels need not look)
                    }
                    seg_entry(tab.e[tab.n], tab.ntiles, rn.nt, lead, pos0, sg.adj_off + (uint32_t)rn.t0 * 64u * (uint32_t)nch, sg.prog,
                              sg.ztab >= 0 ? (uint32_t)sg.ztab : 0u,
                              ((1u << sg.nslots) - 1u) | (((uint32_t)sg.ev & 0xFFu) << 8) | (sg.ztab >= 0 ? 1u << 16 : 0u),
                              (kind >= 8 && sg.aff >= 0) ? (uint32_t)sg.aff + (uint32_t)rn.t0 * (uint32_t)nch : NSK_NO_STREAM,
                              rn.push_off, wide_off);
                    tab.ntiles += kind >= 8 ? seg_quad_tiles(rn.nt, lead) : rn.nt;
                    if (++tab.n == NSK_SEG_MAX) flush();
                }
                flush();
            }
        }
    // The border waves of the sweep's first class THAT HAS BORDER TILES wait for the peers' flags of the previous
    // exchange (later classes find them raised: the stream is in order).  Not simply the first class with sampled
    // segments: a cut whose boundary variables all have the other colour (a chain, a bipartite cut) has no border tile
    // there, and then nothing in the sweep would wait -- ghosts read before they arrived, pushes over a block a peer
    // still reads.
    if (o.fused) {
        int first_border = -1;
        for (size_t ph = 0; ph < nphase && first_border < 0; ph++)
            for (const SegLaunchPlan &pl : r.by_class[ph])
                for (int i = 0; i < pl.tab.n && first_border < 0; i++)
                    if (pl.tab.e[i].push_off != NSK_NO_STREAM) first_border = (int)ph;
        if (first_border >= 0) r.first_phase = first_border;
    }
    r.border_all = r.border_all && r.border_total == (uint32_t)bt.size();
    for (const auto &v : r.by_class)
        for (const SegLaunchPlan &pl : v) {
            r.all_tab = r.all_tab && pl.kind >= 8;
            r.all_wide = r.all_wide && pl.kind >= 8 && pl.tab.wide;
        }
    return r;
}

// ---- learning ----
// One prepared learning segment launch (Compiled::learn_seg): the segment table -- in whole quads, with the quads that
// are not wide ones, when the wide kernel takes the launch (wide); tile by tile otherwise -- and its grid, the wide
// launch's front blocks included, the service blocks of a SMALLW table launch not
struct LearnSegPlan { bool wide = false; SegTable tab = {}; uint32_t nrest = 0, rest[NSK_TABW_REST_MAX] = {}; int grid = 0; };

static inline LearnSegPlan plan_learn_segment(const Compiled &c, const Compiled::SegLaunch &sl, const SegPlanOpts &o) {
    LearnSegPlan p;
    SegTable &tab = p.tab;
    const bool use_tab = sl.tab && o.use_tab;
    const auto nt = [&](int i) { return i < sl.n ? sl.tile_start[i + 1] - sl.tile_start[i] : 0; };
    const auto zmask_ev = [&](int i) { return (sl.zmask[i] & 0xFFu) | (((uint32_t)sl.ev[i] & 0xFFu) << 8); };
    // (mostly) wide quads: the wide learning kernel, its tiles numbered in whole quads like the inference launches
    if (use_tab && o.byte_values) {
        memset(&tab, 0, sizeof(tab));
        tab.n = sl.n;
        int nwide = 0;
        for (int i = 0; i < NSK_SEG_MAX; i++) {
            if (i >= sl.n) { tab.e[i].tile_start = tab.ntiles; continue; }
            const int64_t pos0 = sl.pos0[i];
            const int lead = seg_lead(pos0);
            const uint32_t wide_off = sl.wide[i] >= 0 ? (uint32_t)sl.wide[i] : NSK_NO_STREAM;     // (the descriptors start at the quad of pos0)
            seg_entry(tab.e[i], tab.ntiles, nt(i), lead, pos0, sl.adj_off[i], sl.prog[i], sl.zoff[i], zmask_ev(i), sl.aff[i], NSK_NO_STREAM, wide_off);
            if (wide_off != NSK_NO_STREAM) nwide += seg_wide_quads(c, wide_off, sl.nch, pos0, nt(i)).whole;
            tab.ntiles += seg_quad_tiles(nt(i), lead);
        }
        p.wide = 8 * nwide >= tab.ntiles && tab.ntiles > 0 && tab.ntiles / 4 >= o.wide_learn_min_quads && !o.no_wide_learn;
        if (p.wide) {
            p.nrest = seg_rest_list(c, tab, sl.nch, !o.no_tabw_rest, p.rest);
            p.grid = nsk_learn_tabw_grid(tab.ntiles, o.learn_tabw_grid_cap) + nsk_tabw_front_blocks(p.nrest);
            return p;
        }
    }
    // tile by tile; table launches number their tiles virtually: every segment is padded to whole trips
    memset(&tab, 0, sizeof(tab));
    tab.n = sl.n;
    int vt = 0;
    for (int i = 0; i < NSK_SEG_MAX; i++) {
        seg_entry(tab.e[i], use_tab ? vt : sl.tile_start[std::min(i, (int)sl.n)], nt(i), 0, sl.pos0[i], sl.adj_off[i], sl.prog[i], sl.zoff[i],
                  zmask_ev(i), use_tab ? sl.aff[i] : NSK_NO_STREAM, 0u, 0u);       // (implicit adjacency: the table kernels)
        vt += (nt(i) + SEG_LEARN_TPW - 1) / SEG_LEARN_TPW * SEG_LEARN_TPW;
    }
    tab.ntiles = use_tab ? vt : sl.tile_start[sl.n];
    p.grid = nsk_learn_seg_grid(sl.tile_start[sl.n], use_tab, o);      // (from the real tile count)
    return p;
}

}  // namespace nsk
