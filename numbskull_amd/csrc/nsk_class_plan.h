// nsk_class_plan.h -- which launches a colour class gets.  The sweep drivers (nsk_gibbs.hip, nsk_learn.hip) take a
// class's plan and issue its launches; the decisions -- kernel variant, tile range, hub / group / rest blocks, grid,
// stream -- are made here, once per call, from the layout and a handful of options.  Host only and pure: no HIP type, no
// environment variable, nothing of the handle (tests/test_class_plan_cpu.py pins the plans down without a GPU).
// The segment launches of a class -- which segments share one, their tables and grids -- are planned beside this, by the
// same rule: nsk_seg_plan.h.
// Invariant: every hub, general tile, rest tile, generic position (and, in learning, learn-rest and per-lane-header
// tile) of a class is sampled by exactly one launch of its plan, and every grid is the sum of its parts.
#pragma once

#include "nsk_compile.h"

namespace nsk {

// Block size and the caps of the learning kernels' persistent grids: the kernels' own (NSK_BLOCK, NSK_LEARN_*_BLOCKS in
// nsk_kernels_gibbs.h, a device header this one cannot include); the drivers assert that the copies agree.
constexpr int PLAN_BLOCK = 256;
constexpr int PLAN_LEARN_FAST_BLOCKS = 2048, PLAN_LEARN_LIST_BLOCKS = 512, PLAN_LEARN_GEN_BLOCKS = 2048,
              PLAN_LEARN_HEAVY_BLOCKS = 512, PLAN_LEARN_GENERAL_BLOCKS = 2048;

static inline int plan_quarter(int n) { return (n + 3) / 4; }              // blocks of four waves: one wave per item
static inline int plan_rounds(int blocks) { return 8 * ((blocks + 7) / 8); }   // whole rounds of XCDs

// The ranges and counts of one colour class, each computed once.  Positions: [fb, fe) tiles, [fe, he) hubs, [he, e)
// generic lanes.  Tiles are relative to the class's first (wb_base): [gt0, ntiles) general, from gtb on all-binary.
struct ClassShape {
    int fb = 0, fe = 0, he = 0, e = 0;
    int wb_base = 0, ntiles = 0;
    int gt0 = 0, gtb = 0;
    int hub0 = 0;                   // first hub descriptor
    int nbh = 0, bh0 = 0;           // hubs with long lists (a block each in an entry-parallel class)
    int ngroups = 0, group0 = 0;    // entry-parallel groups
    int nrest = 0, rest0 = 0;       // tiles outside segments (inference)
    int nlrest = 0, lrest0 = 0;     // tiles outside segment launches (learning)
    int ndyn = 0, dyn0 = 0;         // tiles with per-lane headers
    bool ep = false;                // the general tiles are laid out as groups
};

static inline ClassShape class_shape(const Compiled &c, size_t ph) {
    const auto at = [ph](const std::vector<int64_t> &v) { return ph < v.size() ? (int)v[ph] : 0; };
    const auto span = [ph](const std::vector<int64_t> &base, int &first, int &n) {     // (a layout without the feature: no list)
        const bool has = ph + 1 < base.size();
        first = has ? (int)base[ph] : 0;
        n = has ? (int)(base[ph + 1] - base[ph]) : 0;
    };
    ClassShape s;
    s.fb = at(c.phase_start); s.fe = at(c.phase_fast_end); s.he = at(c.phase_heavy_end); s.e = at(c.phase_end);
    span(c.phase_wb_base, s.wb_base, s.ntiles);
    s.gt0 = at(c.phase_gen_tile); s.gtb = at(c.phase_gen_bin_tile);
    s.hub0 = at(c.phase_hub_base);
    span(c.phase_bighub_base, s.bh0, s.nbh);
    span(c.phase_ep_base, s.group0, s.ngroups);
    span(c.phase_rest_base, s.rest0, s.nrest);
    span(c.phase_learn_rest_base, s.lrest0, s.nlrest);
    span(c.phase_dyn_base, s.dyn0, s.ndyn);
    s.ep = ph < c.phase_ep.size() && c.phase_ep[ph] != 0;
    return s;
}

enum PlanStream { PLAN_MAIN = -1, PLAN_SIDE0 = 0, PLAN_SIDE1 = 1, PLAN_SIDE2 = 2 };   // the handle's stream / nsk_graph::side[i]

// What the decisions read besides the layout.  The drivers read the diagnostic switches and pass the values in.
struct PlanOpts {
    bool overlap = true;            // side streams (off: NSK_NO_OVERLAP, everything on the main stream)
    size_t value_bytes = 0;         // nid * vbytes: the value array
    int ep_per_cu = 0;              // NSK_EP_PER_CU (plan_per_cu), 0: not set
    // learning only
    bool smallw = false;            // gradients accumulate in LDS (at most NSK_SMALLW weights)
    int64_t nweight = 0;
    bool has_kstat = false;         // the layout has structural visit counts (ep_kstat)
    int regularization = 0;
    int seg_tiles = 0;              // tiles of the class's segment launches (Compiled::learn_seg)
    // diagnostic (NSK_CLASS_GRID_CAP): the limit of every persistent grid that walks its items in trips is at most this
    // many blocks (rounded up to whole rounds of XCDs where the launch is), 0: no cap.  The grid is no part of the
    // semantics: small classes then take the later trips that only very large ones take otherwise (tests/class_trips.py)
    int grid_cap = 0;
};
static inline int plan_per_cu(const char *env) { return env ? std::max(1, std::min(32, atoi(env))) : 0; }
static inline int plan_grid_cap(const char *env) { return env ? std::max(1, std::min(1 << 20, atoi(env))) : 0; }
static inline int plan_cap(const PlanOpts &o, int limit) { return o.grid_cap > 0 ? std::min(o.grid_cap, limit) : limit; }

// One launch of a general-tile family -- k_gibbs_general / k_gibbs_ep*, k_learn_general / k_learn_ep*: the general tiles
// [tile0, tile0 + ntiles) of the class; in front of them `hblocks` blocks for its hubs (0: not in this launch), behind
// them `rblocks` for its rest tiles (inference: nrest of them; learning: every block walks them, rblocks are extra).
struct GeneralLaunch {
    bool on = false;
    bool ep = false;                // the entry-parallel kernels, over the class's groups
    int maxc = 8;                   // candidate values a lane holds: 8, or 2 for all-binary tiles
    bool capped = false;            // the register-capped twin (k_gibbs_ep_w5 / k_learn_ep_w4)
    bool behind_generic = false;    // enqueued behind the generic kernel's fork (inference: the all-binary launch)
    int stream = PLAN_MAIN;
    int tile0 = 0, ntiles = 0;
    int nblocks = 0;                // blocks the tiles need, four tiles each (k_gibbs_general's argument; gblocks rounds it up)
    int hblocks = 0, gblocks = 0, rblocks = 0, grid = 0;    // grid = hblocks + gblocks + rblocks
    int nrest = 0;                  // rest tiles this launch samples
};
// a launch over a range or a list, one kernel: n items in `grid` blocks
struct SimpleLaunch { bool on = false; int stream = PLAN_MAIN, n = 0, grid = 0; };

static inline int plan_stream(const PlanOpts &o, PlanStream side) { return o.overlap ? (int)side : (int)PLAN_MAIN; }

// ---- inference: enqueued as general (unless behind_generic), generic, general (behind_generic), segments, fast ----
struct GibbsClassPlan {
    GeneralLaunch general;          // k_gibbs_ep* (general.ep) or k_gibbs_general<maxc>
    SimpleLaunch generic;           // k_gibbs_phase over positions [he, e)
    bool segments = false;          // the class's segment launches (nsk_seg_plan.h plan_segments), main stream
    SimpleLaunch fast;              // k_gibbs_fast over the rest tiles no general launch took
};

static inline GibbsClassPlan plan_gibbs_class(const ClassShape &s, const PlanOpts &o) {
    GibbsClassPlan p;
    GeneralLaunch &L = p.general;
    const bool tiles = s.fe > s.fb;
    const int hubs = plan_quarter(s.he - s.fe);
    if (tiles && s.ep) {
        // entry-parallel groups: hubs, the class's general tiles and its rest tiles in one launch on the main stream.
        // Grid: 7 workgroups per CU, whole rounds of XCDs.  Five of them are resident (90 / 86 vector registers since the
        // wave index is a scalar); the others start as those end, which deals the groups' uneven costs out dynamically --
        // per class on the 5M LR graph (NSK_EP_PER_CU): 3 workgroups per CU 68.4 us, 4 58.6, 5 65.6, 6 66.8, 7 58.3
        L.on = L.ep = true;
        L.maxc = s.gtb > s.gt0 ? 8 : 2;
        // (value array within the L2s: the register-capped twin with a fifth wave per SIMD)
        L.capped = L.maxc == 8 && o.value_bytes <= ((size_t)24 << 20);
        L.tile0 = s.gt0; L.ntiles = s.ntiles - s.gt0;
        L.hblocks = s.nbh + hubs;
        L.gblocks = plan_rounds(std::min(s.ngroups, plan_cap(o, 256 * (o.ep_per_cu ? o.ep_per_cu : 7))));
        L.nrest = s.nrest;
    } else if (tiles && s.gtb > s.gt0) {
        // a class with categorical tiles walks ALL its general tiles in one launch of the 8-candidate kernel, on the
        // main stream, with its hubs and rest tiles: the fork / join events of a side stream cost more (~20 us per
        // class) than the binary tiles lose by running the 8-candidate code
        L.on = true;
        L.tile0 = s.gt0; L.ntiles = s.ntiles - s.gt0;
        L.hblocks = hubs;
        L.nrest = s.nrest;
    } else if (tiles && s.ntiles > s.gtb) {
        // all-binary general tiles only (IMPLY_MLN, mixed tails): the hubs and the rest tiles ride in their launch on
        // the main stream (no side stream, no fork / join events for this class)
        L.on = L.behind_generic = true;
        L.maxc = 2;
        L.tile0 = s.gtb; L.ntiles = s.ntiles - s.gtb;
        L.hblocks = hubs;
        L.nrest = s.nrest;
    } else if (hubs > 0) {
        // no general tiles: the hubs (one wave per variable) alone, beside the class's other launches
        L.on = true;
        L.stream = plan_stream(o, PLAN_SIDE0);
        L.tile0 = tiles ? s.gt0 : 0;
        L.hblocks = hubs;
    }
    if (L.on) {
        L.nblocks = plan_quarter(L.ntiles);
        if (!L.ep) L.gblocks = plan_rounds(L.nblocks);
        L.rblocks = plan_quarter(L.nrest);
        L.grid = L.hblocks + L.gblocks + L.rblocks;
    }
    if (s.e > s.he) {               // generic CSR kernel, one lane per variable
        p.generic.on = true;
        p.generic.stream = plan_stream(o, PLAN_SIDE1);
        p.generic.n = s.e - s.he;
        p.generic.grid = (p.generic.n + PLAN_BLOCK - 1) / PLAN_BLOCK;
    }
    p.segments = tiles;
    if (tiles && s.nrest > 0 && L.nrest == 0) {
        p.fast.on = true;
        p.fast.n = s.nrest;
        p.fast.grid = plan_rounds(plan_quarter(s.nrest));
    }
    return p;
}

// ---- learning: enqueued as generic, heavy, general, segment launches, fast, dyn ----
struct LearnClassPlan {
    bool skip = false;              // an empty class: no launch, no update, not counted as a class
    SimpleLaunch generic;           // k_learn_phase, range mode, over [he, e): n = its items of 64 positions
    SimpleLaunch heavy;             // k_learn_heavy over the hubs [fe, he) when no general launch carries them
    GeneralLaunch general;          // k_learn_ep* (general.ep) or k_learn_general<maxc>
    bool kstat = false;             // the entry-parallel launch skips zero-gradient visits, the update adds the structural counts
    SimpleLaunch fast;              // k_learn_fast over the learn-rest tiles no general launch took
    SimpleLaunch dyn;               // k_learn_phase, list mode, over the tiles with per-lane headers
    bool update = false;            // a weight update follows the class
};

static inline LearnClassPlan plan_learn_class(const ClassShape &s, const PlanOpts &o) {
    LearnClassPlan p;
    if (s.e <= s.fb) { p.skip = true; return p; }
    if (s.e > s.he) {               // variables outside the fast path
        p.generic.on = true;
        p.generic.stream = plan_stream(o, PLAN_SIDE1);
        p.generic.n = (s.e - s.he + 63) / 64;
        p.generic.grid = std::min(plan_cap(o, PLAN_LEARN_GEN_BLOCKS), plan_quarter(p.generic.n));
    }
    // hubs ride as extra blocks of a general-tile launch when the class has one
    const int hubs = std::min(plan_cap(o, PLAN_LEARN_HEAVY_BLOCKS), plan_quarter(s.he - s.fe));
    const bool hubs_in_general = (s.gtb > s.gt0 || s.ntiles > s.gtb) && s.he > s.fe;
    if (s.he > s.fe && !hubs_in_general) {      // ... else one wave per variable in a launch of their own
        p.heavy.on = true;
        p.heavy.stream = plan_stream(o, PLAN_SIDE2);
        p.heavy.n = s.he - s.fe;
        p.heavy.grid = hubs;
    }
    // the class's uniform / shape tiles outside segment launches ride in the general launch
    const bool rest_in_general = s.ntiles > s.gt0 && s.nlrest > 0;
    // a class with a lot of both general tiles and other tiles runs the two groups side by side (side stream 0);
    // smaller ones are not worth the fork / join events
    const int other_tiles = (rest_in_general ? 0 : s.nlrest) + o.seg_tiles;
    const bool aside = s.ntiles - s.gt0 >= 2048 && other_tiles >= 2048 && o.overlap;
    GeneralLaunch &L = p.general;
    L.ep = s.fe > s.fb && s.ep && s.ntiles > s.gt0;
    // as in inference: a class with categorical tiles walks all its general tiles in one launch of the 8-candidate
    // kernel (+10 % over two concurrent launches)
    L.maxc = s.gtb > s.gt0 ? 8 : 2;
    L.on = L.ep || s.gtb > s.gt0 || s.ntiles > s.gtb;
    if (L.on) {
        L.stream = aside ? (int)PLAN_SIDE0 : (int)PLAN_MAIN;
        L.tile0 = L.maxc == 8 || L.ep ? s.gt0 : s.gtb;
        L.ntiles = s.ntiles - L.tile0;
        L.nblocks = plan_quarter(L.ntiles);
        L.hblocks = hubs_in_general ? hubs : 0;
        L.nrest = rest_in_general ? s.nlrest : 0;
        if (L.ep) {
            // grid: 10 workgroups per CU (4 are resident -- 128 with the cap of k_learn_ep_w4 / 114 vector registers --, the
            // others start as those end: dynamic dealing of uneven groups).  Per class (NSK_EP_PER_CU), 5M LR graph:
            // 3 workgroups per CU 142.4 us, 4 149.2, 5 139.5, 6 135.4, 7 134.2, 8 132.9, 10 134.7, 16 135.6; 50M LR graph:
            // 4 1362 us, 7 1247, 10 1189 -- and at 5M, twice each: 10 per CU 4.95 / 4.97e9 updates/s, 7 per CU 5.04 /
            // 5.06e9.  Hence 10 when a workgroup walks four groups or more, 7 otherwise (the shards of an 8-rank run of
            // the 50M graph are of the second kind).
            const int per_cu = o.ep_per_cu ? o.ep_per_cu : (s.ngroups >= 4 * 2560 ? 10 : 7);
            L.capped = L.maxc == 8;
            L.gblocks = plan_rounds(std::min(plan_cap(o, 256 * per_cu), s.ngroups));
            L.hblocks += s.nbh;             // a block per long-list hub
            // the rest tiles (shape tiles: graphs with individual weights) are walked by all of these workgroups, one
            // wave per tile: when the groups alone bring too few, more workgroups (they skip the group walk) -- the
            // weighted boolean graph has 750 groups and 7 000 rest tiles per colour
            L.rblocks = std::max(0, plan_rounds(std::min(plan_cap(o, 2560), plan_quarter(L.nrest))) - L.gblocks);
        } else {
            L.gblocks = plan_rounds(std::min(plan_cap(o, PLAN_LEARN_GENERAL_BLOCKS / 2), L.nblocks));
        }
        L.grid = L.hblocks + L.gblocks + L.rblocks;
    }
    // structural visit counts (not with L1: its truncation coins are counted per visit)
    p.kstat = L.ep && !o.smallw && o.has_kstat && o.regularization != 1;
    if (s.nlrest > 0 && !rest_in_general) {     // the other uniform and shape tiles: descriptor-driven kernel
        p.fast.on = true;
        p.fast.n = s.nlrest;
        p.fast.grid = std::min(plan_cap(o, PLAN_LEARN_FAST_BLOCKS), plan_quarter(s.nlrest));
    }
    if (s.ndyn > 0) {
        p.dyn.on = true;
        p.dyn.n = s.ndyn;
        p.dyn.grid = std::min(plan_cap(o, PLAN_LEARN_LIST_BLOCKS), plan_quarter(s.ndyn));
    }
    p.update = o.nweight > 0;
    return p;
}

// The plans of every class as the int32 records of nsk_graph_plan_classes (nsk_class_records.cpp): `opts` as a sweep
// driver fills them but for what it sets per class (seg_tiles; ep_per_cu, which counts from the first class laid out as
// groups on); rec[NSK_CLASS_REC * classes].
void compiled_class_records(const Compiled &c, bool learning, const PlanOpts &opts, int32_t *rec);

}  // namespace nsk
