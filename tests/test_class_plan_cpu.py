"""The launches of a colour class are decided by pure host functions (numbskull_amd/csrc/nsk_class_plan.h: class_shape,
plan_gibbs_class, plan_learn_class).  A stand-alone program fills the phase_* vectors of a Compiled by hand -- the class
under test is class 1, behind a class 0 that makes every base non-zero -- and asserts each plan against values worked
out by hand from the rules of the sweep drivers as they stood before the plans existed, the smallest classes that
exercise each rule, every one with side streams on and off.  On top of the literal values, for every case: each hub,
general tile, rest tile, learn-rest tile, per-lane-header tile and generic position of the class is covered by exactly
one launch of the plan, and every grid is the sum of its parts.  The same once more under the diagnostic grid cap
(PlanOpts::grid_cap, NSK_CLASS_GRID_CAP) at 1, 3 and 9 blocks: the literal grids of every class kind, worked out by hand
again, and every invariant -- the cap shrinks the persistent grids and nothing else.  Built with the host compiler under AddressSanitizer and
UndefinedBehaviorSanitizer (-fno-sanitize-recover); a clean exit is the pass."""

import subprocess

import pytest

from test_alloc_ledger_cpu import CSRC, _compiler

PROGRAM = r"""
#undef NDEBUG
#include <cassert>
#include <cstdio>
#include "nsk_class_plan.h"

using namespace nsk;

struct Cls { int fb, ntiles, nhub, ngeneric; int gt0, gtb; int nbh, ngroups, nrest, nlrest, ndyn; bool ep; bool tiles; };

// class 1 of a two-class layout; a class without tiles (tiles = false: fe == fb) keeps its tile-side numbers as garbage
static Compiled layout(const Cls &k) {
    Compiled c;
    const int64_t fe = k.fb + (k.tiles ? 64 * (int64_t)k.ntiles : 0), he = fe + k.nhub, e = he + k.ngeneric;
    c.phase_start = {0, k.fb, e + 128};
    c.phase_end = {0, e}; c.phase_fast_end = {0, fe}; c.phase_heavy_end = {0, he};
    c.phase_wb_base = {0, 10, 10 + (k.tiles ? k.ntiles : 0)};
    c.phase_gen_tile = {0, k.gt0}; c.phase_gen_bin_tile = {0, k.gtb};
    c.phase_hub_base = {0, 5, 5 + k.nhub};
    c.phase_bighub_base = {0, 3, 3 + k.nbh};
    c.phase_ep_base = {0, 7, 7 + k.ngroups};
    c.phase_rest_base = {0, 11, 11 + k.nrest};
    c.phase_learn_rest_base = {0, 13, 13 + k.nlrest};
    c.phase_dyn_base = {0, 17, 17 + k.ndyn};
    c.phase_ep = {0, (uint8_t)(k.ep ? 1 : 0)};
    return c;
}

static void check_general(const GeneralLaunch &L) {
    if (!L.on) return;
    assert(L.grid == L.hblocks + L.gblocks + L.rblocks && L.grid > 0);
    assert(L.maxc == 8 || L.maxc == 2);
    assert(L.nblocks == (L.ntiles + 3) / 4);
}
static void check_simple(const SimpleLaunch &L) { if (L.on) assert(L.n > 0 && L.grid > 0); }

// a persistent grid's limit under the diagnostic cap (restated, not plan_cap: 0 is no cap)
static int capped(const PlanOpts &o, int limit) { return o.grid_cap > 0 && o.grid_cap < limit ? o.grid_cap : limit; }
static int rounds(int blocks) { return (blocks + 7) / 8 * 8; }

// every item of the class in exactly one launch; grids = the sum of their parts
static void check_gibbs(const ClassShape &s, const GibbsClassPlan &p, const PlanOpts &o) {
    const GeneralLaunch &L = p.general;
    check_general(L); check_simple(p.generic); check_simple(p.fast);
    const bool tiles = s.fe > s.fb;
    assert(((L.on && L.hblocks > 0) ? 1 : 0) == (s.he > s.fe ? 1 : 0));
    if (s.he > s.fe) assert(L.hblocks == (L.ep ? s.nbh : 0) + (s.he - s.fe + 3) / 4);        // a wave per hub, a block per long-list hub
    for (int t = tiles ? s.gt0 : 0; t < (tiles ? s.ntiles : 0); t++) assert(L.on && t >= L.tile0 && t < L.tile0 + L.ntiles);
    if (L.on && L.ntiles > 0) assert(tiles && L.tile0 >= s.gt0 && L.tile0 + L.ntiles == s.ntiles);
    if (L.on && !L.ep) assert(L.gblocks >= L.nblocks && L.gblocks % 8 == 0);                   // a wave per tile
    // (what the driver's dispatch relies on: behind the generic fork goes the all-binary launch of k_gibbs_general, on the main stream)
    if (L.on) assert(L.behind_generic == (!L.ep && L.maxc == 2) && (!L.behind_generic || L.stream == PLAN_MAIN));
    if (L.on && L.ep) assert(L.gblocks > 0 && L.gblocks % 8 == 0 && L.gblocks <= (s.ngroups + 7) / 8 * 8);
    if (L.on && L.ep) assert(L.gblocks == rounds(std::min(s.ngroups, capped(o, 256 * (o.ep_per_cu ? o.ep_per_cu : 7)))));
    for (int r = 0; r < (tiles ? s.nrest : 0); r++) assert(((L.on && r < L.nrest) ? 1 : 0) + ((p.fast.on && r < p.fast.n) ? 1 : 0) == 1);
    if (L.on) assert(L.rblocks == (L.nrest + 3) / 4 && L.nrest <= (tiles ? s.nrest : 0));
    if (p.fast.on) assert(tiles && p.fast.n == s.nrest && p.fast.grid >= (p.fast.n + 3) / 4 && p.fast.grid % 8 == 0 && p.fast.stream == PLAN_MAIN);
    assert(p.generic.on == (s.e > s.he));
    if (p.generic.on) assert(p.generic.n == s.e - s.he && p.generic.grid == (p.generic.n + 255) / 256);
    assert(p.segments == tiles);
}
static void check_learn(const ClassShape &s, const LearnClassPlan &p, const PlanOpts &o) {
    const GeneralLaunch &L = p.general;
    if (p.skip) { assert(s.e <= s.fb && !L.on && !p.generic.on && !p.heavy.on && !p.fast.on && !p.dyn.on && !p.update); return; }
    check_general(L); check_simple(p.generic); check_simple(p.heavy); check_simple(p.fast); check_simple(p.dyn);
    assert(((L.on && L.hblocks > (L.ep ? s.nbh : 0)) ? 1 : 0) + (p.heavy.on ? 1 : 0) == (s.he > s.fe ? 1 : 0));
    if (p.heavy.on) assert(p.heavy.n == s.he - s.fe && p.heavy.grid == std::min(capped(o, 512), (p.heavy.n + 3) / 4));
    for (int t = s.gt0; t < s.ntiles; t++) assert(L.on && t >= L.tile0 && t < L.tile0 + L.ntiles);
    if (L.on) assert(L.tile0 >= s.gt0 && L.tile0 + L.ntiles == s.ntiles && L.ntiles > 0);
    // the persistent grids: whole rounds of XCDs for the tiles / groups, hubs and rest blocks beside them
    if (L.on) assert(L.gblocks > 0 && L.gblocks % 8 == 0);
    if (L.on && L.hblocks > (L.ep ? s.nbh : 0)) assert(L.hblocks - (L.ep ? s.nbh : 0) == std::min(capped(o, 512), (s.he - s.fe + 3) / 4));
    if (L.on && !L.ep) assert(L.gblocks == rounds(std::min(capped(o, 1024), L.nblocks)) && L.rblocks == 0);
    if (L.on && L.ep) {
        const int per_cu = o.ep_per_cu ? o.ep_per_cu : (s.ngroups >= 10240 ? 10 : 7);
        assert(L.gblocks == rounds(std::min(capped(o, 256 * per_cu), s.ngroups)));
        assert(L.rblocks == std::max(0, rounds(std::min(capped(o, 2560), (L.nrest + 3) / 4)) - L.gblocks));
    }
    for (int r = 0; r < s.nlrest; r++) assert(((L.on && r < L.nrest) ? 1 : 0) + ((p.fast.on && r < p.fast.n) ? 1 : 0) == 1);
    if (p.fast.on) assert(p.fast.n == s.nlrest && p.fast.grid == std::min(capped(o, 2048), (p.fast.n + 3) / 4) && p.fast.stream == PLAN_MAIN);
    assert(p.dyn.on == (s.ndyn > 0));
    if (p.dyn.on) assert(p.dyn.n == s.ndyn && p.dyn.grid == std::min(capped(o, 512), (s.ndyn + 3) / 4) && p.dyn.stream == PLAN_MAIN);
    assert(p.generic.on == (s.e > s.he));
    if (p.generic.on) assert(p.generic.n == (s.e - s.he + 63) / 64 && p.generic.grid == std::min(capped(o, 2048), (p.generic.n + 3) / 4));
    if (p.kstat) assert(L.on && L.ep);
}

static GibbsClassPlan gibbs(const Cls &k, const PlanOpts &o) {
    const Compiled c = layout(k);
    const ClassShape s = class_shape(c, 1);
    assert(s.wb_base == 10 && s.hub0 == 5 && s.bh0 == 3 && s.group0 == 7 && s.rest0 == 11 && s.lrest0 == 13 && s.dyn0 == 17);
    assert(s.fb == k.fb && s.he - s.fe == k.nhub && s.e - s.he == k.ngeneric && s.nbh == k.nbh && s.ngroups == k.ngroups &&
           s.nrest == k.nrest && s.nlrest == k.nlrest && s.ndyn == k.ndyn && s.ep == k.ep && s.gt0 == k.gt0 && s.gtb == k.gtb);
    assert(s.ntiles == (k.tiles ? k.ntiles : 0) && s.fe - s.fb == 64 * s.ntiles);
    const ClassShape s0 = class_shape(c, 0);       // the class in front has no position (its lists are only there to move the bases)
    assert(s0.fb == 0 && s0.e == 0 && s0.wb_base == 0 && s0.ntiles == 10 && s0.rest0 == 0 && s0.nrest == 11 && s0.ngroups == 7 && !s0.ep);
    const GibbsClassPlan p = plan_gibbs_class(s, o);
    check_gibbs(s, p, o);
    const GibbsClassPlan p0 = plan_gibbs_class(s0, o);
    assert(!p0.general.on && !p0.generic.on && !p0.segments && !p0.fast.on);
    return p;
}
static LearnClassPlan learn(const Cls &k, const PlanOpts &o) {
    const Compiled c = layout(k);
    const ClassShape s = class_shape(c, 1);
    const LearnClassPlan p = plan_learn_class(s, o);
    check_learn(s, p, o);
    assert(plan_learn_class(class_shape(c, 0), o).skip);
    return p;
}

// the general launch: on, ep, maxc, capped, behind_generic, stream, tile0, ntiles, nblocks, hblocks, gblocks, rblocks, grid, nrest
static bool is(const GeneralLaunch &L, bool ep, int maxc, bool capped, bool behind, int stream, int tile0, int ntiles, int nblocks,
               int hblocks, int gblocks, int rblocks, int grid, int nrest) {
    return L.on && L.ep == ep && L.maxc == maxc && L.capped == capped && L.behind_generic == behind && L.stream == stream &&
           L.tile0 == tile0 && L.ntiles == ntiles && L.nblocks == nblocks && L.hblocks == hblocks && L.gblocks == gblocks &&
           L.rblocks == rblocks && L.grid == grid && L.nrest == nrest;
}
static bool is(const SimpleLaunch &L, int stream, int n, int grid) { return L.on && L.stream == stream && L.n == n && L.grid == grid; }

static void inference(bool overlap) {
    PlanOpts o;
    o.overlap = overlap;
    o.value_bytes = (size_t)1 << 20;
    const int S0 = overlap ? PLAN_SIDE0 : PLAN_MAIN, S1 = overlap ? PLAN_SIDE1 : PLAN_MAIN, M = PLAN_MAIN;
    //        fb  ntiles nhub ngeneric gt0 gtb nbh ngroups nrest nlrest ndyn ep tiles
    {   // segments only
        const GibbsClassPlan p = gibbs({1024, 10, 0, 0, 10, 10, 0, 0, 0, 0, 0, false, true}, o);
        assert(!p.general.on && !p.generic.on && p.segments && !p.fast.on);
    }
    const int rest_n[3] = {1, 4, 5}, rest_grid[3] = {8, 8, 8};
    for (int i = 0; i < 3; i++) {   // rest tiles only: k_gibbs_fast, whole rounds of XCDs
        const GibbsClassPlan p = gibbs({1024, 10, 0, 0, 10, 10, 0, 0, rest_n[i], 0, 0, false, true}, o);
        assert(!p.general.on && !p.generic.on && p.segments && is(p.fast, M, rest_n[i], rest_grid[i]));
    }
    {   // 40 rest tiles: 10 blocks in 16
        const GibbsClassPlan p = gibbs({1024, 50, 0, 0, 50, 50, 0, 0, 40, 0, 0, false, true}, o);
        assert(is(p.fast, M, 40, 16));
    }
    {   // all-binary general tiles [12, 20) with 6 hubs and 5 rest tiles: one <2> launch on the main stream behind the generic fork
        const GibbsClassPlan p = gibbs({1024, 20, 6, 0, 12, 12, 0, 0, 5, 0, 0, false, true}, o);
        assert(is(p.general, false, 2, false, true, M, 12, 8, 2, 2, 8, 2, 12, 5) && !p.fast.on && !p.generic.on && p.segments);
    }
    {   // categorical [12, 15) + binary [15, 20) general tiles, 6 hubs, 5 rest tiles, 300 generic lanes: one <8> launch over all of them
        const GibbsClassPlan p = gibbs({1024, 20, 6, 300, 12, 15, 0, 0, 5, 0, 0, false, true}, o);
        assert(is(p.general, false, 8, false, false, M, 12, 8, 2, 2, 8, 2, 12, 5) && !p.fast.on && is(p.generic, S1, 300, 2));
    }
    {   // 37 categorical general tiles: 10 blocks in 16, no hubs, no rest
        const GibbsClassPlan p = gibbs({1024, 40, 0, 0, 3, 40, 0, 0, 0, 0, 0, false, true}, o);
        assert(is(p.general, false, 8, false, false, M, 3, 37, 10, 0, 16, 0, 16, 0));
    }
    const int hub_n[3] = {1, 4, 5}, hub_blocks[3] = {1, 1, 2};
    for (int i = 0; i < 3; i++) {   // hubs only, fe == fb: tile and rest counts are taken as 0 whatever the layout holds
        const GibbsClassPlan p = gibbs({1024, 9, hub_n[i], 0, 3, 3, 0, 0, 2, 0, 0, false, false}, o);
        assert(is(p.general, false, 8, false, false, S0, 0, 0, 0, hub_blocks[i], 0, 0, hub_blocks[i], 0));
        assert(!p.segments && !p.fast.on && !p.generic.on);
    }
    {   // hubs only, fe == fb, in a layout that marks the class entry-parallel: not an ep launch
        const GibbsClassPlan p = gibbs({1024, 9, 5, 0, 0, 0, 0, 0, 0, 0, 0, true, false}, o);
        assert(is(p.general, false, 8, false, false, S0, 0, 0, 0, 2, 0, 0, 2, 0));
    }
    {   // hubs beside segment and rest tiles, no general tiles: hubs-only launch on side 0, k_gibbs_fast for the rest
        const GibbsClassPlan p = gibbs({1024, 10, 5, 70, 10, 10, 0, 0, 3, 0, 0, false, true}, o);
        assert(is(p.general, false, 8, false, false, S0, 10, 0, 0, 2, 0, 0, 2, 0) && is(p.fast, M, 3, 8) && is(p.generic, S1, 70, 1) && p.segments);
    }
    {   // generic lanes only
        const GibbsClassPlan p = gibbs({1024, 0, 0, 300, 0, 0, 0, 0, 0, 0, 0, false, false}, o);
        assert(!p.general.on && is(p.generic, S1, 300, 2) && !p.segments && !p.fast.on);
        const GibbsClassPlan q = gibbs({1024, 0, 0, 256, 0, 0, 0, 0, 0, 0, 0, false, false}, o);
        assert(is(q.generic, S1, 256, 1));
    }
    {   // an empty class
        const GibbsClassPlan p = gibbs({1024, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, false, false}, o);
        assert(!p.general.on && !p.generic.on && !p.segments && !p.fast.on);
    }
    // entry-parallel classes: general tiles [8, 40) = 8 groups, categorical up to tile 30; 5 hubs, 6 rest tiles, 10 generic lanes
    {   // value array of exactly 24 MiB: the capped twin
        o.value_bytes = (size_t)24 << 20;
        const GibbsClassPlan p = gibbs({1024, 40, 5, 10, 8, 30, 0, 8, 6, 0, 0, true, true}, o);
        assert(is(p.general, true, 8, true, false, M, 8, 32, 8, 2, 8, 2, 12, 6) && !p.fast.on && is(p.generic, S1, 10, 1) && p.segments);
    }
    {   // one byte more
        o.value_bytes = ((size_t)24 << 20) + 1;
        const GibbsClassPlan p = gibbs({1024, 40, 5, 10, 8, 30, 0, 8, 6, 0, 0, true, true}, o);
        assert(is(p.general, true, 8, false, false, M, 8, 32, 8, 2, 8, 2, 12, 6));
    }
    o.value_bytes = (size_t)1 << 20;
    {   // all-binary: the two-candidate kernel whatever the size
        const GibbsClassPlan p = gibbs({1024, 40, 5, 0, 8, 8, 0, 8, 6, 0, 0, true, true}, o);
        assert(is(p.general, true, 2, false, false, M, 8, 32, 8, 2, 8, 2, 12, 6));
    }
    {   // three long-list hubs among the five: a block each in front
        const GibbsClassPlan p = gibbs({1024, 40, 5, 0, 8, 30, 3, 8, 0, 0, 0, true, true}, o);
        assert(is(p.general, true, 8, true, false, M, 8, 32, 8, 5, 8, 0, 13, 0));
    }
    const int groups[4] = {1784, 1792, 1793, 1800}, gblocks[4] = {1784, 1792, 1792, 1792};     // 7 workgroups per CU: at most 256 * 7
    for (int i = 0; i < 4; i++) {
        const GibbsClassPlan p = gibbs({1024, 4 * groups[i], 0, 0, 0, 4, 0, groups[i], 0, 0, 0, true, true}, o);
        assert(is(p.general, true, 8, true, false, M, 0, 4 * groups[i], groups[i], 0, gblocks[i], 0, gblocks[i], 0));
    }
    {   // NSK_EP_PER_CU
        assert(plan_per_cu(nullptr) == 0 && plan_per_cu("3") == 3 && plan_per_cu("0") == 1 && plan_per_cu("99") == 32);
        o.ep_per_cu = 3;
        const GibbsClassPlan p = gibbs({1024, 4000, 0, 0, 0, 4, 0, 1000, 0, 0, 0, true, true}, o);
        assert(is(p.general, true, 8, true, false, M, 0, 4000, 1000, 0, 768, 0, 768, 0));
        o.ep_per_cu = 0;
    }
}

static void learning(bool overlap) {
    PlanOpts o;
    o.overlap = overlap;
    o.smallw = false; o.nweight = 10; o.has_kstat = true; o.regularization = 2; o.seg_tiles = 0;
    const int S0 = overlap ? PLAN_SIDE0 : PLAN_MAIN, S1 = overlap ? PLAN_SIDE1 : PLAN_MAIN, S2 = overlap ? PLAN_SIDE2 : PLAN_MAIN, M = PLAN_MAIN;
    //        fb  ntiles nhub ngeneric gt0 gtb nbh ngroups nrest nlrest ndyn ep tiles
    {   // general_aside: 2048 general tiles and 2047 / 2048 tiles in segment launches; 2047 general tiles
        const Cls k = {1024, 2058, 0, 0, 10, 100, 0, 0, 0, 0, 0, false, true};
        o.seg_tiles = 2047;
        assert(is(learn(k, o).general, false, 8, false, false, M, 10, 2048, 512, 0, 512, 0, 512, 0));
        o.seg_tiles = 2048;
        assert(is(learn(k, o).general, false, 8, false, false, S0, 10, 2048, 512, 0, 512, 0, 512, 0));
        const Cls k1 = {1024, 2057, 0, 0, 10, 100, 0, 0, 0, 0, 0, false, true};
        assert(is(learn(k1, o).general, false, 8, false, false, M, 10, 2047, 512, 0, 512, 0, 512, 0));
        // the learn-rest tiles a general launch takes do not count as other tiles
        const Cls k2 = {1024, 2058, 0, 0, 10, 100, 0, 0, 0, 3000, 0, false, true};
        o.seg_tiles = 0;
        assert(is(learn(k2, o).general, false, 8, false, false, M, 10, 2048, 512, 0, 512, 0, 512, 3000) && !learn(k2, o).fast.on);
        // all-binary general tiles beside: the two-candidate kernel from gtb on, capped at 1024 blocks
        const Cls k3 = {1024, 6000, 9, 0, 10, 10, 0, 0, 0, 0, 0, false, true};
        o.seg_tiles = 5000;
        assert(is(learn(k3, o).general, false, 2, false, false, S0, 10, 5990, 1498, 3, 1024, 0, 1027, 0));
        o.seg_tiles = 0;
    }
    {   // 10 workgroups per CU from 10240 groups on, 7 below; NSK_EP_PER_CU
        const LearnClassPlan p = learn({1024, 4 * 10239, 0, 0, 0, 4, 0, 10239, 0, 0, 0, true, true}, o);
        assert(is(p.general, true, 8, true, false, M, 0, 4 * 10239, 10239, 0, 1792, 0, 1792, 0) && p.kstat);
        const LearnClassPlan q = learn({1024, 4 * 10240, 0, 0, 0, 4, 0, 10240, 0, 0, 0, true, true}, o);
        assert(is(q.general, true, 8, true, false, M, 0, 4 * 10240, 10240, 0, 2560, 0, 2560, 0));
        o.ep_per_cu = 2;
        const LearnClassPlan r = learn({1024, 4 * 10240, 0, 0, 0, 4, 0, 10240, 0, 0, 0, true, true}, o);
        assert(is(r.general, true, 8, true, false, M, 0, 4 * 10240, 10240, 0, 512, 0, 512, 0));
        o.ep_per_cu = 0;
    }
    {   // rest blocks of an ep launch: what the rest tiles need beyond the group blocks (16 groups; all-binary: k_learn_ep<2>)
        const int nl[4] = {0, 40, 100, 20000}, rb[4] = {0, 0, 16, 2544};
        for (int i = 0; i < 4; i++) {
            const LearnClassPlan p = learn({1024, 70, 5, 0, 6, 6, 2, 16, 0, nl[i], 0, true, true}, o);
            assert(is(p.general, true, 2, false, false, M, 6, 64, 16, 4, 16, rb[i], 20 + rb[i], nl[i]) && !p.fast.on && !p.heavy.on && p.kstat);
        }
    }
    {   // hubs: in the general launch when there is one (categorical; all-binary), else k_learn_heavy on side 2 (capped at 512 blocks)
        const LearnClassPlan p = learn({1024, 20, 5, 0, 12, 15, 0, 0, 0, 7, 0, false, true}, o);
        assert(is(p.general, false, 8, false, false, M, 12, 8, 2, 2, 8, 0, 10, 7) && !p.heavy.on && !p.fast.on && !p.kstat);
        const LearnClassPlan b = learn({1024, 20, 5, 0, 12, 12, 0, 0, 0, 7, 0, false, true}, o);
        assert(is(b.general, false, 2, false, false, M, 12, 8, 2, 2, 8, 0, 10, 7) && !b.heavy.on && !b.fast.on);
        const LearnClassPlan q = learn({1024, 20, 5, 1000, 20, 20, 0, 0, 0, 7, 0, false, true}, o);
        assert(!q.general.on && is(q.heavy, S2, 5, 2) && is(q.fast, M, 7, 2) && is(q.generic, S1, 16, 4));
        const LearnClassPlan r = learn({1024, 0, 4000, 0, 0, 0, 0, 0, 0, 0, 0, false, false}, o);
        assert(!r.general.on && is(r.heavy, S2, 4000, 512) && !r.fast.on && r.update);
    }
    {   // tiles with per-lane headers: list mode
        const LearnClassPlan p = learn({1024, 20, 0, 0, 20, 20, 0, 0, 0, 9, 9, false, true}, o);
        assert(is(p.dyn, M, 9, 3) && is(p.fast, M, 9, 3) && !p.general.on);
        const LearnClassPlan q = learn({1024, 3000, 0, 0, 3000, 3000, 0, 0, 0, 0, 3000, false, true}, o);
        assert(is(q.dyn, M, 3000, 512));
    }
    {   // structural visit counts: an ep launch, global accumulators, the counts in the layout, not L1 -- each alone false
        const Cls k = {1024, 64, 0, 0, 0, 4, 0, 16, 0, 0, 0, true, true};
        assert(learn(k, o).kstat);
        o.smallw = true; assert(!learn(k, o).kstat); o.smallw = false;
        o.has_kstat = false; assert(!learn(k, o).kstat); o.has_kstat = true;
        o.regularization = 1; assert(!learn(k, o).kstat); o.regularization = 2;
        const Cls notep = {1024, 64, 0, 0, 0, 4, 0, 16, 0, 0, 0, false, true};
        assert(!learn(notep, o).kstat && !learn(notep, o).general.ep);
        o.smallw = true;       // SMALLW changes nothing else
        assert(is(learn(k, o).general, true, 8, true, false, M, 0, 64, 16, 0, 16, 0, 16, 0));
        o.smallw = false;
        assert(is(learn(k, o).general, true, 8, true, false, M, 0, 64, 16, 0, 16, 0, 16, 0));
    }
    {   // an empty class is skipped; a graph without weights gets no update
        assert(learn({1024, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, false, false}, o).skip);
        o.nweight = 0;
        const LearnClassPlan p = learn({1024, 0, 0, 100, 0, 0, 0, 0, 0, 0, 0, false, false}, o);
        assert(!p.skip && !p.update && is(p.generic, S1, 2, 1));
        o.nweight = 10;
    }
}

// NSK_CLASS_GRID_CAP = 1, 3, 9: min(cap, limit) blocks, whole rounds of XCDs where the launch has them -- 8, 8, 16
static void capped_plans(bool overlap) {
    const int S0 = overlap ? PLAN_SIDE0 : PLAN_MAIN, S1 = overlap ? PLAN_SIDE1 : PLAN_MAIN, S2 = overlap ? PLAN_SIDE2 : PLAN_MAIN, M = PLAN_MAIN;
    assert(plan_grid_cap(nullptr) == 0 && plan_grid_cap("0") == 1 && plan_grid_cap("3") == 3 && plan_grid_cap("99999999") == 1 << 20);
    const int caps[3] = {1, 3, 9}, rnd[3] = {8, 8, 16};
    for (int i = 0; i < 3; i++) {
        const int c = caps[i], g8 = rnd[i];
        PlanOpts o;
        o.overlap = overlap; o.grid_cap = c;
        assert(plan_cap(o, 2048) == c && plan_cap(o, 1) == 1);
        // ---- learning
        o.smallw = false; o.nweight = 10; o.has_kstat = true; o.regularization = 2;
        //        fb  ntiles nhub ngeneric gt0 gtb nbh ngroups nrest nlrest ndyn ep tiles
        {   // 2048 categorical general tiles beside 2048 segment tiles: 512 blocks become one or two rounds; the stream stays
            o.seg_tiles = 2048;
            assert(is(learn({1024, 2058, 0, 0, 10, 100, 0, 0, 0, 0, 0, false, true}, o).general, false, 8, false, false, S0, 10, 2048, 512, 0, g8, 0, g8, 0));
            o.seg_tiles = 0;
            // ... with 3000 learn-rest tiles behind them: no block more
            assert(is(learn({1024, 2058, 0, 0, 10, 100, 0, 0, 0, 3000, 0, false, true}, o).general, false, 8, false, false, M, 10, 2048, 512, 0, g8, 0, g8, 3000));
            // all-binary, 9 hubs in front: min(cap, 3) hub blocks
            o.seg_tiles = 5000;
            const int hb = std::min(c, 3);
            assert(is(learn({1024, 6000, 9, 0, 10, 10, 0, 0, 0, 0, 0, false, true}, o).general, false, 2, false, false, S0, 10, 5990, 1498, hb, g8, 0, hb + g8, 0));
            o.seg_tiles = 0;
        }
        {   // 8 general tiles, 5 hubs, 7 learn-rest tiles: 2 blocks are one round with or without the cap; min(cap, 2) hub blocks
            const int hb = std::min(c, 2);
            const LearnClassPlan p = learn({1024, 20, 5, 0, 12, 15, 0, 0, 0, 7, 0, false, true}, o);
            assert(is(p.general, false, 8, false, false, M, 12, 8, 2, hb, 8, 0, hb + 8, 7) && !p.heavy.on && !p.fast.on);
        }
        {   // entry-parallel: 10240 groups (10 workgroups per CU: 2560) on min(cap, 2560) blocks; NSK_EP_PER_CU beside the cap
            const LearnClassPlan p = learn({1024, 4 * 10240, 0, 0, 0, 4, 0, 10240, 0, 0, 0, true, true}, o);
            assert(is(p.general, true, 8, true, false, M, 0, 4 * 10240, 10240, 0, g8, 0, g8, 0) && p.kstat);
            o.ep_per_cu = 2;
            assert(is(learn({1024, 4 * 10240, 0, 0, 0, 4, 0, 10240, 0, 0, 0, true, true}, o).general, true, 8, true, false, M, 0, 4 * 10240, 10240, 0, g8, 0, g8, 0));
            o.ep_per_cu = 0;
        }
        {   // 16 groups, 5 hubs of which 2 long-list, rest tiles: the rest tiles' own limit is capped too -- no rest block
            const int nl[4] = {0, 40, 100, 20000}, hb = 2 + std::min(c, 2);
            for (int j = 0; j < 4; j++) {
                const LearnClassPlan p = learn({1024, 70, 5, 0, 6, 6, 2, 16, 0, nl[j], 0, true, true}, o);
                assert(is(p.general, true, 2, false, false, M, 6, 64, 16, hb, g8, 0, hb + g8, nl[j]) && !p.fast.on && !p.heavy.on);
            }
            // 4 groups (one round) and 100 rest tiles (25 blocks): rest blocks only when the cap leaves more than one round
            const LearnClassPlan q = learn({1024, 22, 0, 0, 6, 6, 0, 4, 0, 100, 0, true, true}, o);
            assert(is(q.general, true, 2, false, false, M, 6, 16, 4, 0, 8, g8 - 8, g8, 100));
        }
        {   // the launches of their own: 5 hubs (2 blocks), 7 learn-rest tiles (2), 16 generic items (4); 4000 hubs (512)
            const LearnClassPlan q = learn({1024, 20, 5, 1000, 20, 20, 0, 0, 0, 7, 0, false, true}, o);
            assert(!q.general.on && is(q.heavy, S2, 5, std::min(c, 2)) && is(q.fast, M, 7, std::min(c, 2)) && is(q.generic, S1, 16, std::min(c, 4)));
            const LearnClassPlan r = learn({1024, 0, 4000, 0, 0, 0, 0, 0, 0, 0, 0, false, false}, o);
            assert(!r.general.on && is(r.heavy, S2, 4000, c) && r.update);
        }
        {   // per-lane headers: 9 tiles (3 blocks), 3000 (512)
            const LearnClassPlan p = learn({1024, 20, 0, 0, 20, 20, 0, 0, 0, 9, 9, false, true}, o);
            assert(is(p.dyn, M, 9, std::min(c, 3)) && is(p.fast, M, 9, std::min(c, 3)) && !p.general.on);
            assert(is(learn({1024, 3000, 0, 0, 3000, 3000, 0, 0, 0, 0, 3000, false, true}, o).dyn, M, 3000, c));
        }
        {   // an empty class; two generic items on one block
            assert(learn({1024, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, false, false}, o).skip);
            assert(is(learn({1024, 0, 0, 100, 0, 0, 0, 0, 0, 0, 0, false, false}, o).generic, S1, 2, 1));
        }
        // ---- inference: the group grid alone
        o = PlanOpts();
        o.overlap = overlap; o.grid_cap = c; o.value_bytes = (size_t)1 << 20;
        {   // 1800 groups on min(cap, 1792) blocks; 8 groups stay one round, their hub and rest blocks as they were
            const GibbsClassPlan p = gibbs({1024, 4 * 1800, 0, 0, 0, 4, 0, 1800, 0, 0, 0, true, true}, o);
            assert(is(p.general, true, 8, true, false, M, 0, 4 * 1800, 1800, 0, g8, 0, g8, 0));
            const GibbsClassPlan q = gibbs({1024, 40, 5, 10, 8, 30, 3, 8, 6, 0, 0, true, true}, o);
            assert(is(q.general, true, 8, true, false, M, 8, 32, 8, 5, 8, 2, 15, 6) && is(q.generic, S1, 10, 1));
            o.ep_per_cu = 3;
            assert(is(gibbs({1024, 4000, 0, 0, 0, 4, 0, 1000, 0, 0, 0, true, true}, o).general, true, 8, true, false, M, 0, 4000, 1000, 0, g8, 0, g8, 0));
            o.ep_per_cu = 0;
        }
        {   // the grids without a trip loop are not capped: 37 categorical tiles, 40 rest tiles, 300 generic lanes, 5 hubs
            assert(is(gibbs({1024, 40, 0, 0, 3, 40, 0, 0, 0, 0, 0, false, true}, o).general, false, 8, false, false, M, 3, 37, 10, 0, 16, 0, 16, 0));
            assert(is(gibbs({1024, 50, 0, 0, 50, 50, 0, 0, 40, 0, 0, false, true}, o).fast, M, 40, 16));
            assert(is(gibbs({1024, 0, 0, 300, 0, 0, 0, 0, 0, 0, 0, false, false}, o).generic, S1, 300, 2));
            assert(is(gibbs({1024, 9, 5, 0, 3, 3, 0, 0, 2, 0, 0, false, false}, o).general, false, 8, false, false, S0, 0, 0, 0, 2, 0, 0, 2, 0));
        }
    }
}

int main() {
    inference(true); inference(false);
    learning(true); learning(false);
    capped_plans(true); capped_plans(false);
    std::puts("class plans ok");
    return 0;
}
"""


def test_class_plans_under_sanitizers(tmp_path):
    cxx, san = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    src, exe = tmp_path / "class_plan_main.cpp", tmp_path / "class_plan_main"
    src.write_text(PROGRAM)
    cmd = cxx + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread"] + san + ["-I", CSRC, str(src), "-o", str(exe)]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:       # (a compiler without these switches)
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert "class plans ok" in run.stdout
