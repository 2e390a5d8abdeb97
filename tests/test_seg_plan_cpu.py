"""The segment launches of a sweep are planned by pure host functions (numbskull_amd/csrc/nsk_seg_plan.h: plan_segments,
plan_learn_segment and the grid functions).  A stand-alone program fills Compiled::segments, seg_wide, learn_seg and the
phase vector by hand and asserts each plan against values worked out by hand from the rules of the sweep drivers as they
stood before the planner existed -- per rule the smallest layout that reaches it: batching by (kind, chunk count), eight
entries to a launch, evidence, lead tiles and virtual quads, the wide-quad threshold and its other conditions, the rest
list and its edge at 64, the border / interior split of a fused exchange and its ordering, the grids on both sides of
their caps, and learning's wide choice and tile-by-tile numbering.  On top of the literal values, for every case: every
tile of every sampled segment lies in exactly one entry of exactly one launch of its class, the virtual tile ranges are
disjoint and add up to the table's tile count, the whole wide quads and the listed rest quads of a wide launch are all
its quads, each once, every grid is positive and whole rounds of 8 where the drivers' were, and options that differ
compare unequal.  Built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer
(-fno-sanitize-recover); a clean exit is the pass."""

import subprocess

import pytest

from test_alloc_ledger_cpu import CSRC, _compiler

PROGRAM = r"""
#undef NDEBUG
#include <cassert>
#include <cstdio>
#include <map>
#include <string>
#include "nsk_seg_plan.h"

using namespace nsk;

static const uint32_t NO = NSK_NO_STREAM;

// a layout of two colour classes
static Compiled two_classes() { Compiled c; c.phase_start = {0, 1 << 20, 2 << 20}; return c; }
static void add(Compiled &c, int phase, int64_t pos0, int ntiles, uint32_t kind, uint32_t nslots, int ev = 0, int64_t ztab = -1,
                int64_t aff = -1, int64_t wide = -1, uint32_t adj_off = 0, uint32_t prog = 0) {
    Compiled::Segment s;
    s.phase = phase; s.pos0 = pos0; s.ntiles = ntiles; s.adj_off = adj_off; s.prog = prog; s.nslots = nslots; s.kind = kind; s.ev = ev;
    s.ztab = ztab; s.aff = aff; s.wide = wide;
    c.segments.push_back(s);
}
// quad descriptors, one letter each ('w': a wide quad); returns their first dword
static int64_t quads(Compiled &c, const std::string &pattern, int nch = 1) {
    const int64_t off = (int64_t)c.seg_wide.size();
    for (char ch : pattern)
        for (int j = 0; j < NSK_WIDE_STRIDE(nch); j++) c.seg_wide.push_back(j == 0 && ch != 'w' ? 0xFFFFFFFFu : 7u);
    return off;
}

static bool entry(const SegEntry &e, int tile_start, int nt, int lead, int pos0, uint32_t adj_off, uint32_t prog, uint32_t zoff, uint32_t zmask_ev,
                  uint32_t aff_off, uint32_t push_off, uint32_t wide_off) {
    return e.tile_start == tile_start && e.ntiles_lead == ((uint32_t)nt | ((uint32_t)lead << 30)) && e.pos0 == pos0 && e.adj_off == adj_off &&
           e.prog == prog && e.zoff == zoff && e.zmask_ev == zmask_ev && e.aff_off == aff_off && e.push_off == push_off && e.wide_off == wide_off;
}
static bool padding(const SegTable &t) {          // entries beyond n carry tile_start = ntiles
    for (int i = t.n; i < NSK_SEG_MAX; i++) if (t.e[i].tile_start != t.ntiles) return false;
    return t.n >= 1 && t.n <= NSK_SEG_MAX;
}

// a launch's quads: the whole wide ones and the listed rest are all of them, each once (restated from the kernels' rule:
// a quad is sampled as a wide one when its descriptor is marked and all four of its tiles are the entry's)
static void check_quads(const Compiled &c, const SegTable &t, int nch, uint32_t nrest, const uint32_t *rest, bool listed) {
    std::map<int, int> seen;
    int others = 0;
    for (int i = 0; i < t.n; i++) {
        const SegEntry &e = t.e[i];
        const int end = i + 1 < NSK_SEG_MAX ? t.e[i + 1].tile_start : t.ntiles;
        const int lead = (int)(e.ntiles_lead >> 30), nt = (int)(e.ntiles_lead & 0x3FFFFFFFu);
        assert(e.tile_start % 4 == 0 && end % 4 == 0 && end - e.tile_start == ((nt + lead + 3) & ~3) && lead == ((e.pos0 / 64) & 3));
        for (int Q = e.tile_start / 4; Q < end / 4; Q++) {
            const int first = 4 * Q - e.tile_start - lead;            // the quad's first tile, counted in the entry's own tiles
            const bool whole = first >= 0 && first + 4 <= nt;
            const bool marked = e.wide_off != NO && c.seg_wide[e.wide_off + (size_t)(Q - e.tile_start / 4) * NSK_WIDE_STRIDE(nch)] != 0xFFFFFFFFu;
            if (marked && whole) seen[Q]++; else others++;
        }
    }
    if (!listed || others > NSK_TABW_REST_MAX) { assert(nrest == 0); return; }
    assert((int)nrest == others);
    for (uint32_t k = 0; k < nrest; k++) seen[(int)(rest[k] & 0x7FFFFFFFu)]++;
    assert((int)seen.size() == t.ntiles / 4);
    for (const auto &kv : seen) assert(kv.first >= 0 && kv.first < t.ntiles / 4 && kv.second == 1);
}

// the invariants of every inference case
static SegPlans planned(const Compiled &c, const SegPlanOpts &o) {
    const SegPlans r = plan_segments(c, o);
    assert(r.by_class.size() == c.phase_start.size() - 1);
    bool all_tab = true, all_wide = true;
    for (size_t ph = 0; ph < r.by_class.size(); ph++) {
        std::map<int64_t, int> cover;               // tile (position / 64) -> entries that hold it
        for (const SegLaunchPlan &pl : r.by_class[ph]) {
            const SegTable &t = pl.tab;
            assert(padding(t) && (pl.nch == 1 || pl.nch == 2) && (pl.kind == 0 || (pl.kind >= 2 && pl.kind <= 4) || pl.kind == 8));
            int vt = 0;
            for (int i = 0; i < t.n; i++) {
                const SegEntry &e = t.e[i];
                const int lead = (int)(e.ntiles_lead >> 30), nt = (int)(e.ntiles_lead & 0x3FFFFFFFu);
                assert(e.tile_start == vt && nt > 0 && e.pos0 % 64 == 0);       // disjoint virtual ranges, in order
                assert(pl.kind == 8 ? lead == ((e.pos0 / 64) & 3) : lead == 0);
                vt += pl.kind == 8 ? (nt + lead + 3) & ~3 : nt;
                for (int k = 0; k < nt; k++) cover[e.pos0 / 64 + k]++;
                if (pl.kind < 8) assert(e.aff_off == NO && e.push_off == NO);
                if (!o.fused) assert(e.push_off == NO);
            }
            assert(t.ntiles == vt && (t.wide == 0 || t.wide == 1));
            assert(pl.grid > 0 && pl.grid % 8 == 0 && pl.front % 8 == 0 && pl.front == (int)((pl.nrest + 7) / 8 * 8));
            if (pl.kind < 8) assert(pl.grid >= (t.ntiles + 3) / 4 && pl.grid < (t.ntiles + 3) / 4 + 8);
            if (t.wide) {
                assert(pl.kind == 8 && pl.wide_grid > 0 && pl.wide_grid % 8 == 0 && o.offsets_fit && !o.no_wide_kernel);
                check_quads(c, t, pl.nch, pl.nrest, pl.rest, !o.no_tabw_rest);
            } else assert(pl.nrest == 0 && pl.wide_grid == 0 && pl.front == 0);
            all_tab = all_tab && pl.kind == 8;
            all_wide = all_wide && pl.kind == 8 && t.wide;
        }
        size_t want = 0;
        for (const Compiled::Segment &sg : c.segments)
            if (sg.phase == (int)ph && (sg.ev == 0 || o.sample_evidence))
                for (int k = 0; k < sg.ntiles; k++, want++) assert(cover[sg.pos0 / 64 + k] == 1);
        assert(cover.size() == want);
    }
    assert(r.all_tab == all_tab && r.all_wide == all_wide);
    return r;
}

static void inference() {
    SegPlanOpts o;
    {   // two unequal segments of one (kind, chunks): largest first, cumulative tile_start, padding entries
        Compiled c = two_classes();
        add(c, 0, 0, 3, 3, 4, 0, -1, -1, -1, 100, 7);
        add(c, 0, 192, 5, 3, 3, 0, -1, -1, -1, 292, 9);
        const SegPlans r = planned(c, o);
        assert(r.by_class[0].size() == 1 && r.by_class[1].empty());
        const SegLaunchPlan &p = r.by_class[0][0];
        assert(p.kind == 3 && p.nch == 1 && p.tab.n == 2 && p.tab.ntiles == 8 && p.tab.wide == 0 && p.grid == 8 && p.wide_grid == 0 && p.front == 0);
        assert(entry(p.tab.e[0], 0, 5, 0, 192, 292, 9, 0, 7, NO, NO, NO) && entry(p.tab.e[1], 5, 3, 0, 0, 100, 7, 0, 15, NO, NO, NO));
        for (int i = 2; i < 8; i++) assert(p.tab.e[i].tile_start == 8);
        assert(r.first_phase == 0 && r.border_total == 0 && r.border_all && !r.all_tab && !r.all_wide);
    }
    {   // nine segments of 1 .. 9 tiles in class 1: two launches, 8 + 1
        Compiled c = two_classes();
        int64_t pos = 0;
        for (int n = 1; n <= 9; n++) { add(c, 1, pos, n, 0, 2); pos += 64 * n; }
        const SegPlans r = planned(c, o);
        assert(r.by_class[0].empty() && r.by_class[1].size() == 2 && r.first_phase == 1);
        const SegTable &a = r.by_class[1][0].tab, &b = r.by_class[1][1].tab;
        const int start[8] = {0, 9, 17, 24, 30, 35, 39, 42};
        assert(a.n == 8 && a.ntiles == 44 && b.n == 1 && b.ntiles == 1 && r.by_class[1][0].grid == 16 && r.by_class[1][1].grid == 8);
        for (int i = 0; i < 8; i++) assert(a.e[i].tile_start == start[i] && a.e[i].ntiles_lead == (uint32_t)(9 - i));
        assert(entry(b.e[0], 0, 1, 0, 0, 0, 0, 0, 3, NO, NO, NO));
    }
    for (int tabs = 0; tabs < 2; tabs++) {   // kinds 0 .. 4 and a segment with a draw table: kind 1 batches with 3; kind 8 only under use_tab
        Compiled c = two_classes();
        const int64_t w = quads(c, "w");
        add(c, 0, 0, 1, 0, 4);
        add(c, 0, 64, 2, 1, 4);
        add(c, 0, 192, 1, 2, 4);
        add(c, 0, 256, 1, 3, 4);
        add(c, 0, 320, 3, 4, 4);
        add(c, 0, 1024, 4, 2, 4, 0, 5, 40, w, 600, 11);
        o.use_tab = tabs != 0;
        const SegPlans r = planned(c, o);
        const std::vector<SegLaunchPlan> &v = r.by_class[0];
        assert(v.size() == (tabs ? 5u : 4u) && !r.all_tab && !r.all_wide);
        assert(v[0].kind == 0 && v[1].kind == 2 && v[2].kind == 3 && v[3].kind == 4);
        assert(v[0].tab.n == 1 && v[3].tab.n == 1 && entry(v[3].tab.e[0], 0, 3, 0, 320, 0, 0, 0, 15, NO, NO, NO));
        assert(v[2].tab.n == 2 && v[2].tab.ntiles == 3 && v[2].tab.e[0].pos0 == 64 && v[2].tab.e[1].pos0 == 256);      // kind 1 in front of kind 3
        if (tabs) {
            assert(v[1].tab.n == 1 && v[4].kind == 8 && v[4].nch == 1 && v[4].tab.n == 1 && v[4].tab.ntiles == 4 && v[4].tab.wide == 1);
            assert(entry(v[4].tab.e[0], 0, 4, 0, 1024, 600, 11, 5, 15u | 1u << 16, 40, NO, (uint32_t)w));
            assert(v[4].grid == 8 && v[4].wide_grid == 8 && v[4].nrest == 0 && v[4].front == 0);
        } else {        // among the kind-2 segments, in front (4 tiles against 1): it keeps wide_off and bit 16, and has no implicit adjacency
            assert(v[1].tab.n == 2 && v[1].tab.ntiles == 5 && v[1].tab.wide == 0 && v[1].grid == 8);
            assert(entry(v[1].tab.e[0], 0, 4, 0, 1024, 600, 11, 5, 15u | 1u << 16, NO, NO, (uint32_t)w));
            assert(entry(v[1].tab.e[1], 4, 1, 0, 192, 0, 0, 0, 15, NO, NO, NO));
        }
        o.use_tab = true;
    }
    {   // 4 and 5 slots: separate launches; a run with t0 > 0 (fused, border tile 17): adj_off and aff_off scaled by the chunk count
        Compiled c = two_classes();
        add(c, 0, 0, 4, 3, 4, 0, 3, -1, -1, 500, 1);
        add(c, 0, 1024, 4, 3, 5, 0, 9, 200, -1, 1000, 2);
        const std::vector<int32_t> bt = {17};
        o.fused = true; o.border_tiles = &bt;
        const SegPlans r = planned(c, o);
        const std::vector<SegLaunchPlan> &v = r.by_class[0];
        assert(v.size() == 2 && v[0].kind == 8 && v[0].nch == 1 && v[1].kind == 8 && v[1].nch == 2 && r.all_tab && !r.all_wide);
        assert(v[0].tab.n == 1 && v[0].tab.ntiles == 4 && entry(v[0].tab.e[0], 0, 4, 0, 0, 500, 1, 3, 15u | 1u << 16, NO, NO, NO));
        const SegTable &t = v[1].tab;
        const uint32_t zm = 31u | 1u << 16;
        assert(t.n == 3 && t.ntiles == 12 && t.wide == 0);
        assert(entry(t.e[0], 0, 1, 1, 1088, 1000 + 1 * 64 * 2, 2, 9, zm, 200 + 1 * 2, 0, NO));
        assert(entry(t.e[1], 4, 2, 2, 1152, 1000 + 2 * 64 * 2, 2, 9, zm, 200 + 2 * 2, NO, NO));
        assert(entry(t.e[2], 8, 1, 0, 1024, 1000, 2, 9, zm, 200, NO, NO));
        assert(r.border_total == 1 && r.border_all && r.first_phase == 0);
        o.fused = false; o.border_tiles = nullptr;
    }
    for (int se = 0; se < 2; se++) {   // an evidence segment is included only with sample_evidence; first_phase
        Compiled c = two_classes();
        add(c, 0, 0, 2, 3, 2, 1);
        add(c, 1, 4096, 2, 3, 2, 0);
        o.sample_evidence = se != 0;
        const SegPlans r = planned(c, o);
        assert(r.by_class[0].size() == (se ? 1u : 0u) && r.by_class[1].size() == 1 && r.first_phase == (se ? 0 : 1));
        if (se) assert(entry(r.by_class[0][0].tab.e[0], 0, 2, 0, 0, 0, 0, 0, 3u | 1u << 8, NO, NO, NO));
        o.sample_evidence = false;
    }
    {   // lead 0, 1, 2, 3: virtual tiles in whole quads; 8, 7, 5 and 6 tiles -> 8, 8, 8 and 12 virtual ones
        Compiled c = two_classes();
        const int64_t w0 = quads(c, "ww"), w1 = quads(c, "ww"), w2 = quads(c, "ww"), w3 = quads(c, "www");
        add(c, 1, 0, 8, 3, 4, 0, 0, -1, w0);
        add(c, 1, 4160, 7, 3, 4, 0, 0, -1, w1);
        add(c, 1, 8320, 5, 3, 4, 0, 0, -1, w2);
        add(c, 1, 12480, 6, 3, 4, 0, 0, -1, w3);
        const SegPlans r = planned(c, o);
        assert(r.by_class[1].size() == 1);
        const SegTable &t = r.by_class[1][0].tab;
        const uint32_t zm = 15u | 1u << 16;
        assert(t.n == 4 && t.ntiles == 36 && t.wide == 0);         // whole wide quads 2 + 1 + 1 + 0: 32 < 36
        assert(entry(t.e[0], 0, 8, 0, 0, 0, 0, 0, zm, NO, NO, (uint32_t)w0) && entry(t.e[1], 8, 7, 1, 4160, 0, 0, 0, zm, NO, NO, (uint32_t)w1));
        assert(entry(t.e[2], 16, 6, 3, 12480, 0, 0, 0, zm, NO, NO, (uint32_t)w3) && entry(t.e[3], 28, 5, 2, 8320, 0, 0, 0, zm, NO, NO, (uint32_t)w2));
        assert(r.by_class[1][0].grid == 8 && r.all_tab && !r.all_wide);
    }
    {   // 16 tiles: wide with exactly half the virtual tiles in whole wide quads, not with one quad fewer
        Compiled c = two_classes();
        const int64_t w = quads(c, "ww..");
        add(c, 0, 0, 16, 3, 4, 0, 2, 30, w);
        SegPlans r = planned(c, o);
        const SegLaunchPlan &p = r.by_class[0][0];
        assert(p.tab.wide == 1 && p.tab.ntiles == 16 && p.nrest == 2 && p.rest[0] == 2 && p.rest[1] == 3 && p.front == 8 && p.wide_grid == 8 && p.grid == 8);
        assert(entry(p.tab.e[0], 0, 16, 0, 0, 0, 0, 2, 15u | 1u << 16, 30, NO, (uint32_t)w) && r.all_wide);
        // ... nor when an offset does not fit, nor under the switch
        o.offsets_fit = false;
        r = planned(c, o);
        assert(r.by_class[0][0].tab.wide == 0 && r.by_class[0][0].nrest == 0 && r.by_class[0][0].wide_grid == 0 && r.all_tab && !r.all_wide);
        o.offsets_fit = true; o.no_wide_kernel = true;
        r = planned(c, o);
        assert(r.by_class[0][0].tab.wide == 0 && r.by_class[0][0].tab.e[0].wide_off == (uint32_t)w);
        o.no_wide_kernel = false;
        c.seg_wide[8] = 0xFFFFFFFFu;            // "w..."
        r = planned(c, o);
        assert(r.by_class[0][0].tab.wide == 0 && r.by_class[0][0].tab.e[0].wide_off == (uint32_t)w && !r.all_wide);
        c.seg_wide[0] = 0xFFFFFFFFu;            // "....": no wide quad, the kernels need not look
        r = planned(c, o);
        assert(r.by_class[0][0].tab.wide == 0 && r.by_class[0][0].tab.e[0].wide_off == NO);
    }
    {   // rest list: tiles 1 .. 29 -- a lead quad (marked), a quad that is not marked, a tail quad (marked): bit 31 on the marked ones
        Compiled c = two_classes();
        const int64_t w = quads(c, "ww.wwwww");
        add(c, 0, 64, 29, 3, 4, 0, 2, -1, w);
        const SegPlans r = planned(c, o);
        const SegLaunchPlan &p = r.by_class[0][0];
        assert(p.tab.wide == 1 && p.tab.ntiles == 32 && p.tab.e[0].ntiles_lead == (29u | 1u << 30));        // 5 whole wide quads: 40 >= 32
        assert(p.nrest == 3 && p.rest[0] == 0x80000000u && p.rest[1] == 2u && p.rest[2] == 0x80000007u && p.front == 8 && p.wide_grid == 8);
    }
    for (int n = 64; n <= 65; n++) {   // n quads that are not wide in front of n wide ones: 64 are listed, 65 are not
        Compiled c = two_classes();
        const int64_t w = quads(c, std::string((size_t)n, '.') + std::string((size_t)n, 'w'));
        add(c, 0, 0, 8 * n, 3, 4, 0, 2, -1, w);
        SegPlans r = planned(c, o);
        const SegLaunchPlan &p = r.by_class[0][0];
        assert(p.tab.wide == 1 && p.tab.ntiles == 8 * n && p.nrest == (n == 64 ? 64u : 0u) && p.front == (n == 64 ? 64 : 0) && p.wide_grid == 40);
        if (n == 64) for (uint32_t k = 0; k < 64; k++) assert(p.rest[k] == k);
        o.no_tabw_rest = true;
        r = planned(c, o);
        assert(r.by_class[0][0].tab.wide == 1 && r.by_class[0][0].nrest == 0 && r.by_class[0][0].front == 0 && r.by_class[0][0].wide_grid == 40);
        o.no_tabw_rest = false;
    }
    {   // fused split: tiles 4 .. 13, border tiles 6, 7 and 11 -> five runs, the border runs first, then larger first, stably
        Compiled c = two_classes();
        const int64_t w = quads(c, "www");
        add(c, 1, 256, 10, 3, 4, 0, 6, 50, w, 700, 3);
        const std::vector<int32_t> bt = {6, 7, 11};
        o.fused = true; o.border_tiles = &bt;
        const SegPlans r = planned(c, o);
        assert(r.by_class[1].size() == 1);
        const SegTable &t = r.by_class[1][0].tab;
        const uint32_t zm = 15u | 1u << 16, W = (uint32_t)w;
        assert(t.n == 5 && t.ntiles == 20 && t.wide == 0);
        assert(entry(t.e[0], 0, 2, 2, 384, 700 + 2 * 64, 3, 6, zm, 52, 0, W));
        assert(entry(t.e[1], 4, 1, 3, 704, 700 + 7 * 64, 3, 6, zm, 57, 2, W + 8));          // (wide_off from the run's quad on)
        assert(entry(t.e[2], 8, 3, 0, 512, 700 + 4 * 64, 3, 6, zm, 54, NO, W + 8));
        assert(entry(t.e[3], 12, 2, 0, 256, 700, 3, 6, zm, 50, NO, W));
        assert(entry(t.e[4], 16, 2, 0, 768, 700 + 8 * 64, 3, 6, zm, 58, NO, W + 16));
        assert(r.border_total == 3 && r.border_all && r.first_phase == 1 && r.all_tab);
        o.fused = false;           // not fused: one run, no push rows
        const SegPlans q = planned(c, o);
        assert(q.by_class[1][0].tab.n == 1 && q.border_total == 0 && !q.border_all);        // (three border tiles no launch pushes)
        o.border_tiles = nullptr;
    }
    {   // a border tile in an evidence segment this call does not sample: the fused exchange cannot run
        Compiled c = two_classes();
        add(c, 0, 0, 4, 3, 4, 0, 2);
        add(c, 0, 1024, 4, 3, 4, 1, 2);
        const std::vector<int32_t> bt = {2, 17};
        o.fused = true; o.border_tiles = &bt;
        SegPlans r = planned(c, o);
        assert(!r.border_all && r.border_total == 1 && r.first_phase == 0);
        o.sample_evidence = true;
        r = planned(c, o);
        assert(r.border_all && r.border_total == 2);
        o.sample_evidence = false; o.fused = false; o.border_tiles = nullptr;
    }
    {   // the only border tile in class 1: its launches wait, not those of class 0
        Compiled c = two_classes();
        add(c, 0, 0, 4, 3, 4, 0, 2);
        add(c, 1, 1024, 4, 3, 4, 0, 2);
        const std::vector<int32_t> bt = {18};
        o.fused = true; o.border_tiles = &bt;
        const SegPlans r = planned(c, o);
        assert(r.first_phase == 1 && r.border_all && r.border_total == 1 && r.by_class[1][0].tab.n == 3 && r.by_class[1][0].tab.e[0].push_off == 0);
        o.fused = false;
        assert(planned(c, o).first_phase == 0);
        o.border_tiles = nullptr;
    }
}

static void grids() {
    // k_gibbs_seg_tab: 8192 pairs need 2048 blocks (all of them, in pairs), 8194 need 2056 (the resident 1536); the diagnostic cap
    assert(nsk_tab_grid(16384, 0) == 2048 && nsk_tab_grid(16388, 0) == 1536 && nsk_tab_grid(16384, 8) == 8 && nsk_tab_grid(16388, 8) == 8);
    assert(nsk_tab_grid(4, 0) == 8 && nsk_tab_grid(4, 64) == 8);
    // k_gibbs_seg_tabw: 6 x 256 resident blocks; 6100 quads need 1528, 6128 need 1536, 6200 need 1552
    assert(nsk_tabw_grid(4 * 6100, 0) == 1528 && nsk_tabw_grid(4 * 6128, 0) == 1536 && nsk_tabw_grid(4 * 6200, 0) == 1536);
    assert(nsk_tabw_grid(4 * 6200, 8) == 8 && nsk_tabw_grid(4, 0) == 8 && nsk_tabw_front_blocks(0) == 0 && nsk_tabw_front_blocks(1) == 8 &&
           nsk_tabw_front_blocks(64) == 64);
    // k_learn_seg_tab: 58 weights are one LDS trip, 59 two; 1528 blocks beside the service blocks, 1536 without
    assert(nsk_learn_tab_grid(16000, 58, true, 0) == 1528 && nsk_learn_tab_grid(16000, 59, true, 0) == 1000 && nsk_learn_tab_grid(16000, 59, false, 0) == 1536);
    assert(nsk_learn_tab_grid(100000, 59, true, 0) == 1528 && nsk_learn_tab_grid(100000, 2, false, 0) == 1536 && nsk_learn_tab_grid(20, 2, true, 0) == 8);
    assert(nsk_learn_tab_grid(16000, 2, true, 8) == 8 && nsk_learn_tab_grid(16000, 2, true, 60) == 64 && nsk_learn_tab_grid(0, 2, true, 0) == 8);
    // k_learn_seg_tabw: 1024 blocks below 40 000 quads (the 8 of the rounding included), 2048 from there on
    assert(nsk_learn_tabw_grid(4 * 39991, 0) == 1024 && nsk_learn_tabw_grid(4 * 39992, 0) == 2048 && nsk_learn_tabw_grid(4 * 39992, 8) == 8 &&
           nsk_learn_tabw_grid(16, 0) == 8);
    // a launch without draw tables: a wave per tile, at most 2048 blocks
    SegPlanOpts o;
    assert(nsk_learn_seg_grid(10, false, o) == 3 && nsk_learn_seg_grid(10000, false, o) == 2048 && nsk_learn_seg_grid(8192, false, o) == 2048 &&
           nsk_learn_seg_grid(8188, false, o) == 2047);
    o.nweight = 59; o.smallw = true;
    assert(nsk_learn_seg_grid(16000, true, o) == 1000);
    o.learn_grid_cap = 16;
    assert(nsk_learn_seg_grid(16000, true, o) == 16);
    // the switches as the drivers pass them in
    assert(seg_cap_rounds(nullptr) == 0 && seg_cap_rounds("8") == 8 && seg_cap_rounds("0") == 8 && seg_cap_rounds("-1536") == 1536 && seg_cap_rounds("21") == 16);
    assert(seg_cap_blocks(nullptr) == 0 && seg_cap_blocks("8") == 8 && seg_cap_blocks("0") == 1 && seg_cap_blocks("-3") == 1);
}

// one learning launch of `n` segments: tiles and first positions given, everything else counted up from the index
static Compiled::SegLaunch launch(int n, const int *ntiles, const int *pos0, const int64_t *wide, int tab = 1, int nch = 1) {
    Compiled::SegLaunch sl;
    memset(&sl, 0, sizeof(sl));
    sl.phase = 0; sl.kind = 3; sl.nch = nch; sl.n = n; sl.tab = tab;
    for (int i = 0; i < n; i++) {
        sl.tile_start[i + 1] = sl.tile_start[i] + ntiles[i];
        sl.pos0[i] = pos0[i]; sl.adj_off[i] = 100u + i; sl.prog[i] = 10u + i; sl.zoff[i] = 20u + i; sl.zmask[i] = 15u; sl.aff[i] = 30u + i;
        sl.ev[i] = i & 1; sl.wide[i] = wide ? wide[i] : -1;
    }
    for (int i = n; i < 8; i++) sl.tile_start[i + 1] = sl.tile_start[n];
    return sl;
}
static LearnSegPlan planned(const Compiled &c, const Compiled::SegLaunch &sl, const SegPlanOpts &o) {
    const LearnSegPlan p = plan_learn_segment(c, sl, o);
    const SegTable &t = p.tab;
    const bool use_tab = sl.tab && o.use_tab;
    assert(t.n == sl.n && padding(t) && t.wide == 0 && p.grid > 0);
    int real = 0;
    for (int i = 0; i < t.n; i++) {         // every tile of the launch in exactly one entry, in the launch's order
        const SegEntry &e = t.e[i];
        assert((int)(e.ntiles_lead & 0x3FFFFFFFu) == sl.tile_start[i + 1] - sl.tile_start[i] && e.pos0 == sl.pos0[i] && e.adj_off == sl.adj_off[i] &&
               e.prog == sl.prog[i] && e.zoff == sl.zoff[i] && e.zmask_ev == (15u | (uint32_t)(i & 1) << 8) && e.aff_off == (use_tab ? sl.aff[i] : NO));
        assert(e.tile_start + (int)(e.ntiles_lead & 0x3FFFFFFFu) + (int)(e.ntiles_lead >> 30) <= (i + 1 < NSK_SEG_MAX ? t.e[i + 1].tile_start : t.ntiles));
        real += (int)(e.ntiles_lead & 0x3FFFFFFFu);
    }
    assert(real == sl.tile_start[sl.n]);
    if (p.wide) {
        assert(use_tab && o.byte_values && !o.no_wide_learn && t.ntiles / 4 >= o.wide_learn_min_quads && p.grid % 8 == 0);
        check_quads(c, t, sl.nch, p.nrest, p.rest, !o.no_tabw_rest);
    } else {
        assert(p.nrest == 0 && (!use_tab || p.grid % 8 == 0));
        for (int i = 0; i < t.n; i++) assert(t.e[i].ntiles_lead >> 30 == 0);
    }
    return p;
}

static void learning() {
    SegPlanOpts o;
    o.nweight = 2; o.smallw = true; o.wide_learn_min_quads = 0;
    {   // 16 tiles: wide with two wide quads of four, tile by tile with one
        Compiled c = two_classes();
        const int nt[1] = {16}, pos[1] = {0};
        const int64_t w[1] = {quads(c, "ww..")};
        const Compiled::SegLaunch sl = launch(1, nt, pos, w);
        LearnSegPlan p = planned(c, sl, o);
        assert(p.wide && p.tab.ntiles == 16 && p.nrest == 2 && p.rest[0] == 2 && p.rest[1] == 3 && p.grid == 8 + 8);
        assert(entry(p.tab.e[0], 0, 16, 0, 0, 100, 10, 20, 15, 30, NO, (uint32_t)w[0]));
        o.wide_learn_min_quads = 4; assert(planned(c, sl, o).wide);
        o.wide_learn_min_quads = 5; assert(!planned(c, sl, o).wide);
        o.wide_learn_min_quads = 0;
        o.no_wide_learn = true; assert(!planned(c, sl, o).wide); o.no_wide_learn = false;
        o.byte_values = false; assert(!planned(c, sl, o).wide); o.byte_values = true;           // int32 values
        o.no_tabw_rest = true; p = planned(c, sl, o); assert(p.wide && p.nrest == 0 && p.grid == 8); o.no_tabw_rest = false;
        o.learn_tabw_grid_cap = 8; assert(planned(c, sl, o).grid == 16); o.learn_tabw_grid_cap = 0;
        c.seg_wide[8] = 0xFFFFFFFFu;            // "w...": tile by tile, the entry as the table kernel reads it
        p = planned(c, sl, o);
        assert(!p.wide && p.tab.ntiles == 16 && p.grid == 8 && entry(p.tab.e[0], 0, 16, 0, 0, 100, 10, 20, 15, 30, 0, 0));
    }
    {   // a lead tile in front: the launch's whole wide quads only (tiles 1 .. 12: quads 1 and 2 of 4), 16 >= 16
        Compiled c = two_classes();
        const int nt[1] = {12}, pos[1] = {64};
        const int64_t w[1] = {quads(c, "wwww")};
        const LearnSegPlan p = planned(c, launch(1, nt, pos, w), o);
        assert(p.wide && p.tab.ntiles == 16 && p.tab.e[0].ntiles_lead == (12u | 1u << 30) && p.nrest == 2 && p.rest[0] == 0x80000000u &&
               p.rest[1] == 0x80000003u);
    }
    {   // the default threshold of 12 000 quads: 48 000 tiles are wide, 47 996 are not
        o.wide_learn_min_quads = NSK_WIDE_LEARN_MIN_QUADS;
        Compiled c = two_classes();
        const int pos[1] = {0};
        const int64_t w[1] = {quads(c, std::string(12000, 'w'))};
        const int big[1] = {48000}, small[1] = {47996};
        const LearnSegPlan p = planned(c, launch(1, big, pos, w), o);
        assert(p.wide && p.tab.ntiles == 48000 && p.nrest == 0 && p.grid == 1024);
        const LearnSegPlan q = planned(c, launch(1, small, pos, w), o);
        assert(!q.wide && q.tab.ntiles == 47996 && q.grid == 1528);
        o.wide_learn_min_quads = 0;
    }
    {   // tile by tile: segments of 3 and 5 tiles are padded to whole trips of two under use_tab, and keep their real numbering without
        Compiled c = two_classes();
        const int nt[2] = {3, 5}, pos[2] = {0, 1024};
        const Compiled::SegLaunch sl = launch(2, nt, pos, nullptr);
        LearnSegPlan p = planned(c, sl, o);
        assert(!p.wide && p.tab.ntiles == 10 && p.tab.e[0].tile_start == 0 && p.tab.e[1].tile_start == 4 && p.tab.e[2].tile_start == 10 && p.grid == 8);
        assert(entry(p.tab.e[1], 4, 5, 0, 1024, 101, 11, 21, 15u | 1u << 8, 31, 0, 0));
        o.use_tab = false;
        p = planned(c, sl, o);
        assert(!p.wide && p.tab.ntiles == 8 && p.tab.e[0].tile_start == 0 && p.tab.e[1].tile_start == 3 && p.tab.e[2].tile_start == 8 && p.grid == 2);
        assert(entry(p.tab.e[1], 3, 5, 0, 1024, 101, 11, 21, 15u | 1u << 8, NO, 0, 0));
        o.use_tab = true;
        const Compiled::SegLaunch plain = launch(2, nt, pos, nullptr, 0);       // a launch without draw tables: the same whatever use_tab
        p = planned(c, plain, o);
        assert(p.tab.ntiles == 8 && p.tab.e[1].tile_start == 3 && p.tab.e[0].aff_off == NO && p.grid == 2);
    }
    {   // the table grid counts the launch's real tiles: 7 x 9 + 1 = 64 tiles are 8 blocks, the 72 padded ones would be 9
        Compiled c = two_classes();
        const int nt[8] = {9, 9, 9, 9, 9, 9, 9, 1};
        int pos[8];
        for (int i = 0; i < 8; i++) pos[i] = 1024 * i;
        const LearnSegPlan p = planned(c, launch(8, nt, pos, nullptr), o);
        assert(!p.wide && p.tab.n == 8 && p.tab.ntiles == 72 && p.tab.e[7].tile_start == 70 && p.grid == 8);
    }
}

// options that differ compare unequal
static void options() {
    const SegPlanOpts a;
    const std::vector<int32_t> bt;
    SegPlanOpts b;
    assert(a == b);
#define DIFFERS(FIELD, VALUE) b = a; b.FIELD = VALUE; assert(!(a == b) && !(b == a)); b = a; assert(a == b)
    DIFFERS(sample_evidence, true); DIFFERS(use_tab, false); DIFFERS(byte_values, false); DIFFERS(offsets_fit, false);
    DIFFERS(fused, true); DIFFERS(border_tiles, &bt); DIFFERS(no_wide_kernel, true); DIFFERS(no_tabw_rest, true);
    DIFFERS(tab_grid_cap, 8); DIFFERS(tabw_grid_cap, 8);
    DIFFERS(nweight, 3); DIFFERS(smallw, true); DIFFERS(wide_learn_min_quads, 0); DIFFERS(no_wide_learn, true);
    DIFFERS(learn_grid_cap, 8); DIFFERS(learn_tabw_grid_cap, 8);
#undef DIFFERS
}

int main() {
    inference();
    grids();
    learning();
    options();
    std::puts("segment plans ok");
    return 0;
}
"""


def test_segment_plans_under_sanitizers(tmp_path):
    cxx, san = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    src, exe = tmp_path / "seg_plan_main.cpp", tmp_path / "seg_plan_main"
    src.write_text(PROGRAM)
    cmd = cxx + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread"] + san + ["-I", CSRC, str(src), "-o", str(exe)]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:       # (a compiler without these switches)
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert "segment plans ok" in run.stdout
