"""What the host side of the full-batch learners shares is pure (numbskull_amd/csrc/nsk_steps.h): the checks of the step
parameters, the slot map, the factor counts by slot and the cut of the by-weight list with the work items the statistics
and the moments make of it.  A stand-alone program asserts each against values worked out by hand from the rules as they
stood in nsk_pcd.hip, nsk_bp.hip and nsk_wstats.hip before the header existed: the cut at lengths 0, 1, 16, 17, 2048,
2049 and 5000, two weights of equal length whose first factors are out of order and a list that names one slot twice; the
statistics' single / partial / multi items and the moments' slot-tagged pieces; the slot map with and without a
renumbering; every boundary of the checks with nsk_pcd_steps' message texts.  Built with the host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer (-fno-sanitize-recover); a clean exit is the pass."""

import subprocess

import pytest

from test_alloc_ledger_cpu import CSRC, _compiler

PROGRAM = r"""
#undef NDEBUG
#include <cassert>
#include <cstdio>
#include <limits>
#include "nsk_steps.h"

using namespace nsk;

static bool same(const std::vector<WeightCutShort> &a, const std::vector<WeightCutShort> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) if (a[i].off != b[i].off || a[i].tag != b[i].tag) return false;
    return true;
}
static bool same(const std::vector<WeightCutLong> &a, const std::vector<WeightCutLong> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) if (a[i].off != b[i].off || a[i].len != b[i].len || a[i].tag != b[i].tag) return false;
    return true;
}
static bool same(const std::vector<WeightItem> &a, const std::vector<WeightItem> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) if (a[i].x != b[i].x || a[i].y != b[i].y || a[i].z != b[i].z || a[i].w != b[i].w) return false;
    return true;
}
static bool ends(const WeightCut &c, unsigned int upto1, unsigned int upto2, unsigned int upto15, unsigned int upto16) {
    if (c.len_end.size() != 16) return false;
    for (int k = 0; k < 16; k++)
        if (c.len_end[k] != (k == 0 ? upto1 : k == 1 ? upto2 : k < 15 ? upto15 : upto16)) return false;
    return true;
}

// slots 0 .. 8 of 0, 1, 16, 17, 2048, 2049, 5000, 3 and 3 factors; slot 8's first factor lies before slot 7's
static const std::vector<uint32_t> OFF = {0, 0, 1, 17, 34, 2082, 4131, 9131, 9134, 9137};
static const std::vector<int32_t> FIRST = {0, 40, 7, 5, 9, 11, 2, 90, 20};

static void the_cut() {
    {   // a list in another order than the slots' that names slot 1 twice: the tags are the columns
        const int32_t list[10] = {7, 8, 1, 2, 0, 3, 4, 5, 6, 1};
        const WeightCut c = weight_cut(OFF, FIRST, list, 10, 16);
        // length 1: both columns of slot 1, by tag; length 3: slot 8 (first factor 20) before slot 7 (90); length 16
        assert(same(c.shorts, {{0, 2}, {0, 9}, {9134, 1}, {9131, 0}, {1, 3}}));
        assert(ends(c, 2, 2, 4, 5));
        assert(same(c.longs, {{17, 17, 5}, {34, 2048, 6}, {2082, 2049, 7}, {4131, 5000, 8}}));
        // the statistics: 17 and 2048 entries are one piece that writes its column; 2049 are partials 0, 1 and 5000
        // partials 2, 3, 4, each added by a multi item
        const WstatsItems it = wstats_items(c, 2048);
        assert(same(it.pieces, {{17, 17, 5, 0}, {34, 2048, 6, 0}, {2082, 2048, 0, 1}, {4130, 1, 1, 1},
                                {4131, 2048, 2, 1}, {6179, 2048, 3, 1}, {8227, 904, 4, 1}}));
        assert(same(it.multi, {{0, 2, 7, 0}, {2, 3, 8, 0}}) && it.npartial == 5);
    }
    {   // the list of every slot: the tags are the slots, the moments' pieces name them
        const int32_t all[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
        const WeightCut c = weight_cut(OFF, FIRST, all, 9, 16);
        assert(same(c.shorts, {{0, 1}, {9134, 8}, {9131, 7}, {1, 2}}));
        assert(ends(c, 1, 1, 3, 4));
        assert(same(c.longs, {{17, 17, 3}, {34, 2048, 4}, {2082, 2049, 5}, {4131, 5000, 6}}));
        assert(same(moments_items(c, 2048), {{17, 17, 3, 0}, {34, 2048, 4, 0}, {2082, 2048, 5, 0}, {4130, 1, 5, 0},
                                             {4131, 2048, 6, 0}, {6179, 2048, 6, 0}, {8227, 904, 6, 0}}));
    }
    {   // nothing but weights without a factor
        const int32_t list[2] = {0, 0};
        const WeightCut c = weight_cut(OFF, FIRST, list, 2, 16);
        assert(c.shorts.empty() && c.longs.empty() && ends(c, 0, 0, 0, 0));
        assert(moments_items(c, 2048).empty() && wstats_items(c, 2048).pieces.empty() && wstats_items(c, 2048).npartial == 0);
    }
}

static void the_slot_map() {
    Compiled c;
    c.nweight = 4;
    const double src[4] = {10, 11, 12, 13};
    const long long rows[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    for (int pass = 0; pass < 2; pass++) {
        if (pass) c.wmap = {2, 0, 3, 1};            // the caller's id -> slot
        const SlotMap m(c);
        double by_slot[4] = {-1, -1, -1, -1}, back[4] = {-1, -1, -1, -1};
        int64_t out[8];
        m.to_slots(src, by_slot);
        m.from_slots(by_slot, back);
        m.from_slots(rows, out, 2);
        const double want_slot[2][4] = {{10, 11, 12, 13}, {11, 13, 10, 12}};
        const int64_t want_rows[2][8] = {{0, 1, 2, 3, 4, 5, 6, 7}, {2, 0, 3, 1, 6, 4, 7, 5}};
        for (int i = 0; i < 4; i++) assert(by_slot[i] == want_slot[pass][i] && back[i] == src[i] && m.slot((size_t)i) == (pass ? (size_t)c.wmap[i] : (size_t)i));
        for (int i = 0; i < 8; i++) assert(out[i] == want_rows[pass][i]);
    }
    // the factors of the slots: the records' third word; a slot without a factor counts 1
    c.nfactor = 5;
    const uint32_t slots[5] = {1, 1, 3, 1, 0};
    for (uint32_t s : slots) { c.f_rec.push_back(0x101u); c.f_rec.push_back(0u); c.f_rec.push_back(s); c.f_rec.push_back(0u); }
    assert((factors_per_slot(c) == std::vector<double>{1.0, 3.0, 1.0, 1.0}));
}

static void the_checks() {
    const std::string who = "nsk_pcd_steps";
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    assert(check_nsteps(who, 0, 65536) == "nsk_pcd_steps: nsteps must lie in [1, 65536]");
    assert(check_nsteps(who, 1, 65536).empty() && check_nsteps(who, 65536, 65536).empty());
    assert(check_nsteps(who, 65537, 65536) == "nsk_pcd_steps: nsteps must lie in [1, 65536]");
    assert(check_nsteps("nsk_bp_learn_steps", 4097, 4096) == "nsk_bp_learn_steps: nsteps must lie in [1, 4096]");
    const std::string rates = "nsk_pcd_steps: step, decay and reg_param must be finite, reg_param not negative";
    assert(check_rates(who, 0.1, 0.9, 0.0).empty() && check_rates(who, -0.1, 0.0, 1e-3).empty());
    assert(check_rates(who, nan, 0.9, 0.0) == rates && check_rates(who, 0.1, inf, 0.0) == rates && check_rates(who, 0.1, 0.9, -inf) == rates);
    assert(check_rates(who, 0.1, 0.9, -1e-3) == rates && check_rates(who, 0.1, 0.9, nan) == rates);
    assert(check_normalize(who, 0).empty() && check_normalize(who, 1).empty());
    assert(check_normalize(who, 2) == "nsk_pcd_steps: normalize must be 0 or 1" && check_normalize(who, -1) == "nsk_pcd_steps: normalize must be 0 or 1");
    const double target[3] = {0.5, inf, nan};
    assert(check_target(who, target, 1).empty() && check_target(who, target, 0).empty());
    assert(check_target(who, target, 3) == "nsk_pcd_steps: the target of weight 1 is not finite");
    assert(check_target(who, target + 2, 1) == "nsk_pcd_steps: the target of weight 0 is not finite");
}

int main() {
    the_cut();
    the_slot_map();
    the_checks();
    std::puts("steps ok");
    return 0;
}
"""


def test_the_step_scaffold_under_sanitizers(tmp_path):
    cxx, san = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    src, exe = tmp_path / "steps_main.cpp", tmp_path / "steps_main"
    src.write_text(PROGRAM)
    cmd = cxx + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread"] + san + ["-I", CSRC, str(src), "-o", str(exe)]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:       # (a compiler without these switches)
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert "steps ok" in run.stdout
