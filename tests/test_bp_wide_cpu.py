"""The wide route of a belief-propagation set-up without a GPU: the arrays of bp_plan_wide (numbskull_amd/csrc/
nsk_bp_wide_plan.h) for one hand-written graph, asserted by a stand-alone program built under AddressSanitizer and
UndefinedBehaviorSanitizer as tests/test_bp_plan_cpu.py builds its own, and the rule in numpy
(diagnostics.bp_wide_factor) against the enumeration of a factor's table."""

import itertools
import subprocess

import numpy as np
import pytest

import bp_wide
from numbskull_amd.diagnostics import bp_wide_factor
from test_alloc_ledger_cpu import CSRC, _compiler

PROGRAM = r"""
#undef NDEBUG
#include <cassert>
#include <cstdio>
#include "nsk_bp_wide_plan.h"

using namespace nsk;
typedef std::vector<int32_t> I32;
typedef std::vector<long long> I64;

static Compiled graph(int nvar, const I32 &evidence) {
    Compiled c;
    c.nvar = c.nid = c.npos = nvar;
    c.nweight = 2;
    c.v_card_i.assign((size_t)nvar, 2);
    for (int v = 0; v < nvar; v++) { c.iid.push_back(v); c.p_info.push_back(0x300u); }
    for (int32_t v : evidence) c.p_info[(size_t)v] |= 1u;
    return c;
}
static void factor(Compiled &c, int fn, const I32 &members) {
    const uint32_t rec[4] = {(uint32_t)members.size() << 8 | (uint32_t)(fn + 1), (uint32_t)c.nedge, (uint32_t)(c.nfactor & 1), 0u};
    c.f_rec.insert(c.f_rec.end(), rec, rec + 4);
    for (int32_t m : members) { c.m_rec.push_back(m); c.m_rec.push_back(0); }
    c.nedge = (int64_t)c.m_rec.size() / 2;
    c.nfactor++;
}
static std::string plan(const Compiled &c, int wide_min, BpPlan &p, BpWidePlan &wp) {
    return bp_plan_wide(c, 0, NSK_BP_MAX_MEMBERS, NSK_BP_MAX_TABLE, 16, wide_min, NSK_BP_WIDE_MAX_MEMBERS, p, wp);
}

int main() {
    // 20 binary variables, 2 and 5 evidence: a pair factor, an AND over 18 positions that names the clamped 2 twice, a
    // unary factor, an OR over three that goes wide only under wide_min = 3
    Compiled c = graph(20, {2, 5});
    factor(c, 3, {0, 1});
    I32 wide = {2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 2};
    factor(c, 2, wide);
    factor(c, 4, {3});
    factor(c, 1, {0, 5, 19});
    BpPlan p, q;
    BpWidePlan wp, wq;
    assert(plan(c, 17, p, wp).empty());
    assert(wp.nwide == 1 && wp.max_positions == 18 && (wp.rec == I32{1, 2, 1, 0}) && (wp.pos_off == I32{0, 18}));
    assert((wp.pos == I32{-3, 2, 3, -6, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, -3}));
    assert((wp.narrow == I32{0, 1, 17, 18, 19}));
    assert((p.edge_off == I32{0, 2, 17, 18, 20}) && (p.tab_off == I64{0, 4, 4, 6, 10}) && (p.pm_off == I64{0, 2, 2, 3, 6}));
    assert(p.e_fac.size() == 20 && p.e_fac[2] == 1 && p.e_var[2] == 3 && p.e_fac[16] == 1 && p.e_var[16] == 18 && p.e_var[17] == 3);
    assert(p.msg_off.back() == 40 && p.info.nedges == 20 && p.info.ntable == 10 && p.info.max_table == 4);
    assert((I32(p.v_edges.begin(), p.v_edges.begin() + 5) == I32{0, 18, 1, 2, 17}));      // variables 0, 1, 3
    // wide_min = 3: the OR goes wide too; the AND's refusal-free twin through bp_plan is the table route's refusal
    assert(plan(c, 3, q, wq).empty() && wq.nwide == 2 && (wq.rec == I32{1, 2, 1, 0, 3, 1, 1, 18}) && (wq.pos_off == I32{0, 18, 21}));
    assert(wq.pos[18] == 18 && wq.pos[19] == -6 && wq.pos[20] == 19 && (wq.narrow == I32{0, 1, 17}) && (q.tab_off == I64{0, 4, 4, 6, 6}));
    assert(bp_plan(c, 0, NSK_BP_MAX_MEMBERS, NSK_BP_MAX_TABLE, 16, q) == "nsk_bp_setup: factor 1 has more than NSK_BP_MAX_MEMBERS = 16 distinct members");
    // without a factor beyond the caps: bp_plan's arrays
    Compiled d = graph(4, {1});
    factor(d, 3, {0, 1});
    factor(d, 2, {1, 2, 3, 2});
    assert(plan(d, 17, p, wp).empty() && bp_plan(d, 0, NSK_BP_MAX_MEMBERS, NSK_BP_MAX_TABLE, 16, q).empty() && wp.nwide == 0);
    assert(p.mrec == q.mrec && p.slot_rec == q.slot_rec && p.tab_off == q.tab_off && p.msg_off == q.msg_off && p.v_edges == q.v_edges &&
           p.e_fac == q.e_fac && p.e_var == q.e_var && p.v_list == q.v_list && p.v_eoff == q.v_eoff && p.b_off == q.b_off);
    // the refusals of the wide route name the factor
    wide[17] = 3;
    Compiled e = graph(20, {2, 5});
    factor(e, 3, {0, 1});
    factor(e, 2, wide);
    assert(plan(e, 17, p, wp) == "nsk_bp_setup: factor 1 names a free member twice on the wide route");
    Compiled f = graph(20, {7});                    // (the clamped 7 fills the positions from 20 on)
    factor(f, 2, I32(2049, 7));
    for (int i = 0; i < 20; i++) f.m_rec[2 * (size_t)i] = i;
    assert(plan(f, 17, p, wp) == "nsk_bp_setup: factor 0 has more than NSK_BP_WIDE_MAX_MEMBERS = 2048 member positions on the wide route");
    std::puts("bp wide plan ok");
    return 0;
}
"""


def test_the_wide_plan_under_sanitizers(tmp_path):
    cxx, san = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    src, exe = tmp_path / "bp_wide_plan_main.cpp", tmp_path / "bp_wide_plan_main"
    src.write_text(PROGRAM)
    cmd = cxx + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread"] + san + ["-I", CSRC, str(src), "-o", str(exe)]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:       # (a compiler without these switches)
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert "bp wide plan ok" in run.stdout


@pytest.mark.parametrize("fn", bp_wide.FUNCTIONS)
def test_the_rule_in_numpy_against_enumeration(fn):
    n, w = 6, 0.8 if fn != 1 else -0.8
    rng = np.random.default_rng(fn)
    nu = rng.uniform(0.1, 1.0, (n, 2))
    nu /= nu.sum(1, keepdims=True)
    clamped = np.array([-1, 1, -1, -1, 0 if fn in (1, 9) else 1, -1])      # one delta message of each kind the pattern survives
    old = rng.uniform(0.0, 1.0, (n, 2))
    ind = nu.copy()
    ind[clamped >= 0] = np.eye(2)[clamped[clamped >= 0]]
    x = np.array(list(itertools.product((0, 1), repeat=n)))
    theta = w * bp_wide.feature(fn, x)
    joint = np.exp(theta - theta.max()) * np.prod(ind[np.arange(n), x], axis=1)
    msg, term = bp_wide_factor(fn, w, nu, clamped, damping=0.25, old=old)
    for j in np.nonzero(clamped < 0)[0]:
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.array([np.sum(np.where(x[:, j] == k, joint / ind[j, k], 0.0)) for k in (0, 1)])
        assert np.abs(0.75 * (m / m.sum()) + 0.25 * old[j] - msg[j]).max() <= 4e-15
    b = joint / joint.sum()
    assert abs(np.sum(b[b > 0] * (theta[b > 0] - np.log(b[b > 0]))) - term) <= 2e-14
    assert (msg[clamped >= 0] == 0).all()
