"""Latent-variable learning by belief propagation, the host side: the mirror of nsk_bp_latent_steps (tests/bp_latent.py;
the device is held to it bit for bit in tests/test_bp_latent_gpu.py) against enumeration -- its gradient is
E[S_w | evidence] - E[S_w], its run raises log P(evidence), the host rule of bp_log_evidence is exact on a tree -- and the
liveliness of every case the GPU tests use.  No GPU needed."""

import numpy as np
import pytest

import bp
import bp_learn as bl
import bp_latent as lat
from numbskull_amd import _lib


# ---------------------------------------------------------------------------------------------- the gradient, exact on forests
@pytest.mark.parametrize("name", ["chain9_ends", "tree"])
def test_the_step_0_gradient_equals_enumeration(name):
    """(Mc - M) * 2^-32 against E[S_w | evidence] - E[S_w].  The bound is derived as in test_bp_learn_cpu.py, once per
    set-up: every table entry is rounded to a multiple of 2^-32 (2^-33 each), and a belief is within 1e-12 of the truth
    (tests/test_bp_cpu.py holds that), times at most vmax a factor."""
    p = lat.pair(name)
    o = p.learn(p.w0, 1, 40, 0.0, 0.0, 1, 0.0, 1.0, 0.0, 0)
    assert (o["residual"][0, :, -1] == 0.0).all() and not o["skipped"].any()
    mc, mf, _, _ = p.exact(p.w0)
    got = (o["moments"][0, 0] - o["moments"][0, 1]).astype(np.float64) * 2.0 ** -32
    bound = np.zeros(p.nw)
    for ln in p.side:
        T = np.diff(ln.m.layout["table_off"]).astype(np.float64)
        bound += np.bincount(ln.wid, weights=T, minlength=p.nw) * 2.0 ** -33 + \
            1e-12 * np.bincount(ln.wid, weights=bl.vmax(ln.m.fg.factor), minlength=p.nw)
    err = np.abs(got - (mc - mf))
    live = bound > 0
    print("%s: gradient %s, largest error %.3g, largest error / bound %.3f" % (name, got.tolist(), err.max(), (err[live] / bound[live]).max()))
    assert (err <= bound).all() and np.abs(got).max() > 1e-3
    # ... and gmax is its largest entry (normalize = 0, nothing fixed)
    assert o["gmax"][0] == np.abs(got).max()


def test_the_run_raises_the_log_probability_of_the_evidence():
    """Along the mirror's run on the tree the enumerated log P(evidence) = log Z(evidence held) - log Z(free) rises, and
    the host rule of bp_log_evidence -- bethe_log_z of a converged run, clamped minus free -- is that number at both ends.
    Tolerance: on a tree the Bethe value IS log Z; what differs is rounding.  bethe_log_z sums a few hundred terms
    b (theta - log b) of magnitude at most 2, each within a few ulp: 500 x 2 x 2^-52 = 2.2e-13 would be the worst case.
    Measured against enumeration on the CPU: 3.6e-15 at most over the four values; the bound below is 1e-12, the worst
    case with a margin of 4 and 280 times what was measured."""
    p = lat.pair("tree")
    o = p.learn(p.w0, 25, 12, 0.0, 1e-9, 1, 1.0, 1.0, 0.0, 1)
    assert (o["iters"] > 0).all() and not np.array_equal(o["w"], p.w0)
    le, worst = [], 0.0
    for w in (p.w0, o["w"]):
        _, _, zc, zf = p.exact(w)
        bc, bf = p.log_z(w)
        worst = max(worst, abs(bc - zc), abs(bf - zf))
        assert abs((bc - bf) - (zc - zf)) <= 1e-12
        le.append(zc - zf)
    print("log P(evidence): %.6f -> %.6f, grad_max %.3g -> %.3g, Bethe against enumeration: %.3g" % (le[0], le[1], o["gmax"][0], o["gmax"][-1], worst))
    assert worst <= 1e-12
    assert le[1] > le[0] + 0.05 and o["gmax"][-1] < o["gmax"][0]


# ---------------------------------------------------------------------------------------------- liveliness of the GPU cases
@pytest.mark.parametrize("name", [n for n in lat.STEP_CASES if n != "no_evidence"])
def test_every_case_is_lively(name):
    p = lat.pair(name)
    c, f = p.side
    assert c.m.layout["clamped"].any() and not f.m.layout["clamped"].any(), "evidence and latent variables"
    assert name == "all_evidence" or not c.m.layout["clamped"].all()
    o = lat.mirror(name, lat.SETTINGS[3])           # 3 steps of 6 iterations, warm, tol 0
    free = ~p.fixed
    assert not np.array_equal(o["w"], p.w0) and np.array_equal(o["w"][p.fixed], p.w0[p.fixed])
    assert (o["gmax"] > 0).all() and len(set(o["gmax"].tolist())) == 3
    assert all(not np.array_equal(o["moments"][t, 0][free], o["moments"][t, 1][free]) for t in range(3)), "the two rows of moments differ"
    (f2v_c, v2f_c), (f2v_f, v2f_f) = o["messages"]
    assert len(f2v_c) != len(f2v_f) and (o["residual"][:, 1, 0] > 0).all(), "the free messages move"
    if name != "all_evidence":
        assert (o["residual"][:, 0, 0] > 0).all(), "the clamped messages move"


def test_the_special_cases_are_what_they_are_for():
    # the non-binary variable launch on one side only
    c, f = lat.pair("mixed_cat").side

    def walked(ln):
        L = ln.m.layout
        return [int(L["card"][v]) for v in range(len(L["card"])) if not L["clamped"][v] and L["var_edges"][v]]
    assert walked(c) and all(k == 2 for k in walked(c)) and any(k > 2 for k in walked(f)) and any(k == 2 for k in walked(f))
    assert lat.pair("mixed_cat").fixed.any()
    # one side of every pair launch is empty
    c, f = lat.pair("all_evidence").side
    assert len(c.m.layout["edge_var"]) == 0 and (np.diff(c.m.layout["table_off"]) == 1).all() and len(f.m.layout["edge_var"]) > 0
    o = lat.mirror("all_evidence", lat.SETTINGS[3])
    assert (o["iters"][:, 0] == 1).all() and not o["residual"][:, 0].any()
    # no evidence: both set-ups are the same, the gradient is exactly 0 and the weights move by reg_param alone
    p = lat.pair("no_evidence")
    assert not p.side[0].m.layout["clamped"].any()
    for setting in lat.SETTINGS:
        o = lat.mirror("no_evidence", setting)
        nsteps, _, _, _, normalize, reg = setting
        assert not o["gmax"].any() and np.array_equal(o["moments"][:, 0], o["moments"][:, 1]) and (o["residual"][:, :, 0] > 0).all()
        w, st = p.w0.copy(), lat.step_of(normalize)
        for _ in range(nsteps):
            w, st = w + st * (0.0 - reg * w), st * lat.DECAY
        assert np.array_equal(o["w"], w) and (reg == 0.0) == np.array_equal(w, p.w0)
    # a weight without a factor
    assert lat.pair("chain9_ends").nfac[0] == 0


def test_the_chain_converges_unevenly():
    """clamping shortens the chain: the clamped set-up is at its fixed point iterations before the free one"""
    p = lat.pair("chain9_ends")
    o = p.learn(p.w0, 2, lat.UNEVEN_ITERS, 0.0, lat.UNEVEN_TOL, 1, 0.5, lat.DECAY, 0.0, 1)
    print("iterations (clamped, free) per step:", o["iters"].tolist())
    assert (o["iters"] > 0).all() and (o["iters"][:, 0] + 2 <= o["iters"][:, 1]).all()
    assert (o["iters"] > 1).all() and (o["iters"][:, 1] < lat.UNEVEN_ITERS).all()


def test_the_trips_case_makes_unequal_trips_on_either_side():
    c, f = lat.pair("trips").side
    for what, items, block in (("edges", lambda ln: len(ln.m.layout["edge_var"]), _lib.BP_BLOCK),
                               ("table entries", lambda ln: len(ln.feat), _lib.BP_BLOCK),
                               ("variables", lambda ln: sum(1 for e in ln.m.layout["var_edges"] if e), _lib.BP_VAR_BLOCK)):
        tc, tf = bp.trips(items(c), 1, block), bp.trips(items(f), 1, block)
        print(what, "trips clamped / free:", tc, tf)
        assert min(tc, tf) >= 3 and tc != tf, what
    assert bp.trips(len(c.wid), 1) >= 3             # (the factors are the graph's: the same on both sides)
    o = lat.mirror("trips", lat.TRIP_SETTING)
    assert (o["residual"][:, :, 0] > 0).all() and (o["gmax"] > 0).all()
    assert not np.array_equal(o["moments"][:, 0], o["moments"][:, 1])
