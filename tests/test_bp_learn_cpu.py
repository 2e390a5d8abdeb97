"""Learning by belief propagation, the host side: numbskull_amd.diagnostics.bp_moment_counts and the mirror of
nsk_bp_learn_steps (tests/bp_learn.py; the device is held to both bit for bit in tests/test_bp_learn_gpu.py) against
enumeration on trees, a finite difference of the exact log Z, the chain moments of a clamped state, the NaN graph, the
recovery of planted weights, and the liveliness of every case the GPU tests use.  No GPU needed."""

import warnings

import numpy as np
import pytest

import bp
import bp_learn as bl
import temper
from numbskull_amd import _lib
from numbskull_amd.diagnostics import bp_moment_counts, moment_counts


def _tree(name):
    return bl.learner(name) if name in bp.CASES or name in bl.EXTRA else bl.Learner(bp.TREES[name]())


# ---------------------------------------------------------------------------------------------- exact on trees
@pytest.mark.parametrize("name", sorted(bp.TREES))
def test_the_moments_equal_enumeration_on_trees(name):
    """the bound is derived: every table entry is rounded to a multiple of 2^-32 (2^-33 each), and a belief is within
    1e-12 of the truth (tests/test_bp_cpu.py holds that), times at most vmax a factor"""
    ln = _tree(name)
    r = ln.run(ln.m.w, 40)
    assert r["iters"] > 0 and r["residual"][r["iters"] - 1] == 0.0
    M, skipped = ln.moments(r)
    ex, _ = bl.exact_moments(ln.m.og, ln.m.w, ln.m.x, ln.m.free)
    T = np.diff(ln.m.layout["table_off"]).astype(np.float64)
    bound = np.bincount(ln.wid, weights=T, minlength=ln.nw) * 2.0 ** -33 + \
        1e-12 * np.bincount(ln.wid, weights=bl.vmax(ln.m.fg.factor), minlength=ln.nw)
    err = np.abs(M.astype(np.float64) * 2.0 ** -32 - ex)
    print("%s: largest error %.3g, largest error / bound %.3f" % (name, err.max(), (err / bound).max()))
    assert skipped == 0 and M.dtype == np.int64
    assert (err <= bound).all()


def test_a_central_difference_of_the_exact_log_z():
    """d log Z / d w_k = E[S_k].  h = 1e-4: the truncation error is h^2 / 6 times the third cumulant of S_k, at most 8 for
    one factor with values in [0, 1] (|S - mean| <= 2 is generous): 1.4e-8; the rounding of the two log Z of magnitude L
    gives 2^-52 L / h; the fixed point 2^-33 a table entry.  Observed on the CPU: 1.6e-10."""
    ln = _tree("tree")
    w = ln.m.w.copy()
    M, _ = ln.moments(ln.run(w, 40))
    k, h = 1, 1e-4
    lz = []
    for s in (h, -h):
        ws = w.copy()
        ws[k] += s
        lz.append(temper.exact_log_z(ln.m.og, ws, ln.m.x, ln.m.free))
    fd = (lz[0] - lz[1]) / (2 * h)
    T = int(np.diff(ln.m.layout["table_off"])[ln.wid == k].sum())
    tol = 8 * h * h / 6 + 2.0 ** -52 * max(abs(lz[0]), abs(lz[1])) / h + T * 2.0 ** -33 + 1e-12
    err = abs(fd - M[k] * 2.0 ** -32)
    print("central difference %.12f, Bethe moment %.12f, error %.3g, tolerance %.3g" % (fd, M[k] * 2.0 ** -32, err, tol))
    assert ln.nfac[k] == 1 and err <= tol < 2e-8


# ---------------------------------------------------------------------------------------------- the clamped state
@pytest.mark.parametrize("name", ["mixed_clamped", "tree", "grid6_two"])
def test_an_all_clamped_state_gives_the_chain_moments(name):
    base = bl.learner(name)
    ln = bl.Learner(bl.all_clamped(base.m.g), base.m.hbv)
    assert (np.diff(ln.m.layout["table_off"]) == 1).all() and len(ln.m.layout["edge_var"]) == 0
    M, skipped = ln.moments(ln.run(ln.m.w, 2))
    assert skipped == 0
    assert np.array_equal(M, moment_counts(ln.feat, ln.wid, ln.nw))
    assert np.abs(M).sum() > 0


# ---------------------------------------------------------------------------------------------- NaN
def test_a_nan_factor_is_skipped_and_never_converted():
    ln = bl.learner("nan")
    with np.errstate(invalid="ignore", divide="ignore"):
        r = ln.run(ln.m.w, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with np.errstate(all="raise"):              # nothing of a NaN may reach a product or a conversion
            M, skipped = ln.moments(r)
    assert np.isnan(r["beliefs"]).all()             # psi (1, 0) against a message (0, 1): Z_f = 0, b = 0 / 0
    assert skipped == 2 and M.dtype == np.int64 and not M.any()
    # one sound factor beside them still counts
    g = bp.spec_graph([2, 2], [0, 0], [0, 0], [(4, [0], [0], 800.0), (4, [0], [0], -800.0), (4, [1], [0], 0.4)])
    ln = bl.Learner(g)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = ln.run(ln.m.w, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        M, skipped = ln.moments(r)
    assert skipped == 2 and M[0] == 0 and M[1] == 0 and M[2] > 0


def test_argument_checks_of_the_rule():
    ln = bl.learner("tree")
    r = ln.run(ln.m.w, 1)
    with pytest.raises(ValueError):
        bp_moment_counts(ln.m.layout, ln.feat[:-1], r["psi"], r["v2f"], ln.wid, ln.nw)
    with pytest.raises(IndexError):
        bp_moment_counts(ln.m.layout, ln.feat, r["psi"], r["v2f"], ln.wid, ln.nw - 1)


# ---------------------------------------------------------------------------------------------- recovery
def test_planted_weights_are_recovered_on_a_tree():
    """exact maximum likelihood on a tree: from w = 0 the mirror of learn_bp finds the weights whose exact moments are
    the target.  Measured with the mirror: max |w - w*| = 1.208e-05 after 60 steps of stepsize 2.0."""
    ln = bl.learner("shared_tree")
    target, _ = bl.exact_moments(ln.m.og, bl.W_STAR, ln.m.x, ln.m.free)
    R = bl.RECOVERY
    out = ln.learn(np.zeros(ln.nw), target, R["epochs"], R["iters"], 0.0, R["tol"], 1, R["stepsize"], 1.0, 0.0, 1)
    g = out["gmax"]
    err = float(np.abs(out["w"] - bl.W_STAR).max())
    print("recovery: max |w - w*| = %.4g, grad_max %.3g -> %.3g" % (err, g[0], g[-1]))
    assert (out["iters"] > 0).all() and not out["skipped"].any()
    assert (np.diff(g[R["epochs"] // 2:]) < 0).all()
    assert err <= bl.RECOVERY_BOUND


# ---------------------------------------------------------------------------------------------- liveliness of the GPU cases
def test_the_layouts_reach_every_path_of_the_moment_kernel():
    # several runs of equal slot inside one window of 64 entries
    ln = bl.learner("grid6_two")
    runs = 1 + int((np.diff(ln.entry_wid[:64]) != 0).sum())
    assert len(ln.entry_wid) > 64 and runs >= 8
    # ... and a single run over a whole window
    one = bl.learner("grid6_one")
    assert len(set(one.entry_wid[:64].tolist())) == 1
    # a table across a boundary of 64 entries
    to = bl.learner("truth0_free").m.layout["table_off"]
    T = np.diff(to)
    assert T.max() == 81 and any(to[f] // 64 != (to[f + 1] - 1) // 64 for f in np.nonzero(T == 81)[0])
    # ... and one across a block of 256
    to = bl.learner("limit").m.layout["table_off"]
    assert np.diff(to).max() == 4096 == _lib.BP_MAX_TABLE and to[0] // 256 != (to[1] - 1) // 256
    # the capped case: at least three trips over entries, factors and edges
    L = bl.learner("trips").m.layout
    assert min(bp.trips(int(L["table_off"][-1]), 1), bp.trips(len(L["table_off"]) - 1, 1), bp.trips(len(L["edge_var"]), 1)) >= 3


@pytest.mark.parametrize("name", bl.MOMENT_CASES)
def test_every_moment_case_is_lively(name):
    got = [bl.moments_mirror(name, it)[0] for it in bl.MOMENT_ITERS]
    assert all(bl.moments_mirror(name, it)[1] == 0 for it in bl.MOMENT_ITERS)
    assert np.abs(got[-1]).sum() > 0
    if name != "limit" and not name.startswith("truth"):        # (those are at their fixed point at once)
        assert not np.array_equal(got[0], got[-1]), "the moments move with the iterations"
    else:
        assert len(set(got[0].tolist())) >= 2


@pytest.mark.parametrize("name", sorted(bl.LEARN))
def test_every_learning_case_is_lively(name):
    ln = bl.learner(name)
    assert ln.nw >= 2 and not ln.fixed.all()
    o = bl.learn_mirror(name, bl.SETTINGS[5])       # 8 steps of 6 iterations, warm, tol 0
    assert len(set(o["gmax"].tolist())) == 8 and (o["gmax"] > 0).all()
    assert np.array_equal(o["w"][ln.fixed], ln.m.w[ln.fixed]) and not np.array_equal(o["w"], ln.m.w)
    assert len({tuple(row) for row in o["moments"].tolist()}) == 8
    if name == "grid1x9":
        assert ln.nfac[0] == 0 and not o["moments"][:, 0].any()         # a weight without a factor
    if name == "mixed":
        assert ln.fixed.any()
    if "clamped" in name or name == "mixed":        # the messages move, and a tolerance ends a step early
        assert (o["residual"][:, 0] > 0).all()
        e = bl.learn_mirror(name, bl.SETTINGS[7])   # 8 x 6, cold, tol 1e-6
        print(name, "iterations at tol 1e-6:", e["iters"].tolist())
    else:
        assert not o["residual"].any() and (o["iters"] == 1).all()
