"""Learning by belief propagation on the device (nsk_bp_refresh / nsk_bp_moments / nsk_bp_learn_steps,
FactorGraph.bp_weight_moments / learn_bp).

Yardstick: the numpy mirror of tests/bp_learn.py -- bp_iterate with the oracle's exp_det over ``w[weightId] * feat``,
diagnostics.bp_moment_counts, diagnostics.pcd_step with R = 1.  Device and mirror perform the same IEEE operations in the
same order and the sums are integers, so every comparison is bit for bit or integer for integer.
tests/test_bp_learn_cpu.py ties the mirror to enumeration and shows every case lively."""

import ctypes as C

import numpy as np
import pytest

import bp
import bp_learn as bl
from numbskull_amd import _lib
from numbskull_amd.diagnostics import bp_factor_beliefs
from util import session

pytestmark = pytest.mark.gpu

SEED = 77


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _same(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), (what, float(np.nanmax(np.abs(np.asarray(a) - np.asarray(b)))))


class Dev(object):
    """the C-ABI calls on one handle"""

    def __init__(self, g, hbv=False):
        _, self.fg = session(g, seed=SEED, head_by_vid=hbv)
        self.L, self.h = _lib.lib(), self.fg._engine()
        self.info = _lib.BpInfo()
        self.nw = len(self.fg.weight)

    def setup(self, sev=0, push=True):
        if push:
            self.fg._push(0, 0)
        return self.L.nsk_bp_setup(self.h, _lib.BUF_VALUE, 0, int(sev), C.byref(self.info))

    def run(self, iters, damping=0.0, tol=0.0):
        n, res = C.c_int64(0), np.full(iters, -1.0)
        _lib.check(self.L.nsk_bp_run(self.h, iters, damping, tol, C.byref(n), _lib.ptr(res)))
        return n.value, res

    def get(self, what):
        out = np.zeros(self.info.ntable if what <= _lib.BP_FACTOR_BELIEFS else self.info.nmsg)
        _lib.check(self.L.nsk_bp_download(self.h, what, _lib.ptr(out)))
        return out

    def moments(self):
        M, sk = np.full(self.nw, -7, np.int64), C.c_int64(-1)
        _lib.check(self.L.nsk_bp_moments(self.h, _lib.ptr(M), C.byref(sk)))
        return M, sk.value

    def upload_weights(self, w):
        self.fg.weight_value[0][:] = w
        self.fg._push(0, 0)

    def weights(self):
        w = np.zeros(self.nw)
        _lib.check(self.L.nsk_state_download(self.h, None, None, _lib.ptr(w), None))
        return w

    def learn_rc(self, target, nsteps=2, iters=3, damping=0.0, tol=0.0, warm=1, step=0.1, decay=bl.DECAY, reg=0.0, normalize=1, out=None):
        t = None if target is None else np.ascontiguousarray(target, np.float64)
        o = out or [None] * 5
        return self.L.nsk_bp_learn_steps(self.h, _lib.ptr(t), nsteps, iters, damping, tol, warm, step, decay, reg, normalize,
                                         *[_lib.ptr(a) for a in o])

    def learn(self, target, nsteps, iters, damping, tol, warm, step, decay, reg, normalize):
        o = {"gmax": np.full(nsteps, -1.0), "iters": np.zeros(nsteps, np.int64), "residual": np.full((nsteps, iters), -1.0),
             "moments": np.full((nsteps, self.nw), -7, np.int64), "skipped": np.full(nsteps, -1, np.int64)}
        _lib.check(self.learn_rc(target, nsteps, iters, damping, tol, warm, step, decay, reg, normalize,
                                 [o[k] for k in ("gmax", "iters", "residual", "moments", "skipped")]))
        return o

    def bytes(self):
        return self.fg.info()["device_bytes"]

    def error(self):
        return self.L.nsk_last_error().decode()


def _case(name):
    if name in bl.LEARN:
        build, hbv, _ = bl.LEARN[name]
        return build, hbv, 0
    return bp.CASES[name] if name in bp.CASES else bl.EXTRA[name]


def _dev(name):
    build, hbv, sev = _case(name)
    d = Dev(build(), hbv)
    assert d.setup(sev) == _lib.OK, d.error()
    return d, sev


def _check_learn(got, want, what):
    _same(got["gmax"], want["gmax"], (what, "gmax"))
    assert np.array_equal(got["iters"], want["iters"]), (what, "iters", got["iters"], want["iters"])
    _same(got["residual"], want["residual"], (what, "residual"))
    assert np.array_equal(got["moments"], want["moments"]), (what, "moments")
    assert np.array_equal(got["skipped"], want["skipped"]), (what, "skipped")


# ---------------------------------------------------------------------------------------------- A: the moments
@pytest.mark.parametrize("name", bl.MOMENT_CASES)
def test_moments_equal_the_mirror_integer_for_integer(name):
    ln = bl.learner(name)
    d, sev = _dev(name)
    _same(d.get(_lib.BP_THETA), ln.m.theta, "theta")
    for iters in bl.MOMENT_ITERS:
        assert d.setup(sev, push=False) == _lib.OK
        want, skipped, r = bl.moments_mirror(name, iters)
        n, res = d.run(iters)
        assert n == r["iters"], (name, iters)
        _same(d.get(_lib.BP_V2F), r["v2f"], (name, iters, "v2f"))
        M, sk = d.moments()
        assert sk == skipped == 0
        assert np.array_equal(M, want), (name, iters, M - want)
        M2, _ = d.moments()                         # a second call: the same integers, nothing left behind
        assert np.array_equal(M2, M)


def test_a_weight_without_a_factor_reads_zero():
    ln = bl.learner("grid1x9_clamped")
    d, _ = _dev("grid1x9_clamped")
    d.run(3)
    M, sk = d.moments()
    want, _ = ln.moments(ln.run(ln.m.w, 3))
    assert ln.nfac[0] == 0 and M[0] == 0 and M[1] != 0 and sk == 0
    assert np.array_equal(M, want)
    assert d.L.nsk_bp_moments(d.h, _lib.ptr(M), None) == _lib.OK       # the skip count is optional
    assert d.L.nsk_bp_moments(d.h, None, None) == _lib.E_INVALID


@pytest.mark.parametrize("name", ["mixed_clamped", "grid6_two"])
def test_an_all_clamped_state_equals_the_chain_moments(name):
    build, hbv, _ = _case(name)
    d = Dev(bl.all_clamped(build()), hbv)
    assert d.setup() == _lib.OK, d.error()
    assert d.info.nedges == 0 and d.info.ntable == d.info.nfactor
    n, _ = d.run(2)
    M, sk = d.moments()
    assert d.L.nsk_bp_clear(d.h) == _lib.OK
    chain, R = d.fg.weight_moments(counts=True)
    assert R == 1 and sk == 0 and n == 1
    assert np.array_equal(M, chain) and np.abs(M).sum() > 0


def test_the_nan_graph_is_skipped():
    ln = bl.learner("nan")
    d, _ = _dev("nan")
    d.run(2)
    with np.errstate(invalid="ignore", divide="ignore"):
        want, skipped = ln.moments(ln.run(ln.m.w, 2))
    M, sk = d.moments()
    assert sk == skipped == 2 and np.array_equal(M, want) and not M.any()


# ---------------------------------------------------------------------------------------------- B: refresh
@pytest.mark.parametrize("name", ["grid5x5_clamped", "mixed"])
def test_refresh_continues_under_new_weights(name):
    ln = bl.learner(name)
    damping = bl.LEARN[name][2]
    d, _ = _dev(name)
    w0 = ln.m.w.copy()
    n1, res1 = d.run(3, damping)
    r1 = ln.run(w0, 3, damping)
    _same(res1, r1["residual"], "before")
    # a refresh under unchanged weights leaves theta and psi as they are (psi shows in the factor beliefs)
    theta0, fb0 = d.get(_lib.BP_THETA), d.get(_lib.BP_FACTOR_BELIEFS)
    assert d.L.nsk_bp_refresh(d.h) == _lib.OK
    _same(d.get(_lib.BP_THETA), theta0, "theta after an idle refresh")
    _same(d.get(_lib.BP_FACTOR_BELIEFS), fb0, "factor beliefs after an idle refresh")
    _same(theta0, ln.theta(w0), "theta")
    # new weights
    w1 = w0 + np.linspace(0.3, -0.4, ln.nw)
    d.upload_weights(w1)
    _same(d.get(_lib.BP_THETA), theta0, "an upload alone leaves the tables")
    assert d.L.nsk_bp_refresh(d.h) == _lib.OK
    _same(d.get(_lib.BP_THETA), ln.theta(w1), "theta under the new weights")
    _same(d.get(_lib.BP_V2F), r1["v2f"], "the messages stay")
    n2, res2 = d.run(4, damping)
    r2 = ln.run(w1, 4, damping, messages=(r1["f2v"], r1["v2f"]))
    assert n2 == r2["iters"]
    _same(res2, r2["residual"], "after")
    _same(d.get(_lib.BP_F2V), r2["f2v"], "f2v")
    _same(d.get(_lib.BP_V2F), r2["v2f"], "v2f")
    _same(d.get(_lib.BP_FACTOR_BELIEFS), bp_factor_beliefs(ln.m.layout, r2["psi"], r2["v2f"]), "factor beliefs")
    M, _ = d.moments()
    assert np.array_equal(M, ln.moments(r2)[0])


# ---------------------------------------------------------------------------------------------- C: the learning steps
def _step(normalize, step=0.5):
    return step if normalize else step / 8


@pytest.mark.parametrize("name", sorted(bl.LEARN))
def test_learning_steps_equal_the_mirror(name):
    ln = bl.learner(name)
    damping = bl.LEARN[name][2]
    target = bl.learn_target(name)
    d, _ = _dev(name)
    for setting in bl.SETTINGS:
        nsteps, iters, warm, tol, normalize, reg = setting
        assert d.setup() == _lib.OK                 # the initial weights again, the messages reset
        want = bl.learn_mirror(name, setting)
        got = d.learn(target, nsteps, iters, damping, tol, warm, _step(normalize), bl.DECAY, reg, normalize)
        _check_learn(got, want, (name, setting))
        w = d.weights()
        _same(w, want["w"], (name, setting, "weights"))
        _same(w[ln.fixed], ln.m.w[ln.fixed], "fixed weights")
        _same(d.get(_lib.BP_THETA), want["theta"], (name, setting, "theta agrees with the final weights"))
        _same(d.get(_lib.BP_F2V), want["messages"][0], (name, setting, "f2v"))
        _same(d.get(_lib.BP_V2F), want["messages"][1], (name, setting, "v2f"))
    print(name, "iterations of the last setting:", got["iters"].tolist(), "gmax", got["gmax"].tolist())


def test_a_second_call_continues_and_a_run_follows_under_the_learned_weights():
    name, setting = "grid5x5_clamped", bl.SETTINGS[6]          # 3 steps of 6 iterations, warm, tol 0, normalised, reg 0.01
    nsteps, iters, warm, tol, normalize, reg = setting
    ln, damping, target = bl.learner(name), bl.LEARN[name][2], bl.learn_target(name)
    whole = bl.learn_mirror(name, setting)
    d, _ = _dev(name)
    s0 = _step(normalize)
    a = d.learn(target, 2, iters, damping, tol, 1, s0, bl.DECAY, reg, normalize)
    b = d.learn(target, 1, iters, damping, tol, 1, (s0 * bl.DECAY) * bl.DECAY, bl.DECAY, reg, normalize)
    _check_learn({k: np.concatenate([a[k], b[k]]) for k in a}, whole, "two calls")
    _same(d.weights(), whole["w"], "weights")
    # nsk_bp_run continues under the learned weights
    n, res = d.run(3, damping)
    r = ln.run(whole["w"], 3, damping, messages=whole["messages"])
    _same(res, r["residual"], "a run behind the steps")
    _same(d.get(_lib.BP_V2F), r["v2f"], "v2f")


def test_sweeps_behind_the_steps_run_under_the_learned_weights():
    """weights_dirty: a handle that swept before the steps must rebuild what derives from the weights"""
    name = "grid5x5_clamped"
    build, hbv, _ = bl.LEARN[name]
    target = bl.learn_target(name)
    d = Dev(build(), hbv)
    _, tw = session(build(), seed=SEED, head_by_vid=hbv)
    d.fg._push(0, 0)
    d.fg._sweep(3, False, False)
    assert d.setup(push=False) == _lib.OK, d.error()
    d.learn(target, 3, 4, 0.5, 0.0, 1, 2.0, bl.DECAY, 0.0, 1)
    assert d.L.nsk_bp_clear(d.h) == _lib.OK
    w = d.weights()
    assert not np.array_equal(w, d.fg.weight_value[0])
    d.fg._sweep(5, False, False)
    d.fg._pull(0, 0, weights=False)
    tw._push(0, 0)
    tw._sweep(3, False, False)
    tw._pull(0, 0)
    tw.weight_value[0][:] = w
    tw._push(0, 0)
    tw._sweep(5, False, False)
    tw._pull(0, 0)
    assert np.array_equal(d.fg.var_value[0], tw.var_value[0]) and np.array_equal(d.fg.count, tw.count) and tw.count.any()
    assert d.fg.info()["sweeps_done"] == tw.info()["sweeps_done"] == 8
    # ... and under the old weights they would have ended elsewhere
    _, old = session(build(), seed=SEED, head_by_vid=hbv)
    old.inference(0, 8)
    assert not np.array_equal(old.count, tw.count)


# ---------------------------------------------------------------------------------------------- D: later trips
def test_later_trips_of_the_new_kernels(monkeypatch):
    """NSK_BP_GRID_CAP is read at each call: the same process runs the graph as is and with one block a launch"""
    ln = bl.learner("trips")
    w0 = ln.m.w.copy()
    target = bl.learn_target("trips")
    r = ln.run(w0, bp.TRIP_ITERS)
    want_M, _ = ln.moments(r)
    w1 = w0 + 0.1
    want = ln.learn(w1, target, 2, bp.TRIP_ITERS, 0.0, 0.0, 1, 0.5, bl.DECAY, 0.0, 1, messages=(r["f2v"], r["v2f"]))
    L = ln.m.layout
    assert min(bp.trips(len(ln.feat), 1), bp.trips(len(ln.wid), 1), bp.trips(len(L["edge_var"]), 1)) >= 3
    got = []
    for cap in (None, "1"):
        monkeypatch.delenv("NSK_DIAG", raising=False)
        monkeypatch.delenv("NSK_BP_GRID_CAP", raising=False)
        if cap:
            monkeypatch.setenv("NSK_DIAG", "1")
            monkeypatch.setenv("NSK_BP_GRID_CAP", cap)
        d, _ = _dev("trips")
        d.run(bp.TRIP_ITERS)
        M, sk = d.moments()
        assert np.array_equal(M, want_M) and sk == 0, cap
        d.upload_weights(w1)
        assert d.L.nsk_bp_refresh(d.h) == _lib.OK
        theta = d.get(_lib.BP_THETA)
        _same(theta, ln.theta(w1), ("refresh", cap))
        o = d.learn(target, 2, bp.TRIP_ITERS, 0.0, 0.0, 1, 0.5, bl.DECAY, 0.0, 1)
        _check_learn(o, want, cap)
        _same(d.weights(), want["w"], cap)
        _same(d.get(_lib.BP_THETA), want["theta"], cap)
        got.append((M.astype(np.float64), theta, o["gmax"], o["residual"], o["moments"].astype(np.float64), d.weights(), d.get(_lib.BP_V2F)))
    for a, b in zip(*got):
        _same(a, b, "capped against uncapped")


# ---------------------------------------------------------------------------------------------- E: the ledger, refusals
def test_the_ledger_and_the_refusals():
    name = "mixed"
    ln = bl.learner(name)
    build, hbv, _ = bl.LEARN[name]
    d = Dev(build(), hbv)
    d.fg.log_potential()                            # (the records both share are in place)
    d.weights()                                     # ... and the staging of the weight transfers
    before = d.bytes()
    target = bl.learn_target(name)
    # no set-up: refused
    assert d.L.nsk_bp_refresh(d.h) == _lib.E_INVALID
    assert d.L.nsk_bp_moments(d.h, _lib.ptr(np.zeros(d.nw, np.int64)), None) == _lib.E_INVALID
    assert d.learn_rc(target) == _lib.E_INVALID and "set up" in d.error()
    assert d.bytes() == before
    assert d.setup(push=False) == _lib.OK
    held = d.bytes()
    L = ln.m.layout
    npos, nslot = sum(len(s) for s in L["slots"]), sum(len(m) for m in L["members"])
    nvar, i = len(d.fg.variable), d.info
    nvl = sum(1 for e in L["var_edges"] if e)
    F, E = i.nfactor, i.nedges
    # array by array: theta, psi and the feature table (24 bytes a table entry), both message arrays, the beliefs, the
    # offsets per factor (two of 8 bytes, two of 4, one entry more than factors) and per edge, three int32 an edge, the
    # free variables with an edge and their offsets, member positions and distinct members ...
    known = 24 * i.ntable + 16 * i.nmsg + 8 * i.nbelief + 2 * 8 * (F + 1) + 2 * 4 * (F + 1) + 8 * (E + 1) + 3 * 4 * E + \
        4 * nvl + 4 * (nvl + 1) + 8 * npos + 8 * nslot
    rest = i.device_bytes - known               # ... and 8 bytes an internal id (one more) + 1 for its state
    print("set-up bytes %d: %d beside the per-id arrays of %d ids" % (held - before, known, (rest - 8) // 9))
    assert held - before == i.device_bytes
    assert (rest - 8) % 9 == 0 and (rest - 8) // 9 >= nvar
    d.run(3, 0.5)
    d.moments()
    assert d.bytes() == held
    theta0, w0 = d.get(_lib.BP_THETA), d.weights()
    # every refusal allocates nothing and enqueues nothing
    nan, inf = float("nan"), float("inf")
    bad_t = target.copy()
    bad_t[1] = nan
    refused = [dict(target=None), dict(target=bad_t), dict(nsteps=0), dict(nsteps=4097), dict(iters=0), dict(iters=4097),
               dict(nsteps=4096, iters=17), dict(damping=1.0), dict(damping=-0.1), dict(damping=nan), dict(tol=-1.0), dict(tol=nan),
               dict(warm=2), dict(warm=-1), dict(normalize=2), dict(step=nan), dict(step=inf), dict(decay=nan), dict(decay=inf),
               dict(reg=nan), dict(reg=inf), dict(reg=-1e-3)]
    for kw in refused:
        kw.setdefault("target", target)
        assert d.learn_rc(**kw) == _lib.E_INVALID, kw
        assert d.bytes() == held, kw
    _same(d.weights(), w0, "weights after the refusals")
    _same(d.get(_lib.BP_THETA), theta0, "theta after the refusals")
    # every output is optional
    assert d.learn_rc(target, nsteps=2, iters=3, damping=0.5) == _lib.OK
    assert d.bytes() == held
    assert not np.array_equal(d.weights(), w0)
    d.learn(target, 2, 3, 0.5, 0.0, 1, 0.1, bl.DECAY, 0.0, 1)
    assert d.bytes() == held
    assert d.L.nsk_bp_clear(d.h) == _lib.OK and d.bytes() == before
    assert d.L.nsk_bp_refresh(d.h) == _lib.E_INVALID


# ---------------------------------------------------------------------------------------------- F: the Python API
def test_bp_weight_moments():
    ln = bl.learner("chain9")
    _, fg = session(bp.chain9(), seed=SEED)
    r = ln.run(ln.m.w, 100, 0.0, 1e-9)
    want, _ = ln.moments(r)
    res = fg.bp_weight_moments()
    assert set(res) == {"moments", "iters", "converged", "skipped"}
    assert res["iters"] == r["iters"] and res["converged"] is True and res["skipped"] == 0
    _same(res["moments"], want.astype(np.float64) * 2.0 ** -32, "moments")
    res = fg.bp_weight_moments(max_iters=2, counts=True)
    assert res["converged"] is False and res["iters"] == 2
    assert res["moments"].dtype == np.int64 and np.array_equal(res["moments"], bl.moments_mirror("chain9", 2)[0])
    with pytest.raises(ValueError):
        fg.bp_weight_moments(max_iters=0)
    with pytest.raises(ValueError):
        fg.bp_weight_moments(var_copy="all")


def test_learn_bp_recovers_planted_weights_and_clears_its_set_up():
    ln = bl.learner("shared_tree")
    target, _ = bl.exact_moments(ln.m.og, bl.W_STAR, ln.m.x, ln.m.free)
    R = bl.RECOVERY
    want = ln.learn(np.zeros(ln.nw), target, R["epochs"], R["iters"], 0.0, R["tol"], 1, R["stepsize"], 1.0, 0.0, 1)
    _, fg = session(bl.shared_tree(), seed=SEED)
    res = fg.learn_bp(R["epochs"], R["stepsize"], iters=R["iters"], tol=R["tol"], target=target, moments=True)
    assert set(res) == {"grad_max", "iters", "converged", "residual", "skipped", "target", "factors_per_weight", "moments"}
    w = fg.weight_value[0]
    err = float(np.abs(w - bl.W_STAR).max())
    print("learn_bp: max |w - w*| = %.4g" % err)
    assert err <= bl.RECOVERY_BOUND
    _same(w, want["w"], "weights")
    _same(res["grad_max"], want["gmax"], "grad_max")
    _same(res["residual"], want["residual"], "residual")
    assert np.array_equal(res["iters"], np.abs(want["iters"])) and np.array_equal(res["converged"], want["iters"] > 0)
    assert res["converged"].all() and res["converged"].dtype == np.bool_
    assert np.array_equal(res["moments"], want["moments"]) and not res["skipped"].any()
    assert np.array_equal(res["factors_per_weight"], ln.nfac)
    assert set(fg.learn_bp(1, 0.1, target=target)) == {"grad_max", "iters", "converged", "residual", "skipped", "target", "factors_per_weight"}
    # target=None: the statistics of the evidence chain
    res = fg.learn_bp(2, 0.1)
    _same(res["target"], fg.weight_moments(evidence_chain=True), "the default target")
    # the set-up goes even when the call raises
    before = fg.info()["device_bytes"]
    with pytest.raises(ValueError):
        fg.learn_bp(2, 0.1, damping=1.0, target=target)
    assert fg.info()["device_bytes"] == before
    with pytest.raises(ValueError):
        fg.learn_bp(0, 0.1)
    with pytest.raises(ValueError):
        fg.learn_bp(2, float("nan"))
    assert _lib.lib().nsk_bp_refresh(fg._engine()) == _lib.E_INVALID       # nothing is set up
