"""Latent-variable learning by belief propagation on the device (nsk_bp_select / nsk_bp_selected / nsk_bp_latent_steps,
FactorGraph.learn_bp(latent=True) / bp_log_evidence).

Yardstick: the numpy mirror of tests/bp_latent.py -- two bp_learn.Learners of one graph, evidence held and free, stepped
together with diagnostics.pcd_latent_step.  Device and mirror perform the same IEEE operations in the same order and the
sums are integers, so every comparison is bit for bit or integer for integer.  tests/test_bp_latent_cpu.py ties the mirror
to enumeration and shows every case lively."""

import ctypes as C

import numpy as np
import pytest

import bp
import bp_learn as bl
import bp_latent as lat
from numbskull_amd import _lib
from util import session

pytestmark = pytest.mark.gpu

SEED = 77
KEYS = ("gmax", "iters", "residual", "moments", "skipped")


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _same(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), (what, float(np.nanmax(np.abs(np.asarray(a) - np.asarray(b)))))


class Dev(object):
    """the C-ABI calls on one handle; slot 0 the clamped set-up, slot 1 the free one"""

    def __init__(self, g, hbv=False):
        _, self.fg = session(g, seed=SEED, head_by_vid=hbv)
        self.L, self.h = _lib.lib(), self.fg._engine()
        self.info = [_lib.BpInfo(), _lib.BpInfo()]
        self.nw = len(self.fg.weight)

    def select(self, slot):
        return self.L.nsk_bp_select(self.h, slot)

    def selected(self):
        return self.L.nsk_bp_selected(self.h)

    def setup(self, slot, sev, push=False):
        if push:
            self.fg._push(0, 0)
        assert self.select(slot) == _lib.OK
        return self.L.nsk_bp_setup(self.h, _lib.BUF_VALUE, 0, int(sev), C.byref(self.info[slot]))

    def setup_both(self, push=True):
        assert self.setup(0, 0, push) == _lib.OK, self.error()
        assert self.setup(1, 1) == _lib.OK, self.error()
        assert self.select(0) == _lib.OK

    def run(self, iters, damping=0.0, tol=0.0):
        n, res = C.c_int64(0), np.full(iters, -1.0)
        _lib.check(self.L.nsk_bp_run(self.h, iters, damping, tol, C.byref(n), _lib.ptr(res)))
        return n.value, res

    def get(self, what, slot=None):
        """an array of the selected set-up, or of ``slot`` (the selection is put back)"""
        keep = self.selected()
        if slot is not None:
            assert self.select(slot) == _lib.OK
        info = self.info[self.selected()]
        out = np.zeros(info.ntable if what <= _lib.BP_FACTOR_BELIEFS else info.nmsg)
        _lib.check(self.L.nsk_bp_download(self.h, what, _lib.ptr(out)))
        assert self.select(keep) == _lib.OK
        return out

    def moments(self):
        M, sk = np.full(self.nw, -7, np.int64), C.c_int64(-1)
        _lib.check(self.L.nsk_bp_moments(self.h, _lib.ptr(M), C.byref(sk)))
        return M, sk.value

    def weights(self):
        w = np.zeros(self.nw)
        _lib.check(self.L.nsk_state_download(self.h, None, None, _lib.ptr(w), None))
        return w

    def steps_rc(self, nsteps=2, iters=3, damping=0.0, tol=0.0, warm=1, step=0.1, decay=lat.DECAY, reg=0.0, normalize=1, out=None):
        o = out or [None] * 5
        return self.L.nsk_bp_latent_steps(self.h, nsteps, iters, damping, tol, warm, step, decay, reg, normalize, *[_lib.ptr(a) for a in o])

    def steps(self, nsteps, iters, damping, tol, warm, step, decay, reg, normalize):
        o = {"gmax": np.full(nsteps, -1.0), "iters": np.zeros((nsteps, 2), np.int64), "residual": np.full((nsteps, 2, iters), -1.0),
             "moments": np.full((nsteps, 2, self.nw), -7, np.int64), "skipped": np.full((nsteps, 2), -1, np.int64)}
        _lib.check(self.steps_rc(nsteps, iters, damping, tol, warm, step, decay, reg, normalize, [o[k] for k in KEYS]))
        return o

    def bytes(self):
        return self.fg.info()["device_bytes"]

    def error(self):
        return self.L.nsk_last_error().decode()


def _dev(name):
    build, hbv, damping = lat.CASES[name]
    return Dev(build(), hbv), damping


def _check(got, want, what):
    _same(got["gmax"], want["gmax"], (what, "gmax"))
    assert np.array_equal(got["iters"], want["iters"]), (what, "iters", got["iters"].tolist(), want["iters"].tolist())
    _same(got["residual"], want["residual"], (what, "residual"))
    assert np.array_equal(got["moments"], want["moments"]), (what, "moments")
    assert np.array_equal(got["skipped"], want["skipped"]), (what, "skipped")


def _check_state(d, want, what):
    _same(d.weights(), want["w"], (what, "weights"))
    for slot in (0, 1):
        _same(d.get(_lib.BP_THETA, slot), want["theta"][slot], (what, slot, "theta agrees with the final weights"))
        _same(d.get(_lib.BP_F2V, slot), want["messages"][slot][0], (what, slot, "f2v"))
        _same(d.get(_lib.BP_V2F, slot), want["messages"][slot][1], (what, slot, "v2f"))


# ---------------------------------------------------------------------------------------------- A: the slots
def test_the_two_slots_share_nothing():
    d, damping = _dev("grid5x5_third")
    p = lat.pair("grid5x5_third")
    d.fg.log_potential()                            # (the records both share are in place)
    d.weights()                                     # ... and the staging of the weight transfers
    before = d.bytes()
    assert d.selected() == 0
    assert d.setup(0, 0) == _lib.OK, d.error()   # (log_potential pushed the state)
    d.run(3, damping)
    keep = [d.get(w) for w in (_lib.BP_THETA, _lib.BP_F2V, _lib.BP_V2F)]
    r0 = p.side[0].run(p.w0, 3, damping)
    _same(keep[2], r0["v2f"], "slot 0 against the mirror")
    b0 = d.info[0].device_bytes
    assert d.bytes() == before + b0
    # slot 1: set up, run, download, moments -- slot 0 stays bit for bit
    for bad in (2, -1, 7):
        assert d.select(bad) == _lib.E_INVALID and "slot" in d.error()
        assert d.selected() == 0
    assert d.select(1) == _lib.OK and d.selected() == 1
    assert d.L.nsk_bp_refresh(d.h) == _lib.E_INVALID, "slot 1 is not set up: slot 0 does not answer for it"
    assert d.setup(1, 1) == _lib.OK, d.error()
    b1 = d.info[1].device_bytes
    assert b1 > b0 and d.info[1].nedges > d.info[0].nedges and d.info[1].nclamped == 0 < d.info[0].nclamped
    assert d.bytes() == before + b0 + b1, "device_bytes counts both set-ups"
    d.run(4, damping)
    r1 = p.side[1].run(p.w0, 4, damping)
    _same(d.get(_lib.BP_V2F), r1["v2f"], "slot 1 against the mirror")
    M1, _ = d.moments()
    assert np.array_equal(M1, p.side[1].moments(r1)[0])
    for what, was in zip((_lib.BP_THETA, _lib.BP_F2V, _lib.BP_V2F), keep):
        _same(d.get(what, 0), was, ("slot 0 after work on slot 1", what))
    assert d.selected() == 1
    # clearing one keeps the other
    assert d.L.nsk_bp_clear(d.h) == _lib.OK and d.bytes() == before + b0
    assert d.L.nsk_bp_clear(d.h) == _lib.OK and d.bytes() == before + b0, "a second clear of the empty slot frees nothing"
    assert d.select(0) == _lib.OK
    for what, was in zip((_lib.BP_THETA, _lib.BP_F2V, _lib.BP_V2F), keep):
        _same(d.get(what), was, ("slot 0 after slot 1 was cleared", what))
    M0, _ = d.moments()
    assert np.array_equal(M0, p.side[0].moments(r0)[0])
    # ... and the other way round
    assert d.setup(1, 1) == _lib.OK and d.bytes() == before + b0 + b1
    assert d.select(0) == _lib.OK and d.L.nsk_bp_clear(d.h) == _lib.OK and d.bytes() == before + b1
    assert d.L.nsk_bp_refresh(d.h) == _lib.E_INVALID
    assert d.select(1) == _lib.OK and d.L.nsk_bp_refresh(d.h) == _lib.OK
    assert d.L.nsk_bp_clear(d.h) == _lib.OK and d.bytes() == before
    assert d.select(0) == _lib.OK


def test_destroy_frees_both_set_ups():
    """a handle may go with both set-ups resident and slot 1 selected (every array of both is on its ledger); the handle
    that follows starts with slot 0 and no set-up"""
    d, _ = _dev("chain9_ends")
    d.setup_both()
    assert d.select(1) == _lib.OK
    assert d.bytes() >= d.info[0].device_bytes + d.info[1].device_bytes
    d.fg.close()
    h = d.fg._engine()
    assert d.L.nsk_bp_selected(h) == 0
    for slot in (0, 1):
        assert d.L.nsk_bp_select(h, slot) == _lib.OK and d.L.nsk_bp_refresh(h) == _lib.E_INVALID


# ---------------------------------------------------------------------------------------------- B: the steps against the mirror
@pytest.mark.parametrize("name", lat.STEP_CASES)
def test_latent_steps_equal_the_mirror(name):
    d, damping = _dev(name)
    for setting in lat.SETTINGS:
        nsteps, iters, warm, tol, normalize, reg = setting
        d.setup_both()                              # the initial weights again, both message sets reset
        want = lat.mirror(name, setting)
        got = d.steps(nsteps, iters, damping, tol, warm, lat.step_of(normalize), lat.DECAY, reg, normalize)
        _check(got, want, (name, setting))
        _check_state(d, want, (name, setting))
        assert d.selected() == 0
    p = lat.pair(name)
    _same(d.weights()[p.fixed], p.w0[p.fixed], "fixed weights")
    print(name, "iterations of the last setting:", got["iters"].tolist(), "gmax", got["gmax"].tolist())
    if name == "no_evidence":
        assert not got["gmax"].any() and np.array_equal(got["moments"][:, 0], got["moments"][:, 1])


def test_the_selected_slot_stays():
    d, damping = _dev("chain9_ends")
    d.setup_both()
    assert d.select(1) == _lib.OK
    want = lat.mirror("chain9_ends", lat.SETTINGS[3])
    nsteps, iters, warm, tol, normalize, reg = lat.SETTINGS[3]
    got = d.steps(nsteps, iters, damping, tol, warm, lat.step_of(normalize), lat.DECAY, reg, normalize)
    assert d.selected() == 1
    _check(got, want, "slot 1 selected")           # (index 0 is still slot 0, the clamped set-up)
    _check_state(d, want, "slot 1 selected")


# ---------------------------------------------------------------------------------------------- C: pair against single
@pytest.mark.parametrize("name", ["grid5x5_third", "mixed_cat", "all_evidence"])
def test_the_pair_kernels_equal_the_single_kernels(name):
    """one step with step = 0: the weights stay, and either slot holds what nsk_bp_run and nsk_bp_moments leave on a fresh
    single set-up of its own"""
    d, damping = _dev(name)
    iters, tol = 5, 1e-6
    d.setup_both()
    w0 = d.weights()
    got = d.steps(1, iters, damping, tol, 1, 0.0, 1.0, 0.0, 1)
    _same(d.weights(), w0, "step = 0 leaves the weights")
    pair_msgs = [[d.get(w, slot) for w in (_lib.BP_F2V, _lib.BP_V2F, _lib.BP_THETA)] for slot in (0, 1)]
    assert d.select(1) == _lib.OK and d.L.nsk_bp_clear(d.h) == _lib.OK
    for slot in (0, 1):
        assert d.setup(0, slot) == _lib.OK          # a fresh single set-up: sample_evidence = the slot's
        n, res = d.run(iters, damping, tol)
        M, sk = d.moments()
        assert n == got["iters"][0, slot]
        _same(res, got["residual"][0, slot], (name, slot, "residual"))
        assert np.array_equal(M, got["moments"][0, slot]) and sk == got["skipped"][0, slot]
        for k, what in enumerate((_lib.BP_F2V, _lib.BP_V2F, _lib.BP_THETA)):
            _same(d.get(what), pair_msgs[slot][k], (name, slot, what))


# ---------------------------------------------------------------------------------------------- D: uneven convergence
def test_each_set_up_stops_on_its_own():
    name = "chain9_ends"
    p = lat.pair(name)
    d, damping = _dev(name)
    d.setup_both()
    I = lat.UNEVEN_ITERS
    want = p.learn(p.w0, 2, I, damping, lat.UNEVEN_TOL, 1, 0.5, lat.DECAY, 0.0, 1)
    got = d.steps(2, I, damping, lat.UNEVEN_TOL, 1, 0.5, lat.DECAY, 0.0, 1)
    _check(got, want, name)
    _check_state(d, want, name)
    it = got["iters"]
    print("iterations (clamped, free):", it.tolist())
    assert (it > 1).all() and (it[:, 0] + 2 <= it[:, 1]).all() and (it[:, 1] < I).all()
    for t in range(2):
        for s in range(2):
            row = got["residual"][t, s]
            assert (row[:it[t, s] - 1] > lat.UNEVEN_TOL).all() and row[it[t, s] - 1] <= lat.UNEVEN_TOL
            assert not row[it[t, s]:].any(), "0 behind the set-up's own stop"
        assert got["residual"][t, 1, it[t, 0]] > 0, "the free set-up goes on where the clamped one has stopped"


# ---------------------------------------------------------------------------------------------- E: later trips
def test_later_trips_of_the_pair_kernels(monkeypatch):
    """NSK_BP_GRID_CAP is read at each call: the same process runs the graph as is and with one block a launch and set-up"""
    want = lat.mirror("trips", lat.TRIP_SETTING)
    nsteps, iters, warm, tol, normalize, reg = lat.TRIP_SETTING
    got = []
    for cap in (None, "1"):
        monkeypatch.delenv("NSK_DIAG", raising=False)
        monkeypatch.delenv("NSK_BP_GRID_CAP", raising=False)
        if cap:
            monkeypatch.setenv("NSK_DIAG", "1")
            monkeypatch.setenv("NSK_BP_GRID_CAP", cap)
        d, damping = _dev("trips")
        d.setup_both()
        o = d.steps(nsteps, iters, damping, tol, warm, lat.step_of(normalize), lat.DECAY, reg, normalize)
        _check(o, want, cap)
        _check_state(d, want, cap)
        got.append([o["gmax"], o["residual"], o["moments"].astype(np.float64), d.weights()] +
                   [d.get(w, s) for s in (0, 1) for w in (_lib.BP_THETA, _lib.BP_F2V, _lib.BP_V2F)])
    for a, b in zip(*got):
        _same(a, b, "capped against uncapped")


# ---------------------------------------------------------------------------------------------- F: continuation
def test_a_second_call_continues_and_runs_follow_under_the_learned_weights():
    name, setting = "grid5x5_third", lat.SETTINGS[3]            # 3 steps of 6 iterations, warm, tol 0, normalised, reg 0.01
    nsteps, iters, warm, tol, normalize, reg = setting
    p = lat.pair(name)
    whole = lat.mirror(name, setting)
    d, damping = _dev(name)
    d.setup_both()
    s0 = lat.step_of(normalize)
    a = d.steps(2, iters, damping, tol, 1, s0, lat.DECAY, reg, normalize)
    b = d.steps(1, iters, damping, tol, 1, (s0 * lat.DECAY) * lat.DECAY, lat.DECAY, reg, normalize)
    _check({k: np.concatenate([a[k], b[k]]) for k in a}, whole, "two calls")
    _check_state(d, whole, "two calls")
    # nsk_bp_run continues either set-up under the learned weights
    for slot in (0, 1):
        assert d.select(slot) == _lib.OK
        n, res = d.run(3, damping)
        r = p.side[slot].run(whole["w"], 3, damping, messages=whole["messages"][slot])
        _same(res, r["residual"], ("a run behind the steps", slot))
        _same(d.get(_lib.BP_V2F), r["v2f"], ("v2f", slot))


def test_sweeps_behind_the_steps_run_under_the_learned_weights():
    """weights_dirty: a handle that swept before the steps must rebuild what derives from the weights"""
    build, hbv, damping = lat.CASES["grid5x5_third"]
    d = Dev(build(), hbv)
    _, tw = session(build(), seed=SEED, head_by_vid=hbv)
    d.fg._push(0, 0)
    d.fg._sweep(3, False, False)
    d.setup_both(push=False)
    d.steps(3, 4, damping, 0.0, 1, 2.0, lat.DECAY, 0.0, 1)
    for slot in (1, 0):
        assert d.select(slot) == _lib.OK and d.L.nsk_bp_clear(d.h) == _lib.OK
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


# ---------------------------------------------------------------------------------------------- G: the ledger, refusals
def test_the_ledger_and_the_refusals():
    d, damping = _dev("mixed_cat")
    d.fg.log_potential()
    d.weights()
    before = d.bytes()
    # no set-up, or only one of the two: refused
    assert d.steps_rc() == _lib.E_INVALID and "slot 0" in d.error()
    assert d.setup(0, 0) == _lib.OK               # (log_potential pushed the state)
    assert d.steps_rc() == _lib.E_INVALID and "slot 1" in d.error()
    assert d.bytes() == before + d.info[0].device_bytes
    assert d.L.nsk_bp_clear(d.h) == _lib.OK
    assert d.setup(1, 1) == _lib.OK
    assert d.steps_rc() == _lib.E_INVALID and "slot 0" in d.error()
    assert d.selected() == 1 and d.bytes() == before + d.info[1].device_bytes
    assert d.setup(0, 0) == _lib.OK
    held = d.bytes()
    assert held == before + d.info[0].device_bytes + d.info[1].device_bytes
    theta0, w0 = [d.get(_lib.BP_THETA, s) for s in (0, 1)], d.weights()
    # every refusal allocates nothing and enqueues nothing: the list of test_bp_learn_gpu.py without the target's entries
    nan, inf = float("nan"), float("inf")
    refused = [dict(nsteps=0), dict(nsteps=4097), dict(iters=0), dict(iters=4097),
               dict(nsteps=4096, iters=17), dict(damping=1.0), dict(damping=-0.1), dict(damping=nan), dict(tol=-1.0), dict(tol=nan),
               dict(warm=2), dict(warm=-1), dict(normalize=2), dict(step=nan), dict(step=inf), dict(decay=nan), dict(decay=inf),
               dict(reg=nan), dict(reg=inf), dict(reg=-1e-3)]
    for kw in refused:
        assert d.steps_rc(**kw) == _lib.E_INVALID, kw
        assert d.bytes() == held, kw
    _same(d.weights(), w0, "weights after the refusals")
    for s in (0, 1):
        _same(d.get(_lib.BP_THETA, s), theta0[s], "theta after the refusals")
    # every output is optional, and the per-call buffers are gone afterwards
    assert d.steps_rc(nsteps=2, iters=3, damping=damping) == _lib.OK
    assert d.bytes() == held
    assert not np.array_equal(d.weights(), w0)
    for k in range(5):
        out = [None] * 5
        shape = ((2,), (2, 2), (2, 2, 3), (2, 2, d.nw), (2, 2))[k]
        out[k] = np.zeros(shape, np.float64 if k in (0, 2) else np.int64)
        assert d.steps_rc(nsteps=2, iters=3, damping=damping, out=out) == _lib.OK, k
        assert d.bytes() == held
    d.steps(2, 3, damping, 0.0, 1, 0.1, lat.DECAY, 0.0, 1)
    assert d.bytes() == held
    for slot in (1, 0):
        assert d.select(slot) == _lib.OK and d.L.nsk_bp_clear(d.h) == _lib.OK
    assert d.bytes() == before and d.selected() == 0
    assert d.steps_rc() == _lib.E_INVALID


# ---------------------------------------------------------------------------------------------- H: the Python API
def test_learn_bp_latent():
    name = "grid5x5_third"
    p = lat.pair(name)
    build, hbv, damping = lat.CASES[name]
    E, I = 4, 5
    want = p.learn(p.w0, E, I, damping, 1e-9, 1, 0.5, 0.9, 0.01, 1)
    _, fg = session(build(), seed=SEED, head_by_vid=hbv)
    fg.log_potential()                              # (the records the set-ups share are in place ...
    fg._pull(0, 0, values=False, count=False)       # ... and the staging of the weight transfers)
    before = fg.info()["device_bytes"]
    res = fg.learn_bp(E, 0.5, decay=0.9, reg_param=0.01, iters=I, damping=damping, latent=True, moments=True)
    assert set(res) == {"grad_max", "iters", "converged", "residual", "skipped", "factors_per_weight", "moments"}
    assert res["iters"].shape == res["converged"].shape == res["skipped"].shape == (E, 2)
    assert res["residual"].shape == (E, 2, I) and res["moments"].shape == (E, 2, p.nw) and res["grad_max"].shape == (E,)
    _same(fg.weight_value[0], want["w"], "weights")
    _same(res["grad_max"], want["gmax"], "grad_max")
    _same(res["residual"], want["residual"], "residual")
    assert np.array_equal(res["iters"], np.abs(want["iters"])) and np.array_equal(res["converged"], want["iters"] > 0)
    assert res["converged"].dtype == np.bool_ and res["moments"].dtype == np.int64
    assert np.array_equal(res["moments"], want["moments"]) and not res["skipped"].any()
    assert np.array_equal(res["factors_per_weight"], p.nfac)
    assert set(fg.learn_bp(1, 0.1, latent=True)) == {"grad_max", "iters", "converged", "residual", "skipped", "factors_per_weight"}
    # both set-ups are gone and slot 0 is selected, also when the call raises
    L, h = _lib.lib(), fg._engine()

    def clean():
        assert fg.info()["device_bytes"] == before and L.nsk_bp_selected(h) == 0
        for slot in (1, 0):
            assert L.nsk_bp_select(h, slot) == _lib.OK and L.nsk_bp_refresh(h) == _lib.E_INVALID
    clean()
    with pytest.raises(ValueError):
        fg.learn_bp(2, 0.1, damping=1.0, latent=True)
    clean()
    w = fg.weight_value[0].copy()
    with pytest.raises(ValueError):
        fg.learn_bp(2, 0.1, latent=True, target=np.zeros(p.nw))
    with pytest.raises(ValueError):
        fg.learn_bp(0, 0.1, latent=True)
    clean()
    _same(fg.weight_value[0], w, "a refused call leaves the weights")


def test_learn_bp_without_latent_is_what_it_was():
    name, setting = "grid5x5_clamped", bl.SETTINGS[6]
    nsteps, iters, warm, tol, normalize, reg = setting
    build, hbv, damping = bl.LEARN[name]
    want = bl.learn_mirror(name, setting)
    _, fg = session(build(), seed=SEED, head_by_vid=hbv)
    res = fg.learn_bp(nsteps, 0.5, decay=bl.DECAY, reg_param=reg, iters=iters, damping=damping, tol=tol, warm=bool(warm),
                      sample_evidence=False, target=bl.learn_target(name), normalize=bool(normalize), moments=True)
    assert set(res) == {"grad_max", "iters", "converged", "residual", "skipped", "target", "factors_per_weight", "moments"}
    assert res["iters"].shape == (nsteps,) and res["residual"].shape == (nsteps, iters)
    _same(fg.weight_value[0], want["w"], "weights")
    _same(res["grad_max"], want["gmax"], "grad_max")
    _same(res["residual"], want["residual"], "residual")
    assert np.array_equal(res["moments"], want["moments"]) and np.array_equal(res["iters"], np.abs(want["iters"]))
    assert _lib.lib().nsk_bp_selected(fg._engine()) == 0


def test_bp_log_evidence():
    build, hbv, _ = lat.CASES["chain9_ends"]
    p = lat.pair("chain9_ends")
    _, fg = session(build(), seed=SEED, head_by_vid=hbv)
    res = fg.bp_log_evidence()
    assert set(res) == {"log_evidence", "log_z_clamped", "log_z_free", "converged", "iters"}
    want = p.log_z(p.w0)                            # the numpy composition: bethe_log_z of either mirror run
    runs = [ln.run(p.w0, 100, 0.0, 1e-9) for ln in p.side]
    assert res["log_z_clamped"] == want[0] and res["log_z_free"] == want[1] and res["log_evidence"] == want[0] - want[1]
    assert res["converged"].shape == (2,) and res["converged"].dtype == np.bool_ and res["converged"].all()
    assert res["iters"].dtype == np.int64 and res["iters"].tolist() == [r["iters"] for r in runs]
    _, _, zc, zf = p.exact(p.w0)                    # a forest: exact (the bound of tests/test_bp_latent_cpu.py)
    assert abs(res["log_evidence"] - (zc - zf)) <= 1e-12
    assert _lib.lib().nsk_bp_refresh(fg._engine()) == _lib.E_INVALID       # nothing is left set up
