"""The residual schedule on the device (nsk_bp_residual_run) against nsk_bp_run at frac = 0 and against the numpy mirror
diagnostics.rbp_iterate with the oracle's exp_det (tests/bp_residual.py), bit for bit.  tests/test_bp_residual_cpu.py ties
the mirror to enumeration and shows that every case here is lively."""

import ctypes as C

import numpy as np
import pytest

import bp_residual as br
from numbskull_amd import _lib
from util import session

pytestmark = pytest.mark.gpu


def _same(a, b, what):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert np.array_equal(a.view(np.int64), b.view(np.int64)), (what, float(np.nanmax(np.abs(a - b))))


class Dev(object):
    def __init__(self, case):
        build, hbv, self.sev = case
        _, self.fg = session(build(), seed=77, head_by_vid=hbv)
        self.L, self.h = _lib.lib(), self.fg._engine()
        self.info = _lib.BpInfo()
        self.fg._push(0, 0)
        self.setup()

    def setup(self):
        _lib.check(self.L.nsk_bp_setup(self.h, _lib.BUF_VALUE, 0, self.sev, C.byref(self.info)))

    def flood(self, iters, damping=0.0, tol=0.0):
        n, res = C.c_int64(0), np.full(iters, -1.0)
        _lib.check(self.L.nsk_bp_run(self.h, iters, damping, tol, C.byref(n), _lib.ptr(res)))
        return {"rounds": n.value, "residual": res}

    def residual(self, rounds, frac, damping=0.0, tol=0.0, warm=0):
        n, res = C.c_int64(0), np.full(rounds, -1.0)
        upd, rec = np.full(rounds, -1, np.int64), np.full(rounds, -1, np.int64)
        rc = self.L.nsk_bp_residual_run(self.h, rounds, frac, damping, tol, warm, C.byref(n), _lib.ptr(res), _lib.ptr(upd), _lib.ptr(rec))
        assert rc == _lib.OK, self.L.nsk_last_error().decode()
        return {"rounds": n.value, "residual": res, "updates": upd, "recomputed": rec}

    def state(self):
        i = self.info
        out = {"f2v": np.zeros(i.nmsg), "v2f": np.zeros(i.nmsg), "factor_beliefs": np.zeros(i.ntable),
               "beliefs": np.zeros(int(self.fg.variable["cardinality"].sum()))}
        for key, what in (("f2v", _lib.BP_F2V), ("v2f", _lib.BP_V2F), ("factor_beliefs", _lib.BP_FACTOR_BELIEFS)):
            _lib.check(self.L.nsk_bp_download(self.h, what, _lib.ptr(out[key])))
        _lib.check(self.L.nsk_bp_beliefs(self.h, None, 0, _lib.ptr(out["beliefs"])))
        return out

    bytes = lambda self: self.fg.info()["device_bytes"]      # noqa: E731


def _check(d, got, want, what, counts=True):
    assert got["rounds"] == want.get("rounds", want.get("iters")), what
    _same(got["residual"], want["residual"], (what, "residual"))
    for k in ("updates", "recomputed") if counts else ():
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    state = d.state()
    for k in ("f2v", "v2f", "beliefs", "factor_beliefs"):
        _same(state[k], want[k], (what, k))


@pytest.mark.parametrize("damping", [0.0, 0.5])
@pytest.mark.parametrize("name", sorted(br.FLOOD))
def test_frac_zero_is_the_flooding_schedule(name, damping):
    d = Dev(br.FLOOD[name])
    for n in (1, 2, 7):
        for tol in (0.0, 1e-9):
            d.setup()
            want = d.flood(n, damping, tol)
            want.update(d.state())
            d.setup()
            _check(d, d.residual(n, 0.0, damping, tol), want, (name, damping, n, tol), counts=False)


@pytest.mark.parametrize("name,frac,damping", [(n, f, d) for n in ("grid5", "cat17", "hubs") for f in (0.1, 0.5) for d in (0.0, 0.5)]
                         + [("grid_int32", 0.5, 0.0)])
def test_rounds_equal_the_mirror(name, frac, damping):
    d = Dev(br.CASES[name])
    assert d.fg.info()["value_bytes"] == (4 if name == "grid_int32" else 1)
    for n in (1, 2, 3, 40):
        _check(d, d.residual(n, frac, damping), br.mirror(name, n, frac, damping), (name, frac, damping, n))


@pytest.mark.parametrize("name,rounds", [("grid5", 40), ("trips", 4)])
def test_later_trips_through_the_queues(name, rounds, monkeypatch):
    """one block a launch: the 24 x 24 grid makes three trips and more"""
    monkeypatch.setenv("NSK_DIAG", "1")
    monkeypatch.setenv("NSK_BP_GRID_CAP", "1")
    d = Dev(br.CASES[name])
    _check(d, d.residual(rounds, 0.5), br.mirror(name, rounds, 0.5), name)


def test_a_warm_call_continues_and_flooding_takes_over():
    m, d = br.model("grid5"), Dev(br.CASES["grid5"])
    a = d.residual(3, 0.5, 0.5)
    b = d.residual(4, 0.5, 0.5, warm=1)
    whole = br.mirror("grid5", 7, 0.5, 0.5)
    assert a["rounds"] == -3 and b["rounds"] == -4
    assert np.array_equal(a["recomputed"], whole["recomputed"][:3]) and np.array_equal(b["recomputed"][1:], whole["recomputed"][4:])
    assert b["recomputed"][0] == d.info.nedges and np.array_equal(np.concatenate([a["updates"], b["updates"]]), whole["updates"])
    _check(d, {"rounds": -7, "residual": np.concatenate([a["residual"], b["residual"]])}, whole, "3 + 4 rounds", counts=False)
    _check(d, d.flood(2, 0.5), m.run(2, 0.5, messages=(whole["f2v"], whole["v2f"])), "flooding behind", counts=False)
    _check(d, d.residual(7, 0.5, 0.5), whole, "a cold start resets the messages")


def test_refusals_and_the_ledger():
    d = Dev(br.CASES["hubs"])
    base = d.bytes()
    n = C.c_int64(0)
    run = lambda *a: d.L.nsk_bp_residual_run(d.h, *(a + (C.byref(n), None, None, None)))      # noqa: E731
    for args in ((0, 0.5, 0.0, 0.0, 0), (4097, 0.5, 0.0, 0.0, 0), (3, -0.1, 0.0, 0.0, 0), (3, 1.5, 0.0, 0.0, 0), (3, float("nan"), 0.0, 0.0, 0),
                 (3, 0.5, 1.0, 0.0, 0), (3, 0.5, 0.0, -1.0, 0), (3, 0.5, 0.0, 0.0, 2)):
        assert run(*args) == _lib.E_INVALID and d.bytes() == base, args
    assert d.L.nsk_bp_residual_run(d.h, 3, 0.5, 0.0, 0.0, 0, None, None, None, None) == _lib.E_INVALID
    assert run(3, 0.5, 0.0, 0.0, 0) == _lib.OK and n.value == -3        # every output array may be NULL
    held = d.bytes()
    assert held > base
    assert run(3, 1.0, 0.0, 0.0, 1) == _lib.OK and d.bytes() == held    # the second call allocates nothing that stays
    assert d.L.nsk_bp_clear(d.h) == _lib.OK and d.bytes() == base - d.info.device_bytes
    assert run(3, 0.5, 0.0, 0.0, 0) == _lib.E_INVALID                   # nothing is set up


def test_python_api():
    m = br.model("grid5")
    _, fg = session(br.CASES["grid5"][0](), seed=77)
    res = fg.belief_propagation(max_iters=40, tol=0.0, schedule="residual", factor_beliefs=True)
    r = br.mirror("grid5", 40, 0.5)
    assert res["iters"] == abs(r["rounds"]) and res["converged"] == (r["rounds"] > 0) and res["log_z"] == m.log_z(r)
    for k in ("beliefs", "residual", "factor_beliefs"):
        _same(res[k], r[k], k)
    assert np.array_equal(res["updates"], r["updates"]) and np.array_equal(res["recomputed"], r["recomputed"])
    flood = fg.belief_propagation(max_iters=7, tol=0.0)
    _same(fg.belief_propagation(max_iters=7, tol=0.0, schedule="residual", frac=0.0)["beliefs"], flood["beliefs"], "frac 0")
    a = fg.bp_weight_moments(max_iters=7, tol=0.0, counts=True)
    b = fg.bp_weight_moments(max_iters=7, tol=0.0, counts=True, schedule="residual", frac=0.0)
    assert "updates" not in flood and np.array_equal(a["moments"], b["moments"]) and a["moments"].any() and a["iters"] == b["iters"] == 7
    for kw in ({"schedule": "splash"}, {"schedule": "residual", "frac": 1.5}):
        with pytest.raises(ValueError):
            fg.belief_propagation(**kw)
