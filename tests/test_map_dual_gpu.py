"""Dual MAP bounds on the device (nsk_bp_dual_run / nsk_bp_dual_download / nsk_bp_dual_decode, FactorGraph.map_dual) against
the numpy mirror diagnostics.msd_iterate / msd_terms (tests/map_dual.py), bit for bit: the same sums in the same order,
maxima whose order does not matter.  tests/test_map_dual_cpu.py ties the mirror to enumeration."""

import ctypes as C

import numpy as np
import pytest

import bp
import bp_map
import map_dual
from numbskull_amd import _lib
from test_bp_gpu import Dev, _same, SEED
from util import session

pytestmark = pytest.mark.gpu


class DualDev(Dev):
    def dual_run(self, sweeps, tol=0.0, warm=0):
        n, res = C.c_int64(0), np.full(sweeps, -1.0)
        _lib.check(self.L.nsk_bp_dual_run(self.h, sweeps, tol, warm, C.byref(n), _lib.ptr(res)))
        return n.value, res

    def dual_get(self, what):
        nv, nf = len(self.fg.variable), len(self.fg.factor)
        n = (self.info.nmsg, self.info.nmsg, nf + nv, int(self.fg.variable["cardinality"].sum()))[what]
        out = np.zeros(n)
        _lib.check(self.L.nsk_bp_dual_download(self.h, what, _lib.ptr(out)))
        return out

    def routes(self):
        out = np.zeros(2, np.int64)
        _lib.check(self.L.nsk_bp_dual_routes(self.h, _lib.ptr(out)))
        return out.tolist()

    def decode(self):
        ties = C.c_int64(-1)
        _lib.check(self.L.nsk_bp_dual_decode(self.h, _lib.BUF_VALUE, 0, C.byref(ties)))
        self.fg._pull(0, 0, weights=False, count=False)
        return self.fg.var_value[0].astype(np.int64), ties.value


def _dev(name):
    g, hbv, sev = bp_map.graph(name)
    d = DualDev(g, hbv)
    assert d.setup(sev) == _lib.OK, d.error()
    return d


def _check(d, r, what):
    _same(d.dual_get(_lib.BP_DUAL_D), r["D"], (what, "D"))
    _same(d.dual_get(_lib.BP_DUAL_M), r["M"], (what, "M"))
    _same(d.dual_get(_lib.BP_DUAL_TERMS), np.concatenate([r["tf"], r["tv"]]), (what, "terms"))
    _same(d.dual_get(_lib.BP_DUAL_BV), r["Bv"], (what, "Bv"))


@pytest.mark.parametrize("name", bp_map.CASES)
def test_sweeps_equal_the_mirror_bit_for_bit(name):
    d = _dev(name)
    counts, _, cls, _ = map_dual.plan(name)
    got = np.zeros(len(cls), np.int32)
    _lib.check(d.L.nsk_bp_dual_classes(d.h, _lib.ptr(got)))
    assert d.routes() == counts and np.array_equal(got, cls)
    if name == "routes":
        assert min(counts) > 0
    for sweeps in (1, 2, 8):
        for tol in (0.0, 1e-9):
            r = map_dual.mirror(name, sweeps, tol)
            n, res = d.dual_run(sweeps, tol)                # (warm = 0: every run starts cold)
            assert n == r["sweeps"], (name, sweeps, tol)
            _same(res, r["residual"], (name, sweeps, tol))
            _check(d, r, (name, sweeps, tol))


_OWN = {"trips": bp.trips_grid, "grid40": map_dual.grid40}


@pytest.mark.parametrize("name,knob,cap", [(n, k, c) for n in ("routes", "trips") for k, c in (("0", None), ("4096", None), (None, "1"), ("0", "1"))] +
                         [("grid40", None, "1")])
def test_either_route_and_later_trips_give_the_same_bits(name, knob, cap, monkeypatch):
    """trips: 2 classes of about 245 variables (a wave an item: 62 trips of a capped block; a lane an item: one); grid40:
    800 lane items a class, four trips of a capped block; routes under the cap: several waves' items per class"""
    monkeypatch.setenv("NSK_DIAG", "1")
    for k, v in (("NSK_DUAL_LANE_MAX", knob), ("NSK_BP_GRID_CAP", cap)):
        if v is not None:
            monkeypatch.setenv(k, v)
    d = DualDev(_OWN[name]()) if name in _OWN else _dev(name)
    if name in _OWN:
        assert d.setup() == _lib.OK, d.error()
    lane, wave = d.routes()
    if knob is not None:
        assert (wave > 0 and lane == 0) if knob == "0" else lane > 0
    if name == "grid40":
        assert wave == 0 and bp.trips(lane // 2, 1) >= 3
    r = map_dual.mirror(name, bp.TRIP_ITERS)
    n, res = d.dual_run(bp.TRIP_ITERS)
    _same(res, r["residual"], (knob, cap))
    _check(d, r, (knob, cap))


@pytest.mark.parametrize("name", bp_map.TREES + ("clamped_grid", "mixed_free"))
def test_the_summed_theta_of_an_assignment_is_its_log_potential(name):
    """what makes `upper` comparable with log_potential(): the conditioned tables and the factors without a free member
    carry the clamped part"""
    x, total, margin = map_dual.best(name)
    g, hbv, _ = bp_map.graph(name)
    _, fg = session(g, seed=SEED, head_by_vid=hbv)
    fg.var_value[0][:] = x
    assert abs(fg.log_potential() - total) <= margin


def test_a_set_up_with_wide_factors_is_refused():
    import bp_wide
    _, fg = session(bp_wide.graph(2, 20)[0])
    L, h = _lib.lib(), fg._engine()
    fg._push(0, 0)
    _lib.check(L.nsk_bp_setup_wide(h, _lib.BUF_VALUE, 0, 0, None, None))
    z = np.zeros(len(fg.variable), np.int64)
    calls = [L.nsk_bp_dual_run(h, 2, 0.0, 0, C.byref(C.c_int64(0)), None), L.nsk_bp_dual_routes(h, _lib.ptr(z)),
             L.nsk_bp_dual_classes(h, _lib.ptr(z.astype(np.int32))), L.nsk_bp_dual_download(h, 0, _lib.ptr(z)),
             L.nsk_bp_dual_decode(h, _lib.BUF_VALUE, 0, None)]
    assert all(rc == _lib.E_INVALID for rc in calls), calls
    assert b"wide factors" in L.nsk_last_error()
    L.nsk_bp_clear(h)


def test_a_warm_run_continues_and_the_arrays_go_with_the_set_up():
    name = "clamped_grid"
    g, hbv, sev = bp_map.graph(name)
    d = DualDev(g, hbv)
    d.fg.log_potential()
    d.fg._push(0, 0)
    before = d.bytes()
    assert d.setup(sev, push=False) == _lib.OK
    held = d.bytes()
    for call in (lambda: d.L.nsk_bp_dual_download(d.h, 0, None), lambda: d.L.nsk_bp_dual_decode(d.h, _lib.BUF_VALUE, 0, None)):
        assert call() == _lib.E_INVALID                         # no run yet
    whole = map_dual.mirror(name, 8)
    n1, r1 = d.dual_run(3, warm=1)                              # (new arrays start cold whatever `warm` says)
    grown = d.bytes()
    n2, r2 = d.dual_run(5, warm=1)
    assert (n1, n2) == (-3, -5) and d.bytes() == grown >= held + 16 * d.info.nmsg
    _same(np.concatenate([r1, r2]), whole["residual"], "warm")
    _check(d, whole, "warm")
    for sweeps, tol, warm in ((0, 0.0, 0), (4097, 0.0, 0), (3, -1.0, 0), (3, 0.0, 2)):
        assert d.L.nsk_bp_dual_run(d.h, sweeps, tol, warm, C.byref(C.c_int64(0)), None) == _lib.E_INVALID
    assert d.L.nsk_bp_clear(d.h) == _lib.OK and d.bytes() == before
    assert d.L.nsk_bp_dual_run(d.h, 3, 0.0, 0, C.byref(C.c_int64(0)), None) == _lib.E_INVALID


@pytest.mark.parametrize("name", bp_map.TREES + ("symmetric", "clamped_grid"))
def test_decode(name):
    d = _dev(name)
    d.dual_run(40)
    x, ties = d.decode()
    want = map_dual.mirror(name, 40)["decode"]
    assert (x.tolist(), ties) == (want[0].tolist(), want[1])
    if name == "symmetric":
        assert ties > 0


def test_python_api():
    _, fg = session(bp_map.graph("tree")[0], seed=SEED)
    res = fg.map_dual(max_sweeps=400, tol=1e-12)            # (the mirror needs 211 sweeps for this residual)
    assert set(res) == {"upper", "lower", "gap", "values", "sweeps", "converged", "residual", "ties", "offsets", "reparametrised",
                        "decoded_log_potential", "icm_sweeps_run", "icm_converged"}
    best, total, margin = map_dual.best("tree")
    assert res["converged"] and abs(res["gap"]) <= margin and abs(res["lower"] - total) <= margin
    assert np.array_equal(res["values"], best) and np.array_equal(fg.var_value[0], best) and res["lower"] == fg.log_potential()
    import temper
    _, lg = session(temper.clamped_grid(), seed=SEED)
    res = lg.map_dual(max_sweeps=50)
    assert res["lower"] <= res["upper"] and res["lower"] >= res["decoded_log_potential"]
    assert res["upper"] >= lg.map_bp(max_iters=30, damping=0.5, polish=True)["log_potential"]
    for kw in ({"max_sweeps": 0}, {"var_copy": "all"}):
        with pytest.raises(ValueError):
            lg.map_dual(**kw)
