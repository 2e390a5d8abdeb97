"""Max-product belief propagation on the device (nsk_bp_map_run / nsk_bp_map_decode, FactorGraph.map_bp) against the
numpy mirror diagnostics.ms_iterate / ms_decode (tests/bp_map.py), bit for bit: the same sums in the same order, maxima
whose order does not matter.  tests/test_bp_map_cpu.py ties the mirror to enumeration."""

import ctypes as C

import numpy as np
import pytest

import bp
import bp_map
from numbskull_amd import _lib
from numbskull_amd.diagnostics import ms_decode
from test_bp_gpu import Dev, _same, _check_state, SEED
from util import session

pytestmark = pytest.mark.gpu


class MapDev(Dev):
    def map_run(self, iters, damping=0.0, tol=0.0, warm=0):
        n, res = C.c_int64(0), np.full(iters, -1.0)
        _lib.check(self.L.nsk_bp_map_run(self.h, iters, damping, tol, warm, C.byref(n), _lib.ptr(res)))
        return n.value, res

    def _out(self, fn, n, dtype, *a):
        out = np.zeros(n, dtype)
        _lib.check(fn(self.h, *a, _lib.ptr(out)))
        return out

    def map_get(self, what):
        return self._out(self.L.nsk_bp_map_download, self.info.nmsg, np.float64, what)

    def marginals(self):
        return self._out(self.L.nsk_bp_map_marginals, int(self.fg.variable["cardinality"].sum()), np.float64, None, 0)

    def routes(self):
        return self._out(self.L.nsk_bp_map_routes, 3, np.int64).tolist()

    def decode(self):
        ties = C.c_int64(-1)
        _lib.check(self.L.nsk_bp_map_decode(self.h, _lib.BUF_VALUE, 0, C.byref(ties)))
        self.fg._pull(0, 0, weights=False, count=False)
        return self.fg.var_value[0].astype(np.int64), ties.value


def _dev(name):
    g, hbv, sev = bp_map.graph(name)
    d = MapDev(g, hbv)
    assert d.setup(sev) == _lib.OK, d.error()
    return d, sev


def _check_map(d, r, what):
    _same(d.map_get(_lib.BP_MAP_F), r["F"], (what, "F"))
    _same(d.map_get(_lib.BP_MAP_V), r["V"], (what, "V"))
    _same(d.marginals(), r["max_marginals"], (what, "max-marginals"))


@pytest.mark.parametrize("damping", [0.0, 0.5])
@pytest.mark.parametrize("name", bp_map.CASES)
def test_iterations_equal_the_mirror_bit_for_bit(name, damping):
    m = bp_map.model(name)
    d, sev = _dev(name)
    _same(d.get(_lib.BP_THETA), m.theta, "theta")
    want = [0, 0, 0]
    for shape in m.layout["shapes"]:
        if shape:
            lane = int(np.prod(shape)) < _lib.BP_MAP_LANE_TABLE and sum(shape) <= _lib.BP_MAP_LANE_CARDS
            want[0 if lane else (1 if sum(shape) <= _lib.BP_MAP_LDS else 2)] += 1
    assert d.routes() == want
    if name == "routes":
        sizes = {int(np.prod(s)) for s in m.layout["shapes"] if s}
        assert {4096, 64, 63, 81, 68, 34, 600, 1200, 4, 9, 21, 36, 2} <= sizes and want[1:] == [6, 4] and want[0] > 0
    for iters in (1, 2, 8):
        for tol in (0.0, 1e-9):
            r = bp_map.mirror(name, iters, damping, tol)
            n, res = d.map_run(iters, damping, tol)         # (warm = 0: every run starts cold)
            what = (name, damping, iters, tol)
            assert n == r["iters"], what
            _same(res, r["residual"], what)
            _check_map(d, r, what)


def test_later_trips_of_every_kernel(monkeypatch):
    m = bp_map.model("trips")
    r = bp_map.mirror("trips", bp.TRIP_ITERS, 0.0, 0.0)
    got = []
    for cap in (None, "1"):
        monkeypatch.delenv("NSK_DIAG", raising=False)
        monkeypatch.delenv("NSK_BP_GRID_CAP", raising=False)
        if cap:
            monkeypatch.setenv("NSK_DIAG", "1")
            monkeypatch.setenv("NSK_BP_GRID_CAP", cap)
        d = MapDev(bp.trips_grid())
        assert d.setup() == _lib.OK, d.error()
        assert bp.trips(d.routes()[0], 1) >= 3
        n, res = d.map_run(bp.TRIP_ITERS)
        _same(res, r["residual"], cap)
        _check_map(d, r, cap)
        x, ties = d.decode()
        want = ms_decode(m.layout, r["max_marginals"], m.x)
        assert np.array_equal(x, want[0]) and ties == want[1], cap
        got.append((d.map_get(0), d.map_get(1), d.marginals(), res, x.astype(np.float64)))
    for a, b in zip(*got):
        _same(a, b, "capped against uncapped")


@pytest.mark.parametrize("name", bp_map.TREES + ("symmetric",))
def test_decode(name):
    d, _ = _dev(name)
    n, _ = d.map_run(40)
    assert n == bp_map.mirror(name, 40, 0.0, 0.0)["iters"] > 0
    x, ties = d.decode()
    # (symmetric: the smallest value among the maxima; the row held [1, 1])
    assert (x.tolist(), ties) == (([0, 0], 2) if name == "symmetric" else (bp_map.enumerate_map(name)[0].tolist(), 0))


def test_sum_product_is_untouched_and_clear_returns_the_bytes():
    name = "mixed_free"
    m = bp.model(name)
    d, sev = _dev(name)
    d.fg.log_potential()
    assert d.L.nsk_bp_clear(d.h) == _lib.OK
    before = d.bytes()
    assert d.setup(sev, push=False) == _lib.OK
    held = d.bytes()
    assert d.L.nsk_bp_map_download(d.h, 0, None) == _lib.E_INVALID       # no run yet
    r = bp.mirror(name, 2, 0.0, 0.0)
    d.run(2)
    d.map_run(3)
    _check_state(d, m, r, "after a max-product run")
    assert d.bytes() - held >= 16 * d.info.nmsg + 8 * d.info.nbelief
    grown = d.bytes()
    d.map_run(3)
    assert d.bytes() == grown                                # the arrays are the set-up's; the residuals the call's
    assert d.L.nsk_bp_clear(d.h) == _lib.OK and d.bytes() == before
    assert d.L.nsk_bp_map_run(d.h, 3, 0.0, 0.0, 0, C.byref(C.c_int64(0)), None) == _lib.E_INVALID
    assert d.L.nsk_bp_map_routes(d.h, _lib.ptr(np.zeros(3, np.int64))) == _lib.E_INVALID


def test_a_warm_run_continues_where_a_longer_one_would_be():
    d, _ = _dev("clamped_grid")
    whole = bp_map.mirror("clamped_grid", 7, 0.5, 0.0)
    n1, r1 = d.map_run(3, 0.5, warm=1)                       # (new arrays start cold whatever `warm` says)
    n2, r2 = d.map_run(4, 0.5, warm=1)
    assert n1 == -3 and n2 == -4
    _same(np.concatenate([r1, r2]), whole["residual"], "warm")
    _check_map(d, whole, "warm")
    n, res = d.map_run(1, 0.5, warm=0)
    _same(res, whole["residual"][:1], "cold again")
    for iters, damping, tol, warm in ((0, 0.0, 0.0, 0), (4097, 0.0, 0.0, 0), (3, 1.0, 0.0, 0), (3, 0.0, -1.0, 0), (3, 0.0, 0.0, 2)):
        assert d.L.nsk_bp_map_run(d.h, iters, damping, tol, warm, C.byref(C.c_int64(0)), None) == _lib.E_INVALID


def test_python_api():
    _, fg = session(bp_map.graph("tree")[0], seed=SEED)
    res = fg.map_bp(tol=0.0)
    assert set(res) == {"values", "log_potential", "iters", "converged", "residual", "ties", "offsets", "max_marginals"}
    best = bp_map.enumerate_map("tree")[0]
    r = bp_map.mirror("tree", 40, 0.0, 0.0)
    assert res["iters"] == r["iters"] and res["converged"] is True and res["ties"] == 0
    assert np.array_equal(res["values"], best) and np.array_equal(fg.var_value[0], best) and res["log_potential"] == fg.log_potential()
    _same(res["max_marginals"], r["max_marginals"], "max-marginals")
    import temper
    _, lg = session(temper.clamped_grid(), seed=SEED)
    res = lg.map_bp(max_iters=30, damping=0.5, polish=True)
    assert {"decoded_log_potential", "sweeps", "icm_converged"} <= set(res)
    assert res["log_potential"] >= res["decoded_log_potential"] and res["log_potential"] == lg.log_potential()
    assert np.array_equal(res["values"], lg.var_value[0])
    for kw in ({"max_iters": 0}, {"var_copy": "all"}, {"damping": 1.0}):
        with pytest.raises(ValueError):
            lg.map_bp(**kw)
