"""Tree-reweighted belief propagation on the device (nsk_bp_trw_run, FactorGraph.reweighted_bp / log_z_bounds) against
the numpy mirror diagnostics.trw_iterate (tests/trw.py).  Device and mirror perform the same operations in the same
order but for log and exp, so that comparison has a tolerance: 16 x the rule's own rounding noise -- the difference
between the float64 and the extended-precision run of the mirror -- plus 16 x 2^-52.  Everything the device is compared
with itself on (routes, warm starts, repeats) is bit for bit.  tests/test_trw_cpu.py ties the mirror to enumeration."""

import ctypes as C
import math

import numpy as np
import pytest

import bp
import trw
from numbskull_amd import _lib
from test_bp_gpu import Dev, _same
from util import session

pytestmark = pytest.mark.gpu

KEYS = ("LF", "LN", "beliefs", "factor_beliefs", "residual", "log_z")


class TrwDev(Dev):
    def __init__(self, name):
        m = trw.model(name)
        Dev.__init__(self, m.g, m.hbv)
        assert self.setup(m.sev) == _lib.OK, self.error()

    def trw_run(self, rho, iters, damping=0.0, tol=0.0, warm=0):
        n, res = C.c_int64(0), np.full(iters, -1.0)
        rc = self.L.nsk_bp_trw_run(self.h, _lib.ptr(np.ascontiguousarray(rho, np.float64)), iters, damping, tol, warm, C.byref(n), _lib.ptr(res))
        return rc, n.value, res

    def state(self, rho, iters, damping=0.0, tol=0.0, warm=0):
        """a run and every array it leaves, by the mirror's names"""
        rc, n, res = self.trw_run(rho, iters, damping, tol, warm)
        assert rc == _lib.OK, self.error()
        out = {"iters": n, "residual": res, "beliefs": np.zeros(int(self.fg.variable["cardinality"].sum()))}
        _lib.check(self.L.nsk_bp_trw_beliefs(self.h, None, 0, _lib.ptr(out["beliefs"])))
        nf, nv = len(self.fg.factor), len(self.fg.variable)
        for key, what, n in (("LF", _lib.BP_TRW_LF, self.info.nmsg), ("LN", _lib.BP_TRW_LN, self.info.nmsg),
                             ("factor_beliefs", _lib.BP_TRW_FACTOR_BELIEFS, self.info.ntable), ("terms", _lib.BP_TRW_TERMS, nf + nv)):
            out[key] = np.zeros(n)
            _lib.check(self.L.nsk_bp_trw_download(self.h, what, _lib.ptr(out[key])))
        out["log_z"] = math.fsum(out["terms"].tolist())
        return out

    def routes(self):
        counts = np.zeros(2, np.int64)
        _lib.check(self.L.nsk_bp_trw_routes(self.h, _lib.ptr(counts)))
        return counts.tolist()


def _same_state(a, b, what):
    for key in KEYS[:-1] + ("terms",):
        _same(a[key], b[key], (what, key))
    assert a["iters"] == b["iters"], what


@pytest.mark.parametrize("damping", [0.0, 0.5])
@pytest.mark.parametrize("name", trw.CASES)
def test_iterations_follow_the_mirror_within_its_rounding_noise(name, damping):
    d, rho, worst = TrwDev(name), trw.rho_of(name), 0.0
    for iters in trw.ITERS:
        got, want = d.state(rho, iters, damping), trw.mirror(name, iters, damping)
        for key in KEYS:        # (not `iters`: on a forest the changes end at exactly 0, one iteration sooner or later)
            err, tol = float(np.max(np.abs(np.asarray(got[key]) - want[key]))), trw.bound(name, key, iters, damping)
            worst = max(worst, 16 * err / (tol - 16 * trw.EPS)) if trw.WIDER and tol > 16 * trw.EPS else worst
            print(name, damping, iters, key, "error %.3g" % err, "bound %.3g" % tol)
            assert err <= tol, (name, damping, iters, key, err, tol)
    print(name, damping, "largest device error / spread: %.3g" % worst)


@pytest.mark.parametrize("name", trw.CASES)
def test_both_routes_give_the_same_bits(name, monkeypatch):
    rho, got = trw.rho_of(name), []
    nedged = sum(1 for s in trw.model(name).layout["shapes"] if s)
    monkeypatch.setenv("NSK_DIAG", "1")
    for knob, counts in (("4096", [nedged, 0]), ("0", [0, nedged])):
        monkeypatch.setenv("NSK_TRW_LANE_MAX", knob)
        d = TrwDev(name)
        assert d.routes() == counts
        got.append(d.state(rho, 30, 0.5))
    _same_state(got[0], got[1], name)


@pytest.mark.parametrize("name", sorted(bp.TREES))
def test_rho_one_is_belief_propagation_on_a_forest(name):
    m = bp.model(name)
    _, fg = session(m.g, head_by_vid=m.hbv)
    a, b = fg.belief_propagation(40, 0.0, 1e-12), fg.reweighted_bp(1.0, max_iters=40, damping=0.0, tol=1e-12)
    assert a["converged"] and b["converged"]
    for key in ("beliefs", "log_z"):
        err, tol = float(np.max(np.abs(np.asarray(a[key]) - b[key]))), trw.bound(name, key, 40, 0.0, "one", 1e-12)
        print(name, key, "error %.3g" % err, "bound %.3g" % tol)
        assert err <= tol, (name, key, err, tol)


@pytest.mark.parametrize("name", trw.BOUND)
def test_tree_weights_bound_log_z_from_above(name):
    m = trw.model(name)
    _, fg = session(m.g)
    r = fg.reweighted_bp("trees", trees=16, seed=3)
    assert r["converged"] and np.array_equal(r["rho"], trw.rho_of(name, "trees"))
    assert r["log_z"] >= m.exact()[1]
    both = fg.log_z_bounds("trees", trees=16, seed=3)
    assert both["trw"] == r["log_z"] and both["trw_converged"] and np.isfinite(both["bethe"])


@pytest.mark.parametrize("name", trw.CASES)
def test_warm_continues_and_cold_repeats_bit_for_bit(name):
    d, rho = TrwDev(name), trw.rho_of(name)
    cold = d.state(rho, 30, 0.5)
    _same_state(d.state(rho, 30, 0.5), cold, (name, "cold again"))
    d.state(rho, 7, 0.5)
    warm = d.state(rho, 23, 0.5, warm=1)
    warm["residual"], warm["iters"] = np.concatenate([np.zeros(7), warm["residual"]]), -30
    cold["residual"] = np.concatenate([np.zeros(7), cold["residual"][7:]])
    _same_state(warm, cold, (name, "warm"))


def test_refusals_are_texts():
    d = TrwDev("grid3")
    rho = np.ones(len(d.fg.factor))
    for bad, text in ((0.0, "rho[3]"), (-1.0, "rho[3]"), (np.nan, "rho[3]"), (np.inf, "rho[3]")):
        r = rho.copy()
        r[3] = bad
        assert d.trw_run(r, 4)[0] == _lib.E_INVALID and text in d.error()
    with pytest.raises(ValueError, match="entries"):
        d.fg.reweighted_bp(rho[:-1])
    assert d.L.nsk_bp_trw_download(d.h, _lib.BP_TRW_LF, None) == _lib.E_INVALID and "no tree-reweighted run" in d.error()
    _lib.check(d.L.nsk_bp_clear(d.h))
    assert d.trw_run(rho, 4)[0] == _lib.E_INVALID and "no belief propagation is set up" in d.error()


def test_belief_propagation_and_the_ledger_do_not_see_a_run():
    m = trw.model("tri")
    d = Dev(m.g, m.hbv)
    assert d.setup(m.sev) == _lib.OK, d.error()
    _lib.check(d.L.nsk_bp_clear(d.h))
    before = d.bytes()              # (with the records the first set-up left on the handle)
    assert d.setup(m.sev, push=False) == _lib.OK, d.error()
    d.run(5)
    resident = d.bytes()
    kept = [d.get(_lib.BP_F2V), d.get(_lib.BP_V2F), d.beliefs()]
    n, res = C.c_int64(0), np.zeros(6)
    _lib.check(d.L.nsk_bp_trw_run(d.h, _lib.ptr(trw.rho_of("tri")), 6, 0.5, 0.0, 0, C.byref(n), _lib.ptr(res)))
    assert d.bytes() > resident
    for a, b in zip(kept, [d.get(_lib.BP_F2V), d.get(_lib.BP_V2F), d.beliefs()]):
        _same(a, b, "after the tree-reweighted run")
    d.run(5)
    want = bp.Model(m.g, m.hbv, m.sev).run(10)
    _same(d.get(_lib.BP_F2V), want["f2v"], "ten iterations")
    _same(d.beliefs(), want["beliefs"], "ten iterations")
    _lib.check(d.L.nsk_bp_clear(d.h))
    assert d.bytes() == before
