"""Belief propagation on the device (nsk_bp_setup / nsk_bp_run / nsk_bp_download, FactorGraph.belief_propagation).

Yardstick: the numpy mirror numbskull_amd.diagnostics.bp_iterate with the oracle's exp_det over theta tables built from
the oracle's eval_factor (tests/bp.py).  Device and mirror perform the same IEEE operations in the same order, so every
comparison is bit for bit unless said otherwise.  tests/test_bp_cpu.py ties the mirror to enumeration."""

import ctypes as C

import numpy as np
import pytest

import bp
import truth_tables as tt
from numbskull_amd import _lib
from numbskull_amd.diagnostics import bp_layout
from util import session

pytestmark = pytest.mark.gpu

SEED = 77


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _same(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), (what, float(np.nanmax(np.abs(np.asarray(a) - np.asarray(b)))))


class Dev(object):
    """the C-ABI calls on one handle"""

    def __init__(self, g, hbv=False, **kw):
        _, self.fg = session(g, seed=SEED, head_by_vid=hbv, **kw)
        self.L, self.h = _lib.lib(), self.fg._engine()
        self.info = _lib.BpInfo()

    def setup(self, sev=0, which=_lib.BUF_VALUE, push=True):
        if push:
            self.fg._push(0, 0)
        return self.L.nsk_bp_setup(self.h, which, 0, int(sev), C.byref(self.info))

    def run(self, iters, damping=0.0, tol=0.0):
        n, res = C.c_int64(0), np.full(iters, -1.0)
        _lib.check(self.L.nsk_bp_run(self.h, iters, damping, tol, C.byref(n), _lib.ptr(res)))
        return n.value, res

    def get(self, what):
        out = np.zeros(self.info.ntable if what <= _lib.BP_FACTOR_BELIEFS else self.info.nmsg)
        _lib.check(self.L.nsk_bp_download(self.h, what, _lib.ptr(out)))
        return out

    def beliefs(self):
        out = np.zeros(int(self.fg.variable["cardinality"].sum()))
        _lib.check(self.L.nsk_bp_beliefs(self.h, None, 0, _lib.ptr(out)))
        return out

    def layout(self):
        nf, ne = len(self.fg.factor), self.info.nedges
        out = [np.zeros(nf + 1, np.int64), np.zeros(nf + 1, np.int64), np.zeros(ne, np.int64), np.zeros(ne + 1, np.int64)]
        _lib.check(self.L.nsk_bp_layout(self.h, *[_lib.ptr(a) for a in out]))
        return out

    def bytes(self):
        return self.fg.info()["device_bytes"]

    def error(self):
        return self.L.nsk_last_error().decode()


def _check_layout(d, layout):
    for got, key in zip(d.layout(), ("table_off", "edge_off", "edge_var", "msg_off")):
        assert np.array_equal(got, layout[key]), key


def _check_state(d, m, r, what):
    """messages, beliefs and factor beliefs of the device against a mirror run"""
    _same(d.get(_lib.BP_F2V), r["f2v"], (what, "f2v"))
    _same(d.get(_lib.BP_V2F), r["v2f"], (what, "v2f"))
    _same(d.beliefs(), r["beliefs"], (what, "beliefs"))
    _same(d.get(_lib.BP_FACTOR_BELIEFS), r["factor_beliefs"], (what, "factor beliefs"))


# ---------------------------------------------------------------------------------------------- A: tables
_FNS = tuple(f for f in tt.ALL if f != 30)


def _tables(g, mode):
    g = list(g)
    var = g[1].copy()
    var["isEvidence"] = 0
    if mode == "third":
        var["isEvidence"][::3] = 1
    g[1] = var
    m = bp.Model(tuple(g), hbv=True)
    d = Dev(tuple(g), hbv=True)
    assert d.setup() == _lib.OK, d.error()
    _check_layout(d, m.layout)
    assert d.info.ntable == len(m.theta) and d.info.max_table == int(np.diff(m.layout["table_off"]).max())
    _same(d.get(_lib.BP_THETA), m.theta, "theta")
    return d, m


@pytest.mark.parametrize("mode", ["free", "third"])
@pytest.mark.parametrize("part", [0, 1, 2])
def test_tables_of_every_function_arities_1_to_4(part, mode):
    """every function the call accepts, arities 1 .. 4, members of cardinality 3, every leaf value and both signs"""
    fns = _FNS[part::3]
    g, cells = tt.truth_graph(fns=fns, lcard=3)
    assert {c.fn for c in cells} == set(fns) and {c.arity for c in cells} == {1, 2, 3, 4}
    d, m = _tables(g, mode)
    sizes = np.diff(m.layout["table_off"])
    assert sizes.max() == (81 if mode == "free" else 27) and len(set(sizes.tolist())) >= 5
    assert len(np.unique(m.theta)) >= 3


@pytest.mark.parametrize("mode", ["free", "third"])
def test_tables_of_factors_that_name_a_member_twice(mode):
    g, cells = tt.self_family()
    d, m = _tables(g, mode)
    assert any(len(mem) < len(sl) for mem, sl in zip(m.layout["members"], m.layout["slots"]))


# ---------------------------------------------------------------------------------------------- B: the iterations
def _dev(name, evidence_chain=False):
    build, hbv, sev = bp.CASES[name]
    d = Dev(build(), hbv)
    assert d.setup(sev, _lib.BUF_VALUE_EVID if evidence_chain else _lib.BUF_VALUE) == _lib.OK, d.error()
    return d, sev


@pytest.mark.parametrize("damping", [0.0, 0.5])
@pytest.mark.parametrize("name", sorted(bp.CASES))
def test_iterations_equal_the_mirror_bit_for_bit(name, damping):
    m = bp.model(name)
    d, sev = _dev(name)
    _check_layout(d, m.layout)
    _same(d.get(_lib.BP_THETA), m.theta, "theta")
    if name == "grid_int32":
        assert d.fg.info()["value_bytes"] == 4
    for iters in bp.ITERS:
        for tol in (0.0, 1e-9):
            assert d.setup(sev, push=False) == _lib.OK
            r = bp.mirror(name, iters, damping, tol)
            n, res = d.run(iters, damping, tol)
            what = (name, damping, iters, tol)
            assert n == r["iters"], what
            _same(res, r["residual"], what)
            _check_state(d, m, r, what)
            if n > 0 and n < iters:                 # behind the early exit nothing moved and the residuals read 0
                assert not res[n:].any()
                _check_state(d, m, m.run(n, damping, tol), what)
    print("%s damping %.1f: 30 iterations at tol 1e-9 -> iters %d" % (name, damping, n))


@pytest.mark.parametrize("name", ["clamped_grid", "mixed_free"])
def test_a_second_run_continues_where_a_longer_one_would_be(name):
    m = bp.model(name)
    d, sev = _dev(name)
    n1, r1 = d.run(3, 0.5)
    n2, r2 = d.run(4, 0.5)
    whole = bp.mirror(name, 7, 0.5, 0.0)
    assert n1 == -3 and n2 == -4
    _same(np.concatenate([r1, r2]), whole["residual"], name)
    _check_state(d, m, whole, name)
    assert d.setup(sev, push=False) == _lib.OK      # a set-up resets the messages
    n, res = d.run(1, 0.5)
    _same(res, whole["residual"][:1], name)


@pytest.mark.parametrize("name", ["star", "star7", "tree"])
def test_trees_either_side_of_the_register_walk(name):
    """the star's centre has as many edges as the variable phase keeps in registers, star7's one more; the tree has an
    arity-3 table and cardinality-3 members"""
    m = bp.model(name)
    d = Dev(m.g)
    assert d.setup() == _lib.OK, d.error()
    _check_layout(d, m.layout)
    _same(d.get(_lib.BP_THETA), m.theta, "theta")
    for iters in (1, 2, 8):
        for damping in (0.0, 0.5):
            assert d.setup(push=False) == _lib.OK
            r = m.run(iters, damping)
            n, res = d.run(iters, damping)
            assert n == r["iters"]
            _same(res, r["residual"], (name, iters, damping))
            _check_state(d, m, r, (name, iters, damping))
    assert d.setup(push=False) == _lib.OK
    n, res = d.run(12)
    assert n == bp.mirror(name, 40, 0.0, 0.0)["iters"] and 1 < n < 12 and res[n - 1] == 0.0
    ex, lz = m.exact()
    b = d.beliefs()
    off = m.layout["offsets"]
    assert max(np.abs(b[off[v]:off[v + 1]] - p).max() for v, p in ex.items()) <= 1e-12


def test_the_evidence_chain_is_a_state_of_its_own():
    build, hbv, _ = bp.CASES["mixed_clamped"]
    d = Dev(build(), hbv)
    fg = d.fg
    ev = np.nonzero(fg.variable["isEvidence"] != 0)[0]
    x = fg.var_value_evid[0].copy()
    x[ev] = (x[ev] + 1) % fg.variable["cardinality"][ev]
    fg.var_value_evid[0][:] = x
    m = bp.Model(build(), hbv)
    m.x = x.astype(np.int64)
    m.layout = bp_layout(fg.factor, fg.fmap, fg.variable, m.x)
    m.theta = bp.theta_tables(m.og, m.layout, m.x, m.w)
    assert d.setup(0, _lib.BUF_VALUE_EVID) == _lib.OK, d.error()
    _same(d.get(_lib.BP_THETA), m.theta, "theta of the evidence chain")
    assert not np.array_equal(m.theta, bp.model("mixed_clamped").theta)
    r = m.run(5)
    n, res = d.run(5)
    _same(res, r["residual"], "evidence chain")
    _check_state(d, m, r, "evidence chain")


# ---------------------------------------------------------------------------------------------- C: the hub
def test_the_hub_needs_the_rescale_rule():
    m, red = bp.model("hub"), bp.model("hub_reduced")
    r = bp.mirror("hub", 30, 0.0, 0.0)
    assert r["rescaled"] > 0
    d = Dev(bp.hub())
    assert d.setup() == _lib.OK, d.error()
    n, res = d.run(30)
    assert n == r["iters"]
    _same(res, r["residual"], "hub")
    _check_state(d, m, r, "hub")
    b = d.beliefs()
    assert np.isfinite(b).all()
    ex, _ = red.exact()
    assert np.abs(b[:2] - ex[0]).max() <= 1e-12 and np.abs(b[2:] - ex[1]).max() <= 1e-12


# ---------------------------------------------------------------------------------------------- D: later trips
def test_later_trips_of_every_kernel(monkeypatch):
    """NSK_BP_GRID_CAP is read at each call: the same process runs the graph as is and with one block a launch"""
    m = bp.model("trips")
    r = bp.mirror("trips", bp.TRIP_ITERS, 0.0, 0.0)
    L = m.layout
    nvl = sum(1 for e in L["var_edges"] if e)
    assert min(bp.trips(len(m.theta), 1), bp.trips(len(L["edge_var"]), 1), bp.trips(nvl, 1, _lib.BP_VAR_BLOCK)) >= 3
    got = []
    for cap in (None, "1"):
        monkeypatch.delenv("NSK_DIAG", raising=False)
        monkeypatch.delenv("NSK_BP_GRID_CAP", raising=False)
        if cap:
            monkeypatch.setenv("NSK_DIAG", "1")
            monkeypatch.setenv("NSK_BP_GRID_CAP", cap)
        d = Dev(bp.trips_grid())
        assert d.setup() == _lib.OK, d.error()
        _same(d.get(_lib.BP_THETA), m.theta, ("theta", cap))
        n, res = d.run(bp.TRIP_ITERS)
        _same(res, r["residual"], cap)
        _check_state(d, m, r, cap)
        got.append((d.get(_lib.BP_F2V), d.get(_lib.BP_V2F), d.beliefs(), d.get(_lib.BP_FACTOR_BELIEFS), res))
    for a, b in zip(*got):
        _same(a, b, "capped against uncapped")


# ---------------------------------------------------------------------------------------------- E: limits
def test_limits_and_refusals():
    m = bp.model("limit")
    d = Dev(bp.limit_graph(12, 4))
    assert d.setup() == _lib.OK, d.error()
    assert d.info.max_table == 4096 == _lib.BP_MAX_TABLE and d.info.nedges == 13
    _same(d.get(_lib.BP_THETA), m.theta, "the 12-ary AND over 4 evidence members")
    assert sorted(set(m.theta[:4096].tolist())) == [-0.5, 0.5]
    r = m.run(2)
    n, res = d.run(2)
    _same(res, r["residual"], "limit")
    _check_state(d, m, r, "limit")
    for g, hbv, word in ((bp.limit_graph(13, 0), False, "NSK_BP_MAX_TABLE"), (bp.limit_graph(12, 5), False, "NSK_BP_MAX_MEMBERS"),
                         (bp.limit_graph(2, 1, fn=30), True, "UFO"), (bp.limit_graph(3, 0, fn=13), False, "literal")):
        d = Dev(g, hbv)
        d.fg.log_potential() if word not in ("UFO", "literal") else d.fg._push(0, 0)
        before = d.bytes()
        assert d.setup(push=False) == _lib.E_INVALID
        print(d.error())
        assert "factor 0 " in d.error() and word in d.error()
        assert d.bytes() == before, "a refusal leaves no allocation behind"
        n = C.c_int64(0)
        assert d.L.nsk_bp_run(d.h, 3, 0.0, 0.0, C.byref(n), None) == _lib.E_INVALID        # nothing is set up
        assert d.L.nsk_bp_download(d.h, _lib.BP_F2V, None) == _lib.E_INVALID
    # the offending factor is named where it is not the first
    g = bp.spec_graph([2] * 14, [0] * 14, [0] * 14, [(4, [0], [0], 0.3), (2, list(range(13)), [0] * 13, 0.5), (2, list(range(14)), [0] * 14, 0.5)])
    d = Dev(g)
    assert d.setup() == _lib.E_INVALID and "factor 1 " in d.error()
    with pytest.raises(ValueError, match="factor 1 "):
        d.fg.belief_propagation()
    # the literal head is fine with head_by_vid
    d = Dev(bp.limit_graph(3, 0, fn=13), True)
    assert d.setup() == _lib.OK, d.error()
    # arguments
    n = C.c_int64(0)
    for iters, damping, tol in ((0, 0.0, 0.0), (4097, 0.0, 0.0), (3, 1.0, 0.0), (3, -0.1, 0.0), (3, 0.0, -1.0), (3, float("nan"), 0.0)):
        assert d.L.nsk_bp_run(d.h, iters, damping, tol, C.byref(n), None) == _lib.E_INVALID
    assert d.L.nsk_bp_run(d.h, 3, 0.0, 0.0, None, None) == _lib.E_INVALID
    assert d.L.nsk_bp_setup(d.h, _lib.BUF_WEIGHT, 0, 0, None) == _lib.E_INVALID
    assert d.L.nsk_bp_setup(d.h, _lib.BUF_VALUE, 1, 0, None) == _lib.E_INVALID
    assert d.L.nsk_bp_download(d.h, 4, None) == _lib.E_INVALID
    ids = np.array([0, 99], np.int64)
    assert d.L.nsk_bp_beliefs(d.h, _lib.ptr(ids), 2, _lib.ptr(np.zeros(4))) == _lib.E_INDEX
    # a handle that samples a range of the graph
    import numbskull_amd
    from numbskull_amd.distributed import shard_range
    ns = numbskull_amd.NumbSkull(quiet=True, seed=SEED)
    w, v, f, fm, dm, edges = [x.copy() if isinstance(x, np.ndarray) else x for x in bp.chain17()]
    ns.loadFactorGraph(w, v, f, fm, dm, int(edges), own_range=shard_range(0, 2, len(v)))
    assert d.L.nsk_bp_setup(ns.factorGraphs[0]._engine(), _lib.BUF_VALUE, 0, 0, None) == _lib.E_INVALID


# ---------------------------------------------------------------------------------------------- F: neighbours
def test_sweeps_around_a_run_are_the_sweeps_without_it():
    """a resident one-chain handle of wide quads keeps its tally in the value bytes between sweeps"""
    from numbskull_amd import graphgen
    n = 1000
    g = graphgen.ising_grid(n, n, weight=0.3)
    _, fg = session(g, seed=SEED)
    _, tw = session(g, seed=SEED)
    assert fg.info()["wide_quads"] > 0
    L, h = _lib.lib(), fg._engine()
    fg._push(0, 0)
    fg._sweep(12, False, False)
    info = _lib.BpInfo()
    _lib.check(L.nsk_bp_setup(h, _lib.BUF_VALUE, 0, 0, C.byref(info)))
    it = C.c_int64(0)
    _lib.check(L.nsk_bp_run(h, 3, 0.0, 0.0, C.byref(it), None))
    b = np.zeros(2 * n * n)
    _lib.check(L.nsk_bp_beliefs(h, None, 0, _lib.ptr(b)))
    assert (b == 0.5).all() and it.value == 1 and info.nfree == n * n      # (a free grid: the uniform fixed point)
    _lib.check(L.nsk_bp_clear(h))
    fg._sweep(5, False, False)
    fg._pull(0, 0, weights=False)
    tw.inference(0, 17)
    assert np.array_equal(fg.var_value[0], tw.var_value[0]) and np.array_equal(fg.count, tw.count)
    assert fg.info()["sweeps_done"] == tw.info()["sweeps_done"] == 17


def test_clear_returns_the_device_bytes():
    d = Dev(bp.CASES["mixed_clamped"][0](), True)
    d.fg.log_potential()                            # (the records both share are in place)
    before = d.bytes()
    assert d.setup(push=False) == _lib.OK
    held = d.bytes()
    assert held - before == d.info.device_bytes > 0
    d.run(3)
    d.get(_lib.BP_FACTOR_BELIEFS)
    assert d.bytes() == held                        # the residuals and the factor beliefs live for their call only
    assert d.setup(1, push=False) == _lib.OK        # a second set-up replaces the first
    assert d.L.nsk_bp_clear(d.h) == _lib.OK and d.bytes() == before
    assert d.L.nsk_bp_clear(d.h) == _lib.OK
    n = C.c_int64(0)
    assert d.L.nsk_bp_run(d.h, 3, 0.0, 0.0, C.byref(n), None) == _lib.E_INVALID


# ---------------------------------------------------------------------------------------------- G: the Python API
def test_python_api():
    m = bp.model("chain9")
    _, fg = session(bp.chain9(), seed=SEED)
    res = fg.belief_propagation(tol=0.0, factor_beliefs=True)
    for k in ("offsets", "beliefs", "iters", "converged", "residual", "log_z", "table_offsets", "theta", "factor_beliefs"):
        assert k in res, k
    r = bp.mirror("chain9", 100, 0.0, 0.0)
    assert res["iters"] == 5 == r["iters"] and res["converged"] is True
    _same(res["beliefs"], r["beliefs"], "beliefs")
    _same(res["theta"], m.theta, "theta")
    _same(res["factor_beliefs"], r["factor_beliefs"], "factor beliefs")
    assert np.array_equal(res["offsets"], m.layout["offsets"]) and np.array_equal(res["table_offsets"], m.layout["table_off"])
    _, lz = m.exact()
    assert abs(res["log_z"] - lz) <= 1e-10 and res["log_z"] == m.log_z(r)
    assert set(fg.belief_propagation()) == {"offsets", "beliefs", "iters", "converged", "residual", "log_z"}
    import temper
    _, lg = session(temper.clamped_grid(), seed=SEED)
    res = lg.belief_propagation(max_iters=2)
    assert res["converged"] is False and res["iters"] == 2 and (res["residual"] > 0).all()
    res = lg.belief_propagation(max_iters=200, damping=0.5, tol=1e-12)
    assert res["converged"] and res["iters"] == bp.mirror("clamped_grid", 200, 0.5, 1e-12)["iters"]
    with pytest.raises(ValueError):
        lg.belief_propagation(max_iters=0)
    with pytest.raises(ValueError):
        lg.belief_propagation(var_copy="all")
