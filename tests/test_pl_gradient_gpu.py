"""Pseudo-likelihood gradient and MPLE learning on the device (nsk_pl_gradient, nsk_mple_steps).

Yardsticks: the int64 sums must EQUAL numbskull_amd.diagnostics.pl_gradient_counts on the oracle's entries
(tests/plgrad.py: eval_factor, potential and exp_det of the oracle, the index of the product) -- integers, so "equal"
has no tolerance; the weights, grad_max and skips of nsk_mple_steps must equal a host loop of pl_gradient_counts +
mple_step as bit patterns.  tests/test_pl_gradient_cpu.py ties the twin to central differences of the
log-pseudo-likelihood and checks the planted pair model this file learns from."""

import numpy as np
import pytest

import numbskull_amd
from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import mple_step
from numbskull_amd.numbskulltypes import Weight, Variable, Factor, FactorToVar
from test_hip_parity import _small_graphs, GRAPHS
from test_conditionals_gpu import _selection
from util import orc, session, oracle_of
import plgrad

pytestmark = pytest.mark.gpu

SEED = 77
_CACHE = {}


def _graph(golden, name):
    if not _CACHE:
        _CACHE.update(_small_graphs(golden))
    return _CACHE[name]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _ids(fg):
    sel = _selection(fg)
    return np.arange(len(fg.variable), dtype=np.int64) if sel is None else sel


def _raw(fg, which, first, nchains, ids, want_grad=False):
    """nsk_pl_gradient on the handle as it stands (no push): (grad_q, skipped[, grad])"""
    L, h = _lib.lib(), fg._engine()
    nw = len(fg.weight)
    gq, gd, sk = np.full((nchains, nw), -7, np.int64), np.full((nchains, nw), -7.0), np.full(nchains, -7, np.int64)
    vids = None if ids is None else _lib.as_c(ids, np.int64)
    _lib.check(L.nsk_pl_gradient(h, which, first, nchains, _lib.ptr(vids), 0 if ids is None else len(vids), _lib.ptr(gq),
                                 _lib.ptr(gd) if want_grad else None, _lib.ptr(sk)))
    return (gq, sk, gd) if want_grad else (gq, sk)


# ---------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("name", GRAPHS)
def test_the_sums_equal_the_twin_on_the_oracles_entries(golden, name):
    g, hbv = _graph(golden, name)
    _, fg = session(g, seed=SEED, head_by_vid=hbv)
    og = oracle_of(fg, hbv)
    twin = plgrad.Twin(fg, og, _ids(fg))
    nterms = len(twin.s[1])
    assert nterms > 0

    def check(f, what, **kw):
        got, skipped = f.pl_gradient(twin.ids, counts=True, **kw)
        states = f.var_value_evid if kw.get("evidence_chain") else f.var_value
        assert got.dtype == np.int64
        for i, (mine, ms) in enumerate(zip(np.atleast_2d(got), np.atleast_1d(skipped))):
            want, ws = twin.counts(states[i], f.weight_value[0])
            assert ms == ws == 0, (name, what, i)
            assert np.array_equal(mine, want), (name, what, i, np.nonzero(mine != want)[0][:8])
            assert want.any()
        return got

    fg.inference(2, 3, True)
    q = check(fg, "free")
    assert np.array_equal(_bits(fg.pl_gradient(twin.ids)), _bits(q.astype(np.float64) * plgrad.Q))
    fg.learn(1, 3, 0.01, 0.95, 2, 0.01, 1)
    check(fg, "evidence", evidence_chain=True)
    check(fg, "free after learning")
    _, f3 = session(g, seed=SEED, head_by_vid=hbv, chains=3)
    f3.inference(2, 3, True, var_copy="all")
    rows = check(f3, "three chains", var_copy="all")
    assert rows.shape == (3, len(fg.weight))


# ---------------------------------------------------------------------------------------------- B
def test_both_sides_of_the_lds_switch():
    """256 weights accumulate in the block's LDS bins, 257 go straight to the global sums: each exact against the twin,
    and the 256-weight graph with one unused weight appended -- the same factors on the other path -- gives the same sums"""
    assert _lib.PLGRAD_BINS == 256
    res = {}
    for nw in (256, 257):
        g = graphgen.mixed_lr_graph(3000, seed=5, nweights=nw)
        assert len(g[0]) == nw
        _, fg = session(g, seed=SEED, head_by_vid=True)
        fg.weight_value[0][:] = np.random.default_rng(nw).normal(0.0, 0.5, nw)
        fg.inference(1, 2, True)
        twin = plgrad.Twin(fg, oracle_of(fg, True), _ids(fg))
        got, skipped = fg.pl_gradient(twin.ids, counts=True)
        want, _ = twin.counts(fg.var_value[0], fg.weight_value[0])
        assert skipped == 0 and np.array_equal(got, want) and np.count_nonzero(want) > nw // 4, nw
        res[nw] = (g, fg.var_value[0].copy(), fg.weight_value[0].copy(), twin.ids, got)
    g, x, w, ids, got = res[256]
    g = list(g)
    g[0] = np.concatenate([g[0], np.zeros(1, Weight)])
    _, fg = session(tuple(g), seed=SEED, head_by_vid=True)
    fg.var_value[0][:] = x
    fg.weight_value[0][:256] = w
    more, skipped = fg.pl_gradient(ids, counts=True)
    assert skipped == 0 and np.array_equal(more[:256], got) and more[256] == 0


# ---------------------------------------------------------------------------------------------- C
def test_selections(golden):
    g, hbv = _graph(golden, "lr3000")
    _, fg = session(g, seed=SEED, head_by_vid=hbv, chains=3)
    fg.weight_value[0][:] = np.random.default_rng(1).normal(0.0, 0.5, len(fg.weight))
    fg.inference(1, 2, True, var_copy="all")
    nvar = len(fg.variable)
    fg._push_chains(0, count=False)
    full, sk = _raw(fg, _lib.BUF_VALUE, 0, 3, None)                                 # NULL = every variable
    listed, sk2, grad = _raw(fg, _lib.BUF_VALUE, 0, 3, np.arange(nvar), want_grad=True)
    assert np.array_equal(full, listed) and not sk.any() and not sk2.any()
    assert np.array_equal(_bits(grad), _bits(full.astype(np.float64) * plgrad.Q))
    perm = np.random.default_rng(9).permutation(nvar)
    assert np.array_equal(_raw(fg, _lib.BUF_VALUE, 0, 3, perm)[0], full)            # the order does not matter
    a, b = perm[:1003], perm[1003:]                                                 # disjoint selections add up, exactly
    qa, qb = _raw(fg, _lib.BUF_VALUE, 0, 3, a)[0], _raw(fg, _lib.BUF_VALUE, 0, 3, b)[0]
    assert np.array_equal(qa + qb, full) and qa.any() and qb.any()
    assert np.array_equal(_raw(fg, _lib.BUF_VALUE, 1, 2, a)[0], qa[1:])             # a sub-range of the chains
    for r in range(3):                                                              # ... equals the one-chain handles
        _, one = session(g, seed=SEED, head_by_vid=hbv)
        one.var_value[0][:] = fg.var_value[r]
        one.weight_value[0][:] = fg.weight_value[0]
        q1, s1 = one.pl_gradient(a, counts=True)
        assert s1 == 0 and np.array_equal(q1, qa[r])
    # a value outside its domain: counted in skipped, and the rest is what the twin gives for that state
    og = oracle_of(fg, hbv)
    twin = plgrad.Twin(fg, og, a)
    v = int(a[5])
    _, one = session(g, seed=SEED, head_by_vid=hbv)
    one.var_value[0][:] = fg.var_value[0]
    one.weight_value[0][:] = fg.weight_value[0]
    one.var_value[0][v] = int(fg.variable["cardinality"][v])
    q1, s1 = one.pl_gradient(a, counts=True)
    want, ws = twin.counts(one.var_value[0], one.weight_value[0])
    assert s1 == ws == 1 and np.array_equal(q1, want) and not np.array_equal(q1, qa[0])


def test_a_variable_without_a_position_contributes_nothing():
    x = np.random.default_rng(3).integers(0, 2, 20)
    x[[2, 12]], x[[6, 8]] = 1, 0            # (cell 7's neighbours agree pairwise: its own terms do not cancel)
    out = {}
    for ev in (4, 1):
        g = list(graphgen.ising_grid(4, 5, weight=0.4, two_weights=True))
        var = g[1].copy()
        var["isEvidence"][7] = ev
        var["initialValue"][7] = x[7]
        g[1] = var
        _, fg = session(tuple(g), seed=SEED)
        fg.var_value[0][:] = x
        out[ev] = [fg.pl_gradient(ids, counts=True) for ids in (np.arange(20), np.delete(np.arange(20), 7), [7])]
    (all4, s4), (rest4, _), (only4, _) = out[4]
    (all1, _), (rest1, _), (only1, _) = out[1]
    assert np.array_equal(all4, rest4) and np.array_equal(rest4, rest1) and not only4.any() and s4 == 0
    assert np.array_equal(all1, rest1 + only1) and only1.any()


# ---------------------------------------------------------------------------------------------- D
def test_a_selection_that_fills_no_whole_wave(golden):
    """grid57x33: 1881 variables (8 blocks, the last with 89 lanes at work) and 1003 of them in any order"""
    g, hbv = _graph(golden, "grid57x33")
    _, fg = session(g, seed=SEED, head_by_vid=hbv)
    fg.inference(1, 2, True)
    og = oracle_of(fg, hbv)
    for ids in (np.arange(1881), np.random.default_rng(2).permutation(1881)[:1003]):
        assert len(ids) % 64 != 0
        twin = plgrad.Twin(fg, og, ids)
        got, skipped = fg.pl_gradient(ids, counts=True)
        want, _ = twin.counts(fg.var_value[0], fg.weight_value[0])
        assert skipped == 0 and np.array_equal(got, want) and want.any()


def test_grid_stride_trips_against_the_closed_form():
    """300 x 300 Ising grid, one weight: 90 000 variables on a launch of plgrad_blocks(90 000) = 256 blocks of 256 lanes, so
    24 464 lanes make a second trip and the others do not.  The sum in closed form: a cell's list is its factors to the cells above, to the
    left, to the right and below, in that order (ascending factor ids); EQUAL is +1 / -1."""
    n, w = 300, 0.3
    lanes = _lib.plgrad_blocks(n * n) * _lib.PLGRAD_BLOCK
    assert lanes == 256 * 256 and lanes < n * n < 2 * lanes
    assert [_lib.plgrad_blocks(k) for k in (0, 1, 257, 65536, 65537, 131072, 131585, 10 ** 7)] == [1, 1, 2, 256, 256, 256, 258, 2048]
    x = np.random.default_rng(12).integers(0, 2, (n, n))
    _, fg = session(graphgen.ising_grid(n, n, weight=w, initial=x.ravel()), seed=SEED)
    got, skipped = fg.pl_gradient(counts=True)
    i, j = np.divmod(np.arange(n * n), n)
    ok, eq = [], []
    for di, dj in ((-1, 0), (0, -1), (0, 1), (1, 0)):
        ii, jj = i + di, j + dj
        ok.append((ii >= 0) & (ii < n) & (jj >= 0) & (jj < n))
        eq.append(x[np.clip(ii, 0, n - 1), np.clip(jj, 0, n - 1)])
    p = np.zeros((2, n * n))
    for k in (0, 1):
        for m, nb in zip(ok, eq):
            p[k] = p[k] + np.where(m, w * np.where(nb == k, 1.0, -1.0), 0.0)
    u, inv = np.unique(p, return_inverse=True)
    e = orc.exp_det(u)[inv].reshape(p.shape)
    z = e[0] + e[1]
    total = 0
    for k in (0, 1):
        c = (x.ravel() == k).astype(np.float64) - e[k] / z
        for m, nb in zip(ok, eq):
            q = np.rint((c * np.where(nb == k, 1.0, -1.0)) * 2.0 ** 32).astype(np.int64)
            total += int(q[m].sum())
    assert skipped == 0 and got.shape == (1,) and int(got[0]) == total and total != 0


# ---------------------------------------------------------------------------------------------- E
def _state(fg):
    L = _lib.lib()
    n, nw = len(fg.variable), len(fg.weight)
    vv, ve, wv, cnt = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(nw), np.zeros(len(fg.count), np.int64)
    _lib.check(L.nsk_state_download(fg._engine(), _lib.ptr(vv), _lib.ptr(ve), _lib.ptr(wv), _lib.ptr(cnt)))
    return vv, ve, _bits(wv), cnt, fg.info()["sweeps_done"]


@pytest.mark.parametrize("name", ["grid57x33", "lr3000", "gencat_i32"])
def test_the_gradient_only_reads_and_the_learner_only_writes_weights(golden, name):
    L = _lib.lib()
    g, hbv = _graph(golden, name)
    _, a = session(g, seed=SEED, head_by_vid=hbv)
    _, b = session(g, seed=SEED, head_by_vid=hbv)
    _, c = session(g, seed=SEED, head_by_vid=hbv)
    _, d = session(g, seed=SEED, head_by_vid=hbv)
    for fg in (a, b, c, d):
        fg.learn(1, 2, 0.01, 0.95, 2, 0.01, 1)
        fg.inference(1, 4, True)
    h = a._engine()
    out = np.zeros(int(a.variable["cardinality"].sum()))
    # a trace whose rows must stay
    _lib.check(L.nsk_trace_setup(h, None, 0, 1, 4))
    _lib.check(L.nsk_gibbs_sweeps(h, 2, 1, 0))
    _lib.check(L.nsk_gibbs_sweeps(b._engine(), 2, 1, 0))
    _lib.check(L.nsk_gibbs_sweeps(c._engine(), 2, 1, 0))
    _lib.check(L.nsk_gibbs_sweeps(d._engine(), 2, 1, 0))
    rows = np.zeros((2, 1, len(a.variable)), np.int8 if a.info()["value_bytes"] == 1 else np.int32)
    _lib.check(L.nsk_trace_download(h, 0, 2, _lib.ptr(rows), None))
    _lib.check(L.nsk_conditionals(h, _lib.BUF_VALUE, 0, 1, None, 0, 1, _lib.ptr(out)))
    _lib.check(L.nsk_conditionals(b._engine(), _lib.BUF_VALUE, 0, 1, None, 0, 1, _lib.ptr(out)))
    before, bytes_before = _state(a), a.info()["device_bytes"]
    for which in (_lib.BUF_VALUE, _lib.BUF_VALUE_EVID):
        q, sk = _raw(a, which, 0, 1, None)
        assert q.any() and not sk.any()
    for x, y in zip(before, _state(a)):
        assert np.array_equal(x, y)
    assert a.info()["device_bytes"] == bytes_before                         # selection and sums lived for the call only
    # the first call of either entry point on a handle leaves what one nsk_conditionals call leaves
    _raw(c, _lib.BUF_VALUE, 0, 1, None)
    assert c.info()["device_bytes"] == b.info()["device_bytes"]
    _lib.check(L.nsk_mple_steps(d._engine(), _lib.BUF_VALUE, 0, 1, None, 0, 2, 0.05, 1.0, 0.0, None, None))
    assert d.info()["device_bytes"] == b.info()["device_bytes"]
    gmax, skipped = np.zeros(3, np.int64), np.zeros(3, np.int64)
    _lib.check(L.nsk_mple_steps(h, _lib.BUF_VALUE_EVID, 0, 1, None, 0, 3, 0.05, 0.9, 0.01, _lib.ptr(gmax), _lib.ptr(skipped)))
    after = _state(a)
    assert a.info()["device_bytes"] == bytes_before
    for k in (0, 1, 3, 4):
        assert np.array_equal(before[k], after[k])                          # values, tally, sweeps_done
    fixed = a.weight["isFixed"].astype(bool)
    assert (fixed.all() or gmax.min() > 0) and not skipped.any()
    assert np.array_equal(before[2][fixed], after[2][fixed]) and (fixed.all() or (before[2][~fixed] != after[2][~fixed]).any())
    again = np.zeros_like(rows)
    _lib.check(L.nsk_trace_download(h, 0, 2, _lib.ptr(again), None))
    assert np.array_equal(rows, again)
    _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
    # continuing the chain of the handle that only asked for gradients gives the samples of a twin that never asked
    _raw(b, _lib.BUF_VALUE, 0, 1, None)
    for fg in (b, c):
        _lib.check(L.nsk_gibbs_sweeps(fg._engine(), 3, 1, 0))
    for x, y in zip(_state(b), _state(c)):
        assert np.array_equal(x, y)


def _ufo_graph(n):
    """n binary variables, each with one UFO factor of arity 1, all on weight 0: B_0 = n x 2 x 1e6"""
    variable = np.zeros(n, Variable)
    variable["cardinality"] = 2
    factor, fmap = np.zeros(n, Factor), np.zeros(n, FactorToVar)
    factor["factorFunction"] = 30
    factor["featureValue"] = 1.0
    factor["arity"] = 1
    factor["ftv_offset"] = np.arange(n)
    fmap["vid"] = np.arange(n)
    return np.zeros(1, Weight), variable, factor, fmap, np.zeros(n, np.bool_), n


def test_refusals(golden):
    L = _lib.lib()
    g, hbv = _graph(golden, "gencat_i32")
    _, fg = session(g, seed=SEED, head_by_vid=hbv, chains=2)
    h = fg._engine()
    fg._chains()
    nvar, nw = len(fg.variable), len(fg.weight)
    gq, sk = np.zeros((2, nw), np.int64), np.zeros(2, np.int64)
    ids = _lib.as_c([5, 3, nvar - 1], np.int64)

    def grad(which=_lib.BUF_VALUE, first=0, n=1, vids=ids, nvids=None):
        return L.nsk_pl_gradient(h, which, first, n, _lib.ptr(vids), (0 if vids is None else len(vids)) if nvids is None else nvids,
                                 _lib.ptr(gq), None, _lib.ptr(sk))

    def steps(which=_lib.BUF_VALUE, first=0, n=1, vids=ids, nvids=None, nsteps=2, step=0.1, decay=1.0, reg=0.0):
        return L.nsk_mple_steps(h, which, first, n, _lib.ptr(vids), (0 if vids is None else len(vids)) if nvids is None else nvids,
                                nsteps, step, decay, reg, None, None)

    w0 = _state(fg)[2]
    for f in (grad, steps):
        for which in (-1, _lib.BUF_WEIGHT, 7):
            assert f(which=which) == _lib.E_INVALID
        assert f(first=2) == _lib.E_INVALID and f(first=1, n=2) == _lib.E_INVALID and f(first=-1) == _lib.E_INVALID
        assert f(n=0) == _lib.E_INVALID
        assert f(which=_lib.BUF_VALUE_EVID, first=1) == _lib.E_INVALID and f(which=_lib.BUF_VALUE_EVID, n=2) == _lib.E_INVALID
        assert f(vids=_lib.as_c([0, nvar], np.int64)) == _lib.E_INDEX and f(vids=_lib.as_c([-1], np.int64)) == _lib.E_INDEX
        assert f(vids=None, nvids=3) == _lib.E_INVALID and f(nvids=-1) == _lib.E_INVALID
        assert f(vids=_lib.as_c([5, 3, 5], np.int64)) == _lib.E_INVALID                    # the selection is a set
    for kw in (dict(nsteps=0), dict(nsteps=65537), dict(step=np.nan), dict(step=np.inf), dict(decay=np.inf), dict(reg=-1e-3),
               dict(reg=np.nan)):
        assert steps(**kw) == _lib.E_INVALID, kw
    assert np.array_equal(_state(fg)[2], w0)                                                # nothing refused touched the weights
    assert grad(n=2) == _lib.OK and grad(which=_lib.BUF_VALUE_EVID) == _lib.OK and grad(vids=None, n=2) == _lib.OK
    assert steps(n=2) == _lib.OK
    with pytest.raises(ValueError):
        fg.pl_gradient([5, 5])
    # an own_range handle
    from numbskull_amd.distributed import shard_range
    ns = numbskull_amd.NumbSkull(quiet=True, seed=SEED)
    w, v, f, fm, dm, edges = [x.copy() if isinstance(x, np.ndarray) else x for x in _graph(golden, "grid57x33")[0]]
    ns.loadFactorGraph(w, v, f, fm, dm, int(edges), own_range=shard_range(0, 2, len(v)))
    sh = ns.factorGraphs[0]
    one = np.zeros(1, np.int64)
    assert L.nsk_pl_gradient(sh._engine(), _lib.BUF_VALUE, 0, 1, None, 0, _lib.ptr(one), None, None) == _lib.E_INVALID
    assert L.nsk_mple_steps(sh._engine(), _lib.BUF_VALUE, 0, 1, None, 0, 1, 0.1, 1.0, 0.0, None, None) == _lib.E_INVALID
    # the range of the int64 sums, from the graph and the selection alone: 2 x 1e6 per UFO entry of a binary variable
    _, uf = session(_ufo_graph(600), seed=SEED, chains=2)
    hu = uf._engine()
    uf._chains()
    q = np.zeros((2, 1), np.int64)
    every = _lib.as_c(np.arange(600), np.int64)
    sel = lambda n: _lib.ptr(every)                                                         # noqa: E731  (the first n of them)
    assert 536 * 2e6 < 2 ** 30 <= 537 * 2e6
    assert L.nsk_pl_gradient(hu, _lib.BUF_VALUE, 0, 1, sel(537), 537, _lib.ptr(q), None, None) == _lib.E_RANGE
    assert L.nsk_pl_gradient(hu, _lib.BUF_VALUE, 0, 1, None, 0, _lib.ptr(q), None, None) == _lib.E_RANGE
    assert L.nsk_mple_steps(hu, _lib.BUF_VALUE, 0, 1, sel(537), 537, 1, 0.1, 1.0, 0.0, None, None) == _lib.E_RANGE
    assert L.nsk_pl_gradient(hu, _lib.BUF_VALUE, 0, 2, sel(269), 269, _lib.ptr(q), None, None) == _lib.E_RANGE    # ... x chains
    assert L.nsk_pl_gradient(hu, _lib.BUF_VALUE, 0, 1, sel(536), 536, _lib.ptr(q), None, None) == _lib.OK
    assert L.nsk_pl_gradient(hu, _lib.BUF_VALUE, 0, 2, sel(268), 268, _lib.ptr(q), None, None) == _lib.OK
    with pytest.raises(OverflowError):
        uf.pl_gradient(np.arange(600))


# ---------------------------------------------------------------------------------------------- F
@pytest.mark.parametrize("name", ["mixed", "lr3000", "gencat_i32"])
@pytest.mark.parametrize("reg", [0.0, 0.01])
def test_mple_steps_equal_the_host_loop_bit_for_bit(golden, name, reg):
    L = _lib.lib()
    g, hbv = _graph(golden, name)
    g = list(g)
    nvar = len(g[1])
    ids = np.sort(np.random.default_rng(4).choice(nvar, min(nvar, 500), replace=False)).astype(np.int64)
    g[0] = g[0].copy()
    g[0]["isFixed"] = False
    probe = session(tuple(g), seed=SEED, head_by_vid=hbv)[1]
    fixed_w = int(plgrad.structure(probe, plgrad.positioned(probe, ids))[4][0])      # a weight the selection reaches
    g[0]["isFixed"][fixed_w] = True
    g = tuple(g)
    _, fg = session(g, seed=SEED, head_by_vid=hbv)
    _, tw = session(g, seed=SEED, head_by_vid=hbv)
    og = oracle_of(fg, hbv)
    for f in (fg, tw):
        f.inference(1, 2, True)                                                      # tables built under the first weights
    twin = plgrad.Twin(fg, og, ids)
    nsteps, step, decay = 12, 0.1, 0.9
    w, fixed = fg.weight_value[0].astype(np.float64).copy(), fg.weight["isFixed"].astype(bool)
    state = fg.var_value_evid[0].copy()
    n = len(twin.ids)
    want_gmax, want_skipped, st = np.zeros(nsteps), np.zeros(nsteps, np.int64), step
    for t in range(nsteps):
        s, want_skipped[t] = twin.counts(state, w)
        want_gmax[t] = float(np.abs(s[~fixed]).max()) * plgrad.Q / n
        w = mple_step(w, fixed, s, n, st, reg)
        st = st * decay
    res = fg.learn_mple(nsteps, step, decay=decay, reg_param=reg, var_ids=ids, evidence_chain=True)
    assert res["n"] == n
    assert np.array_equal(_bits(fg.weight_value[0]), _bits(w)), np.nonzero(_bits(fg.weight_value[0]) != _bits(w))[0][:8]
    assert np.array_equal(_bits(res["grad_max"]), _bits(want_gmax)) and np.array_equal(res["skipped"], want_skipped)
    assert fg.weight_value[0][fixed_w] == g[0]["initialValue"][fixed_w] and want_gmax.min() > 0
    # sweeps on the handle as the learner left it equal those of a twin that had the same weights uploaded: the tables
    # derived from the weights were rebuilt
    _lib.check(L.nsk_gibbs_sweeps(fg._engine(), 3, 1, 0))
    fg._pull(0, 0)
    tw.weight_value[0][:] = w
    tw.inference(0, 3, True)
    assert np.array_equal(fg.var_value[0], tw.var_value[0]) and np.array_equal(fg.count, tw.count)
    assert np.array_equal(_bits(fg.weight_value[0]), _bits(w))


def test_mple_update_across_a_block_edge():
    """tests/pcd_latent.py edge_graph(): NSK_BLOCK + 1 = 257 weights, so k_mple_update's second block holds slot 256 alone;
    slot 255, the first block's last lane, and two more are fixed.  Two chains, each an example, all variables, 2 steps:
    weights, grad_max and skips are the host loop's bit for bit, weights on both sides of the edge move and the sums differ
    between the steps."""
    import pcd_latent
    g = pcd_latent.edge_graph()
    _, fg = session(g, seed=SEED, head_by_vid=True, chains=2)
    og = oracle_of(fg, True)
    # a second example: other values for the variables that are not evidence
    card, ev = fg.variable["cardinality"], fg.variable["isEvidence"] != 0
    fg.var_value[1] = np.where(ev, fg.var_value[1], np.random.default_rng(3).integers(0, card))
    states = fg.var_value.copy()
    assert (states[0] != states[1]).any()
    ids = np.arange(len(fg.variable), dtype=np.int64)
    twin = plgrad.Twin(fg, og, ids)
    fixed = fg.weight["isFixed"].astype(bool)
    edge = list(pcd_latent.EDGE_FIXED)
    assert len(fixed) == pcd_latent.EDGE_WEIGHTS == 257 and fixed[edge].all() and fixed.sum() == len(edge) and not fixed[256]
    nsteps, step, decay, reg = 2, 0.1, 0.9, 0.01
    w0 = fg.weight_value[0].astype(np.float64).copy()
    w, n, st = w0.copy(), 2 * len(twin.ids), step
    want_gmax, want_skipped, sums = np.zeros(nsteps), np.zeros(nsteps, np.int64), []
    for t in range(nsteps):
        parts = [twin.counts(x, w) for x in states]
        s = parts[0][0] + parts[1][0]
        want_skipped[t] = parts[0][1] + parts[1][1]
        want_gmax[t] = float(np.abs(s[~fixed]).max()) * plgrad.Q / n
        sums.append(s)
        w = mple_step(w, fixed, s, n, st, reg)
        st = st * decay
    res = fg.learn_mple(nsteps, step, decay=decay, reg_param=reg, var_ids=ids, var_copy="all")
    assert np.array_equal(fg.weight_slots()[edge], edge)                # a fixed weight's slot is its id
    assert res["n"] == n
    assert np.array_equal(_bits(fg.weight_value[0]), _bits(w)), np.nonzero(_bits(fg.weight_value[0]) != _bits(w))[0][:8]
    assert np.array_equal(_bits(res["grad_max"]), _bits(want_gmax)) and np.array_equal(res["skipped"], want_skipped)
    assert np.array_equal(_bits(w[fixed]), _bits(w0[fixed])) and want_gmax.min() > 0
    assert (w[:256] != w0[:256]).any() and w[256] != w0[256] and (sums[0] != sums[1]).any(), "the case stands still"
    fg.close()


# ---------------------------------------------------------------------------------------------- G
def test_mple_learns_the_planted_pairs_from_four_chains():
    """2000 planted pairs as four chains of a 500-pair graph -- four independent draws of it; 400 plain steps from
    weights 0 at the step size chosen on the host twin.  The device optimum lies within 1e-8 of the host optimum of the
    CPU test's procedure on the same data (two orders above the quantisation floor n_terms * 2^-33 / N)."""
    x, y = plgrad.planted_state()
    parts = [(x[i:i + 500], y[i:i + 500]) for i in range(0, 2000, 500)]
    _, fg = session(plgrad.planted_graph(500, *parts[0]), seed=SEED, chains=4)
    assert fg.var_value.shape == (4, 1000)
    for r, (px, py) in enumerate(parts):
        fg.var_value[r][0::2] = px
        fg.var_value[r][1::2] = py
    host, host_gmax = plgrad.pairs_mple(parts)
    ids = np.arange(1000)
    res = fg.learn_mple(plgrad.MPLE_STEPS, plgrad.MPLE_STEP, var_ids=ids, var_copy="all")
    got = fg.weight_value[0].copy()
    print("device optimum", got, "host", host, "equal bits:", np.array_equal(_bits(got), _bits(host)),
          "last grad_max %.3g" % res["grad_max"][-1])
    assert res["n"] == 4000 and not res["skipped"].any()
    assert np.abs(got - host).max() <= 1e-8
    assert res["grad_max"][-1] <= 1e-9
    assert np.array_equal(_bits(res["grad_max"]), _bits(host_gmax))
    learned = fg.log_pseudo_likelihood(ids, var_copy="all").sum()
    fg.weight_value[0][:] = plgrad.PLANTED
    planted = fg.log_pseudo_likelihood(ids, var_copy="all").sum()
    assert learned >= planted
    assert abs(learned - sum(plgrad.pairs_lpl(got, px, py) for px, py in parts)) <= 1e-8
