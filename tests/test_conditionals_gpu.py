"""Per-variable conditionals on the device (nsk_conditionals, the Rao-Blackwell accumulators of a sample trace).

Yardsticks: potentials must EQUAL the oracle's potential() (oracle.binding.Graph.potential, pinned to the reference) and
probabilities the numpy twin (numbskull_amd.diagnostics.conditional_probabilities) on those potentials with the oracle's
exp_det -- both as int64 bit patterns; the accumulators must equal the sequential sum, in row order, of the per-row
probabilities bit for bit.  tests/test_conditionals_cpu.py ties the twin to the ratio of joint probabilities."""

import ctypes as C

import numpy as np
import pytest

import numbskull_amd
from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import conditional_probabilities, tally_layout
from test_hip_parity import _small_graphs, GRAPHS
from util import orc, session, oracle_of, exact_marginals

pytestmark = pytest.mark.gpu

SEED = 77
_CACHE = {}


def _graph(golden, name):
    if not _CACHE:
        _CACHE.update(_small_graphs(golden))
    return _CACHE[name]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _selection(fg):
    """every variable of a small graph (None: the NULL selection); of a larger one a seeded sample of 1500 plus every
    variable of cardinality above 8 plus every variable with a list of 32 entries or more"""
    nvar = len(fg.variable)
    if nvar <= 2000:
        return None
    card = fg.variable["cardinality"].astype(np.int64)
    vtf = fg.variable["vtf_offset"].astype(np.int64)
    n = np.diff(np.concatenate([vtf, [len(fg.vmap)]]))
    longest = np.zeros(nvar, np.int64)
    np.maximum.at(longest, np.repeat(np.arange(nvar), n), fg.vmap["factor_index_length"].astype(np.int64))
    pick = np.random.default_rng(5).choice(nvar, 1500, replace=False)
    return np.unique(np.concatenate([pick, np.nonzero(card > 8)[0], np.nonzero(longest >= 32)[0]])).astype(np.int64)


def _oracle(og, sel, state, weights):
    """(offsets, potentials, probabilities) of the selection on `state` through the oracle and the twin"""
    state = np.ascontiguousarray(state, np.int64)
    weights = np.ascontiguousarray(weights, np.float64)
    card = og.variable["cardinality"].astype(np.int64)
    ids = np.arange(len(card)) if sel is None else np.asarray(sel)
    off = np.concatenate([[0], np.cumsum(card[ids])]).astype(np.int64)
    pot = np.zeros(int(off[-1]))
    for i, v in enumerate(ids):
        for k in range(card[v]):
            rc, pot[off[i] + k] = og.potential(int(v), k, state, weights)
            assert rc == 0, ("oracle refuses variable", v)
    assert np.isfinite(pot).all()
    prob = conditional_probabilities(off, pot, exp=orc.exp_det)
    assert np.isfinite(prob).all()
    return off, pot, prob


def _check(fg, og, sel, state, what, **kw):
    off, pot, prob = _oracle(og, sel, state, fg.weight_value[0])
    o1, p1 = fg.conditionals(sel, potentials=True, **kw)
    o2, p2 = fg.conditionals(sel, **kw)
    assert np.array_equal(o1, off) and np.array_equal(o2, off) and o1.dtype == np.int64
    assert p1.shape == pot.shape and p1.dtype == np.float64
    assert np.array_equal(_bits(p1), _bits(pot)), what
    assert np.array_equal(_bits(p2), _bits(prob)), what


# ---------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("name", GRAPHS)
def test_potentials_and_probabilities_equal_the_oracle(golden, name):
    g, hbv = _graph(golden, name)
    _, fg = session(g, seed=SEED, head_by_vid=hbv)
    og = oracle_of(fg, hbv)
    sel = _selection(fg)
    fg.inference(2, 3, True)
    _check(fg, og, sel, fg.var_value[0], name + " free")
    fg.learn(1, 3, 0.01, 0.95, 2, 0.01, 1)
    _check(fg, og, sel, fg.var_value_evid[0], name + " evidence", evidence_chain=True)
    _check(fg, og, sel, fg.var_value[0], name + " free after learning")
    _, f3 = session(g, seed=SEED, head_by_vid=hbv, chains=3)
    f3.inference(2, 3, True, var_copy="all")
    off, pots = f3.conditionals(sel, var_copy="all", potentials=True)
    _, probs = f3.conditionals(sel, var_copy="all")
    assert pots.shape == probs.shape == (3, int(off[-1]))
    for r in range(3):
        _, pot, prob = _oracle(og, sel, f3.var_value[r], f3.weight_value[0])
        assert np.array_equal(_bits(pots[r]), _bits(pot)), (name, r)
        assert np.array_equal(_bits(probs[r]), _bits(prob)), (name, r)


# ---------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("name", ["lr3000", "gencat_i32", "hubs"])
def test_selections(golden, name):
    L = _lib.lib()
    g, hbv = _graph(golden, name)
    _, fg = session(g, seed=SEED, head_by_vid=hbv, chains=3)
    fg.inference(1, 2, True, var_copy="all")
    nvar = len(fg.variable)
    for pot in (True, False):
        off, full = fg.conditionals(var_copy="all", potentials=pot)                     # NULL = every variable
        o2, listed = fg.conditionals(np.arange(nvar), var_copy="all", potentials=pot)
        assert np.array_equal(off, o2) and np.array_equal(_bits(full), _bits(listed))
        ids = np.random.default_rng(9).permutation(nvar)[:300]
        ids = np.concatenate([ids, ids[:40], [ids[0]] * 3])                           # shuffled, with repeats
        so, sub = fg.conditionals(ids, var_copy="all", potentials=pot)
        assert np.array_equal(np.diff(so), np.diff(off)[ids])
        want = np.concatenate([full[:, off[v]:off[v + 1]] for v in ids], axis=1)
        assert np.array_equal(_bits(sub), _bits(want))
        # a sub-range of the chains
        h = fg._engine()
        part = np.zeros((2, int(so[-1])))
        vids = _lib.as_c(ids, np.int64)
        _lib.check(L.nsk_conditionals(h, _lib.BUF_VALUE, 1, 2, _lib.ptr(vids), len(vids), 0 if pot else 1, _lib.ptr(part)))
        assert np.array_equal(_bits(part), _bits(sub[1:]))


def test_a_variable_without_a_position_reads_nan():
    x = np.random.default_rng(3).integers(0, 2, 20)
    out = {}
    for ev in (4, 1):
        g = list(graphgen.ising_grid(4, 5, weight=0.4))
        var = g[1].copy()
        var["isEvidence"][7] = ev
        var["initialValue"][7] = x[7]
        g[1] = var
        _, fg = session(tuple(g), seed=SEED)
        fg.var_value[0][:] = x
        out[ev] = [fg.conditionals(potentials=p)[1] for p in (True, False)] + [fg.conditionals([7, 3, 7])[1], fg.conditionals([7])[1]]
    for a, b in zip(out[4][:2], out[1][:2]):
        assert np.isnan(a[14:16]).all() and np.isfinite(b).all()
        keep = np.ones(40, bool)
        keep[14:16] = False
        assert np.array_equal(_bits(a[keep]), _bits(b[keep]))
    assert np.isnan(out[4][2][[0, 1, 4, 5]]).all() and np.array_equal(_bits(out[4][2][2:4]), _bits(out[1][2][2:4]))
    assert np.isnan(out[4][3]).all() and np.isfinite(out[1][3]).all()      # (a selection of such variables only: no launch)


# ---------------------------------------------------------------------------------------------- C
def _accumulate(fg, nchains, ids, epochs, thin, keep_rows):
    """burn-in 2, then `epochs` tallied sweeps under a trace of all variables with the accumulators on `ids`;
    returns (rows or None, sums, rows accumulated)"""
    L, h = _lib.lib(), fg._engine()
    vc = "all" if nchains > 1 else 0
    fg.burnIn(2, True, var_copy=vc)
    if nchains > 1:
        fg._chains()
    nrows = epochs // thin
    _lib.check(L.nsk_trace_setup(h, None, 0, thin, nrows))
    vids = None if ids is None else _lib.as_c(ids, np.int64)
    _lib.check(L.nsk_trace_conditionals(h, _lib.ptr(vids), 0 if ids is None else len(vids)))
    fg.inference(0, epochs, True, var_copy=vc)
    card = fg.variable["cardinality"].astype(np.int64)
    total = int(card.sum() if ids is None else card[np.asarray(ids)].sum())
    sums, got = np.full((nchains, total), -1.0), C.c_int64(-1)
    _lib.check(L.nsk_trace_download_conditionals(h, _lib.ptr(sums), C.byref(got)))
    rows = None
    if keep_rows:
        rows = np.zeros((nrows, nchains, len(card)), np.int8 if fg.info()["value_bytes"] == 1 else np.int32)
        _lib.check(L.nsk_trace_download(h, 0, nrows, _lib.ptr(rows), None))
    _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
    return rows, sums, got.value


@pytest.mark.parametrize("name", ["grid57x33", "lr3000", "gencat_i32", "hubs"])
@pytest.mark.parametrize("nchains", [1, 3])
@pytest.mark.parametrize("thin", [1, 3])
def test_accumulators_are_the_sequential_sum_of_the_rows(golden, name, nchains, thin):
    g, hbv = _graph(golden, name)
    vc = "all" if nchains > 1 else 0
    _, a = session(g, seed=SEED, head_by_vid=hbv, chains=nchains)
    _, b = session(g, seed=SEED, head_by_vid=hbv, chains=nchains)
    _, c = session(g, seed=SEED, head_by_vid=hbv, chains=nchains)
    _, d = session(g, seed=SEED, head_by_vid=hbv, chains=nchains)
    _, tw = session(g, seed=SEED, head_by_vid=hbv)
    rows, sums, got = _accumulate(a, nchains, None, 10, thin, True)
    assert got == 10 // thin == rows.shape[0]
    off = None
    want = np.zeros_like(sums)
    for i in range(rows.shape[0]):
        for r in range(nchains):
            tw.var_value[0][:] = rows[i, r]
            off, p = tw.conditionals()
            want[r] = want[r] + p
    assert np.isfinite(want).all()
    assert np.array_equal(_bits(sums), _bits(want))
    # the call with the accumulators leaves what the one without leaves
    plain = b.sample(10, thin=thin, burnin_epochs=2, sample_evidence=True, var_copy=vc)
    assert np.array_equal(rows, plain)
    assert np.array_equal(a.var_value, b.var_value) and np.array_equal(a.count, b.count)
    assert np.array_equal(a.chain_count, b.chain_count)
    assert a.info()["sweeps_done"] == b.info()["sweeps_done"]
    # a subset selection (any order, repeats) equals slices of the full one
    ids = [len(a.variable) - 1, 3, 0, 3]
    _, sub, got_sub = _accumulate(c, nchains, ids, 10, thin, False)
    assert got_sub == got
    assert np.array_equal(_bits(sub), _bits(np.concatenate([sums[:, off[v]:off[v + 1]] for v in ids], axis=1)))
    # ... and the method divides those sums by the rows
    rb = d.rao_blackwell(10, ids, thin=thin, burnin_epochs=2, sample_evidence=True)
    assert rb["rows"] == got and np.array_equal(_bits(rb["per_chain"]), _bits(sub / float(got)))
    assert np.array_equal(rb["marginals"], (sub / float(got)).mean(axis=0))
    assert np.isnan(rb["stderr"]).all() if nchains == 1 else np.isfinite(rb["stderr"]).all()
    assert np.array_equal(d.var_value, b.var_value) and np.array_equal(d.count, b.count)


# ---------------------------------------------------------------------------------------------- D
def test_packed_tally_rows_of_the_million_grid():
    """a one-chain handle of wide quads keeps its tally in bits 1-7 of the value bytes between the runs of a traced
    call: the accumulate launch must read bit 0 only"""
    n = 1000
    g = graphgen.ising_grid(n, n, weight=0.3)
    _, fg = session(g, seed=SEED)
    _, tw = session(g, seed=SEED)
    assert fg.info()["wide_quads"] > 0
    L, h = _lib.lib(), fg._engine()
    ids = _lib.as_c(np.arange(0, n * n, 251), np.int64)
    fg._push(0, 0)
    _lib.check(L.nsk_trace_setup(h, None, 0, 4, 3))
    _lib.check(L.nsk_trace_conditionals(h, _lib.ptr(ids), len(ids)))
    fg.inference(0, 12)
    sums, got = np.zeros((1, 2 * len(ids))), C.c_int64(0)
    _lib.check(L.nsk_trace_download_conditionals(h, _lib.ptr(sums), C.byref(got)))
    rows = np.zeros((3, 1, n * n), np.int8)
    _lib.check(L.nsk_trace_download(h, 0, 3, _lib.ptr(rows), None))
    _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
    assert got.value == 3 and rows.min() == 0 and rows.max() == 1
    assert np.array_equal(rows[2, 0], fg.var_value[0])
    want, closed = np.zeros(2 * len(ids)), np.zeros(2 * len(ids))
    i, j = ids // n, ids % n
    for r in range(3):
        tw.var_value[0][:] = rows[r, 0]
        want = want + tw.conditionals(ids)[1]
        x = rows[r, 0].astype(np.int64).reshape(n, n)
        p = np.zeros((2, len(ids)))
        for di, dj in ((-1, 0), (0, -1), (1, 0), (0, 1)):
            ii, jj = i + di, j + dj
            ok = (ii >= 0) & (ii < n) & (jj >= 0) & (jj < n)
            nb = x[np.clip(ii, 0, n - 1), np.clip(jj, 0, n - 1)]
            for k in (0, 1):
                p[k] += np.where(ok, np.where(nb == k, 0.3, -0.3), 0.0)
        e = np.exp(p)
        closed += (e / e.sum(axis=0)).T.reshape(-1)
    assert np.array_equal(_bits(sums[0]), _bits(want))
    print("1M grid: largest |sum - closed form| %.3g" % np.abs(sums[0] - closed).max())
    assert np.abs(sums[0] - closed).max() <= 1e-14


# ---------------------------------------------------------------------------------------------- E
def test_refusals_and_lifecycle(golden):
    L = _lib.lib()
    g, hbv = _graph(golden, "gencat_i32")
    _, fg = session(g, seed=SEED, head_by_vid=hbv, chains=2)
    _, tw = session(g, seed=SEED, head_by_vid=hbv)
    h = fg._engine()
    fg._chains()
    nvar = len(fg.variable)
    card = fg.variable["cardinality"].astype(np.int64)
    out = np.full(2 * int(card.sum()), 7.0)
    ids = _lib.as_c([5, 3, 5, nvar - 1], np.int64)
    total = int(card[ids].sum())

    def cond(which=_lib.BUF_VALUE, first=0, n=1, vids=ids, nvids=None, what=1, o=out):
        return L.nsk_conditionals(h, which, first, n, _lib.ptr(vids), (0 if vids is None else len(vids)) if nvids is None else nvids, what, _lib.ptr(o))

    assert L.nsk_trace_conditionals(h, None, 0) == _lib.E_INVALID           # no trace
    assert L.nsk_trace_conditionals(h, None, -1) == _lib.E_INVALID
    assert L.nsk_trace_download_conditionals(h, _lib.ptr(out), None) == _lib.E_INVALID
    for which in (-1, _lib.BUF_WEIGHT, 7):
        assert cond(which=which) == _lib.E_INVALID
    assert cond(first=2) == _lib.E_INVALID                                  # chain >= chains
    assert cond(first=1, n=2) == _lib.E_INVALID
    assert cond(first=-1) == _lib.E_INVALID
    assert cond(n=0) == _lib.E_INVALID
    assert cond(which=_lib.BUF_VALUE_EVID, first=1) == _lib.E_INVALID       # the evidence chain exists once
    assert cond(which=_lib.BUF_VALUE_EVID, n=2) == _lib.E_INVALID
    for what in (-1, 2):
        assert cond(what=what) == _lib.E_INVALID
    assert cond(vids=_lib.as_c([0, nvar], np.int64)) == _lib.E_INDEX
    assert cond(vids=_lib.as_c([-1], np.int64)) == _lib.E_INDEX
    assert cond(vids=None, nvids=3) == _lib.E_INVALID
    assert cond(nvids=-1) == _lib.E_INVALID
    assert cond(o=None) == _lib.E_INVALID
    before = fg.info()["device_bytes"]
    assert cond(nvids=0) == _lib.OK                                         # a list of no ids: nothing done
    assert (out == 7.0).all() and fg.info()["device_bytes"] == before
    assert cond(n=2) == _lib.OK and cond(which=_lib.BUF_VALUE_EVID) == _lib.OK and cond(vids=None, n=2) == _lib.OK
    # the accumulators: the arrays of the walk are up, so a selection costs its list and its sums
    assert L.nsk_trace_setup(h, None, 0, 2, 4) == _lib.OK
    bytes_trace = fg.info()["device_bytes"]
    assert L.nsk_trace_download_conditionals(h, _lib.ptr(out), None) == _lib.E_INVALID      # no selection
    assert L.nsk_trace_conditionals(h, _lib.ptr(ids), len(ids)) == _lib.OK
    ndev = 3
    assert fg.info()["device_bytes"] == bytes_trace + 4 * ndev + 8 * (ndev + 1) + 2 * 8 * int(card[[5, 3, nvar - 1]].sum())
    assert L.nsk_trace_conditionals(h, _lib.ptr(_lib.as_c([nvar], np.int64)), 1) == _lib.E_INDEX    # ... leaves the old one
    assert L.nsk_trace_conditionals(h, None, 2) == _lib.E_INVALID
    assert L.nsk_gibbs_sweeps(h, 4, 0, 0) == _lib.OK
    sums, got = np.zeros((2, total)), C.c_int64(-1)
    assert L.nsk_trace_download_conditionals(h, _lib.ptr(sums), C.byref(got)) == _lib.OK
    assert got.value == 2 and sums.min() > 0
    assert np.allclose(sums[:, :card[5]].sum(axis=1), 2.0, rtol=0, atol=1e-12)
    # nsk_trace_clear zeroes the sums and their row count
    assert L.nsk_trace_clear(h) == _lib.OK
    assert L.nsk_trace_download_conditionals(h, _lib.ptr(sums), C.byref(got)) == _lib.OK
    assert got.value == 0 and not sums.any()
    assert L.nsk_gibbs_sweeps(h, 2, 0, 0) == _lib.OK
    assert L.nsk_trace_download_conditionals(h, _lib.ptr(sums), C.byref(got)) == _lib.OK
    now = np.zeros((2, total))
    assert cond(n=2, o=now) == _lib.OK
    assert got.value == 1 and np.array_equal(_bits(sums), _bits(now))
    # calling again replaces the selection and zeroes the sums
    one = _lib.as_c([3], np.int64)
    assert L.nsk_trace_conditionals(h, _lib.ptr(one), 1) == _lib.OK
    assert fg.info()["device_bytes"] == bytes_trace + 4 + 16 + 2 * 8 * int(card[3])
    s1 = np.full((2, int(card[3])), -1.0)
    assert L.nsk_trace_download_conditionals(h, _lib.ptr(s1), C.byref(got)) == _lib.OK
    assert got.value == 0 and not s1.any()
    # switched off: the buffers go, the trace stays
    assert L.nsk_trace_conditionals(h, None, -1) == _lib.OK
    assert fg.info()["device_bytes"] == bytes_trace
    assert L.nsk_trace_download_conditionals(h, _lib.ptr(s1), None) == _lib.E_INVALID
    assert L.nsk_gibbs_sweeps(h, 2, 0, 0) == _lib.OK
    # replacing the trace resets them to off, and so does tearing it down
    assert L.nsk_trace_conditionals(h, None, 0) == _lib.OK
    assert L.nsk_trace_setup(h, None, 0, 1, 2) == _lib.OK
    assert L.nsk_trace_download_conditionals(h, _lib.ptr(out), None) == _lib.E_INVALID
    assert L.nsk_gibbs_sweeps(h, 1, 0, 0) == _lib.OK
    assert L.nsk_trace_conditionals(h, None, 0) == _lib.OK
    with_sums = fg.info()["device_bytes"]
    assert L.nsk_trace_setup(h, None, 0, 1, 0) == _lib.OK
    assert fg.info()["device_bytes"] < with_sums - 2 * 8 * int(card.sum())
    assert L.nsk_gibbs_sweeps(h, 3, 0, 0) == _lib.OK
    assert L.nsk_trace_conditionals(h, None, 0) == _lib.E_INVALID
    assert L.nsk_trace_download_conditionals(h, _lib.ptr(out), None) == _lib.E_INVALID
    # an own_range handle
    from numbskull_amd.distributed import shard_range
    ns = numbskull_amd.NumbSkull(quiet=True, seed=SEED)
    w, v, f, fm, dm, edges = [x.copy() if isinstance(x, np.ndarray) else x for x in _graph(golden, "grid57x33")[0]]
    ns.loadFactorGraph(w, v, f, fm, dm, int(edges), own_range=shard_range(0, 2, len(v)))
    sh = ns.factorGraphs[0]
    assert L.nsk_conditionals(sh._engine(), _lib.BUF_VALUE, 0, 1, None, 0, 1, _lib.ptr(np.zeros(2 * len(v)))) == _lib.E_INVALID
    with pytest.raises(ValueError):
        sh.conditionals()


# ---------------------------------------------------------------------------------------------- F
@pytest.mark.parametrize("name", ["grid57x33", "lr3000", "gencat_i32", "hubs"])
def test_the_calls_only_read(golden, name):
    L = _lib.lib()
    g, hbv = _graph(golden, name)
    _, a = session(g, seed=SEED, head_by_vid=hbv)
    _, b = session(g, seed=SEED, head_by_vid=hbv)
    for fg in (a, b):
        fg.learn(1, 2, 0.01, 0.95, 2, 0.01, 1)
        fg.inference(1, 4, True)

    def state(fg):
        n, nw = len(fg.variable), len(fg.weight)
        vv, ve, wv, cnt = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(nw), np.zeros(len(fg.count), np.int64)
        _lib.check(L.nsk_state_download(fg._engine(), _lib.ptr(vv), _lib.ptr(ve), _lib.ptr(wv), _lib.ptr(cnt)))
        return vv, ve, wv, cnt, fg.info()["sweeps_done"]

    before = state(a)
    h = a._engine()
    out = np.zeros(int(a.variable["cardinality"].sum()))
    for which in (_lib.BUF_VALUE, _lib.BUF_VALUE_EVID):
        for what in (0, 1):
            assert L.nsk_conditionals(h, which, 0, 1, None, 0, what, _lib.ptr(out)) == _lib.OK
    for x, y in zip(before, state(a)):
        assert np.array_equal(x, y)
    a.conditionals()
    a.log_pseudo_likelihood()
    # continuing the chain gives the samples of a twin that never asked
    for fg in (a, b):
        fg.inference(0, 3, True)
        fg.learn(0, 1, 0.01, 0.95, 2, 0.01, 1)
    assert np.array_equal(a.var_value, b.var_value) and np.array_equal(a.var_value_evid, b.var_value_evid)
    assert np.array_equal(a.count, b.count) and np.array_equal(_bits(a.weight_value), _bits(b.weight_value))


def test_log_pseudo_likelihood_is_the_sum_over_the_query_variables(golden):
    g, hbv = _graph(golden, "lr3000")
    _, fg = session(g, seed=SEED, head_by_vid=hbv, chains=2)
    fg.inference(1, 2, True, var_copy="all")
    free = np.nonzero(fg.variable["isEvidence"] == 0)[0]
    off, prob = fg.conditionals(free, var_copy="all")
    lpl = fg.log_pseudo_likelihood(var_copy="all")
    assert lpl.shape == (2,)
    for r in range(2):
        want = np.log(prob[r][off[:-1] + fg.var_value[r][free]]).sum()
        assert abs(lpl[r] - want) <= 1e-12 * len(free)
    one = fg.log_pseudo_likelihood(free[:50], var_copy=1)
    assert isinstance(one, float) and abs(one - np.log(prob[1][off[:50] + fg.var_value[1][free[:50]]]).sum()) <= 1e-10


# ---------------------------------------------------------------------------------------------- G
def test_nothing_is_held_until_asked(golden):
    L = _lib.lib()
    g, hbv = _graph(golden, "grid57x33")
    nvar, nfactor, nedge = len(g[1]), len(g[2]), int(g[5])
    res = {}
    for order in ("conditionals first", "sequential scan and log-potential first"):
        _, fg = session(g, seed=SEED)
        h = fg._engine()
        fg.inference(1, 2)
        created = fg.info()["device_bytes"]                                  # (with the staging of the state transfers)
        fg.inference(0, 2)
        assert fg.info()["device_bytes"] == created                          # the grid lives in tiles: no generic arrays, nothing for the walk
        lp = np.zeros(1)
        steps = {}
        for step in (("cond", "seq", "lp") if order.startswith("cond") else ("seq", "lp", "cond")):
            b0 = fg.info()["device_bytes"]
            if step == "cond":
                off, pot = fg.conditionals(potentials=True)
                _, prob = fg.conditionals()
                again = fg.info()["device_bytes"]
                fg.conditionals()
                assert fg.info()["device_bytes"] == again                     # the second query uploads nothing
            elif step == "seq":
                _lib.check(L.nsk_set_scan(h, _lib.SCAN_SEQUENTIAL))
            else:
                _lib.check(L.nsk_log_potential(h, _lib.BUF_VALUE, 0, 1, _lib.ptr(lp)))
            steps[step] = fg.info()["device_bytes"] - b0
        res[order] = (steps, fg.info()["device_bytes"] - created, pot, prob, lp[0])
        if order.startswith("cond"):
            # the documented arrays: 4 bytes a position, 4 a list slot + 4, 4 a list entry; 16 a factor, 8 an edge, 4 a variable
            # (positions and list slots include the padding of the colour classes: at least one per variable)
            lists = nedge
            low = 4 * nvar + 4 * (nvar + 1) + 4 * lists + 16 * nfactor + 8 * nedge + 4 * nvar
            assert low <= steps["cond"] <= low + 3 * 4 * (nvar + 1024), (steps, low)
        else:
            assert steps["cond"] == 0                                           # the sequential scan's arrays serve the walk
    (sa, ta, pa, qa, la), (sb, tb, pb, qb, lb) = res.values()
    assert ta == tb                                                             # either order ends with the same arrays, once each
    assert np.array_equal(_bits(pa), _bits(pb)) and np.array_equal(_bits(qa), _bits(qb)) and _bits(la)[0] == _bits(lb)[0]


# ---------------------------------------------------------------------------------------------- J
def test_rao_blackwell_marginals_against_exact_enumeration():
    """3 x 4 Ising grid, weight 0.5, variables 0, 5, 11 evidence at 1, 0, 1; 64 chains x 3200 tallied sweeps after 10 of
    burn-in.  0.01 is the project's tolerance for a marginal at 2 x 10^5 sweeps; on the CPU oracle
    the estimator's largest error over three seed sets of that size was 0.0041 / 0.0005 / 0.0011 (the tally's 0.0058 /
    0.0009 / 0.0024)."""
    g = list(graphgen.ising_grid(3, 4, weight=0.5))
    var = g[1].copy()
    var["isEvidence"][[0, 5, 11]] = 1
    var["initialValue"][[0, 5, 11]] = [1, 0, 1]
    g[1] = var
    _, fg = session(tuple(g), seed=SEED, chains=64)
    og = oracle_of(fg)
    exact = exact_marginals(og, fg.weight_value[0], sample_mask=var["isEvidence"] == 0)
    rb = fg.rao_blackwell(3200, burnin_epochs=10)
    free = np.nonzero(var["isEvidence"] == 0)[0]
    assert rb["rows"] == 3200 and rb["per_chain"].shape == (64, 18) and np.array_equal(rb["offsets"], 2 * np.arange(10))
    want = np.concatenate([exact[int(v)] for v in free])
    err_rb = np.abs(rb["marginals"] - want).max()
    err_tally = np.abs(fg.marginals[fg.cstart[free]] - want[1::2]).max()
    print("largest error against exact enumeration: Rao-Blackwell %.5f, tally %.5f; largest stderr %.5f"
          % (err_rb, err_tally, rb["stderr"].max()))
    assert err_rb <= 0.01
    assert np.array_equal(tally_layout(rb["offsets"], rb["marginals"])[1], rb["marginals"][1::2])
