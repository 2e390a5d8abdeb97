"""Pairwise joint marginals from the trace on the device (nsk_trace_pair_counts, FactorGraph.pairwise).  The yardstick
is the trace itself, downloaded with nsk_trace_download: the device's integers must equal diagnostics.pair_counts of
those rows (np.array_equal, no tolerance), and FactorGraph.pairwise diagnostics.pair_tables of them, float for float --
both sides go through that one function.  One trace of 300 rows is recorded per graph and chain count; the cases are
windows of it.  The last test holds the tables to the exact joint of a 12-variable grid, enumerated."""

import ctypes as C

import numpy as np
import pytest

from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import factor_pairs, pair_counts, pair_tables
from test_hip_parity import _small_graphs
from test_trace_ess_gpu import _download, _everything, _grid_with_evidence, _record
from util import oracle_of, session

pytestmark = pytest.mark.gpu

SEED = 92
ROWS = 300
# (first row, rows): one row, a partial block, exactly one, one and a row, two and a row, four and a partial one; then
# windows that do not start at row 0 (the last ends with the last row recorded)
WINDOWS = [(0, 1), (0, 63), (0, 64), (0, 65), (0, 129), (0, 300), (1, 299), (37, 200), (296, 4)]
_RECORDED = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_recorded():
    yield
    _RECORDED.clear()


def _recorded(golden, name, nchains):
    """(handle, its ROWS rows) of every variable of a small graph, listed (the caller's columns = the variables)"""
    key = (name, nchains)
    if key not in _RECORDED:
        g = _small_graphs(golden)[name][0]
        nvar = len(g[1])
        assert (g[1]["cardinality"] == 2).all()
        fg = _record(g, nchains, np.arange(nvar), ROWS, seed=SEED)
        rows = _download(fg, 0, ROWS, nvar)
        assert rows.shape == (ROWS, nchains, nvar)
        rows.setflags(write=False)
        _RECORDED[key] = (fg, rows)
    return _RECORDED[key]


def _counts(fg, first, nrows, pairs):
    pairs = _lib.as_c(np.asarray(pairs).reshape(-1, 2), np.int64)
    nchains = _lib.lib().nsk_get_chains(fg._engine())
    out = np.full((len(pairs), nchains, 3), -7, np.int64)
    _lib.check(_lib.lib().nsk_trace_pair_counts(fg._engine(), first, nrows, _lib.ptr(pairs), len(pairs), _lib.ptr(out)))
    return out


def _pair_list(nvar):
    """the pairs the layout can get wrong, then random ones up to about 300"""
    last = nvar - 1
    special = [(0, last), (last, 0), (last, last), (0, 0), (3, 3), (0, 1), (1, 0), (5, 17), (5, 17), (17, 5)]
    if nvar > 65:
        special += [(63, 64), (64, 63), (63, 63), (64, 64), (62, 63), (64, 65)]  # bit 63 of one word, bit 0 of the next
    if nvar == 57 * 33:
        assert last // 64 == 29 and last % 64 == 24                              # 30 words, the last one partial
        special += [(0, 63), (127, 128), (last, last - 1), (last - 24, last),    # the last word: its bits 0 and 24
                    (last, 63), (1855, 1856), (700, 1300), (1300, 700), (1, 1879)]
    rng = np.random.default_rng(nvar)
    rand = rng.integers(0, nvar, (300 - len(special) if nvar == 57 * 33 else 60, 2))
    return np.array(special + rand.tolist(), np.int64)


@pytest.mark.parametrize("nchains", [1, 3])
@pytest.mark.parametrize("name", ["grid57x33", "grid4x5", "pairs"])
def test_counts_equal_numpy_on_the_rows(golden, name, nchains):
    fg, rows = _recorded(golden, name, nchains)
    nvar = rows.shape[2]
    pairs = _pair_list(nvar)
    if name == "grid57x33":
        words = pairs // 64
        assert (words[:, 0] == words[:, 1]).sum() > 10 and (words[:, 0] != words[:, 1]).sum() > 200
        assert len(np.unique(words)) == 30                                       # every word is touched
    for first, nrows in WINDOWS:
        want = pair_counts(rows[first:first + nrows], pairs)
        got = _counts(fg, first, nrows, pairs)
        assert got.shape == want.shape and np.array_equal(got, want), (first, nrows, np.argwhere(got != want)[:5])
    # liveliness: the columns move, and not together
    if name == "grid57x33":
        full = pair_counts(rows, pairs)
        n11, na, nb = full[:, :, 0], full[:, :, 1], full[:, :, 2]
        assert (na > 0).all() and (na < ROWS).all()
        assert (n11[pairs[:, 0] != pairs[:, 1]] < np.minimum(na, nb)[pairs[:, 0] != pairs[:, 1]]).all()
    # a selection inside one word, and one pair alone: other word lists, other slots
    for sel in (pairs[(pairs // 64 == (pairs // 64)[:, :1]).all(axis=1)][:7], pairs[:1], pairs[-1:]):
        assert np.array_equal(_counts(fg, 37, 200, sel), pair_counts(rows[37:237], sel))


def test_columns_repeated_unsorted_and_an_evidence_variable():
    g, ev = _grid_with_evidence()
    n = len(g[1])
    ids = [n - 1, 5, 700, int(ev[1]), 5, 0, 123, n - 1, 64, 63, 65, 1279]        # ev[1] = 1000 is fixed at 0, 64 at 1
    for nchains in (1, 3):
        fg = _record(g, nchains, ids, 131, se=False, seed=SEED)
        rows = _download(fg, 0, 131, len(ids))
        assert rows[:, :, 3].max() == 0 and rows[:, :, 8].min() == 1             # evidence stays
        pairs = np.array([(8, 1), (1, 8), (3, 2), (2, 3), (0, 7), (4, 1), (9, 10), (11, 6), (3, 8), (8, 8), (3, 3), (5, 5)])
        for first, nrows in ((0, 131), (2, 65)):
            got = _counts(fg, first, nrows, pairs)
            assert np.array_equal(got, pair_counts(rows[first:first + nrows], pairs))
            assert np.array_equal(got[0, :, 0], got[0, :, 2]) and np.array_equal(got[1, :, 0], got[1, :, 1])     # against ones: the other's n1
            assert (got[0, :, 1] == nrows).all()
            assert (got[2, :, 0] == 0).all() and (got[3, :, 0] == 0).all() and (got[2, :, 1] == 0).all()          # against zeros
            assert (got[8] == [0, 0, nrows]).all() and (got[9] == nrows).all() and (got[10] == 0).all()
            assert np.array_equal(got[5, :, 0], got[5, :, 1]) and np.array_equal(got[5, :, 0], got[5, :, 2])     # one variable in two columns
            assert (got[5, :, 0] > 0).all() and (got[5, :, 0] < nrows).all() and (got[4] == nrows).all()


def test_full_state_trace_equals_the_listed_trace_of_a_twin():
    """vids = NULL: the dense record kernel's rows, every internal id -- the caller's columns are not the device's"""
    g = graphgen.ising_grid(57, 33, weight=0.3)
    n = 57 * 33
    dense = _record(g, 2, None, 131, seed=SEED)
    listed = _record(g, 2, np.arange(n), 131, seed=SEED)
    rows = _download(listed, 0, 131, n)
    assert np.array_equal(_download(dense, 0, 131, n), rows)
    pairs = _pair_list(n)
    want = pair_counts(rows[1:131], pairs)
    assert np.array_equal(_counts(listed, 1, 130, pairs), want)
    assert np.array_equal(_counts(dense, 1, 130, pairs), want)


def test_the_call_changes_nothing(golden):
    """values, tallies, sweeps_done, the rows and device_bytes (the buffers are the call's alone); the profiling
    bracket counts none of its launches; later sweeps go on as on a twin that never asked"""
    L = _lib.lib()
    g = _small_graphs(golden)["grid57x33"][0]
    n = len(g[1])
    fg = _record(g, 2, None, 140, capacity=149, seed=SEED)
    twin = _record(g, 2, None, 140, capacity=149, seed=SEED)
    before = _everything(fg, 131, n)
    ms, nl = C.c_double(), C.c_int64()
    _lib.check(L.nsk_profile_begin(fg._engine()))
    _counts(fg, 0, 140, _pair_list(n))
    _counts(fg, 3, 131, [(5, 1880), (64, 64)])
    _lib.check(L.nsk_profile_end(fg._engine(), C.byref(ms), C.byref(nl)))
    assert nl.value == 0
    for a, b in zip(before, _everything(fg, 131, n)):
        assert np.array_equal(a, b)
    fg.inference(0, 9, True, var_copy="all")
    twin.inference(0, 9, True, var_copy="all")
    for a, b in zip(_everything(fg, 140, n), _everything(twin, 140, n)):
        assert np.array_equal(a, b)


def test_refusals(golden):
    """each decided on the host before a launch"""
    L = _lib.lib()
    fg, rows = _recorded(golden, "grid57x33", 3)
    h, n = fg._engine(), rows.shape[2]
    one = np.array([[0, 1]], np.int64)
    out = np.zeros((4, 3, 3), np.int64)

    def call(first, nrows, p=one, npairs=None, handle=h, o=out):
        return L.nsk_trace_pair_counts(handle, first, nrows, _lib.ptr(p), len(p) if npairs is None else npairs, _lib.ptr(o))

    assert call(0, ROWS) == _lib.OK
    assert call(0, 1, handle=None) == _lib.E_INVALID                   # null graph
    assert call(0, 0) == _lib.E_INVALID and call(0, -3) == _lib.E_INVALID          # nrows < 1
    assert call(-1, 8) == _lib.E_INVALID                               # first_row < 0
    assert call(0, 8, npairs=-1) == _lib.E_INVALID                     # npairs < 0
    assert call(0, 8, p=None, npairs=1) == _lib.E_INVALID and call(0, 8, o=None) == _lib.E_INVALID     # null with pairs to serve
    assert call(0, ROWS + 1) == _lib.E_INVALID                         # rows beyond those recorded
    assert b"recorded" in L.nsk_last_error()
    assert call(ROWS - 4, 4) == _lib.OK and call(ROWS - 4, 5) == _lib.E_INVALID and call(ROWS, 1) == _lib.E_INVALID
    assert b"recorded" in L.nsk_last_error()
    assert call(ROWS - 1, 1) == _lib.OK
    assert call(0, 8, np.array([[0, n]], np.int64)) == _lib.E_INDEX
    assert call(0, 8, np.array([[3, 4], [-1, 2]], np.int64)) == _lib.E_INDEX
    assert b"column index" in L.nsk_last_error()
    assert call(0, 8, np.array([[n - 1, n - 1]], np.int64)) == _lib.OK
    assert L.nsk_trace_pair_counts(h, 0, 8, None, 0, None) == _lib.OK          # no pairs: nothing to do
    # no trace; plain rows
    g = _small_graphs(golden)["grid57x33"][0]
    _, bare = session(g, seed=SEED)
    bare.inference(0, 1, True)
    assert call(0, 1, handle=bare._engine()) == _lib.E_INVALID
    assert b"no trace" in L.nsk_last_error()
    gc = _small_graphs(golden)["gencat"][0]
    assert (gc[1]["cardinality"] > 2).any()
    plain = _record(gc, 2, None, 8, seed=SEED)
    packed = C.c_int64(1)
    _lib.check(L.nsk_trace_rows(plain._engine(), None, None, C.byref(packed)))
    assert packed.value == 0
    assert call(0, 8, handle=plain._engine()) == _lib.E_INVALID
    assert b"bit-packed" in L.nsk_last_error()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def test_pairwise_is_the_table_of_the_downloaded_trace(golden):
    """FactorGraph.pairwise against pair_tables(pair_counts(sample(...))) of a twin, every field equal; state and
    tallies as the twin's; the trace torn down"""
    g, ev = _grid_with_evidence()
    n = len(g[1])
    explicit = np.array([(n - 2, 5), (5, n - 2), (700, 700), (63, 65), (int(ev[0]), 65), (int(ev[1]), 0), (5, 700), (1279, 123)])
    for thin, pairs in ((1, explicit), (2, "factors"), (2, explicit), (1, "factors")):
        _, a = session(g, seed=SEED, chains=3)
        _, b = session(g, seed=SEED, chains=3)
        epochs = 70 * thin + (thin - 1)
        t = a.pairwise(epochs, pairs, thin=thin, burnin_epochs=3)
        plist = factor_pairs(a.factor, a.fmap) if isinstance(pairs, str) else pairs
        vids, cols = np.unique(plist, return_inverse=True)
        rows = b.sample(epochs, var_ids=vids, thin=thin, burnin_epochs=3, sample_evidence=False, var_copy="all")
        assert rows.shape == (70, 3, len(vids))
        want = pair_tables(pair_counts(rows, cols.reshape(-1, 2)), 70)
        assert t.samples == want.samples == 210 and len(t.cov) == len(plist)
        for name in ("joint", "cov", "corr", "mi", "counts"):
            assert _same(getattr(t, name), getattr(want, name)), name
        if isinstance(pairs, str):
            assert len(plist) == 56 * 33 + 57 * 32 and np.isfinite(t.corr).mean() > 0.99 and np.nanmean(t.corr) > 0.05
        else:
            assert np.isnan(t.corr[[4, 5]]).all() and np.isfinite(t.corr[[0, 1, 2, 3, 6, 7]]).all() and t.corr[2] == 1.0
            assert np.array_equal(t.joint[0], t.joint[1].T) and t.joint[4][0].sum() == 0 and t.joint[5][1].sum() == 0
        assert np.array_equal(a.var_value, b.var_value) and np.array_equal(a.count, b.count)
        assert np.array_equal(a.chain_count, b.chain_count) and a.info()["sweeps_done"] == b.info()["sweeps_done"]
        assert np.array_equal(a.marginals, b.marginals) and np.array_equal(a.rhat, b.rhat, equal_nan=True)
        rows_left, cap = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().nsk_trace_rows(a._engine(), C.byref(rows_left), C.byref(cap), None))
        assert (rows_left.value, cap.value) == (0, 0)          # torn down


def test_pairwise_one_chain_nothing_to_count_and_what_it_refuses(golden):
    g = _small_graphs(golden)["grid57x33"][0]
    n = len(g[1])
    _, one = session(g, seed=SEED)
    _, twin = session(g, seed=SEED)
    t = one.pairwise(40, [(3, 4), (4, 3)])
    rows = twin.sample(40, var_ids=[3, 4], var_copy="all")
    assert rows.shape == (40, 1, 2) and t.samples == 40
    want = pair_tables(pair_counts(rows, [(0, 1), (1, 0)]), 40)
    for name in ("joint", "cov", "corr", "mi", "counts"):
        assert _same(getattr(t, name), getattr(want, name)), name
    assert np.array_equal(one.var_value, twin.var_value) and np.array_equal(one.count, twin.count)
    # no rows, no pairs: no trace, and the sweeps still run
    _, few = session(g, seed=SEED, chains=2)
    _, ref = session(g, seed=SEED, chains=2)
    t = few.pairwise(3, [(0, 1)], thin=4)
    assert t.samples == 0 and t.joint.shape == (1, 2, 2) and np.isnan(t.joint).all() and np.isnan(t.mi).all()
    t = few.pairwise(5, np.zeros((0, 2), np.int64))
    assert t.samples == 10 and t.joint.shape == (0, 2, 2) and t.counts.shape == (0, 2, 3)
    ref.inference(0, 3, False, var_copy="all")
    ref.inference(0, 5, False, var_copy="all")
    assert np.array_equal(few.var_value, ref.var_value) and np.array_equal(few.chain_count, ref.chain_count)
    with pytest.raises(ValueError):
        few.pairwise(8, [(0, 1)], thin=0)
    with pytest.raises(ValueError):
        few.pairwise(8, [0, 1, 2])
    with pytest.raises(ValueError):
        few.pairwise(8, "edges")
    with pytest.raises(IndexError):
        few.pairwise(8, [(0, n)])
    with pytest.raises(IndexError):
        few.pairwise(8, [(-1, 0)])
    gc = _small_graphs(golden)["gencat"][0]
    _, cat = session(gc, seed=SEED, chains=2)
    wide = int(np.argmax(gc[1]["cardinality"] > 2))
    with pytest.raises(ValueError, match="binary"):
        cat.pairwise(8, [(wide, wide)])
    rows_left, cap = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().nsk_trace_rows(cat._engine(), C.byref(rows_left), C.byref(cap), None))
    assert (rows_left.value, cap.value) == (0, 0)


def _exact_edge_joints(og, weight_value, pairs):
    """The loop of util.exact_marginals for pairs: every assignment of the (binary, all free) variables weighed with
    the oracle's eval_factor; returns (npairs, 2, 2), indexed [value of a][value of b]"""
    n = len(og.variable)
    assert (og.variable["cardinality"] == 2).all() and n <= 16
    total = 1 << n
    logp = np.zeros(total)
    states = np.zeros((total, n), np.int64)
    for s in range(total):
        x = np.array([(s >> i) & 1 for i in range(n)], np.int64)
        states[s] = x
        e = 0.0
        for fid in range(len(og.factor)):
            rc, val = og.eval_factor(fid, -1, 0, x)
            assert rc == 0
            e += weight_value[int(og.factor[fid]["weightId"])] * val
        logp[s] = e
    p = np.exp(logp - logp.max())
    p /= p.sum()
    out = np.zeros((len(pairs), 2, 2))
    for j, (a, b) in enumerate(pairs):
        for va in (0, 1):
            for vb in (0, 1):
                out[j, va, vb] = p[(states[:, a] == va) & (states[:, b] == vb)].sum()
    return out


def test_edge_joints_match_exact_enumeration():
    """Ground truth without the generator: the 4 x 3 Ising grid with w = 0.5 of test_marginals_match_exact_enumeration,
    4 chains x 50 000 rows after 100 burn-in sweeps (its 200 000 samples), every cell of the joint of each of the 17
    edges against the enumeration of the 4096 states.  A cell is a Bernoulli mean: its standard error is
    <= 0.5 / sqrt(N_eff) ~ 2.5e-3 at N_eff ~ N / 5, so the tolerance is that test's 0.01."""
    g = graphgen.ising_grid(4, 3, weight=0.5)
    _, fg = session(g, seed=123, chains=4)
    og = oracle_of(fg, False)
    t = fg.pairwise(50000, "factors", burnin_epochs=100, sample_evidence=True)
    pairs = factor_pairs(fg.factor, fg.fmap)
    assert len(pairs) == 17 and t.samples == 200000 and t.joint.shape == (17, 2, 2)
    exact = _exact_edge_joints(og, og.weight["initialValue"].astype(float), pairs)
    np.testing.assert_allclose(exact.sum(axis=(1, 2)), 1.0, atol=1e-12)
    err = np.abs(t.joint - exact)
    print("largest cell error %.5f" % err.max())
    assert err.max() < 0.01, (np.argwhere(err >= 0.01), t.joint, exact)
    assert (t.corr > 0.1).all() and (t.mi > 0).all()                   # w = 0.5 couples the ends of every edge
