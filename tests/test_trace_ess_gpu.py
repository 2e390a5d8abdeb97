"""Effective sample size from the trace on the device (nsk_trace_ess, nsk_trace_autocov_counts, FactorGraph.mixing).
The yardstick is the trace itself, downloaded with nsk_trace_download: the device's integers must equal
diagnostics.autocov_counts of those rows, and its four result arrays diagnostics.ess_from_counts of those integers,
bit for bit (np.array_equal, NaNs equal): the epilogue is integer -> float64 conversions and correctly rounded float64
+ - x / in one fixed order on both sides.  One trace of 300 rows is recorded per graph and chain count; the cases are
windows of it."""

import ctypes as C

import numpy as np
import pytest

from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import autocov_counts, effective_sample_size, ess_from_counts
from test_hip_parity import _small_graphs
from util import session

pytestmark = pytest.mark.gpu

SEED = 91
ROWS = 300
LAGS = (1, 2, 31, 62, 63)
_RECORDED = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_recorded():
    yield
    _RECORDED.clear()


def _record(g, nchains, vids, rows, se=True, seed=SEED, capacity=None):
    """a handle with `rows` trace rows of `vids` (None: every variable), one sweep a row"""
    L = _lib.lib()
    _, fg = session(g, seed=seed, chains=nchains)
    h = fg._engine()
    if nchains > 1:
        fg._chains()
    ids = None if vids is None else _lib.as_c(np.asarray(vids), np.int64)
    _lib.check(L.nsk_trace_setup(h, _lib.ptr(ids), 0 if ids is None else len(ids), 1, capacity or rows))
    fg.inference(0, rows, se, var_copy="all" if nchains > 1 else 0)
    return fg


def _download(fg, first, nrows, ncols):
    nchains = _lib.lib().nsk_get_chains(fg._engine())
    out = np.zeros((nrows, nchains, ncols), np.int8 if fg.info()["value_bytes"] == 1 else np.int32)
    _lib.check(_lib.lib().nsk_trace_download(fg._engine(), first, nrows, _lib.ptr(out), None))
    return out


def _recorded(golden, name, nchains):
    """(handle, its ROWS rows) of every variable of a small graph, listed (device columns = the variables)"""
    key = (name, nchains)
    if key not in _RECORDED:
        g = _small_graphs(golden)[name][0]
        nvar = len(g[1])
        assert (g[1]["cardinality"] == 2).all()
        fg = _record(g, nchains, np.arange(nvar), ROWS)
        rows = _download(fg, 0, ROWS, nvar)
        rows.setflags(write=False)
        _RECORDED[key] = (fg, rows)
    return _RECORDED[key]


def _counts(fg, first, nrows, max_lag, cols):
    """nsk_trace_autocov_counts as (A (L + 1, ncols), S1, S2)"""
    lag = min(max_lag, nrows // 2 - 1)
    cols = _lib.as_c(np.asarray(cols), np.int64)
    out = np.full((len(cols), lag + 3), -7, np.int64)
    _lib.check(_lib.lib().nsk_trace_autocov_counts(fg._engine(), first, nrows, max_lag, _lib.ptr(cols), len(cols), _lib.ptr(out)))
    return out[:, :lag + 1].T.copy(), out[:, lag + 1].copy(), out[:, lag + 2].copy()


def _summary(fg, first, nrows, max_lag, ncols):
    mean, tau, rhat2 = (np.full(ncols, -7.0) for _ in range(3))
    truncated = np.full(ncols, 7, np.uint8)
    _lib.check(_lib.lib().nsk_trace_ess(fg._engine(), first, nrows, max_lag, _lib.ptr(mean), _lib.ptr(tau), _lib.ptr(rhat2),
                                        _lib.ptr(truncated)))
    return mean, tau, rhat2, truncated


def _check_window(fg, rows, first, nrows, max_lag, cols=None):
    """both entry points on rows [first, first + nrows) against numpy on the downloaded rows"""
    ncols = rows.shape[2]
    cols = np.arange(ncols) if cols is None else np.asarray(cols)
    x = rows[first:first + nrows]
    n, H, A, S1, S2 = autocov_counts(x, max_lag)
    dA, dS1, dS2 = _counts(fg, first, nrows, max_lag, cols)
    assert dA.shape == (A.shape[0], len(cols))
    assert np.array_equal(dA, A[:, cols]) and np.array_equal(dS1, S1[cols]) and np.array_equal(dS2, S2[cols])
    want = ess_from_counts(n, H, A, S1, S2)
    got = _summary(fg, first, nrows, max_lag, ncols)
    for what, a, b in zip(("mean", "tau", "rhat2", "truncated"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (what, first, nrows, max_lag)
    return want


@pytest.mark.parametrize("s", [9, 127, 128, 131, 257, 260])
@pytest.mark.parametrize("nchains", [2, 3])
@pytest.mark.parametrize("name", ["grid57x33", "grid4x5", "pairs"])
def test_counts_and_summary_equal_numpy_on_the_rows(golden, name, nchains, s):
    """n = 4, 63, 64, 65, 128, 130: one partial block, exactly one block, a carry across the block boundary, two blocks
    and a partial one; grid57x33 is 30 words with a partial last one, the others less than a word"""
    fg, rows = _recorded(golden, name, nchains)
    for max_lag in LAGS:
        _check_window(fg, rows, 0, s, max_lag)


@pytest.mark.parametrize("first,nrows", [(1, 131), (37, 260), (170, 130), (296, 4)])
def test_windows_that_start_later(golden, first, nrows):
    fg, rows = _recorded(golden, "grid57x33", 3)
    for max_lag in (2, 63):
        _check_window(fg, rows, first, nrows, max_lag)


def test_one_chain_at_the_c_level(golden):
    fg, rows = _recorded(golden, "grid57x33", 1)
    assert rows.shape[1] == 1
    for max_lag in (1, 31, 63):
        mean, tau, rhat2, truncated = _check_window(fg, rows, 0, 131, max_lag)
    assert np.isfinite(tau).mean() > 0.9 and np.isfinite(rhat2).all()


def _grid_with_evidence():
    g = list(graphgen.ising_grid(57, 33, weight=0.3))
    g[1] = g[1].copy()
    ev = np.array([64, 1000, 1880])
    g[1]["isEvidence"][ev] = 1
    g[1]["initialValue"][ev] = [1, 0, 1]
    return tuple(g), ev


def test_columns_repeated_unsorted_and_an_evidence_variable():
    g, ev = _grid_with_evidence()
    n = len(g[1])
    ids = [n - 1, 5, 700, int(ev[1]), 5, 0, 123, n - 1, 64, 63, 65, 1279]
    fg = _record(g, 3, ids, 131, se=False)
    rows = _download(fg, 0, 131, len(ids))
    assert rows[:, :, 3].max() == 0 and rows[:, :, 0].min() == 1 and rows[:, :, 8].min() == 1      # evidence stays
    sel = [3, 0, 11, 3, 7, 1, 4, 8, 2]
    for max_lag in (2, 31, 63):
        mean, tau, rhat2, truncated = _check_window(fg, rows, 0, 131, max_lag, cols=sel)
        assert np.isnan(tau[[0, 3, 7, 8]]).all() and np.isnan(rhat2[[0, 3, 7, 8]]).all() and not truncated[[0, 3, 7, 8]].any()
        assert mean[3] == 0.0 and mean[0] == 1.0 and mean[8] == 1.0
        assert tau[1] == tau[4] and np.isfinite(tau[[1, 2, 5, 6]]).all()


def test_full_state_trace_equals_the_listed_trace_of_a_twin():
    """vids = NULL: the dense record kernel's rows, every internal id (padding ids computed and dropped)"""
    g = graphgen.ising_grid(57, 33, weight=0.3)
    n = 57 * 33
    dense = _record(g, 2, None, 131)
    listed = _record(g, 2, np.arange(n), 131)
    rows = _download(listed, 0, 131, n)
    assert np.array_equal(_download(dense, 0, 131, n), rows)
    sel = np.random.default_rng(2).permutation(n)[:200]
    for max_lag in (1, 63):
        want = _check_window(listed, rows, 0, 131, max_lag, cols=sel)
        _check_window(dense, rows, 0, 131, max_lag, cols=sel)
        for a, b in zip(_summary(dense, 0, 131, max_lag, n), want):
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _everything(fg, nrows, ncols):
    L, h = _lib.lib(), fg._engine()
    nchains = L.nsk_get_chains(h)
    vv = np.zeros((nchains, len(fg.variable)), np.int64)
    cc = np.zeros((nchains, len(fg.count)), np.int64)
    _lib.check(L.nsk_chains_download(h, _lib.ptr(vv), _lib.ptr(cc)))
    rows, cap, packed = C.c_int64(), C.c_int64(), C.c_int64()
    _lib.check(L.nsk_trace_rows(h, C.byref(rows), C.byref(cap), C.byref(packed)))
    info = fg.info()
    return (vv, cc, _download(fg, 0, nrows, ncols), np.array([rows.value, cap.value, packed.value, info["sweeps_done"], info["device_bytes"]]))


def test_the_calls_change_nothing(golden):
    """values, tallies, sweeps_done, the rows and device_bytes (the result buffers are the call's alone); the profiling
    bracket counts none of their launches; later sweeps go on as on a twin that never asked"""
    L = _lib.lib()
    g = _small_graphs(golden)["grid57x33"][0]
    n = len(g[1])
    fg = _record(g, 2, None, 140, capacity=149)
    twin = _record(g, 2, None, 140, capacity=149)
    before = _everything(fg, 131, n)
    ms, nl = C.c_double(), C.c_int64()
    _lib.check(L.nsk_profile_begin(fg._engine()))
    _summary(fg, 0, 131, 63, n)
    _counts(fg, 3, 131, 31, [5, 1880, 64])
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
    fg, rows = _recorded(golden, "grid57x33", 2)
    h, n = fg._engine(), rows.shape[2]
    out = np.zeros(n)
    cols = np.array([0], np.int64)
    cnt = np.zeros(66, np.int64)

    def ess(first, nrows, lag):
        return L.nsk_trace_ess(h, first, nrows, lag, _lib.ptr(out), None, None, None)

    def counts(first, nrows, lag, c=cols):
        return L.nsk_trace_autocov_counts(h, first, nrows, lag, _lib.ptr(c), len(c), _lib.ptr(cnt))

    assert ess(0, 131, 63) == _lib.OK and counts(0, 131, 63) == _lib.OK
    for call in (ess, counts):
        assert call(0, 3, 1) == _lib.E_INVALID                     # fewer than 4 rows
        assert call(0, ROWS + 1, 5) == _lib.E_INVALID              # rows beyond those recorded
        assert b"recorded" in L.nsk_last_error()
        assert call(ROWS - 4, 4, 1) == _lib.OK and call(ROWS - 4, 5, 1) == _lib.E_INVALID
        assert call(-1, 8, 1) == _lib.E_INVALID
        assert call(0, 131, 0) == _lib.E_INVALID and call(0, 131, 64) == _lib.E_INVALID
        assert b"max_lag" in L.nsk_last_error()
        # two chains, H = 4: 4 H n^3 reaches 2^63 at n = 2^(59/3); decided before the rows recorded are looked at
        assert call(0, 2 * 832256, 63) == _lib.E_RANGE
        assert b"2^63" in L.nsk_last_error()
        assert call(0, 2 * 832255, 63) == _lib.E_INVALID           # fits; the rows are not there
        assert b"recorded" in L.nsk_last_error()
    assert counts(0, 131, 5, np.array([n], np.int64)) == _lib.E_INDEX
    assert counts(0, 131, 5, np.array([3, -1], np.int64)) == _lib.E_INDEX
    assert L.nsk_trace_autocov_counts(h, 0, 131, 5, None, 0, None) == _lib.OK      # no columns: nothing to do
    # no trace; plain rows
    g = _small_graphs(golden)["grid57x33"][0]
    _, bare = session(g, seed=SEED)
    bare.inference(0, 1, True)
    assert L.nsk_trace_ess(bare._engine(), 0, 8, 3, _lib.ptr(out), None, None, None) == _lib.E_INVALID
    assert b"no trace" in L.nsk_last_error()
    gc = _small_graphs(golden)["gencat"][0]
    assert (gc[1]["cardinality"] > 2).any()
    plain = _record(gc, 2, None, 8)
    packed = C.c_int64(1)
    _lib.check(L.nsk_trace_rows(plain._engine(), None, None, C.byref(packed)))
    assert packed.value == 0
    assert L.nsk_trace_ess(plain._engine(), 0, 8, 3, None, None, None, None) == _lib.E_INVALID
    assert b"bit-packed" in L.nsk_last_error()
    assert L.nsk_trace_autocov_counts(plain._engine(), 0, 8, 3, _lib.ptr(cols), 1, _lib.ptr(cnt)) == _lib.E_INVALID


def test_mixing_is_the_estimator_of_the_downloaded_trace(golden):
    """FactorGraph.mixing against effective_sample_size(sample(...)) of a twin: 128 rows, n = 64, so max_lag = 63 is the
    whole window; state and tallies as the twin's"""
    g = _small_graphs(golden)["grid57x33"][0]
    n = len(g[1])
    for kw, ids in (({"thin": 1}, None), ({"thin": 2}, [n - 1, 5, 700, 5, 0, 64])):
        _, a = session(g, seed=SEED, chains=3)
        _, b = session(g, seed=SEED, chains=3)
        epochs = 128 * kw["thin"]
        m = a.mixing(epochs, var_ids=ids, burnin_epochs=3, sample_evidence=False, **kw)
        rows = b.sample(epochs, var_ids=ids, burnin_epochs=3, sample_evidence=False, var_copy="all", **kw)
        assert rows.shape[0] == 128 and m.samples == 128 * 3
        ref = effective_sample_size(rows)
        assert m.ess.shape == ref.shape and np.array_equal(np.isnan(m.ess), np.isnan(ref))
        ok = ~np.isnan(ref)
        assert ok.mean() > 0.9
        np.testing.assert_allclose(m.ess[ok], ref[ok], rtol=1e-9, atol=0)
        assert not m.truncated.any() and m.truncated.dtype == np.uint8
        np.testing.assert_allclose(m.mean, rows.mean(axis=(0, 1)), rtol=1e-14)
        np.testing.assert_allclose(m.ess[ok] * m.tau[ok], m.samples, rtol=1e-14)
        assert np.all(m.rhat[ok] > 0.9) and np.all(m.rhat[ok] < 2.0)
        assert np.array_equal(a.var_value, b.var_value) and np.array_equal(a.count, b.count)
        assert np.array_equal(a.chain_count, b.chain_count) and a.info()["sweeps_done"] == b.info()["sweeps_done"]
        rows_left, cap = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().nsk_trace_rows(a._engine(), C.byref(rows_left), C.byref(cap), None))
        assert (rows_left.value, cap.value) == (0, 0)          # torn down


def test_mixing_one_chain_few_rows_and_other_cardinalities(golden):
    g = _small_graphs(golden)["grid57x33"][0]
    n = len(g[1])
    _, one = session(g, seed=SEED)
    _, twin = session(g, seed=SEED)
    m = one.mixing(40, var_ids=[3, 4])
    twin.inference(0, 40, False, var_copy="all")
    assert np.array_equal(one.var_value, twin.var_value) and np.array_equal(one.count, twin.count)
    for a in (m.ess, m.tau, m.rhat, m.mean):
        assert a.shape == (2,) and np.isnan(a).all()
    assert not m.truncated.any()
    _, few = session(g, seed=SEED, chains=2)
    m = few.mixing(3)
    assert m.ess.shape == (n,) and np.isnan(m.ess).all() and np.isnan(m.mean).all()
    with pytest.raises(ValueError):
        few.mixing(8, max_lag=64)
    with pytest.raises(ValueError):
        few.mixing(8, thin=0)
    with pytest.raises(IndexError):
        few.mixing(8, var_ids=[n])
    gc = _small_graphs(golden)["gencat"][0]
    _, cat = session(gc, seed=SEED, chains=2)
    with pytest.raises(ValueError, match="binary"):
        cat.mixing(8)
    with pytest.raises(ValueError, match="binary"):
        cat.mixing(8, var_ids=[int(np.argmax(gc[1]["cardinality"] > 2))])


def test_liveliness(golden):
    """from the downloaded rows alone: the chains move, the autocorrelation of nearly every column ends inside 31 lags,
    and one lag is too short a window for some"""
    _, rows = _recorded(golden, "grid57x33", 3)
    x = rows[:131]
    n, H, A, S1, S2 = autocov_counts(x, 31)
    _, tau, _, truncated = ess_from_counts(n, H, A, S1, S2)
    assert np.isfinite(n * H / tau).mean() >= 0.9
    assert truncated.mean() < 0.05
    n, H, A, S1, S2 = autocov_counts(x, 1)
    assert ess_from_counts(n, H, A, S1, S2)[3].any()
