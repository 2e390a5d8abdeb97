"""The trace statistics for categorical variables on the device (nsk_trace_value_autocov_counts, nsk_trace_value_ess,
nsk_trace_value_pair_counts, FactorGraph.mixing_values, FactorGraph.contingency).  The yardstick is the trace itself,
downloaded with nsk_trace_download: the device's integers must equal diagnostics.autocov_counts / pair_counts of
diagnostics.indicators of those rows (np.array_equal, no tolerance), the summaries diagnostics.ess_from_counts of those
integers and the tables diagnostics.contingency_tables of them, float for float.  One trace of 300 rows is recorded per
graph and chain count; the cases are windows of it."""

import ctypes as C

import numpy as np
import pytest

from numbskull_amd import _lib
from numbskull_amd.diagnostics import (autocov_counts, contingency_tables, ess_from_counts, factor_pairs, indicators,
                                       pair_counts)
from test_hip_parity import _small_graphs
from test_trace_ess_gpu import _download, _everything, _record
from util import session

pytestmark = pytest.mark.gpu

SEED = 93
ROWS = 300
LAGS = (1, 2, 31, 62, 63)
WINDOWS = [(0, 1), (0, 63), (0, 64), (0, 65), (0, 129), (0, 300), (1, 299), (37, 200), (296, 4)]
GRAPHS = ["hubs", "gencat", "gencat_i32", "lr_bigcard"]
_RECORDED = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_recorded():
    yield
    _RECORDED.clear()


def _ids(name, nvar):
    """the variables traced, as the caller lists them"""
    if name != "gencat":
        return np.arange(nvar)                                         # hubs: 903 columns, an odd count of int8
    rng = np.random.default_rng(5)
    ids = np.concatenate([rng.integers(0, nvar // 3, 1200), rng.integers(nvar // 3, nvar, 799)])     # unsorted, with repeats
    rng.shuffle(ids)
    assert len(ids) == 1999 and len(np.unique(ids)) < len(ids)
    return ids


def _recorded(golden, name, nchains):
    """(handle, its ROWS rows, the cardinality of every column)"""
    key = (name, nchains)
    if key not in _RECORDED:
        g = _small_graphs(golden)[name][0]
        ids = _ids(name, len(g[1]))
        fg = _record(g, nchains, ids, ROWS, seed=SEED)
        packed = C.c_int64(1)
        _lib.check(_lib.lib().nsk_trace_rows(fg._engine(), None, None, C.byref(packed)))
        assert packed.value == 0
        rows = _download(fg, 0, ROWS, len(ids))
        assert rows.dtype == (np.int32 if name in ("gencat_i32", "lr_bigcard") else np.int8)
        card = g[1]["cardinality"][ids].astype(np.int64)
        assert rows.min() >= 0 and (rows.max(axis=(0, 1)) < card).all()
        rows.setflags(write=False)
        _RECORDED[key] = (fg, rows, card)
    return _RECORDED[key]


def _c_sel(sel, width=2):
    return _lib.as_c(np.asarray(sel, np.int64).reshape(-1, width), np.int64)


def _counts(fg, first, nrows, max_lag, sel):
    """nsk_trace_value_autocov_counts as (A (L + 1, nsel), S1, S2)"""
    lag = min(max_lag, nrows // 2 - 1)
    sel = _c_sel(sel)
    out = np.full((len(sel), lag + 3), -7, np.int64)
    _lib.check(_lib.lib().nsk_trace_value_autocov_counts(fg._engine(), first, nrows, max_lag, _lib.ptr(sel), len(sel), _lib.ptr(out)))
    return out[:, :lag + 1].T.copy(), out[:, lag + 1].copy(), out[:, lag + 2].copy()


def _summary(fg, first, nrows, max_lag, sel):
    sel = _c_sel(sel)
    mean, tau, rhat2 = (np.full(len(sel), -7.0) for _ in range(3))
    truncated = np.full(len(sel), 7, np.uint8)
    _lib.check(_lib.lib().nsk_trace_value_ess(fg._engine(), first, nrows, max_lag, _lib.ptr(sel), len(sel), _lib.ptr(mean), _lib.ptr(tau),
                                              _lib.ptr(rhat2), _lib.ptr(truncated)))
    return mean, tau, rhat2, truncated


def _pairs(fg, first, nrows, quads):
    quads = _c_sel(quads, 4)
    nchains = _lib.lib().nsk_get_chains(fg._engine())
    out = np.full((len(quads), nchains, 3), -7, np.int64)
    _lib.check(_lib.lib().nsk_trace_value_pair_counts(fg._engine(), first, nrows, _lib.ptr(quads), len(quads), _lib.ptr(out)))
    return out


def _check_window(fg, rows, first, nrows, sel, lags=LAGS):
    """both entry points on rows [first, first + nrows) against numpy on the downloaded rows.  A(k) does not depend on
    the lag cut, so the reference integers are computed once, for 63 lags, and cut"""
    sel = np.asarray(sel).reshape(-1, 2)
    n, H, A, S1, S2 = autocov_counts(indicators(rows[first:first + nrows], sel), 63)
    want = None
    for max_lag in lags:
        L = min(max_lag, n - 1)
        dA, dS1, dS2 = _counts(fg, first, nrows, max_lag, sel)
        assert dA.shape == (L + 1, len(sel))
        assert np.array_equal(dA, A[:L + 1]) and np.array_equal(dS1, S1) and np.array_equal(dS2, S2), (first, nrows, max_lag)
        want = ess_from_counts(n, H, A[:L + 1], S1, S2)
        got = _summary(fg, first, nrows, max_lag, sel)
        for what, a, b in zip(("mean", "tau", "rhat2", "truncated"), got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (what, first, nrows, max_lag)
    return (n, H, A, S1, S2), want


def _all_values(card, cols):
    return np.array([(c, v) for c in cols for v in range(int(card[c]))], np.int64).reshape(-1, 2)


def _main_sel(card, total=700):
    """about `total` indicators, unsorted: the first and the last column with their first and last value, every value of
    the column of the largest cardinality and of two others, one indicator three times, then random ones"""
    ncols = len(card)
    rng = np.random.default_rng(ncols)
    last, big = ncols - 1, int(np.argmax(card))
    head = [(last, int(card[last]) - 1), (0, 0), (0, int(card[0]) - 1), (last, 0), (5, 1), (5, 1)]
    runs = np.concatenate([_all_values(card, [big]), _all_values(card, [ncols // 2, 7])[::-1]])
    cols = rng.integers(0, ncols, total - len(head) - len(runs) - 1)
    rand = np.stack([cols, (rng.random(len(cols)) * card[cols]).astype(np.int64)], axis=1)
    sel = np.concatenate([np.array(head, np.int64), runs, rand, [(5, 1)]])
    assert len(sel) == total >= 11 * 64 - 63 and (sel[:, 1] < card[sel[:, 0]]).all()
    return sel


@pytest.mark.parametrize("s", [9, 127, 128, 131, 257, 260])
@pytest.mark.parametrize("nchains", [2, 3])
@pytest.mark.parametrize("name", GRAPHS)
def test_counts_and_summary_equal_numpy_on_the_rows(golden, name, nchains, s):
    """n = 4, 63, 64, 65, 128, 130: one partial block, exactly one block, a carry across the block boundary, two blocks
    and a partial one; about 700 indicators are 11 waves of planes, the last one partial"""
    fg, rows, card = _recorded(golden, name, nchains)
    _check_window(fg, rows, 0, s, _main_sel(card))


@pytest.mark.parametrize("first,nrows", [(1, 131), (37, 260), (1, 4), (37, 4), (296, 4)])
@pytest.mark.parametrize("name", ["hubs", "gencat_i32"])
def test_windows_that_start_later(golden, name, first, nrows):
    fg, rows, card = _recorded(golden, name, 3)
    _check_window(fg, rows, first, nrows, _main_sel(card), lags=(2, 63))


@pytest.mark.parametrize("name", GRAPHS)
def test_indicator_lists_the_layout_can_get_wrong(golden, name):
    fg, rows, card = _recorded(golden, name, 2)
    ncols = len(card)
    sel = _main_sel(card)
    for count in (1, 63, 64, 65):
        _check_window(fg, rows, 3, 131, sel[:count], lags=(31,))
    # value 0 and value cardinality - 1 of every column: every device column, the first and the last among them
    ends = np.concatenate([np.stack([np.arange(ncols), np.zeros(ncols, np.int64)], axis=1), np.stack([np.arange(ncols), card - 1], axis=1)])
    _check_window(fg, rows, 0, 131, ends, lags=(5,))
    # every value of one variable: the series partition the rows, so the S1 add up to H n; a single device column,
    # listed backwards and with a repeat
    for col in (0, ncols - 1, int(np.argmax(card))):
        one = np.concatenate([_all_values(card, [col])[::-1], [(col, 0)]])
        (n, H, A, S1, S2), _ = _check_window(fg, rows, 0, 260, one, lags=(63,))
        assert S1[:-1].sum() == H * n and S1[-1] == S1[-2]
    # one indicator repeated: equal results
    (n, H, A, S1, S2), want = _check_window(fg, rows, 0, 131, [(5, 1), (9, 0), (5, 1), (5, 1)], lags=(31,))
    assert np.array_equal(A[:, 0], A[:, 2]) and np.array_equal(want[1][[0, 2]], want[1][[2, 3]], equal_nan=True)


def test_one_variable_in_two_caller_columns(golden):
    fg, rows, card = _recorded(golden, "gencat", 3)
    ids = _ids("gencat", 6000)
    vals, first_at, n_at = np.unique(ids, return_index=True, return_counts=True)
    twice = vals[n_at > 1][:5]
    sel = []
    for v in twice:
        a, b = np.nonzero(ids == v)[0][:2]
        assert np.array_equal(rows[:, :, a], rows[:, :, b])
        sel += [(a, 0), (b, 0), (b, int(card[b]) - 1), (a, int(card[a]) - 1)]
    (n, H, A, S1, S2), want = _check_window(fg, rows, 0, 260, sel, lags=(63,))
    assert np.array_equal(A[:, 0::4], A[:, 1::4]) and np.array_equal(A[:, 2::4], A[:, 3::4])
    q = [(sel[0][0], 0, sel[1][0], 0), (sel[0][0], 0, sel[1][0], 1)]
    got = _pairs(fg, 0, ROWS, q)
    assert np.array_equal(got[0, :, 0], got[0, :, 1]) and (got[1, :, 0] == 0).all()


def _quad_list(card, count=300):
    """the pairs the layout can get wrong, the full grid of one pair, then random ones"""
    ncols = len(card)
    last, big = ncols - 1, int(np.argmax(card))
    rng = np.random.default_rng(ncols + 1)
    special = [(0, 0, last, int(card[last]) - 1), (last, 0, 0, 0), (last, 0, last, 0), (3, 1, 3, 1), (3, 0, 3, 1), (3, 1, 3, 0),
               (big, 0, big, int(card[big]) - 1), (5, 1, 17, 0), (5, 1, 17, 0), (17, 0, 5, 1), (63, 0, 64, 0), (64, 1, 63, 1)]
    a, b = 7, ncols // 2
    grid = [(a, va, b, vb) for va in range(int(card[a])) for vb in range(int(card[b]))]
    cols = rng.integers(0, ncols, (count, 2))
    vals = (rng.random((count, 2)) * card[cols]).astype(np.int64)
    rand = np.stack([cols[:, 0], vals[:, 0], cols[:, 1], vals[:, 1]], axis=1)
    return np.concatenate([np.array(special, np.int64), np.array(grid, np.int64), rand]), len(special), len(grid)


def _numpy_pairs(rows, quads):
    quads = np.asarray(quads, np.int64).reshape(-1, 4)
    sel, inv = np.unique(quads.reshape(-1, 2), axis=0, return_inverse=True)
    return pair_counts(indicators(rows, sel), inv.reshape(-1, 2))


@pytest.mark.parametrize("nchains", [1, 3])
@pytest.mark.parametrize("name", GRAPHS)
def test_pair_counts_equal_numpy_on_the_rows(golden, name, nchains):
    fg, rows, card = _recorded(golden, name, nchains)
    quads, nspecial, ngrid = _quad_list(card)
    for first, nrows in WINDOWS:
        want = _numpy_pairs(rows[first:first + nrows], quads)
        got = _pairs(fg, first, nrows, quads)
        assert got.shape == want.shape and np.array_equal(got, want), (first, nrows, np.argwhere(got != want)[:5])
        assert np.array_equal(got[2, :, 0], got[2, :, 1]) and np.array_equal(got[3, :, 0], got[3, :, 2])      # a == b, one value: n11 = n1
        assert (got[4, :, 0] == 0).all() and (got[5, :, 0] == 0).all() and (got[6, :, 0] == 0).all()          # two values of one column
        assert (got[nspecial:nspecial + ngrid, :, 0].sum(axis=0) == nrows).all()                              # the full grid of a pair
    for some in (quads[:1], quads[-1:], quads[nspecial:nspecial + 3]):
        assert np.array_equal(_pairs(fg, 37, 200, some), _numpy_pairs(rows[37:237], some))


def test_twin_check_against_the_packed_kernels(golden):
    """the binary variables of hubs with one categorical one give plain rows; on a second handle with the same seed the
    binary variables alone give packed rows: the packed kernels' integers are those of the value-1 indicators"""
    L = _lib.lib()
    g = _small_graphs(golden)["hubs"][0]
    card = g[1]["cardinality"]
    binary = np.nonzero(card == 2)[0]
    assert len(binary) == 702 and card[1] == 5
    plain = _record(g, 3, np.concatenate([binary[:400], [1], binary[400:]]), 140, seed=SEED)
    twin = _record(g, 3, binary, 140, seed=SEED)
    packed, packed_twin = C.c_int64(), C.c_int64()
    _lib.check(L.nsk_trace_rows(plain._engine(), None, None, C.byref(packed)))
    _lib.check(L.nsk_trace_rows(twin._engine(), None, None, C.byref(packed_twin)))
    assert (packed.value, packed_twin.value) == (0, 1)
    plain_cols = np.concatenate([np.arange(400), np.arange(401, 703)])
    cols = _lib.as_c(np.arange(702), np.int64)
    for first, nrows, max_lag in ((0, 140, 63), (3, 131, 31), (136, 4, 1)):
        lag = min(max_lag, nrows // 2 - 1)
        want = np.full((702, lag + 3), -7, np.int64)
        _lib.check(L.nsk_trace_autocov_counts(twin._engine(), first, nrows, max_lag, _lib.ptr(cols), 702, _lib.ptr(want)))
        dA, dS1, dS2 = _counts(plain, first, nrows, max_lag, np.stack([plain_cols, np.ones(702, np.int64)], axis=1))
        assert np.array_equal(dA, want[:, :lag + 1].T) and np.array_equal(dS1, want[:, lag + 1]) and np.array_equal(dS2, want[:, lag + 2])
        assert (dS1 > 0).sum() > 351
    rng = np.random.default_rng(3)
    pairs = _lib.as_c(np.concatenate([rng.integers(0, 702, (200, 2)), [(0, 701), (701, 701), (399, 400)]]), np.int64)
    for first, nrows in ((0, 140), (5, 65), (139, 1)):
        want = np.full((len(pairs), 3, 3), -7, np.int64)
        _lib.check(L.nsk_trace_pair_counts(twin._engine(), first, nrows, _lib.ptr(pairs), len(pairs), _lib.ptr(want)))
        quads = np.stack([plain_cols[pairs[:, 0]], np.ones(len(pairs), np.int64), plain_cols[pairs[:, 1]], np.ones(len(pairs), np.int64)], axis=1)
        assert np.array_equal(_pairs(plain, first, nrows, quads), want)


def test_evidence_held_fixed(golden):
    """sample_evidence=False: an evidence variable's held value is a series of ones, every other value one of zeros"""
    g = _small_graphs(golden)["hubs"][0]
    var = g[1]
    fg = _record(g, 2, np.arange(len(var)), 131, se=False, seed=SEED)
    ev = np.nonzero(var["isEvidence"] != 0)[0]
    ev = ev[var["cardinality"][ev] > 2][:40]
    assert len(ev) == 40
    card = var["cardinality"].astype(np.int64)
    sel = _all_values(card, ev)
    held = sel[:, 1] == var["initialValue"][sel[:, 0]]
    assert held.sum() == 40
    for max_lag in (2, 63):
        A, S1, S2 = _counts(fg, 0, 131, max_lag, sel)
        n, H = 65, 4
        assert (S1[held] == H * n).all() and (S1[~held] == 0).all() and (A == 0).all()
        mean, tau, rhat2, truncated = _summary(fg, 0, 131, max_lag, sel)
        assert (mean[held] == 1.0).all() and (mean[~held] == 0.0).all()
        assert np.isnan(tau).all() and np.isnan(rhat2).all() and not truncated.any()


def test_liveliness(golden):
    """the indicators move: at least half of them are neither never nor always on (hubs; gencat's variables of
    cardinality at most 8 -- a value of a cardinality-30 variable may never appear in 300 rows)"""
    for name in ("hubs", "gencat"):
        fg, rows, card = _recorded(golden, name, 3)
        sel = _all_values(card, np.nonzero(card <= 8)[0][:300])
        A, S1, S2 = _counts(fg, 0, ROWS, 1, sel)
        H, n = 6, ROWS // 2
        assert ((S1 > 0) & (S1 < H * n)).mean() >= 0.5


def test_refusals(golden):
    """every rule in the order the header states, each decided on the host before a launch; a refused call writes nothing"""
    L = _lib.lib()
    fg, rows, card = _recorded(golden, "gencat", 2)
    h, ncols = fg._engine(), len(card)
    good = np.array([[0, 0]], np.int64)
    good4 = np.array([[0, 0, 1, 0]], np.int64)
    bad_col = np.array([[0, 0], [ncols, 0]], np.int64)
    bad_val = np.array([[0, 0], [1, int(card[1])]], np.int64)
    both = np.array([[1, int(card[1])], [-1, 0]], np.int64)            # the bad value is listed first: the column still decides
    cnt = np.full((4, 66), -7, np.int64)
    res = [np.full(4, -7.0) for _ in range(3)] + [np.full(4, 249, np.uint8)]
    pc = np.full((4, 2, 3), -7, np.int64)

    def counts(first, nrows, lag, s=good, nsel=None, handle=h, out=cnt):
        return L.nsk_trace_value_autocov_counts(handle, first, nrows, lag, _lib.ptr(s), len(s) if nsel is None else nsel, _lib.ptr(out))

    def ess(first, nrows, lag, s=good, nsel=None, handle=h, out=None):
        return L.nsk_trace_value_ess(handle, first, nrows, lag, _lib.ptr(s), len(s) if nsel is None else nsel, *[_lib.ptr(r) for r in res])

    def pairs(first, nrows, q=good4, npairs=None, handle=h, out=pc):
        return L.nsk_trace_value_pair_counts(handle, first, nrows, _lib.ptr(q), len(q) if npairs is None else npairs, _lib.ptr(out))

    def untouched():
        return (cnt == -7).all() and all((r == -7.0).all() for r in res[:3]) and (res[3] == 249).all() and (pc == -7).all()

    # no trace; bit-packed rows (the message points to the binary entry point)
    g = _small_graphs(golden)["grid4x5"][0]
    _, bare = session(g, seed=SEED)
    bare.inference(0, 1, True)
    packed = _record(g, 2, None, 8, seed=SEED)
    for call, binary in ((counts, b"nsk_trace_autocov_counts"), (ess, b"nsk_trace_ess")):
        assert call(0, 8, 3, handle=None) == _lib.E_INVALID            # null graph
        assert call(0, 8, 3, handle=bare._engine()) == _lib.E_INVALID
        assert b"no trace" in L.nsk_last_error()
        assert call(0, 3, 64, handle=packed._engine()) == _lib.E_INVALID           # (before the row count and the lag)
        assert b"bit-packed" in L.nsk_last_error() and binary in L.nsk_last_error()
    assert pairs(0, 8, handle=None) == _lib.E_INVALID
    assert pairs(0, 8, handle=bare._engine()) == _lib.E_INVALID
    assert b"no trace" in L.nsk_last_error()
    assert pairs(0, 0, handle=packed._engine()) == _lib.E_INVALID
    assert b"bit-packed" in L.nsk_last_error() and b"nsk_trace_pair_counts" in L.nsk_last_error()
    for call in (counts, ess):
        # rule 1, each ahead of what follows it
        assert call(0, 3, 64) == _lib.E_INVALID and b"4 rows" in L.nsk_last_error()
        assert call(-1, 8, 64) == _lib.E_INVALID and b"max_lag" in L.nsk_last_error()
        assert call(0, 8, 0) == _lib.E_INVALID and b"max_lag" in L.nsk_last_error()
        assert call(-1, 8, 1, nsel=-1) == _lib.E_INVALID and b"recorded" in L.nsk_last_error()
        assert call(0, 2 * 832256, 63, nsel=-1) == _lib.E_INVALID and b"null" in L.nsk_last_error()
        assert call(0, 2 * 832256, 63, s=None, nsel=1) == _lib.E_INVALID and b"null" in L.nsk_last_error()
        # rule 2: two chains, H = 4: 4 H n^3 reaches 2^63 at n = 2^(59/3); ahead of a bad column
        assert call(0, 2 * 832256, 63, s=bad_col) == _lib.E_RANGE and b"2^63" in L.nsk_last_error()
        assert call(0, 2 * 832255, 63) == _lib.E_INVALID and b"recorded" in L.nsk_last_error()      # fits; the rows are not there
        # rules 3, 4, 5
        assert call(0, ROWS + 1, 5, s=both) == _lib.E_INDEX and b"column index" in L.nsk_last_error()
        assert call(0, ROWS + 1, 5, s=bad_col) == _lib.E_INDEX
        assert call(0, ROWS + 1, 5, s=bad_val) == _lib.E_RANGE and b"cardinality" in L.nsk_last_error()
        assert call(0, 8, 5, s=np.array([[2, -1]], np.int64)) == _lib.E_RANGE
        assert call(0, ROWS + 1, 5) == _lib.E_INVALID and b"recorded" in L.nsk_last_error()
        assert call(ROWS - 4, 5, 1) == _lib.E_INVALID and call(ROWS, 4, 1) == _lib.E_INVALID
        assert call(0, 8, 5, nsel=0) == _lib.OK and call(0, 8, 5, s=None, nsel=0) == _lib.OK        # nothing to do
    assert L.nsk_trace_value_autocov_counts(h, 0, 8, 5, _lib.ptr(good), 1, None) == _lib.E_INVALID  # counts need their output
    assert pairs(0, 0) == _lib.E_INVALID and b"1 row" in L.nsk_last_error()
    assert pairs(-1, 8, npairs=-1) == _lib.E_INVALID and b"recorded" in L.nsk_last_error()
    assert pairs(0, ROWS + 1, npairs=-1) == _lib.E_INVALID and b"null" in L.nsk_last_error()
    assert pairs(0, 8, q=None, npairs=1) == _lib.E_INVALID and pairs(0, 8, out=None) == _lib.E_INVALID
    assert pairs(0, ROWS + 1, q=np.array([[1, int(card[1]), 0, 0], [0, 0, ncols, 0]], np.int64)) == _lib.E_INDEX
    assert pairs(0, ROWS + 1, q=np.array([[0, 0, 1, int(card[1])]], np.int64)) == _lib.E_RANGE
    assert pairs(0, ROWS + 1) == _lib.E_INVALID and b"recorded" in L.nsk_last_error()
    assert pairs(ROWS, 1) == _lib.E_INVALID and pairs(0, 8, npairs=0) == _lib.OK
    assert untouched()
    # ... and the calls that are in order write
    assert counts(ROWS - 4, 4, 1) == _lib.OK and ess(ROWS - 4, 4, 63) == _lib.OK and pairs(ROWS - 1, 1) == _lib.OK
    assert (cnt.reshape(-1)[:4] != -7).all() and res[0][0] != -7.0 and (pc[0] != -7).all()
    assert (cnt.reshape(-1)[4:] == -7).all() and (res[0][1:] == -7.0).all() and (pc[1:] == -7).all()
    assert L.nsk_trace_value_ess(h, 0, 8, 3, _lib.ptr(good), 1, None, None, None, None) == _lib.OK


def test_the_calls_change_nothing(golden):
    """values, tallies, sweeps_done, the rows and device_bytes (the buffers are the calls' alone); the profiling bracket
    counts none of their launches; later sweeps go on as on a twin that never asked"""
    L = _lib.lib()
    g = _small_graphs(golden)["hubs"][0]
    n = len(g[1])
    card = g[1]["cardinality"].astype(np.int64)
    fg = _record(g, 2, None, 140, capacity=149, seed=SEED)
    twin = _record(g, 2, None, 140, capacity=149, seed=SEED)
    before = _everything(fg, 131, n)
    ms, nl = C.c_double(), C.c_int64()
    _lib.check(L.nsk_profile_begin(fg._engine()))
    sel = _main_sel(card)
    rows = _download(fg, 0, 140, n)
    _check_window(fg, rows, 3, 131, sel, lags=(63,))                   # (a full-state trace: the columns are not the device's)
    quads, _, _ = _quad_list(card)
    assert np.array_equal(_pairs(fg, 0, 140, quads), _numpy_pairs(rows, quads))
    _lib.check(L.nsk_profile_end(fg._engine(), C.byref(ms), C.byref(nl)))
    assert nl.value == 0
    for a, b in zip(before, _everything(fg, 131, n)):
        assert np.array_equal(a, b)
    fg.inference(0, 9, True, var_copy="all")
    twin.inference(0, 9, True, var_copy="all")
    for a, b in zip(_everything(fg, 140, n), _everything(twin, 140, n)):
        assert np.array_equal(a, b)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _left_as_inference_leaves_it(a, b):
    assert np.array_equal(a.var_value, b.var_value) and np.array_equal(a.count, b.count)
    assert np.array_equal(a.chain_count, b.chain_count) and a.info()["sweeps_done"] == b.info()["sweeps_done"]
    assert np.array_equal(a.marginals, b.marginals) and np.array_equal(a.rhat, b.rhat, equal_nan=True)
    rows_left, cap = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().nsk_trace_rows(a._engine(), C.byref(rows_left), C.byref(cap), None))
    assert (rows_left.value, cap.value) == (0, 0)                      # torn down


def test_mixing_values_is_the_estimator_of_the_downloaded_trace(golden):
    g = _small_graphs(golden)["hubs"][0]
    card = g[1]["cardinality"].astype(np.int64)
    nvar = len(card)
    for thin, ids, ind in ((1, None, None), (2, [nvar - 1, 1, 5, 700, 5, 0], None), (1, None, [(1, 4), (nvar - 1, 0), (1, 4), (5, 1), (1, 0)])):
        _, a = session(g, seed=SEED, chains=3)
        _, b = session(g, seed=SEED, chains=3)
        epochs = 131 * thin + (thin - 1)
        m = a.mixing_values(epochs, var_ids=ids, indicators=ind, thin=thin, burnin_epochs=3, max_lag=31)
        if ind is None:
            listed = np.arange(nvar) if ids is None else np.asarray(ids)
            assert np.array_equal(m.offset, np.concatenate([[0], np.cumsum(card[listed])]))
            want_var = np.repeat(listed, card[listed])
            want_value = np.concatenate([np.arange(k) for k in card[listed]])
        else:
            assert m.offset is None
            want_var, want_value = np.asarray(ind)[:, 0], np.asarray(ind)[:, 1]
        assert np.array_equal(m.var, want_var) and np.array_equal(m.value, want_value)
        vids, cols = np.unique(want_var, return_inverse=True)
        rows = b.sample(epochs, var_ids=vids, thin=thin, burnin_epochs=3, sample_evidence=False, var_copy="all")
        assert rows.shape == (131, 3, len(vids)) and m.samples == 2 * 65 * 3
        n, H, A, S1, S2 = autocov_counts(indicators(rows, np.stack([cols.reshape(-1), want_value], axis=1)), 31)
        mean, tau, rhat2, truncated = ess_from_counts(n, H, A, S1, S2)
        with np.errstate(invalid="ignore"):
            for got, want in ((m.mean, mean), (m.tau, tau), (m.rhat, np.sqrt(rhat2)), (m.truncated, truncated), (m.ess, m.samples / tau)):
                assert _same(got, want)
        assert np.isfinite(m.ess).any()
        _left_as_inference_leaves_it(a, b)


def test_contingency_is_the_table_of_the_downloaded_trace(golden):
    g = _small_graphs(golden)["hubs"][0]
    card = g[1]["cardinality"].astype(np.int64)
    nvar = len(card)
    explicit = np.array([(1, nvar - 1), (nvar - 1, 1), (1, 1), (0, 1), (5, 700), (2, nvar - 2)])
    for thin, pairs in ((1, explicit), (2, "factors")):
        _, a = session(g, seed=SEED, chains=3)
        _, b = session(g, seed=SEED, chains=3)
        epochs = 70 * thin + (thin - 1)
        t = a.contingency(epochs, pairs, thin=thin, burnin_epochs=3)
        plist = factor_pairs(a.factor, a.fmap) if isinstance(pairs, str) else pairs
        vids, cols = np.unique(plist, return_inverse=True)
        cols = cols.reshape(-1, 2)
        rows = b.sample(epochs, var_ids=vids, thin=thin, burnin_epochs=3, sample_evidence=False, var_copy="all")
        assert rows.shape == (70, 3, len(vids))
        quads = np.array([(ca, va, cb, vb) for ca, cb in cols for va in range(card[vids[ca]]) for vb in range(card[vids[cb]])])
        want = contingency_tables(_numpy_pairs(rows, quads)[:, :, 0], card[plist], 70)
        assert t.samples == want.samples == 210 and len(t.joint) == len(plist) == len(t.counts)
        assert _same(t.mi, want.mi)
        for j in range(len(plist)):
            assert _same(t.joint[j], want.joint[j]) and _same(t.counts[j], want.counts[j])
            assert t.joint[j].shape == (card[plist[j][0]], card[plist[j][1]])
        if isinstance(pairs, str):
            assert len(plist) == 900 and (t.mi >= 0).all()
        else:
            assert np.array_equal(t.joint[0], t.joint[1].T) and np.array_equal(t.joint[2], np.diag(np.diag(t.joint[2])))
        _left_as_inference_leaves_it(a, b)


def test_what_the_methods_refuse(golden):
    g = _small_graphs(golden)["hubs"][0]
    nvar = len(g[1])
    _, fg = session(g, seed=SEED, chains=2)
    with pytest.raises(ValueError, match="binary"):
        fg.mixing_values(8, var_ids=[0, 3, 4])
    with pytest.raises(ValueError, match="binary"):
        fg.mixing_values(8, indicators=[(0, 1)])
    with pytest.raises(ValueError, match="binary"):
        fg.contingency(8, [(0, 3)])
    with pytest.raises(ValueError):
        fg.mixing_values(8, thin=0)
    with pytest.raises(ValueError):
        fg.mixing_values(8, max_lag=64)
    with pytest.raises(ValueError):
        fg.mixing_values(8, indicators=[1, 2, 3])
    with pytest.raises(ValueError, match="domain"):
        fg.mixing_values(8, indicators=[(1, 5)])
    with pytest.raises(ValueError, match="domain"):
        fg.mixing_values(8, indicators=[(1, -1)])
    with pytest.raises(IndexError):
        fg.mixing_values(8, var_ids=[nvar])
    with pytest.raises(IndexError):
        fg.mixing_values(8, indicators=[(-1, 0)])
    with pytest.raises(ValueError):
        fg.contingency(8, [(0, 1)], thin=0)
    with pytest.raises(ValueError):
        fg.contingency(8, "edges")
    with pytest.raises(ValueError):
        fg.contingency(8, [0, 1, 2])
    with pytest.raises(IndexError):
        fg.contingency(8, [(1, nvar)])
    rows_left, cap = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().nsk_trace_rows(fg._engine(), C.byref(rows_left), C.byref(cap), None))
    assert (rows_left.value, cap.value) == (0, 0)
    # one chain, few rows: NaN, and the sweeps still run
    _, one = session(g, seed=SEED)
    _, ref = session(g, seed=SEED)
    m = one.mixing_values(40, var_ids=[1])
    assert m.ess.shape == (5,) and np.isnan(m.ess).all() and np.isnan(m.mean).all() and not m.truncated.any()
    t = one.contingency(3, [(1, 2)], thin=4)
    assert t.samples == 0 and t.joint[0].shape == (5, 2) and np.isnan(t.joint[0]).all() and np.isnan(t.mi).all()
    ref.inference(0, 40, False, var_copy="all")
    ref.inference(0, 3, False, var_copy="all")
    assert np.array_equal(one.var_value, ref.var_value) and np.array_equal(one.count, ref.count)
