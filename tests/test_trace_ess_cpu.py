"""The numpy restatement of the device estimator (diagnostics.autocov_counts, diagnostics.ess_from_counts; what
nsk_trace_ess computes from a bit-packed trace) against the FFT estimator the library already has
(diagnostics.effective_sample_size), on seeded synthetic 0 / 1 traces.  No GPU."""

import numpy as np
import pytest

from numbskull_amd.diagnostics import (autocov_counts, counts_fit_int64, effective_sample_size, ess_from_counts)

RTOL = 1e-9
SHAPES = [(9, 2), (37, 3), (64, 4), (131, 2), (200, 3)]
_TRACES = {}


def sticky_trace(s, chains, ncols=48, seed=0):
    """0 / 1 Markov chains with per-column flip probabilities from 0.02 (slow) to 0.5 (white); column 5 is constant"""
    key = (s, chains, ncols, seed)
    if key not in _TRACES:
        rng = np.random.default_rng(1000 * s + 10 * chains + seed)
        p = np.linspace(0.02, 0.5, ncols)
        x = np.zeros((s, chains, ncols), np.int8)
        x[0] = rng.integers(0, 2, (chains, ncols))
        for t in range(1, s):
            x[t] = np.where(rng.random((chains, ncols)) < p, 1 - x[t - 1], x[t - 1])
        x[:, :, 5] = 1
        x.setflags(write=False)
        _TRACES[key] = x
    return _TRACES[key]


def _ess(x, max_lag):
    n, H, A, S1, S2 = autocov_counts(x, max_lag)
    mean, tau, rhat2, truncated = ess_from_counts(n, H, A, S1, S2)
    with np.errstate(invalid="ignore"):
        return n * H / tau, mean, rhat2, truncated


@pytest.mark.parametrize("s,chains", SHAPES)
def test_full_window_is_the_existing_estimator(s, chains):
    """max_lag = n - 1: the same NaN columns, finite values within rtol = 1e-9 of the FFT path (the largest relative
    difference over these ten traces, two seeds a shape, measured 2.3e-15), nothing truncated, the mean
    the plain mean of the rows used."""
    for seed in (0, 1):
        x = sticky_trace(s, chains, seed=seed)
        n = s // 2
        ess, mean, rhat2, truncated = _ess(x, n - 1)
        ref = effective_sample_size(x)
        assert np.array_equal(np.isnan(ess), np.isnan(ref))
        assert np.isnan(ess[5]) and np.isnan(rhat2[5]) and mean[5] == 1.0
        ok = ~np.isnan(ref)
        assert ok.sum() >= 40
        worst = np.max(np.abs(ess[ok] - ref[ok]) / np.abs(ref[ok]))
        print("s=%d chains=%d seed=%d: largest relative difference %.3g" % (s, chains, seed, worst))
        assert worst <= RTOL
        assert not truncated.any()
        halves = np.concatenate([x[:n], x[s - n:]], axis=1)
        np.testing.assert_allclose(mean, halves.mean(axis=(0, 1)), rtol=1e-14)
        assert np.all(rhat2[ok] > 0)


@pytest.mark.parametrize("max_lag", [1, 15, 31, 63])
@pytest.mark.parametrize("s,chains", SHAPES)
def test_cut_window(s, chains, max_lag):
    """columns whose positive sequence ends inside the window equal the full estimator; a truncated column's ESS is
    an upper bound (its tau sums fewer positive pairs)"""
    x = sticky_trace(s, chains)
    n = s // 2
    ess, _, _, truncated = _ess(x, max_lag)
    ref = effective_sample_size(x)
    done, cut = truncated == 0, truncated == 1
    if max_lag >= n - 1:
        assert not cut.any()
    assert np.array_equal(np.isnan(ess[done]), np.isnan(ref[done]))
    ok = done & ~np.isnan(ref)
    assert np.all(np.abs(ess[ok] - ref[ok]) <= RTOL * np.abs(ref[ok]))
    # (tau = -1 + 2 sum P can fail to be positive on either side -- a strongly anticorrelated column: NaN is no bound)
    both = cut & ~np.isnan(ref) & ~np.isnan(ess)
    assert np.all(ess[both] >= ref[both] * (1 - RTOL))
    if max_lag == 1 and n > 8:
        assert cut.any()                           # the slow columns do not decorrelate in two lags


def test_counts_against_a_direct_float_autocovariance():
    """A(k) / n^3 is the sum over half-chains of the biased autocovariance at lag k, S1 and S2 the sums of the
    half-chain totals and of their squares"""
    x = sticky_trace(37, 3, ncols=12, seed=4)
    s, m, ncol = x.shape
    n, H, A, S1, S2 = autocov_counts(x, 9)
    assert (n, H) == (18, 6) and A.shape == (10, ncol) and A.dtype == np.int64
    h = np.concatenate([x[:n], x[s - n:]], axis=1).astype(np.float64)
    d = h - h.mean(axis=0)
    for k in range(10):
        acov = (d[:n - k] * d[k:]).sum(axis=0) / n                  # (H, columns)
        np.testing.assert_allclose(A[k] / float(n) ** 3, acov.sum(axis=0), rtol=0, atol=1e-12)
    assert np.array_equal(S1, h.sum(axis=(0, 1)).astype(np.int64))
    assert np.array_equal(S2, (h.sum(axis=0) ** 2).sum(axis=0).astype(np.int64))
    # lags beyond n - 1 do not exist: the window is cut there
    assert autocov_counts(x, 63)[2].shape == (18, ncol)
    # one chain is allowed at this level
    assert autocov_counts(x[:, :1], 3)[1] == 2


def test_arguments():
    x = sticky_trace(9, 2)
    with pytest.raises(ValueError):
        autocov_counts(x[:3], 1)
    with pytest.raises(ValueError):
        autocov_counts(x, 0)
    with pytest.raises(ValueError):
        autocov_counts(x[0], 1)
    with pytest.raises(ValueError):
        autocov_counts(x * 2, 1)


def test_int64_range_bound():
    """4 H n^3 < 2^63: the largest term of A(k), n^2 c_h(k) <= n^3, summed over H half-chains with the two other
    terms of its size, stays inside int64"""
    assert counts_fit_int64(1 << 20, 2) is False                   # 4 * 2 * 2^60 = 2^63
    assert counts_fit_int64((1 << 20) - 1, 2) is True
    assert counts_fit_int64(104031, 2048) is True and counts_fit_int64(104032, 2048) is False
    assert counts_fit_int64(4, 2) is True
    # the all-ones column of the largest n that fits for two chains of a small trace: the terms cancel exactly
    x = np.ones((64, 2, 1), np.int8)
    n, H, A, S1, S2 = autocov_counts(x, 31)
    assert not A.any() and S1[0] == 128 and S2[0] == 4 * 32 * 32
