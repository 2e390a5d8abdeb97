"""numbskull_amd.diagnostics (autocorrelation, effective sample size) on synthetic chains: no GPU."""

import numpy as np
import pytest

from numbskull_amd.diagnostics import autocorrelation, effective_sample_size

LENGTH, CHAINS = 100_000, 4

# phi: (relative margin of ESS, absolute margin of the lag-1 autocorrelation) = four standard deviations of the spread
# measured over the 30 seeds 100 .. 129 (see test_ar1_against_the_closed_form)
MARGINS = {0.0: (4 * 0.0070, 4 * 0.00182), 0.3: (4 * 0.0124, 4 * 0.00172),
           0.6: (4 * 0.0148, 4 * 0.00146), 0.9: (4 * 0.0305, 4 * 0.00083)}


def _ar1(phi, length, chains, seed):
    """stationary AR(1), unit innovations: (length, chains, 1)"""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((length, chains))
    x = np.empty((length, chains))
    x[0] = e[0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, length):
        x[t] = phi * x[t - 1] + e[t]
    return x[:, :, None]


@pytest.mark.parametrize("phi", sorted(MARGINS))
def test_ar1_against_the_closed_form(phi):
    """ESS of an AR(1) process with coefficient phi is N (1 - phi) / (1 + phi), its lag-1 autocorrelation phi.
    Spread of the estimators over the 30 seeds 100 .. 129, 4 chains of 100 000 samples (N = 400 000), measured on
    the CPU before these margins were written:

        phi   ESS / closed form: mean, sd     lag-1 autocorrelation - phi: mean, sd
        0.0   0.9953  0.0070                  0.00047  0.00182
        0.3   0.9937  0.0124                  0.00052  0.00172
        0.6   0.9953  0.0148                  0.00041  0.00146
        0.9   0.9941  0.0305                  0.00011  0.00083

    The test allows four of those standard deviations around the closed form: 2.8 %, 5.0 %, 5.9 % and 12.2 % of
    the ESS (the largest is below 15 %: at 50 000 samples per chain the spread at phi = 0.9 was 0.048, 19 %, hence
    the chain length), 0.0073 to 0.0033 of the autocorrelation.  The estimator's mean sits 0.5 % below the closed
    form (the initial positive sequence truncates a positive tail), well inside the margin.  Seeds 0 .. 4 here."""
    rel, absolute = MARGINS[phi]
    assert rel < 0.15
    for seed in range(5):
        x = _ar1(phi, LENGTH, CHAINS, seed)
        want = LENGTH * CHAINS * (1.0 - phi) / (1.0 + phi)
        ess = effective_sample_size(x)
        assert ess.shape == (1,)
        assert abs(ess[0] / want - 1.0) < rel, (phi, seed, ess[0], want)
        rho = autocorrelation(x, 3)
        assert rho.shape == (4, 1) and abs(rho[0, 0] - 1.0) < 1e-3
        assert abs(rho[1, 0] - phi) < absolute, (phi, seed, rho[1, 0])


def test_columns_are_independent_and_integer_traces_work():
    rng = np.random.default_rng(3)
    a = _ar1(0.6, 4000, 4, 1)
    b = (rng.random((4000, 4, 1)) < 0.3).astype(np.int8)
    both = np.concatenate([a, b.astype(np.float64)], axis=2)
    ess = effective_sample_size(both)
    # (a batched FFT may round differently from a single one: float64 round-off, nothing more)
    assert np.allclose(ess, np.concatenate([effective_sample_size(a), effective_sample_size(b)]), rtol=1e-9)
    assert 0.7 * 16000 < ess[1] < 1.3 * 16000           # independent draws: about one effective sample each


def test_constant_columns_short_traces_and_single_chains_give_nan():
    x = _ar1(0.5, 200, 4, 0)
    const = np.concatenate([x, np.full((200, 4, 1), 7.0)], axis=2)
    ess = effective_sample_size(const)
    assert np.isfinite(ess[0]) and ess[0] > 0 and np.isnan(ess[1])
    rho = autocorrelation(const, 5)
    assert rho.shape == (6, 2) and np.isfinite(rho[:, 0]).all() and np.isnan(rho[:, 1]).all()
    assert np.isnan(effective_sample_size(x[:, :1])).all()          # one chain
    assert np.isnan(autocorrelation(x[:, :1], 2)).all()
    assert np.isnan(effective_sample_size(x[:3])).all()             # fewer than 4 samples
    assert np.isnan(autocorrelation(x[:3], 2)).all()
    assert effective_sample_size(np.zeros((0, 4, 2))).shape == (2,)
    assert effective_sample_size(np.zeros((10, 4, 0))).shape == (0,)
    assert np.isnan(autocorrelation(x[:8], 20)[4:]).all()           # lags beyond the half-chains
    with pytest.raises(ValueError):
        effective_sample_size(np.zeros((10, 4)))
