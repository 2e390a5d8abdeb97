"""Host side of the log-potential feature: diagnostics.best_sample, and the ESS of an lp array through the existing
estimator (no GPU)."""

import numpy as np
import pytest

from numbskull_amd.diagnostics import best_sample, effective_sample_size


def test_best_sample_finds_the_largest_log_potential():
    lp = np.array([[-3.0, -1.5, -2.0],
                   [-0.5, -4.0, -0.25],
                   [-7.0, -0.75, -9.0]])
    assert best_sample(lp) == (1, 2)
    assert best_sample(-lp) == (2, 2)
    assert all(isinstance(k, int) for k in best_sample(lp))


def test_best_sample_ties_go_to_the_first_in_row_major_order():
    lp = np.full((4, 3), -2.0)
    assert best_sample(lp) == (0, 0)
    lp[2, 1] = lp[1, 2] = lp[3, 0] = 5.0
    assert best_sample(lp) == (1, 2)
    lp[1, 0] = 5.0
    assert best_sample(lp) == (1, 0)


def test_best_sample_of_a_single_row_and_a_single_entry():
    assert best_sample(np.array([[-1.0, -0.5, -0.5, -3.0]])) == (0, 1)
    assert best_sample(np.array([[-1.0], [2.0], [2.0]])) == (1, 0)
    assert best_sample([[4.25]]) == (0, 0)


def test_best_sample_refuses_what_is_not_a_samples_by_chains_array():
    for bad in (np.zeros(5), np.zeros((2, 3, 1)), np.zeros((0, 3)), np.zeros((3, 0))):
        with pytest.raises(ValueError):
            best_sample(bad)


def test_ess_of_an_lp_array_has_the_documented_shape():
    """effective_sample_size(lp[:, :, None]) is the ESS of the joint: one column, so one number; an AR(1) series of
    coefficient 0.5 has autocorrelation time (1 + 0.5) / (1 - 0.5) = 3"""
    rng = np.random.default_rng(3)
    n, m = 4000, 4
    lp = np.zeros((n, m))
    x = rng.standard_normal(m)
    for i in range(n):
        x = 0.5 * x + np.sqrt(0.75) * rng.standard_normal(m)
        lp[i] = -100.0 + x
    ess = effective_sample_size(lp[:, :, None])
    assert ess.shape == (1,) and ess.dtype == np.float64
    assert 0.8 * n * m / 3 < ess[0] < 1.25 * n * m / 3
    assert np.isnan(effective_sample_size(lp[:, :1, None])).all()       # one chain: undefined, as documented
    with pytest.raises(ValueError):
        effective_sample_size(lp)                                      # (samples, chains) needs the column axis
