"""Per-weight statistics, the parts that need no GPU: diagnostics.moment_gap on synthetic series, the C-ABI
declarations of numbskull_amd._lib, and the argument checks of FactorGraph.sample that precede any device work."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import effective_sample_size, moment_gap
from util import session

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "numbskull_amd.h")


def _ar1(phi, n, m, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, m))
    x[0] = rng.standard_normal(m) / np.sqrt(1.0 - phi * phi)       # stationary start
    eps = rng.standard_normal((n, m))
    for i in range(1, n):
        x[i] = phi * x[i - 1] + eps[i]
    return x


def test_moment_gap_of_an_ar1_series():
    """AR(1) with coefficient phi: autocorrelation time (1 + phi) / (1 - phi), marginal variance 1 / (1 - phi^2)"""
    phi, n, m, mu = 0.5, 4000, 4, 3.25
    stats = np.zeros((n, m, 3))
    stats[:, :, 0] = mu + _ar1(phi, n, m, 1)
    stats[:, :, 1] = 7.0                                            # never moves
    stats[:, :, 2] = -2.0 + _ar1(0.0, n, m, 2)                      # white noise
    target = np.array([mu, 6.5, -2.0])
    gap, mcse = moment_gap(stats, target)
    assert gap.shape == (3,) and mcse.shape == (3,)
    assert gap[1] == 0.5 and np.isnan(mcse[1])
    flat = stats.reshape(-1, 3)
    assert np.allclose(gap, flat.mean(axis=0) - target, rtol=0, atol=1e-12)
    # the definition: sd / sqrt(ESS)
    ess = effective_sample_size(stats)
    assert np.allclose(mcse[[0, 2]], flat.std(axis=0, ddof=1)[[0, 2]] / np.sqrt(ess[[0, 2]]), rtol=1e-12)
    # ... and the value theory gives, within the estimator's own noise (the ESS of 16000 draws is good to ~10 %)
    want0 = np.sqrt(1.0 / (1.0 - phi * phi) * (1.0 + phi) / (1.0 - phi) / (n * m))
    want2 = np.sqrt(1.0 / (n * m))
    assert abs(mcse[0] / want0 - 1.0) < 0.25 and abs(mcse[2] / want2 - 1.0) < 0.25, (mcse, want0, want2)
    assert abs(gap[0]) <= 5 * mcse[0] and abs(gap[2]) <= 5 * mcse[2]
    # a shifted target shows as a gap of many standard errors
    gap_off, _ = moment_gap(stats, target + np.array([0.5, 0.0, 0.0]))
    assert abs(gap_off[0]) > 5 * mcse[0]


def test_moment_gap_refuses_other_shapes():
    with pytest.raises(ValueError):
        moment_gap(np.zeros((10, 2)), np.zeros(2))
    with pytest.raises(ValueError):
        moment_gap(np.zeros((10, 2, 3)), np.zeros(2))
    with pytest.raises(ValueError):
        moment_gap(np.zeros((0, 2, 3)), np.zeros(3))
    # one chain: the effective sample size is undefined, the gap is not
    gap, mcse = moment_gap(np.arange(12.0).reshape(12, 1, 1), np.zeros(1))
    assert gap[0] == 5.5 and np.isnan(mcse[0])


def test_the_binding_declares_the_new_entry_points():
    names = ("nsk_weight_stats", "nsk_trace_weight_stats", "nsk_trace_download_weight_stats")
    text = open(HEADER).read()
    for name in names:
        assert name in _lib.SYMBOLS
        assert re.search(r"^int %s\(nsk_graph \*g," % name, text, re.M), name
    assert re.search(r"int nsk_weight_stats\(nsk_graph \*g, int which, int64_t first_chain, int64_t nchains, int scaled,\s*"
                     r"double \*out", text)
    assert re.search(r"int nsk_trace_weight_stats\(nsk_graph \*g, const int64_t \*wids, int64_t nwids, int scaled\);", text)
    assert re.search(r"int nsk_trace_download_weight_stats\(nsk_graph \*g, int64_t first_row, int64_t nrows,\s*double \*out", text)
    assert (_lib.BUF_VALUE, _lib.BUF_VALUE_EVID) == (0, 1) and _lib.E_INDEX == -3 and _lib.E_NOMEM == -6
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        assert L.nsk_weight_stats.argtypes == [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
        assert L.nsk_trace_weight_stats.argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
        assert L.nsk_trace_download_weight_stats.argtypes == [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]


def test_sample_checks_its_arguments_before_it_touches_the_device():
    _, fg = session(graphgen.ising_grid(4, 5, two_weights=True))
    with pytest.raises(ValueError):
        fg.sample(4, weight_statistics=[])                          # a list needs at least one id
    with pytest.raises(ValueError):
        fg.sample(4, weight_statistics=[[0, 1]])
    with pytest.raises(ValueError):
        fg.sample(4, weight_statistics=[0.5])
    with pytest.raises(IndexError):
        fg.sample(4, weight_statistics=[0, 2])
    with pytest.raises(IndexError):
        fg.sample(4, weight_statistics=[-1])
    with pytest.raises(ValueError):
        fg.sample(4, feature_scaled=True)                           # nothing to scale
    with pytest.raises(ValueError):
        fg.sample(4, thin=0, weight_statistics=True)
    with pytest.raises(ValueError):
        fg.weight_statistics(var_copy="all", evidence_chain=True)
    assert fg._handle is None                                       # none of this created the device handle
