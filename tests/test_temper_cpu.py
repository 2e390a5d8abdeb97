"""Host side of the tempered schedules (FactorGraph.tempered_sweeps / log_partition / log_evidence / anneal,
nsk_tempered_sweeps): the numpy estimators of numbskull_amd.diagnostics against hand-written loops, the annealed-
importance-sampling estimate against the exact log Z of graphs small enough to enumerate -- the oracle as the sampler
(tests/temper.py: the mirror the GPU tests hold the device to) --, the argument errors raised before a device is touched
and the export of the entry point (no GPU).

The statistical check is deterministic: the oracle's run is a function of the seed.  Measured (64 chains, betas =
linspace(0, 1, 21), one sweep a step, seed 5): grid 0.3 AIS 9.136088 against 9.119036, 0.50 standard errors, ESS 59.6,
thermodynamic integral 9.139954; grid 1.0 0.17 se, ESS 21.3 (integral 17.27 against 17.82: the trapezoid's bias, which is
why it gets no tolerance); clamped grid 0.17 se; mixed clamped 1.12 se; mixed free 0.87 se."""

import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from numbskull_amd import _lib
from numbskull_amd.diagnostics import ais_log_weights, log_mean_exp, ais_estimate, thermodynamic_integral
import temper
from util import REPO, session, oracle_of


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def test_ais_log_weights_is_the_plain_fold_bit_for_bit():
    rng = np.random.default_rng(1)
    betas = np.concatenate([[0.0], np.sort(rng.random(11)), [1.0, 1.7, 0.3]])      # up, past 1 and down again
    lp = rng.normal(-300.0, 77.0, (len(betas), 5))
    want = np.zeros(5)
    for r in range(5):
        acc = 0.0
        for t in range(len(betas) - 1):
            d = float(betas[t + 1]) - float(betas[t])
            term = d * float(lp[t, r])
            acc = acc + term
        want[r] = acc
    got = ais_log_weights(betas, lp)
    assert got.dtype == np.float64 and np.array_equal(_bits(got), _bits(want))
    # the fold is not the dot product: somewhere the roundings differ (else the comparison above shows nothing)
    assert not np.array_equal(_bits(got), _bits(np.diff(betas) @ lp[:-1]))
    # one step: nothing to fold; the last row never enters
    assert np.array_equal(ais_log_weights([0.5], [[3.0, 4.0]]), [0.0, 0.0])
    lp2 = lp.copy()
    lp2[-1] = np.nan
    assert np.array_equal(_bits(ais_log_weights(betas, lp2)), _bits(want))
    for bad in (([0.0, 1.0], np.zeros((3, 2))), ([0.0, 1.0], np.zeros(2)), (np.zeros((2, 1)), np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            ais_log_weights(*bad)


def test_log_mean_exp_is_shifted_by_the_maximum():
    x = np.array([1000.0, 1001.0, 999.0])
    with np.errstate(over="ignore"):
        assert np.isinf(np.log(np.mean(np.exp(x))))                     # overflows without the shift
    want = 1001.0 + math.log((math.exp(-1.0) + 1.0 + math.exp(-2.0)) / 3.0)
    assert abs(log_mean_exp(x) - want) <= 4 * 2.0 ** -53 * want
    y = np.array([-1000.0, -1001.0])                                    # underflows to log(0) without it
    assert abs(log_mean_exp(y) - (-1000.0 + math.log((1.0 + math.exp(-1.0)) / 2.0))) <= 1e-12
    assert log_mean_exp([2.5]) == 2.5 and log_mean_exp([-np.inf, -np.inf]) == -np.inf and math.isnan(log_mean_exp([]))
    z = np.random.default_rng(2).normal(0, 1, 100)
    assert abs(log_mean_exp(z) - math.log(sum(math.exp(v) for v in z) / 100.0)) <= 1e-13


def test_ais_estimate_against_a_hand_written_loop():
    lw = np.random.default_rng(3).normal(700.0, 1.5, 17)               # exp(700) x 17 overflows the unshifted mean's sum of squares
    lz, se, ess = ais_estimate(lw, 3.25)
    m = max(lw)
    w = [math.exp(v - m) for v in lw]
    mean = sum(w) / len(w)
    var = sum((v - mean) ** 2 for v in w) / (len(w) - 1)
    assert abs(lz - (3.25 + m + math.log(mean))) <= 1e-12 * abs(lz)
    assert abs(se - math.sqrt(var) / (mean * math.sqrt(len(w)))) <= 1e-12 * se
    assert abs(ess - sum(w) ** 2 / sum(v * v for v in w)) <= 1e-12 * ess and 1.0 <= ess <= 17.0
    # equal weights: the estimate is exact, no spread, every chain counts; one chain has no error bar
    lz, se, ess = ais_estimate([2.0] * 8, 1.0)
    assert lz == 3.0 and se == 0.0 and ess == 8.0
    lz, se, ess = ais_estimate([2.0], 1.0)
    assert lz == 3.0 and math.isnan(se) and ess == 1.0
    with pytest.raises(ValueError):
        ais_estimate([], 0.0)


def test_thermodynamic_integral_is_the_trapezoid_of_the_chain_mean():
    betas = np.array([0.0, 0.25, 0.5, 1.0])
    lp = np.array([[1.0, 3.0], [2.0, 6.0], [4.0, 4.0], [8.0, 0.0]])   # chain means 2, 4, 4, 4
    assert thermodynamic_integral(betas, lp, 10.0) == 10.0 + 0.25 * 3.0 + 0.25 * 4.0 + 0.5 * 4.0
    assert thermodynamic_integral([0.3], [[5.0]], 1.5) == 1.5


@pytest.mark.parametrize("name", sorted(temper.SMALL))
def test_the_estimate_lands_within_three_standard_errors_of_the_enumeration(name):
    build, hbv, se, exact = temper.SMALL[name]
    _, fg = session(build(), seed=5, head_by_vid=hbv)
    og = oracle_of(fg, hbv, layout=False)
    color, _ = fg.plan()
    assert og.check_coloring(color) == (-1, -1)
    vv, _, w0, _ = og.initial_state()
    enumerated = temper.exact_log_z(og, w0, vv, temper.sampled_mask(og, color, se))
    assert abs(enumerated - exact) <= 1e-6, (enumerated, exact)        # the figure the issue was written with
    betas = np.linspace(0, 1, 21)
    run = temper.Schedule(og, color, 5, [vv] * 64, w0, betas, 1, se)
    assert all(run.moved), run.moved                                    # the mirror cannot pass by standing still
    if not se:                                                          # clamped evidence stays where it is
        ev = og.variable["isEvidence"] != 0
        assert all(np.array_equal(x[ev], vv[ev]) for x in run.final)
    log_z, stderr, ess, ti = run.estimate(temper.log_z0(og, color, se))
    print("%s: exact %.6f AIS %.6f stderr %.4f error %.2f se ESS %.1f thermodynamic integral %.6f" %
          (name, enumerated, log_z, stderr, abs(log_z - enumerated) / stderr, ess, ti))
    assert stderr > 0 and 1.0 <= ess <= 64.0
    assert abs(log_z - enumerated) <= 3 * stderr, (log_z, enumerated, stderr)
    assert math.isfinite(ti)


def test_schedule_errors_come_before_the_device():
    _, fg = session(temper.clamped_grid())
    for bad in ([0.1, 0.5, 1.0], [0.0, 0.5, 0.9], [0.0], [1.0, 0.0], [0.0, float("nan"), 1.0], [0.0, -0.5, 1.0], [[0.0, 1.0]]):
        with pytest.raises(ValueError):
            fg.log_partition(betas=bad)
        with pytest.raises(ValueError):
            fg.log_evidence(betas=bad)
    with pytest.raises(ValueError):
        fg.log_partition(steps=0)
    for bad in ([], [0.0, float("inf")], [-1.0]):
        with pytest.raises(ValueError):
            fg.tempered_sweeps(bad)
        with pytest.raises(ValueError):
            fg.anneal(bad)
    with pytest.raises(ValueError):
        fg.tempered_sweeps([0.0, 1.0], sweeps=0)
    assert fg._handle is None


def test_header_declares_and_library_exports_the_entry_point():
    hdr = open(os.path.join(REPO, "include", "numbskull_amd.h")).read()
    assert re.search(r"\bint nsk_tempered_sweeps\(nsk_graph \*g, const double \*betas[^,]*, int64_t nsteps, int64_t sweeps_per_step,\s*"
                     r"int sample_evidence, double \*log_weight /\*[^*]*\*/,\s*double \*lp /\*[^*]*\*/,\s*"
                     r"int64_t \*best_values /\*[^*]*\*/,\s*double \*best_lp /\*[^*]*\*/\);", hdr)
    assert "nsk_tempered_sweeps" in _lib.SYMBOLS
    assert hasattr(C.CDLL(_lib.LIB_PATH), "nsk_tempered_sweeps")
    assert _lib.lib().nsk_tempered_sweeps.argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int] + [C.c_void_p] * 4
