"""Host side of population annealing (FactorGraph.smc_sweeps / log_partition(resample=...), nsk_smc_sweeps): the numpy
restatement of the device's resampling rule against a hand-written loop and against the properties of systematic
resampling, the estimator against a hand-written sum, the estimate of the oracle's mirror (tests/smc.py: the mirror the GPU
tests hold the device to) against the exact log Z of graphs small enough to enumerate, the argument errors raised before a
device is touched and the export of the entry point (no GPU).

The statistical check is deterministic: the oracle's runs are functions of the seeds in tests/smc.py.  Measured (16 runs of
32 chains, one sweep a step, threshold 0.5; the figures are printed by the test and kept in DESIGN.md section 4):
grid 1.0, betas linspace(0, 1, 5): plain AIS ESS median 2.53, largest 5.80; mean of exp(log_z - exact) 0.8834, standard
error 0.1340; 1 - 3 events of 4 in every run.  Clamped grid 0.6, betas (0, 0.05, 0.9, 1): plain AIS ESS median 6.59,
largest 12.19; mean 0.9783, standard error 0.1086; the step of 0.05 never resamples, the step to 0.9 always does, and the
last step folds over the copied states: the estimate differs from plain AIS's by 0.0014 to 0.147 in log.  The ESS bound of
8 is asserted on the median over the runs: on the clamped grid no schedule puts every run under it (the single step (0, 1)
leaves one at 10.6).  In every run of both graphs a fold follows an event, which the test asserts: an event behind the
last fold alone would give plain AIS's number whatever the ancestors."""

import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from numbskull_amd import _lib
from numbskull_amd.diagnostics import smc_resample, smc_estimate, log_mean_exp, ais_estimate
from oracle import binding as orc
import smc
import temper
from util import REPO, session, oracle_of


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _resample_by_hand(lw, u, threshold, exp):
    """the header's rule, step 5, in plain Python floats"""
    R = len(lw)
    ident = list(range(R))
    if any(v != v for v in lw):
        return False, ident
    m = max(lw)
    if math.isinf(m):
        return False, ident
    w = [float(exp(np.array([v - m]))[0]) for v in lw]
    c, q = [w[0]], [w[0] * w[0]]
    for r in range(1, R):
        c.append(c[-1] + w[r])
        q.append(q[-1] + w[r] * w[r])
    S, Q = c[-1], q[-1]
    thrR = threshold * float(R)
    if not S * S < thrR * Q:
        return False, ident
    step = S / float(R)
    n = [0] * R
    for i in range(R):
        target = (float(i) + u) * step
        a = sum(1 for j in range(R) if c[j] <= target)
        n[min(a, R - 1)] += 1
    donors = [j for j in range(R) for _ in range(n[j] - 1)]
    dead = [j for j in range(R) if n[j] == 0]
    assert len(donors) == len(dead)
    anc = ident[:]
    for slot, j in zip(dead, donors):
        anc[slot] = j
    return True, anc


def _rows():
    rng = np.random.default_rng(11)
    rows = {}
    for R in (2, 3, 7, 64, 65, 200, 1024):
        rows["normal_%d" % R] = rng.normal(-40.0, 2.5, R)
        rows["wide_%d" % R] = rng.normal(300.0, 30.0, R)             # most weights underflow against the largest
    rows["two_levels"] = np.log(np.array([1.0, 1.0, 0.5, 0.5, 0.25, 0.25, 0.125, 0.125] * 4))
    rows["some_minus_inf"] = np.where(np.arange(40) % 3 == 0, -np.inf, rng.normal(0.0, 3.0, 40))
    return rows


# Where R w_j / S is an integer k up to the roundings of the running sums, the count may be k - 1 or k + 1 instead of k:
# the cases the rows above produce (row, u, threshold, chain, k, count).  Both are the last target, (R - 1 + u) * (S / R) with
# u one ulp under 1, rounding up to S itself: the count of c_j <= target is R, the clamp hands the offspring to chain
# R - 1, whose weight here is 0.  (A uniform of 53 random bits hits that u once in 2^53 draws.)
ONE_ULP_CASES = [("some_minus_inf", 1.0 - 2.0 ** -53, 0.3, 39, 0, 1), ("some_minus_inf", 1.0 - 2.0 ** -53, 1.0, 39, 0, 1)]


@pytest.mark.parametrize("exp", [np.exp, orc.exp_det], ids=["np.exp", "exp_det"])
def test_smc_resample_is_the_headers_rule(exp):
    edges = []
    for name, lw in sorted(_rows().items()):
        R = len(lw)
        for u in (0.0, 0.37, 1.0 - 2.0 ** -53):
            for thr in (0.3, 1.0):
                flag, anc, S, Q = smc_resample(lw, u, thr, exp=exp)
                hflag, hanc = _resample_by_hand([float(v) for v in lw], u, thr, exp)
                assert flag == hflag and anc.dtype == np.int32 and anc.tolist() == hanc, (name, u, thr)
                w = np.asarray(exp(lw - lw.max()), np.float64)
                assert flag == bool(S * S < thr * R * Q)
                assert abs(S - math.fsum(w)) <= R * 2.0 ** -52 * S and abs(Q - math.fsum(w * w)) <= R * 2.0 ** -52 * Q
                if not flag:
                    assert anc.tolist() == list(range(R))
                    continue
                n = np.bincount(anc, minlength=R)
                assert n.sum() == R                                                # the offspring counts sum to R
                assert all(anc[j] == j for j in range(R) if n[j] >= 1)             # survivors keep their slot
                assert all(n[anc[j]] >= 2 for j in range(R) if anc[j] != j)        # a donor has offspring to spare
                # dead slots ascending take donors ascending
                filled = anc[anc != np.arange(R)]
                assert np.array_equal(filled, np.sort(filled))
                # each count is floor or ceil of R w_j / S (exact rationals of the doubles)
                tot = sum(Fraction(float(v)) for v in w)
                for j in range(R):
                    x = Fraction(float(w[j])) * R / tot
                    if math.floor(x) <= n[j] <= math.ceil(x):
                        continue
                    k = round(x)
                    assert abs(x - k) <= R * 2.0 ** -50 and abs(int(n[j]) - k) == 1, (name, u, thr, j, float(x), n[j])
                    if exp is orc.exp_det:
                        edges.append((name, u, thr, j, k, int(n[j])))
    if exp is orc.exp_det:
        print("one-ulp cases:", edges)
        assert edges == ONE_ULP_CASES


def test_smc_resample_edge_rows():
    # equal weights never resample, whatever the threshold
    for R in (1, 2, 5, 64):
        flag, anc, S, Q = smc_resample(np.full(R, -3.25), 0.5, 1.0)
        assert not flag and anc.tolist() == list(range(R)) and S == R and Q == R
    # one weight that dominates by 700 in log: every slot holds that chain
    lw = np.zeros(9)
    lw[4] = 700.0
    flag, anc, S, Q = smc_resample(lw, 0.9, 0.5, exp=orc.exp_det)
    assert flag and anc.tolist() == [4] * 9
    # a row without a finite maximum, or with a NaN: no resampling
    for bad in (np.full(4, -np.inf), np.array([0.0, np.nan, 1.0]), np.array([0.0, np.inf]), np.array([np.nan])):
        flag, anc, S, Q = smc_resample(bad, 0.1, 1.0)
        assert not flag and anc.tolist() == list(range(len(bad))) and math.isnan(S) and math.isnan(Q)
    # a single -inf among finite log-weights is a dead chain, not a refusal
    flag, anc, S, Q = smc_resample(np.array([0.0, -np.inf, 0.0, -np.inf]), 0.25, 0.9)
    assert flag and anc.tolist() == [0, 0, 2, 2]
    # threshold 0 and R = 1 never resample
    spread = np.array([0.0, -50.0, -60.0, -70.0])
    assert smc_resample(spread, 0.3, 0.5)[0] and not smc_resample(spread, 0.3, 0.0)[0]
    for thr in (0.0, 0.5, 1.0):
        flag, anc, S, Q = smc_resample(np.array([123.0]), 0.3, thr)
        assert not flag and anc.tolist() == [0] and S == 1.0 and Q == 1.0
    for bad in ((spread, 1.0, 0.5), (spread, -0.1, 0.5), (spread, 0.5, 1.5), (spread, 0.5, float("nan")), (np.zeros((2, 2)), 0.5, 0.5),
                (np.zeros(0), 0.5, 0.5)):
        with pytest.raises(ValueError):
            smc_resample(*bad)


def test_smc_estimate_against_a_hand_written_sum():
    rng = np.random.default_rng(4)
    pre = rng.normal(650.0, 2.0, (5, 9))                               # exp overflows without the shift
    flag = np.array([0, 1, 0, 1, 0])
    lw = rng.normal(-3.0, 1.0, 9)

    def lme(row):
        m = max(row)
        return m + math.log(sum(math.exp(v - m) for v in row) / len(row))

    want = 2.5 + lme(pre[1]) + lme(pre[3]) + lme(lw)
    log_z, ess, events = smc_estimate(pre, flag, lw, 2.5)
    assert abs(log_z - want) <= 1e-12 * abs(want) and events == 2
    w = [math.exp(v - max(lw)) for v in lw]
    assert abs(ess - sum(w) ** 2 / sum(v * v for v in w)) <= 1e-12 * ess and 1.0 <= ess <= 9.0
    # no event: the estimate of plain AIS
    log_z, ess, events = smc_estimate(pre, np.zeros(5, bool), lw, 2.5)
    a = ais_estimate(lw, 2.5)
    assert abs(log_z - a[0]) <= 1e-12 * abs(a[0]) and abs(ess - a[2]) <= 1e-12 * ess and events == 0
    # one step: nothing in front of the final weights
    assert smc_estimate(np.zeros((0, 3)), [], [0.0, 0.0, 0.0], 1.0) == (1.0, 3.0, 0)
    assert len(smc_estimate(pre, flag, lw, 0.0)) == 3                  # no standard error is offered
    for bad in ((pre, flag[:4], lw, 0.0), (pre[:, :8], flag, lw, 0.0), (pre, flag, [], 0.0)):
        with pytest.raises(ValueError):
            smc_estimate(*bad)


def test_fold_resets_behind_an_event():
    rng = np.random.default_rng(6)
    betas = np.array([0.0, 0.2, 0.5, 0.6, 1.0])
    lp = rng.normal(-30.0, 7.0, (5, 3))
    pre, lw = smc.fold(betas, lp, [0, 1, 0, 0])
    want = np.zeros((4, 3))
    for r in range(3):
        acc = 0.0
        for t in range(4):
            acc = acc + (float(betas[t + 1]) - float(betas[t])) * float(lp[t, r])
            want[t, r] = acc
            if t == 1:
                acc = 0.0
    assert np.array_equal(_bits(pre), _bits(want)) and np.array_equal(_bits(lw), _bits(want[3]))
    from numbskull_amd.diagnostics import ais_log_weights
    pre0, lw0 = smc.fold(betas, lp, [0, 0, 0, 0])
    assert np.array_equal(_bits(lw0), _bits(ais_log_weights(betas, lp))) and np.array_equal(_bits(pre0[3]), _bits(lw0))


@pytest.mark.parametrize("name", sorted(smc.STAT_BETAS))
def test_the_mean_estimate_of_z_lands_within_three_standard_errors_of_the_enumeration(name):
    build, hbv, se, exact = temper.SMALL[name]
    _, fg = session(build(), seed=5, head_by_vid=hbv)
    og = oracle_of(fg, hbv, layout=False)
    color, _ = fg.plan()
    assert og.check_coloring(color) == (-1, -1)
    vv, _, w0, _ = og.initial_state()
    lz0 = temper.log_z0(og, color, se)
    betas, R = smc.STAT_BETAS[name], smc.STAT_R
    ratios, plain_ess = [], []
    for seed in smc.STAT_SEEDS:
        offsets = np.random.default_rng(seed + 1).random(len(betas) - 1)
        plain = temper.Schedule(og, color, seed, [vv] * R, w0, betas, 1, se)
        run = smc.Schedule(og, color, seed, [vv] * R, w0, betas, 1, se, smc.STAT_THRESHOLD, offsets)
        assert all(run.moved), run.moved
        log_z, ess, events = run.estimate(lz0)
        plain_z, _, pess, _ = plain.estimate(lz0)
        print("%s seed %d: plain AIS %.4f ESS %.2f | resampled %.4f final ESS %.2f events %s" %
              (name, seed, plain_z, pess, log_z, ess, "".join("R" if f else "." for f in run.resampled)))
        # every run has an event and a step without one
        assert 1 <= events < len(betas) - 1, run.resampled
        # ... and an event that a fold follows, so that the estimate rests on the copied states: it is not plain AIS's
        # (an event behind the last fold alone would leave AIS's number whatever the ancestors)
        assert any(run.resampled[:-1]), run.resampled
        assert log_z != plain_z
        # an event copies states, nothing else does, and the fold starts afresh behind it
        for t, flag in enumerate(run.resampled):
            assert flag == (not np.array_equal(run.ancestors[t], np.arange(R)))
        pre, lw = smc.fold(betas, run.lp, run.resampled)
        assert np.array_equal(_bits(pre), _bits(run.logw_pre)) and np.array_equal(_bits(lw), _bits(run.log_weights))
        ratios.append(math.exp(log_z - exact))
        plain_ess.append(pess)
    ratios = np.array(ratios)
    mean, stderr = float(ratios.mean()), float(ratios.std(ddof=1) / math.sqrt(len(ratios)))
    print("%s: exact %.6f; plain AIS ESS median %.2f largest %.2f of %d; mean of exp(log_z - exact) %.4f standard error %.4f: %.2f se from 1" %
          (name, exact, float(np.median(plain_ess)), max(plain_ess), R, mean, stderr, abs(mean - 1.0) / stderr))
    assert float(np.median(plain_ess)) < 8.0, plain_ess               # what makes the case worth having
    assert stderr > 0 and abs(mean - 1.0) <= 3.0 * stderr, (mean, stderr)


def test_argument_errors_come_before_the_device():
    _, fg = session(temper.clamped_grid())
    good = [0.0, 0.5, 1.0]
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            fg.smc_sweeps(good, threshold=bad)
    for bad in (0.0, -0.5, 1.01, float("nan")):
        with pytest.raises(ValueError):
            fg.log_partition(betas=good, resample=bad)
        with pytest.raises(ValueError):
            fg.log_evidence(betas=good, resample=bad)
    for bad in ([], [0.0, float("inf")], [-1.0], [[0.0, 1.0]]):
        with pytest.raises(ValueError):
            fg.smc_sweeps(bad)
    with pytest.raises(ValueError):
        fg.smc_sweeps(good, sweeps=0)
    for bad in ([0.1, 0.5, 1.0], [0.0, 0.5, 0.9], [0.0]):
        with pytest.raises(ValueError):
            fg.log_partition(betas=bad, resample=0.5)
    assert fg._handle is None


def test_header_declares_and_library_exports_the_entry_point():
    hdr = open(os.path.join(REPO, "include", "numbskull_amd.h")).read()
    assert re.search(r"\bint nsk_smc_sweeps\(nsk_graph \*g, const double \*betas[^,]*, int64_t nsteps, int64_t sweeps_per_step,\s*"
                     r"int sample_evidence, double threshold, const double \*offsets /\*[^*]*\*/,\s*"
                     r"double \*log_weight /\*[^*]*\*/,\s*double \*lp /\*[^*]*\*/,\s*double \*logw_pre /\*[^*]*\*/,\s*"
                     r"int32_t \*ancestors /\*[^*]*\*/,\s*int32_t \*resampled /\*[^*]*\*/\);", hdr)
    assert "nsk_smc_sweeps" in _lib.SYMBOLS
    assert hasattr(C.CDLL(_lib.LIB_PATH), "nsk_smc_sweeps")
    assert _lib.lib().nsk_smc_sweeps.argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_double] + [C.c_void_p] * 6
