"""The host side of the population-annealing tests (nsk_smc_sweeps, FactorGraph.smc_sweeps / log_partition(resample=...)):
the fold with its resets, the oracle's mirror of a resampled schedule and the runs of the statistical check, shared by
tests/test_smc_cpu.py (the estimator against the enumeration, the oracle as the sampler) and tests/test_smc_gpu.py (the
device against the mirror).  The graphs, the log-potential and the enumeration are those of tests/temper.py.

The mirror extends ``temper.Schedule``: the same chains (``seed ^ (r << 32)``), the same sweeps under ``betas[t] * w0``,
the same ``math.fsum`` log-potentials; behind the fold of every step but the last it asks
``numbskull_amd.diagnostics.smc_resample`` with the oracle's ``exp_det`` and copies the states by the ancestors.  A chain's
generator is keyed by its slot, so a copied state goes on under the slot's stream, as on the device."""

import numpy as np

import util  # noqa: F401  (puts the repository on sys.path)
from util import phases_from_colors
from oracle import binding as orc
from numbskull_amd.diagnostics import smc_resample, smc_estimate
import temper

M64 = temper.M64

# the statistical check of tests/test_smc_cpu.py: K independent runs of R chains a graph, every run its own chain seed and
# its own offsets; a schedule a graph, short enough that plain AIS rests on a few chains (the median of its ESS over the
# runs lies under 8 of 32).  The clamped grid is easy for plain AIS: from four even steps on its ESS is 14 and more, and
# even the single step (0, 1) leaves a run at 10.6, so no schedule puts every run under 8.  Its schedule is one small
# step, which never resamples, one large step, which always does, and a last step of 0.1: a fold FOLLOWS the event, over
# the copied states, so the estimate is not plain AIS's and depends on the ancestors (an event behind the last fold
# would leave log_z0 + log-mean-exp of the row in front of it, which is AIS whatever is copied).
STAT_K, STAT_R, STAT_THRESHOLD = 16, 32, 0.5
STAT_SEEDS = tuple(1000 + 17 * k for k in range(STAT_K))            # chain seeds; the offsets come from default_rng(seed + 1)
STAT_BETAS = {"grid_w1.0": np.linspace(0.0, 1.0, 5), "grid_w0.6_clamped": np.array([0.0, 0.05, 0.9, 1.0])}


def fold(betas, lp, resampled):
    """``(logw_pre, log_weights)`` as nsk_smc_sweeps folds them: ``ais_log_weights``' plain loop -- one rounded difference,
    product and addition -- with the row kept in front of every decision and a reset to 0.0 behind a resampling"""
    b, u = np.asarray(betas, np.float64), np.asarray(lp, np.float64)
    T, R = u.shape
    logw, pre = np.zeros(R), np.zeros((T - 1, R))
    for t in range(T - 1):
        d = b[t + 1] - b[t]
        term = d * u[t]
        logw = logw + term
        pre[t] = logw
        if resampled[t]:
            logw = np.zeros(R)
    return pre, logw


class Schedule(temper.Schedule):
    """The oracle's run of a resampled schedule.  Beside what ``temper.Schedule`` keeps (``states[t]`` are the states
    behind step t's copy): ``logw_pre`` (T - 1, R), ``resampled`` (T - 1,) bool, ``ancestors`` (T - 1, R), ``log_weights``
    (R,) the fold since the last resampling, ``SQ`` (T - 1, 2) the sums behind every decision.  ``ancestors`` given: the
    decisions of somebody else (the device's) are applied instead of the mirror's own, which are still taken and kept in
    ``own_resampled`` / ``own_ancestors``."""

    def __init__(self, og, color, seed, x0, w0, betas, sweeps_per_step, sample_evidence, threshold, offsets, sweep0=0,
                 resampled=None, ancestors=None):
        order, ps = phases_from_colors(color)
        betas = np.asarray(betas, np.float64)
        x = [np.ascontiguousarray(r, np.int64).copy() for r in x0]
        w0 = np.ascontiguousarray(w0, np.float64)
        R, T = len(x), len(betas)
        cnt = np.zeros(int(og.cstart[-1]), np.int64)
        self.states, self.moved = [], []
        self.lp, self.bound = np.zeros((T, R)), np.zeros((T, R))
        self.logw_pre, self.SQ = np.zeros((T - 1, R)), np.zeros((T - 1, 2))
        self.own_resampled, self.own_ancestors = np.zeros(T - 1, bool), np.zeros((T - 1, R), np.int32)
        logw = np.zeros(R)
        sweep = int(sweep0)
        for t in range(T):
            w = np.ascontiguousarray(betas[t] * w0)
            moved = False
            for r in range(R):
                last = x[r].copy()
                for s in range(sweeps_per_step):
                    assert og.gibbs_dev(order, ps, x[r], w, cnt, int(seed) ^ (r << 32), (sweep + s) & M64, bool(sample_evidence),
                                        burnin=True) == 0
                moved = moved or bool((last != x[r]).any())
                self.lp[t, r], self.bound[t, r] = temper.log_potential(og, x[r], w0)
            sweep += sweeps_per_step
            self.moved.append(moved)
            if t + 1 < T:
                d = betas[t + 1] - betas[t]
                term = d * self.lp[t]
                logw = logw + term
                self.logw_pre[t] = logw
                flag, anc, S, Q = smc_resample(logw, offsets[t], threshold, exp=orc.exp_det)
                self.own_resampled[t], self.own_ancestors[t], self.SQ[t] = flag, anc, (S, Q)
                if ancestors is not None:
                    flag, anc = bool(resampled[t]), np.asarray(ancestors[t])
                if flag:
                    logw = np.zeros(R)
                    x = [x[int(a)].copy() for a in anc]
            self.states.append([r.copy() for r in x])
        assert not cnt.any()                    # burn-in sweeps tally nothing
        self.betas, self.final, self.sweep = betas, x, sweep & M64
        self.log_weights = logw
        self.resampled = self.own_resampled if ancestors is None else np.asarray(resampled).astype(bool)
        self.ancestors = self.own_ancestors if ancestors is None else np.asarray(ancestors, np.int32)

    def estimate(self, lz0):
        """(log_z, ess, resamplings) of the run"""
        return smc_estimate(self.logw_pre, self.resampled, self.log_weights, lz0)
