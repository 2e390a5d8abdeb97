"""The host side of the latent-variable PCD tests (nsk_pcd_latent_steps, FactorGraph.learn_pcd(clamped=K)): the graphs and
the oracle's mirror of a run, shared by tests/test_pcd_latent_cpu.py (the rule against a hand-written loop, the liveliness
of every GPU case, the exact likelihood of a learned model with the oracle as the sampler) and
tests/test_pcd_latent_gpu.py (the device against the mirror, bit for bit) so that the two cannot drift apart.

The mirror extends tests/pcd.py Run.  The handle's R chains are two populations: rows [0, K) clamped, rows [K, R) free.
Step t, from the sweep index s: every clamped row r sweeps ``k`` times at the indices s .. s + k - 1 with
sample_evidence = False, then every free row r at s + k .. s + 2 k - 1 with the free phase's flag; in the phase whose
population starts at row r0, row r is an oracle run in device mode seeded ``seed ^ ((r - r0) << 32)``.  Then Mc and Mf are
``moment_counts`` of the two populations and the update is ``numbskull_amd.diagnostics.pcd_latent_step``.  With ``clamp``
the initial values of the evidence variables (isEvidence 1, 2 or 3) are first written into the clamped rows."""

import numpy as np

import util  # noqa: F401  (puts the repository on sys.path)
from util import phases_from_colors
from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import pcd_latent_step
import pcd
import temper
import wide_trips

M64 = temper.M64

# the parity cases: graphs of tests/pcd.py (mixed_clamped needs head_by_vid and keeps weight 0 fixed) and the populations
PARITY_GRAPHS = ("grid_w0.6_clamped", "mixed_clamped", "grid_int32")
PARITY_CHAINS = ((2, 1), (3, 1), (3, 2), (5, 2), (64, 32), (65, 1), (65, 64))
STEPS, DECAY, SEED = 4, 0.9, 9
# Which launches a population of several chains takes.  The 3 x 4 grid lives in table segments (every variable routes to
# a table): one class launch serves all chains of a population.  The mixed graph (general tiles) and the int32 grid (its
# 200-valued variable and that one's neighbours leave the tables) sweep chain after chain.  The host-side plan says so in
# tests/test_pcd_latent_cpu.py, the launch counts in tests/test_pcd_latent_gpu.py.
BATCHED = {"grid_w0.6_clamped": True, "mixed_clamped": False, "grid_int32": False}
DISTURB = (2, 2)            # two nsk_gibbs_sweeps(h, 2, 1, 1) calls in front of a case: the clamp has something to restore


def parity_calls(name, RK):
    return pcd.CALLS[(PARITY_GRAPHS.index(name) + PARITY_CHAINS.index(RK)) % 2]


# The update kernel across a block edge: NSK_BLOCK + 1 = 257 weights, one lane each, so slot 256 is the second block's only
# lane.  Fixed weights keep their ids as slots: 255, the first block's last lane, is fixed, with two more inside the block.
EDGE_WEIGHTS, EDGE_FIXED, EDGE_RK, EDGE_STEPS = 257, (3, 100, 255), (3, 2), 2


def edge_graph():
    """graphgen.mixed_lr_graph(3000, seed=5) over EDGE_WEIGHTS weights (head_by_vid), all free but EDGE_FIXED"""
    return pcd.learnable(graphgen.mixed_lr_graph(3000, seed=5, nweights=EDGE_WEIGHTS), fixed=EDGE_FIXED)


def evidence_mask(og):
    ev = og.variable["isEvidence"]
    return (ev >= 1) & (ev <= 3)


def likelihood_graph():
    """temper.clamped_grid() with its weight free and three more evidence variables: 6 of 12 observed"""
    g = list(pcd.learnable(temper.clamped_grid()))
    var = g[1].copy()
    var["isEvidence"][[2, 6, 9]] = 1
    var["initialValue"][[2, 6, 9]] = [1, 1, 0]
    g[1] = var
    return tuple(g)


def launch_graph():
    """wide_trips.learning_grid(True) -- 28 x 1000, the lower half of the rows evidence -- with its two weights free"""
    return pcd.learnable(wide_trips.learning_grid(True))


def handle_graph():
    """grid16x1000 with rows 4 and 11 evidence at seeded values and a free weight"""
    g = list(pcd.learnable(wide_trips.graph("grid16x1000")))
    var = g[1].copy()
    rows = np.arange(len(var)) // 1000
    ev = (rows == 4) | (rows == 11)
    var["isEvidence"][ev] = 1
    var["initialValue"][ev] = np.random.default_rng(4).integers(0, 2, int(ev.sum()))
    g[1] = var
    return tuple(g)


def equal_values(og, x):
    """the factor values of a graphgen.ising_grid, restated: EQUAL over (first, second), +1 / -1 (pinned against
    eval_factor in tests/test_pcd_latent_cpu.py)"""
    vid = og.fmap["vid"].astype(np.int64)
    x = np.asarray(x)
    return np.where(x[vid[0::2]] == x[vid[1::2]], 1.0, -1.0)


def all_tables(routes, color):
    """every variable a sweep may sample -- evidence or not, so under either sample_evidence flag -- is a table variable"""
    kind = _lib.route_fields(np.asarray(routes))["kind"]
    return bool((kind[np.asarray(color) >= 0] == _lib.ROUTE_TABLE).all())


def disturbed(og, color, seed, x0, w0, calls=DISTURB):
    """the rows after ``nsk_gibbs_sweeps(h, n, 1, 1)`` for n in ``calls`` on the whole handle from sweep 0; returns
    (rows, sweep index)"""
    order, ps = phases_from_colors(color)
    cnt = np.zeros(int(og.cstart[-1]), np.int64)
    x = [np.ascontiguousarray(r, np.int64).copy() for r in x0]
    total = int(sum(calls))
    for r in range(len(x)):
        for s in range(total):
            assert og.gibbs_dev(order, ps, x[r], np.ascontiguousarray(w0, np.float64), cnt, int(seed) ^ (r << 32), s, True, burnin=True) == 0
    return x, total


class Run(object):
    """The oracle's run of nsk_pcd_latent_steps.  Per step t: ``states[t][r]``, ``moments[t]`` = (Mc, Mf), ``weights[t]``,
    ``gmax[t]``; ``moved_latent[t]`` / ``moved_free[t]`` / ``moved_free_evidence[t]`` whether the step's sweeps changed a
    latent variable of a clamped row / a variable of a free row / an evidence variable of a free row; ``restored`` whether
    the clamp changed a value; ``final`` / ``w`` / ``sweep`` what the call leaves."""

    def __init__(self, og, color, seed, x0, w0, K, nsteps, sweeps_per_step, free_sample_evidence, step, decay, reg_param, normalize,
                 sweep0=0, clamp=True, values=pcd.factor_values):
        order, ps = phases_from_colors(color)
        x = [np.ascontiguousarray(r, np.int64).copy() for r in x0]
        w = np.ascontiguousarray(w0, np.float64).copy()
        R, K, k = len(x), int(K), int(sweeps_per_step)
        assert 1 <= K < R
        self.K, self.R, self.reg_param = K, R, float(reg_param)
        fixed, n_w = og.weight["isFixed"].astype(bool), pcd.factors_per_weight(og)
        ev = evidence_mask(og)
        init = og.variable["initialValue"].astype(np.int64)
        self.restored = False
        if clamp:
            for r in range(K):
                self.restored = self.restored or bool((x[r][ev] != init[ev]).any())
                x[r][ev] = init[ev]
        cnt = np.zeros(int(og.cstart[-1]), np.int64)
        self.states, self.moments, self.weights, self.gmax = [], [], [], []
        self.moved_latent, self.moved_free, self.moved_free_evidence = [], [], []
        sweep, st = int(sweep0), np.float64(step)
        for t in range(nsteps):
            last = [r.copy() for r in x]
            for r0, r1, se in ((0, K, False), (K, R, bool(free_sample_evidence))):
                for r in range(r0, r1):
                    for s in range(k):
                        assert og.gibbs_dev(order, ps, x[r], w, cnt, int(seed) ^ ((r - r0) << 32), (sweep + s) & M64, se, burnin=True) == 0
                sweep += k
            for r in range(K):
                assert np.array_equal(x[r][ev], last[r][ev])            # a clamped phase holds the evidence
            self.moved_latent.append(any(bool((x[r][~ev] != last[r][~ev]).any()) for r in range(K)))
            self.moved_free.append(any(bool((x[r] != last[r]).any()) for r in range(K, R)))
            self.moved_free_evidence.append(any(bool((x[r][ev] != last[r][ev]).any()) for r in range(K, R)))
            Mc, Mf = pcd.moments_of(og, x[:K], values), pcd.moments_of(og, x[K:], values)
            w, gmax = pcd_latent_step(w, fixed, Mc, K, Mf, R - K, n_w, st, reg_param, normalize)
            w = np.ascontiguousarray(w)
            st = st * np.float64(decay)
            self.states.append([r.copy() for r in x])
            self.moments.append(np.stack([Mc, Mf]))
            self.weights.append(w.copy())
            self.gmax.append(gmax)
        assert not cnt.any()                    # burn-in sweeps tally nothing
        self.final, self.w, self.w0, self.sweep = x, w, np.array(w0, np.float64), sweep & M64
        self.moments, self.gmax = np.stack(self.moments), np.array(self.gmax)

    def changed_weights(self, free):
        """per weight of ``free``: does it change at some step of the call"""
        return (np.diff(np.vstack([self.w0] + self.weights), axis=0) != 0)[:, free].any(axis=0)

    def lively(self, free, free_sample_evidence, most=False):
        """Every weight of ``free`` changes at every step at which the rule lets it: the two populations' statistics are
        sums of a few integers, so a weight's two means now and then coincide EXACTLY, and then g = 0 and, without a
        penalty, the rule itself keeps the weight -- a weight may stand still at such a step and at no other; at every
        step (``most``: at more than half of them) some weight changes (``changed_weights``: which change at some step).  The clamped rows' latent variables
        and the free rows move at every step -- ``most``: at more than half of them, as one or two chains of a dozen
        variables now and then sit still through a step's sweeps --, the free rows' evidence variables at some step when
        they are sampled; Mc != Mf at some step."""
        ws = np.vstack([self.w0] + self.weights)
        changed = (np.diff(ws, axis=0) != 0)[:, free]
        K, F = np.float64(self.K), np.float64(self.R - self.K)
        g = (self.moments[:, 0].astype(np.float64) * 2.0 ** -32) / K - (self.moments[:, 1].astype(np.float64) * 2.0 ** -32) / F
        may_rest = (g[:, free] == 0.0) & ((self.reg_param == 0.0) | (ws[:-1][:, free] == 0.0))
        ok = (lambda m: 2 * sum(m) > len(m)) if most else all
        changing = bool((changed | may_rest).all() and ok(list(changed.any(axis=1))))
        moved = ok(self.moved_latent) and ok(self.moved_free) and (any(self.moved_free_evidence) or not free_sample_evidence)
        return changing and moved and bool((self.moments[:, 0] != self.moments[:, 1]).any())
