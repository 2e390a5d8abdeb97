"""The host side of the tempered-schedule tests (nsk_tempered_sweeps, FactorGraph.tempered_sweeps / log_partition /
log_evidence / anneal): the graphs, the oracle's mirror of a schedule and the exact log Z by enumeration, shared by
tests/test_temper_cpu.py (the estimator against the enumeration, the oracle as the sampler) and tests/test_temper_gpu.py
(the device against the mirror) so that the two cannot drift apart.

The mirror: chain r is an oracle run in device mode seeded ``seed ^ (r << 32)``; step t is ``sweeps_per_step`` calls of
``gibbs_dev`` under the weights ``betas[t] * w0`` (numpy's elementwise product: one rounded float64 product a weight, as
the scale kernel's) with burnin = True and a sweep counter that runs on; the log-potential U of a state is the
``math.fsum`` of ``w0[weightId] * eval_factor`` over all factors, every factor asked as its first member sees it (what
tests/resident.py Mirror.lp does), with the header's bound ``(nfactor + 1) 2^-53 sum |term|`` beside it."""

import math

import numpy as np

import util  # noqa: F401  (puts the repository on sys.path)
from util import phases_from_colors
from numbskull_amd import graphgen
from numbskull_amd.diagnostics import ais_log_weights, ais_estimate, thermodynamic_integral

M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------------- the graphs
def clamped_grid(weight=0.6):
    """3 x 4 Ising grid, variables 0, 5, 11 evidence at 1, 0, 1"""
    g = list(graphgen.ising_grid(3, 4, weight=weight))
    var = g[1].copy()
    var["isEvidence"][[0, 5, 11]] = 1
    var["initialValue"][[0, 5, 11]] = [1, 0, 1]
    g[1] = var
    return tuple(g)


def small_mixed():
    """10 variables of cardinalities 2, 4 and 8, OR / IMPLY_MLN / *_CAT factors of arity 1 .. 4 under six seeded weights;
    needs head_by_vid"""
    g = list(graphgen.mixed_lr_graph(10, seed=5, nweights=6, window=6, evidence_frac=0.3))
    w = g[0].copy()
    w["initialValue"] = np.random.default_rng(3).normal(0, 0.7, 6)
    g[0] = w
    return tuple(g)


# name -> (graph builder, head_by_vid, sample_evidence, the exact log Z by enumeration)
SMALL = {
    "grid_w0.3": (lambda: graphgen.ising_grid(3, 4, weight=0.3), False, 0, 9.119036),
    "grid_w1.0": (lambda: graphgen.ising_grid(3, 4, weight=1.0), False, 0, 17.816647),
    "grid_w0.6_clamped": (clamped_grid, False, 0, 8.119758),
    "mixed_clamped": (small_mixed, True, 0, 10.348639),
    "mixed_free": (small_mixed, True, 1, 16.287320),
}


# ------------------------------------------------------------------------------------------------------- log-potential
def factor_terms(og, x, w0):
    """w0[weightId] * eval_factor for every factor on the state x, each factor as its first member sees it"""
    f, vid = og.factor, og.fmap["vid"]
    e = np.zeros(len(f))
    for fid in range(len(f)):
        s, a = int(f[fid]["ftv_offset"]), int(f[fid]["arity"])
        vs = int(vid[s]) if a >= 1 and int(f[fid]["factorFunction"]) != -1 else -1
        rc, e[fid] = og.eval_factor(fid, vs, int(x[vs]) if vs >= 0 else 0, x)
        assert rc == 0, ("the oracle refuses factor", fid)
    return w0[f["weightId"].astype(np.int64)] * e


def log_potential(og, x, w0):
    """(the exactly rounded sum, the header's bound on what the device's sum may differ from it)"""
    t = factor_terms(og, x, w0)
    return math.fsum(t.tolist()), (len(t) + 1) * 2.0 ** -53 * math.fsum(np.abs(t).tolist())


def sampled_mask(og, color, sample_evidence):
    return (np.asarray(color) >= 0) & ((og.variable["isEvidence"] == 0) | bool(sample_evidence))


def log_z0(og, color, sample_evidence):
    """the log of the number of states of the variables a sweep samples"""
    return float(np.log(og.variable["cardinality"].astype(np.float64)[sampled_mask(og, color, sample_evidence)]).sum())


def exact_log_z(og, w0, base, free):
    """log of the sum of exp(U) over every assignment of the variables ``free`` (a mask), the others held at ``base``:
    every factor's table over its free members, added into the grid of all assignments by broadcasting."""
    free = [int(v) for v in np.nonzero(free)[0]]
    card = [int(og.variable[v]["cardinality"]) for v in free]
    assert np.prod(card, dtype=np.float64) <= 1 << 24, card
    axis = {v: i for i, v in enumerate(free)}
    logp = np.zeros(card if card else (1,))
    f, vid = og.factor, og.fmap["vid"]
    x = np.ascontiguousarray(base, np.int64).copy()
    for fid in range(len(f)):
        s, a, fn = int(f[fid]["ftv_offset"]), int(f[fid]["arity"]), int(f[fid]["factorFunction"])
        members = [int(v) for v in vid[s:s + a]] if fn != -1 else []
        mine = sorted({v for v in members if v in axis})
        vs = members[0] if members else -1
        shape = [card[axis[v]] for v in mine]
        table = np.zeros(shape if shape else ())
        for idx in np.ndindex(*shape):
            for v, k in zip(mine, idx):
                x[v] = k
            rc, table[idx] = og.eval_factor(fid, vs, int(x[vs]) if vs >= 0 else 0, x)
            assert rc == 0
        for v in mine:
            x[v] = base[v]
        full = [1] * max(len(card), 1)
        for v in mine:
            full[axis[v]] = card[axis[v]]
        # (`mine` is sorted by variable id and so are the axes: the table's axes are already in grid order)
        logp = logp + float(w0[int(f[fid]["weightId"])]) * table.reshape(full)
    m = logp.max()
    return float(m + np.log(np.exp(logp - m).sum()))


# ------------------------------------------------------------------------------------------------------- the mirror
class Schedule(object):
    """The oracle's run of a schedule: ``states[t][r]`` the state of chain r after step t, ``lp`` (T, R) the fsum
    log-potentials, ``bound`` (T, R) the header's bound, ``moved[t]`` whether step t changed a value in some chain,
    ``sweep`` the sweep counter afterwards.  ``x0``: (R, nvar) starting states."""

    def __init__(self, og, color, seed, x0, w0, betas, sweeps_per_step, sample_evidence, sweep0=0):
        order, ps = phases_from_colors(color)
        betas = np.asarray(betas, np.float64)
        x = [np.ascontiguousarray(r, np.int64).copy() for r in x0]
        w0 = np.ascontiguousarray(w0, np.float64)
        R, T = len(x), len(betas)
        cnt = np.zeros(int(og.cstart[-1]), np.int64)
        self.states, self.moved = [], []
        self.lp, self.bound = np.zeros((T, R)), np.zeros((T, R))
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
                self.lp[t, r], self.bound[t, r] = log_potential(og, x[r], w0)
            sweep += sweeps_per_step
            self.states.append([r.copy() for r in x])
            self.moved.append(moved)
        assert not cnt.any()                    # burn-in sweeps tally nothing
        self.betas, self.final, self.sweep = betas, x, sweep & M64
        self.log_weights = ais_log_weights(betas, self.lp)

    def best(self):
        """per chain: (the first step of largest log-potential, that state)"""
        steps = np.argmax(self.lp, axis=0)
        return steps, [self.states[int(t)][r] for r, t in enumerate(steps)]

    def estimate(self, lz0):
        """(log_z, stderr, ess, the thermodynamic integral) of the run"""
        return ais_estimate(self.log_weights, lz0) + (thermodynamic_integral(self.betas, self.lp, lz0),)
