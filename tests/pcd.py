"""The host side of the PCD tests (nsk_weight_moments, nsk_pcd_steps, FactorGraph.weight_moments / learn_pcd): the graphs
and the oracle's mirror of a run, shared by tests/test_pcd_cpu.py (the numpy rules against hand-written loops, the
liveliness of every GPU case, the recovery of planted weights with the oracle as the sampler) and tests/test_pcd_gpu.py (the
device against the mirror, bit for bit) so that the two cannot drift apart.

The mirror extends the pattern of tests/temper.py: chain r is an oracle run in device mode seeded ``seed ^ (r << 32)``; step
t is ``sweeps_per_step`` calls of ``gibbs_dev`` under the CURRENT weights with burnin = True and a sweep counter that runs
on; the moments M are ``numbskull_amd.diagnostics.moment_counts`` of ``eval_factor`` of every factor as its first member
sees it (``temper.factor_terms`` under weights of 1.0: the product with 1.0 is exact); the update is
``numbskull_amd.diagnostics.pcd_step``."""

import numpy as np

import util  # noqa: F401  (puts the repository on sys.path)
from util import phases_from_colors
from numbskull_amd import graphgen
from numbskull_amd.diagnostics import moment_counts, pcd_step
from numbskull_amd.numbskulltypes import Weight, Variable, Factor, FactorToVar
import temper

M64 = temper.M64
ISTRUE, RATIO, UFO = 4, 8, 30


# ------------------------------------------------------------------------------------------------------- the graphs
def learnable(g, fixed=()):
    """the graph with every weight free but those of ``fixed``"""
    g = list(g)
    w = g[0].copy()
    w["isFixed"] = False
    w["isFixed"][list(fixed)] = True
    g[0] = w
    return tuple(g)


def grid_int32():
    """the clamped grid with an evidence variable of 200 values: int32 values on the device"""
    g = list(temper.clamped_grid())
    var = g[1].copy()
    var["cardinality"][5] = 200
    g[1] = var
    return tuple(g)


def ratio_graph():
    """8 binary variables; RATIO factors over (i, i + 1, i + 2) under weights 0 and 1 in turn -- their values are log(k + 1),
    k the members that agree with the last: not integers -- and an ISTRUE factor a variable under weight 2"""
    n, nr = 8, 6
    variable = np.zeros(n, Variable)
    variable["cardinality"] = 2
    variable["initialValue"] = [1, 0, 1, 1, 0, 1, 0, 0]
    weight = np.zeros(3, Weight)
    weight["initialValue"] = [0.3, -0.2, 0.1]
    factor = np.zeros(nr + n, Factor)
    factor["featureValue"] = 1.0
    factor["factorFunction"] = [RATIO] * nr + [ISTRUE] * n
    factor["weightId"] = [i % 2 for i in range(nr)] + [2] * n
    factor["arity"] = [3] * nr + [1] * n
    factor["ftv_offset"] = np.cumsum(factor["arity"]) - factor["arity"]
    fmap = np.zeros(3 * nr + n, FactorToVar)
    fmap["vid"] = [i + k for i in range(nr) for k in range(3)] + list(range(n))
    return weight, variable, factor, fmap, np.zeros(n, np.bool_), len(fmap)


def unary_graph(counts, fixed=(), seed=0):
    """Independent binary variables, each under one ISTRUE factor; weight w owns ``counts[w]`` of them, dealt in a
    seeded shuffle so that no weight's factors are neighbours.  The weights start at 0.1, 0.2, ... with alternating signs."""
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum())
    variable = np.zeros(n, Variable)
    variable["cardinality"] = 2
    variable["initialValue"] = np.random.default_rng(seed + 1).integers(0, 2, n)
    weight = np.zeros(len(counts), Weight)
    weight["initialValue"] = [0.1 * (1 + w % 7) * (-1) ** w for w in range(len(counts))]
    weight["isFixed"][list(fixed)] = True
    factor, fmap = np.zeros(n, Factor), np.zeros(n, FactorToVar)
    factor["factorFunction"] = ISTRUE
    factor["featureValue"] = 1.0
    factor["arity"] = 1
    factor["ftv_offset"] = np.arange(n)
    factor["weightId"] = np.random.default_rng(seed).permutation(np.repeat(np.arange(len(counts)), counts))
    fmap["vid"] = np.arange(n)
    return weight, variable, factor, fmap, np.zeros(n, np.bool_), n


# the kernel cuts where the statistics cut: one lane up to 16 factors, one wave's piece up to 2048
CUT_COUNTS = (0, 1, 16, 17, 2048, 2049, 5000)
CUT_FIXED = 3           # the weight of 17 factors


def cuts_graph():
    return unary_graph(CUT_COUNTS, fixed=(CUT_FIXED,), seed=11)


# Later trips under NSK_MOMENTS_GRID_CAP = 8 blocks (the smallest cap: one round of XCDs): 8 x 256 lanes take 2048 short
# weights a trip, 8 x 4 waves 32 pieces, so 4097 short weights and 65 weights of one piece are the fewest with a third trip
TRIP_CAP, TRIP_SHORTS, TRIP_PIECES = 8, 4097, 65


def trips_graph():
    return unary_graph([1] * TRIP_SHORTS + [17] * TRIP_PIECES, seed=13)


def ufo_graph(n):
    """n binary variables, each with one UFO factor of arity 1, all on weight 0: B_0 = n x 1e6"""
    variable = np.zeros(n, Variable)
    variable["cardinality"] = 2
    factor, fmap = np.zeros(n, Factor), np.zeros(n, FactorToVar)
    factor["factorFunction"] = UFO
    factor["featureValue"] = 1.0
    factor["arity"] = 1
    factor["ftv_offset"] = np.arange(n)
    fmap["vid"] = np.arange(n)
    return np.zeros(1, Weight), variable, factor, fmap, np.zeros(n, np.bool_), n


# name -> (graph builder, head_by_vid, sample_evidence): the graphs of the parity cases.  The mixed graph keeps weight 0 fixed.
GRAPHS = {k: ((lambda b=v[0], k=k: learnable(b(), fixed=(0,) if k.startswith("mixed") else ())), v[1], v[2]) for k, v in temper.SMALL.items()}
GRAPHS["grid_int32"] = (lambda: learnable(grid_int32()), False, 0)
GRAPHS["ratio"] = (ratio_graph, False, 1)
GRAPHS["cuts"] = (cuts_graph, False, 1)
GRAPHS["trips"] = (trips_graph, False, 1)

PARITY_GRAPHS = sorted(temper.SMALL) + ["grid_int32"]
PARITY_CHAINS = (1, 2, 3, 64, 65)
STEPS, DECAY = 6, 0.9
# the two calls of a parity case, one behind the other on the same handle: (sweeps_per_step, normalize, reg_param), so that
# normalize and reg_param meet in all four ways over the cases
CALLS = (((1, 1, 0.0), (2, 0, 0.01)), ((2, 1, 0.01), (1, 0, 0.0)))


def parity_calls(name, R):
    return CALLS[(PARITY_GRAPHS.index(name) + PARITY_CHAINS.index(R)) % 2] if name in PARITY_GRAPHS and R in PARITY_CHAINS else CALLS[0]


def stepsize(normalize):
    """the gradient of a weight of n factors is n times as large without the normalisation"""
    return 0.3 if normalize else 0.03


def target_of(og):
    """a target that is not the chains' own mean: a quarter of every weight's factor count, alternating in sign"""
    n = factors_per_weight(og)
    return 0.25 * n * np.where(np.arange(len(n)) % 2 == 0, 1.0, -1.0)


def factors_per_weight(og):
    return np.bincount(og.factor["weightId"].astype(np.int64), minlength=len(og.weight)).astype(np.int64)


def factor_values(og, x):
    """eval_factor of every factor on the state x, each factor as its first member sees it"""
    return temper.factor_terms(og, x, np.ones(len(og.weight)))


def moments_of(og, states, values=factor_values):
    """the int64 moments of the chains ``states``"""
    e = np.stack([values(og, x) for x in states])
    return moment_counts(e, og.factor["weightId"], len(og.weight))


# ------------------------------------------------------------------------------------------------------- the mirror
class Run(object):
    """The oracle's run of nsk_pcd_steps.  Per step t: ``states[t][r]`` the state of chain r behind the step's sweeps,
    ``moments[t]`` its M, ``weights[t]`` the weights behind its update, ``gmax[t]``, ``moved[t]`` whether the sweeps changed
    a value in some chain; ``final`` / ``w`` / ``sweep`` what the call leaves.  ``x0``: (R, nvar) starting states;
    ``values``: the factor values of a state (default: ``factor_values``, through the oracle's eval_factor)."""

    def __init__(self, og, color, seed, x0, w0, target, nsteps, sweeps_per_step, sample_evidence, step, decay, reg_param, normalize,
                 sweep0=0, values=factor_values):
        order, ps = phases_from_colors(color)
        x = [np.ascontiguousarray(r, np.int64).copy() for r in x0]
        w = np.ascontiguousarray(w0, np.float64).copy()
        target = np.ascontiguousarray(target, np.float64)
        R = len(x)
        fixed, n_w = og.weight["isFixed"].astype(bool), factors_per_weight(og)
        cnt = np.zeros(int(og.cstart[-1]), np.int64)
        self.states, self.moved, self.moments, self.weights, self.gmax = [], [], [], [], []
        sweep, st = int(sweep0), np.float64(step)
        for t in range(nsteps):
            moved = False
            for r in range(R):
                last = x[r].copy()
                for s in range(sweeps_per_step):
                    assert og.gibbs_dev(order, ps, x[r], w, cnt, int(seed) ^ (r << 32), (sweep + s) & M64, bool(sample_evidence),
                                        burnin=True) == 0
                moved = moved or bool((last != x[r]).any())
            sweep += sweeps_per_step
            M = moments_of(og, x, values)
            w, gmax = pcd_step(w, fixed, M, R, target, n_w, st, reg_param, normalize)
            w = np.ascontiguousarray(w)
            st = st * np.float64(decay)
            self.states.append([r.copy() for r in x])
            self.moved.append(moved)
            self.moments.append(M)
            self.weights.append(w.copy())
            self.gmax.append(gmax)
        assert not cnt.any()                    # burn-in sweeps tally nothing
        self.final, self.w, self.w0, self.sweep = x, w, np.array(w0, np.float64), sweep & M64
        self.moments, self.gmax = np.stack(self.moments), np.array(self.gmax)

    def lively(self, free, most=False):
        """the weights ``free`` change at every step, the states move at every step -- ``most``: at more than half of them;
        one to three chains of a dozen variables now and then sit still through a sweep -- and M differs between steps"""
        ws = np.vstack([self.w0] + self.weights)[:, free]
        changing = bool((np.diff(ws, axis=0) != 0).all())
        moved = 2 * sum(self.moved) > len(self.moved) if most else all(self.moved)
        return changing and moved and len({m.tobytes() for m in self.moments}) > 1
