"""The host side of the parallel-tempering tests (nsk_pt_sweeps, FactorGraph.parallel_tempering): the graphs, the cases and
the oracle's mirror of a run, shared by tests/test_pt_cpu.py (the rule, the paths, the cases shown lively, the method shown
to work, the oracle as the sampler) and tests/test_pt_gpu.py (the device against the mirror) so that the two cannot drift
apart.  The log-potential and the small graphs are those of tests/temper.py.

The mirror: chain r is an oracle in device mode seeded ``seed ^ (r << 32)`` that sweeps under ``betas[r] * w0`` (numpy's
elementwise product: one rounded float64 product a weight, as the scale kernel's); step t is ``sweeps_per_step`` sweeps of
every chain at the sweep indices ``sweep0 + t * sweeps_per_step + i`` -- burn-in sweeps, but tallied ones for chain
``tally_chain`` -- then U = ``temper.log_potential``'s fsum with its bound, then the decisions of
``numbskull_amd.diagnostics.pt_swap_rule`` with the oracle's ``exp_det`` on the mirror's own U -- or on a given ``lp`` matrix,
so that a GPU test drives the mirror with the device's log-potentials -- and the states of the accepted pairs change places.

The device keys a variable's generator by its position in the compiled layout.  ``tests/golden/pt_generators.npz`` holds
those ids for every graph here, so that a test without a GPU runs the very chains the device runs; the GPU tests hold the
file to the handle's layout."""

import os

import numpy as np

import util  # noqa: F401  (puts the repository on sys.path)
from util import phases_from_colors, session, oracle_of
from oracle import binding as orc
from numbskull_amd import graphgen
from numbskull_amd.diagnostics import pt_swap_rule, pt_ladder
import temper

M64 = temper.M64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pt_generators.npz")


# ------------------------------------------------------------------------------------------------------- the graphs
def grid_held15():
    """6 x 6 Ising grid with 15 variables that are read and never sampled (isEvidence == 4): they get no position, so a
    chain has 64 k + 16 value slots -- whole 16-byte accesses and nothing behind them"""
    g = list(graphgen.ising_grid(6, 6, weight=0.7))
    var = g[1].copy()
    held = np.sort(np.random.RandomState(4).permutation(36)[:15])
    var["isEvidence"][held] = 4
    var["initialValue"][held] = np.arange(15) % 2
    g[1] = var
    return tuple(g)


def grid_int32():
    """the clamped grid with an evidence variable of 200 values: int32 slots on the device"""
    g = list(temper.clamped_grid())
    var = g[1].copy()
    var["cardinality"][5] = 200
    g[1] = var
    return tuple(g)


def grid_96():
    """96 x 96: more than 8192 value bytes a chain, three trips of one 256-lane block through the swap's loop"""
    return graphgen.ising_grid(96, 96, weight=0.4)


# name -> (graph builder, head_by_vid, sample_evidence)
GRAPHS = {
    "grid_w1.0": temper.SMALL["grid_w1.0"][:3],
    "grid_held15": (grid_held15, False, 0),
    "grid_int32": (grid_int32, False, 0),
    "mixed_clamped": temper.SMALL["mixed_clamped"][:3],
    "mixed_free": temper.SMALL["mixed_free"][:3],
    "grid_96": (grid_96, False, 0),
}
# name -> (value slots of a chain, bytes of a slot): asserted on the device, so that a layout change fails there instead of
# hollowing the byte counts out (449 bytes: 28 whole accesses and 1 byte; 464: 29 and none; 2052: 128 and 4 bytes; 9473: 592 and 1)
SLOTS = {"grid_w1.0": (449, 1), "grid_held15": (464, 1), "grid_int32": (513, 4), "grid_96": (9473, 1)}

# ------------------------------------------------------------------------------------------------------- the cases
SEED = 9
SPS = 1
PRE = 3         # tallied sweeps of every chain in front of the call: all chains have counts, the uint8 tally is pending at entry
PARITY_GRAPHS = ("grid_w1.0", "grid_held15", "grid_int32", "mixed_clamped", "mixed_free")
CHAINS = (1, 2, 3, 8, 9)


def case_steps(R):
    """two chains have one pair, proposed at even steps only: twice the steps for as many proposals"""
    return 16 if R == 2 else 8


def case_betas(name, R):
    """a geometric ladder up to 1.0 whose neighbours are close enough to swap and far enough to refuse; a lone chain at
    0.5, so that its weights are scaled too (and the grid at coupling 1.0 leaves the all-0 state it starts in)"""
    if R == 1:
        return np.array([0.5])
    return pt_ladder(R, 0.2 if R > 3 else 0.6)


# On graphs this small a state that arrives in a slot often coalesces with the one that left within a sweep or two -- both
# go on under the slot's uniforms -- and the slot's tally is then what it would have been without the swap.  The cases
# tally a chain whose tally the swaps do change (tests/test_pt_cpu.py asserts it): the middle one of three, where the
# cold one's does not.
TALLY = {("mixed_clamped", 9): 6}


def case_tally(name, R):
    """the chain whose sweeps a parity case tallies: the only one, the hot one of two, the middle one of three, none of
    eight, the cold one of nine"""
    return TALLY.get((name, R), {1: 0, 2: 0, 3: 1, 8: -1, 9: 8}[R])


# (graph, chains) -> the seed of the uniforms, where the default leaves a case without an accepted and a refused proposal,
# without an accepted swap of two different states, or too close to a tie (tests/test_pt_cpu.py asserts all three)
UNIFORM_SEED = {("grid_w1.0", 2): 10, ("grid_w1.0", 9): 2, ("grid_held15", 2): 1, ("grid_held15", 9): 2, ("mixed_clamped", 2): 3,
                ("mixed_free", 2): 1, ("mixed_free", 9): 2}


def case_uniforms(name, R):
    return np.random.RandomState(UNIFORM_SEED.get((name, R), 100 + R)).random_sample((case_steps(R), R - 1))


# ------------------------------------------------------------------------------------------------------- the oracle
def device_generators(fg):
    """what the device keys every variable's generator by (needs a GPU): tests/util.py oracle_of hands the same to the oracle"""
    ids, color, gen = fg.layout(), fg.colors(), fg.generators()
    return np.where(np.asarray(color) >= 0, gen, ids).astype(np.int64)


def host_oracle(name, seed=SEED):
    """(og, color, fg) without a GPU: the colouring of FactorGraph.plan(), the generators of the golden file"""
    build, hbv, _ = GRAPHS[name]
    _, fg = session(build(), seed=seed, head_by_vid=hbv)
    og = oracle_of(fg, hbv, layout=False)
    og.set_rng_ids(np.load(GOLDEN)[name])
    return og, fg.plan()[0], fg


def case_run(name, R, swaps=True):
    """the mirror of the parity case (name, R) of tests/test_pt_gpu.py, without a GPU: PRE tallied sweeps of every chain from
    the initial values, then the call"""
    og, color, _ = host_oracle(name)
    se = GRAPHS[name][2]
    order, ps = phases_from_colors(color)
    vv, _, w0, cnt = og.initial_state()
    x, c = [vv.copy() for _ in range(R)], [cnt.copy() for _ in range(R)]
    for s in range(PRE):
        for r in range(R):
            assert og.gibbs_dev(order, ps, x[r], w0, c[r], SEED ^ (r << 32), s, bool(se), burnin=False) == 0
    T = case_steps(R)
    u = case_uniforms(name, R) if R > 1 else np.zeros((T, 0))
    return Run(og, color, SEED, x, w0, case_betas(name, R), T, SPS, se, u, case_tally(name, R), sweep0=PRE, swaps=swaps, cnt0=c)


# ------------------------------------------------------------------------------------------------------- the mirror
class Run(object):
    """The oracle's run of nsk_pt_sweeps.  ``x0``: (R, nvar) starting states.  Keeps ``lp`` and ``bound`` (T, R), the
    fsum log-potentials behind every step's sweeps and the header's bound; ``own`` (T, R - 1) int32, the decisions of
    ``pt_swap_rule`` on the mirror's own U; ``accepted``, the decisions APPLIED -- those on the rows of ``lp`` where a
    matrix is given, none where ``swaps`` is False, else ``own``; ``safe`` (T, R - 1) bool, whether a proposed pair's decision
    stands wherever its two U move within their bounds; ``differing[t]``, the accepted pairs of step t whose states
    differed; ``states[t]`` the states behind step t's swaps; ``final``, ``sweep``, and ``cnt`` (R, ncount), the tallies,
    which only chain ``tally_chain`` grows."""

    def __init__(self, og, color, seed, x0, w0, betas, nsteps, sweeps_per_step, sample_evidence, uniforms, tally_chain=-1,
                 sweep0=0, lp=None, swaps=True, cnt0=None):
        order, ps = phases_from_colors(color)
        betas = np.ascontiguousarray(betas, np.float64)
        x = [np.ascontiguousarray(r, np.int64).copy() for r in x0]
        w0 = np.ascontiguousarray(w0, np.float64)
        R, T = len(x), int(nsteps)
        assert len(betas) == R
        uniforms = np.ascontiguousarray(uniforms, np.float64).reshape(T, R - 1)
        nc = int(og.cstart[-1])
        cnt = [np.zeros(nc, np.int64) if cnt0 is None else np.ascontiguousarray(cnt0[r], np.int64).copy() for r in range(R)]
        start = [c.copy() for c in cnt]
        w = [np.ascontiguousarray(betas[r] * w0) for r in range(R)]
        self.lp, self.bound = np.zeros((T, R)), np.zeros((T, R))
        self.own, self.accepted = np.full((T, R - 1), -1, np.int32), np.full((T, R - 1), -1, np.int32)
        self.safe = np.ones((T, R - 1), bool)
        self.states, self.differing = [], []
        sweep = int(sweep0)
        for t in range(T):
            for r in range(R):
                for s in range(sweeps_per_step):
                    assert og.gibbs_dev(order, ps, x[r], w[r], cnt[r], int(seed) ^ (r << 32), (sweep + s) & M64,
                                        bool(sample_evidence), burnin=r != tally_chain) == 0
                self.lp[t, r], self.bound[t, r] = temper.log_potential(og, x[r], w0)
            sweep += sweeps_per_step
            self.own[t] = pt_swap_rule(betas, self.lp[t], uniforms[t], t, exp=orc.exp_det)
            self.safe[t] = decision_margins(betas, self.lp[t], self.bound[t], uniforms[t], t)
            acc = self.own[t] if lp is None else pt_swap_rule(betas, lp[t], uniforms[t], t, exp=orc.exp_det)
            if not swaps:
                acc = np.where(acc == 1, 0, acc).astype(np.int32)
            self.accepted[t] = acc
            n = 0
            for r in np.nonzero(acc == 1)[0]:
                n += int((x[r] != x[r + 1]).any())
                x[r], x[r + 1] = x[r + 1], x[r]
            self.differing.append(n)
            self.states.append([r.copy() for r in x])
        for r in range(R):
            assert r == tally_chain or np.array_equal(cnt[r], start[r])        # burn-in sweeps tally nothing
        self.betas, self.final, self.sweep, self.cnt = betas, x, sweep & M64, np.stack(cnt)
        self.tally = self.cnt - np.stack(start)


def decision_margins(betas, U, bound, uniforms, t):
    """(R - 1,) bool: a pair not proposed at step t is True; a proposed pair is True when its decision is the same for every
    pair of log-potentials within ``bound`` of ``U``.  The two U move d by at most ``dd = |betas[r] - betas[r + 1]| (bound[r]
    + bound[r + 1])``, widened by the roundings of the two differences and the product; the decision stands if d - dd >=
    0 (accepted whatever the uniform), or the uniform lies below exp(d - dd) (accepted either way), or d + dd < 0 and the
    uniform lies above exp(d + dd) (refused either way) -- the exponentials widened by 1e-12 relative, a thousand times
    what separates the specified exp from the exact one."""
    R = len(betas)
    out = np.ones(R - 1, bool)
    for r in range(int(t) & 1, R - 1, 2):
        db, du = betas[r] - betas[r + 1], U[r + 1] - U[r]
        d = db * du
        if not np.isfinite(d):
            out[r] = False
            continue
        dd = abs(db) * (bound[r] + bound[r + 1]) + 4 * 2.0 ** -52 * (abs(d) + abs(db) * (abs(U[r]) + abs(U[r + 1])))
        lo, hi = np.exp(min(d - dd, 0.0)) * (1 - 1e-12), np.exp(min(d + dd, 0.0)) * (1 + 1e-12)
        out[r] = bool(d - dd >= 0.0 or uniforms[r] < lo or (d + dd < 0.0 and uniforms[r] > hi))
    return out


def permutation(accepted, R):
    """where[s] = the starting slot of the state in slot s behind the swaps of ``accepted`` (T, R - 1)"""
    where = list(range(R))
    for row in np.asarray(accepted).reshape(-1, R - 1):
        for r in np.nonzero(row == 1)[0]:
            where[r], where[r + 1] = where[r + 1], where[r]
    return where
