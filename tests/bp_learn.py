"""The host side of the tests of learning by belief propagation (nsk_bp_refresh / nsk_bp_moments / nsk_bp_learn_steps,
FactorGraph.bp_weight_moments / learn_bp): the cases, the exact moments by enumeration and the numpy mirror of a run,
shared by tests/test_bp_learn_cpu.py (the rule against enumeration, the liveliness of every GPU case) and
tests/test_bp_learn_gpu.py (the device against the mirror, bit for bit) so that the two cannot drift apart.

The mirror extends tests/bp.py: ``feat = bp.theta_tables(og, layout, x, ones)`` (the product ``1.0 * e`` is exact), a
step's theta is ``w[weightId] * feat`` (numpy's elementwise product: one rounded product an entry), its iterations are
``bp_iterate`` with the oracle's exp_det -- fed the previous step's messages when warm --, its moments
``diagnostics.bp_moment_counts`` and its update ``diagnostics.pcd_step`` with ``R = 1``."""

import functools

import numpy as np

import util  # noqa: F401  (puts the repository on sys.path)
import bp
import pcd
import temper
import truth_tables as tt
from numbskull_amd import graphgen
from numbskull_amd.diagnostics import bp_iterate, bp_moment_counts, pcd_step
from numbskull_amd.numbskulltypes import Weight
from oracle import binding as orc

MOMENT_ITERS = (1, 2, 30)
DECAY = 0.9


# ------------------------------------------------------------------------------------------------------- the graphs
def grid(n, m, two_weights=True, evidence=(), weight=(0.3, -0.2)):
    """an n x m Ising grid with learnable weights, 0 on the vertical and 1 on the horizontal edges with ``two_weights``;
    ``evidence`` [(variable, value)] clamps"""
    g = list(graphgen.ising_grid(n, m, weight=weight[0], fixed=False, two_weights=two_weights))
    if two_weights:
        w = g[0].copy()
        w["initialValue"] = weight
        g[0] = w
    g = tuple(g)
    if evidence:
        g = bp.with_evidence(g, [v for v, _ in evidence], [x for _, x in evidence])
    return g


def shared_tree():
    """a tree of nine variables under three shared learnable weights: EQUAL along a chain of seven (weight 0), two
    branches by AND_CAT into cardinality-3 leaves (weight 1), unary ISTRUE / ISTRUE-of-a-value factors (weight 2)"""
    cards = [2, 2, 2, 2, 2, 2, 2, 3, 3]
    f = [(3, [i + 1, i], [0, 0], 0.0) for i in range(6)]
    f += [(12, [2, 7], [1, 2], 0.0), (12, [8, 5], [0, 1], 0.0)]
    f += [(4, [0], [0], 0.0), (4, [3], [0], 0.0), (15, [7], [1], 0.0), (4, [6], [0], 0.0), (15, [8], [2], 0.0)]
    g = list(bp.spec_graph(cards, [0] * 9, [0] * 9, f))
    fac = g[2].copy()
    fac["weightId"] = [0] * 6 + [1] * 2 + [2] * 5
    g[2] = fac
    g[0] = np.zeros(3, Weight)
    return tuple(g)


W_STAR = np.array([0.7, -0.9, 0.5])         # the planted weights of the recovery test
# chosen with the mirror: grad_max falls monotonically over the last half, max |w - w*| = 1.208e-05 at the end
RECOVERY = dict(epochs=60, stepsize=2.0, iters=12, tol=1e-9)
RECOVERY_BOUND = 10 * 1.208e-05             # ten times what the mirror reaches: slack for a changed step count, no more


def nan_graph():
    """weights +800 and -800 on one variable: psi is (1, 0) and (0, 1), every product 0, 0 / 0"""
    return bp.spec_graph([2], [0], [0], [(4, [0], [0], 800.0), (4, [0], [0], -800.0)])


def all_clamped(g):
    g = list(g)
    var = g[1].copy()
    var["isEvidence"] = 1
    g[1] = var
    return tuple(g)


TRUTH_GROUPS = ((8, 13), (7, 14), (2, 21))


def truth(part, mode):
    """the truth-table graphs of tests/test_bp_gpu.py for one group of functions, arities 1 .. 4, leaves of cardinality 3.
    The groups hold the two functions whose values are no indicators (RATIO, LINEAR), a positional one, a categorical
    one, AND and a DP_GEN function: two functions a group keep the mirror of a case at a few seconds."""
    fns = TRUTH_GROUPS[part]
    g, _ = tt.truth_graph(fns=fns, lcard=3)
    g = list(g)
    var = g[1].copy()
    var["isEvidence"] = 0
    if mode == "third":
        var["isEvidence"][::3] = 1
    g[1] = var
    return tuple(g)


# name -> (graph builder, head_by_vid, sample_evidence): the cases of the moments beside bp.CASES
EXTRA = {
    "star7": (bp.star7, False, 0), "tree": (bp.tree, False, 0), "hub": (bp.hub, False, 0), "limit": (bp.limit_graph, False, 0),
    "grid6_one": (lambda: grid(6, 6, two_weights=False, evidence=((0, 1), (14, 0), (35, 1))), False, 0),
    "grid6_two": (lambda: grid(6, 6, evidence=((0, 1), (14, 0), (35, 1))), False, 0),
    "trips": (lambda: pcd.learnable(bp.trips_grid()), False, 0),
    "nan": (nan_graph, False, 0),
    "shared_tree": (shared_tree, False, 0),
}
EXTRA.update({"truth%d_%s" % (p, mode): ((lambda p=p, mode=mode: truth(p, mode)), True, 0) for p in (0, 1, 2) for mode in ("free", "third")})
MOMENT_CASES = sorted(bp.CASES) + ["star7", "tree", "hub", "limit", "grid6_one", "grid6_two"] + \
    ["truth%d_%s" % (p, mode) for p in (0, 1, 2) for mode in ("free", "third")]

# the cases of nsk_bp_learn_steps: name -> (graph builder, head_by_vid, damping).  The plain grids are free: their
# messages stay uniform and the tables alone move; the clamped ones and the mixed graph move their messages too.
LEARN = {
    "grid1x9": (lambda: grid(1, 9), False, 0.0),
    "grid5x5": (lambda: grid(5, 5), False, 0.5),
    "grid1x9_clamped": (lambda: grid(1, 9, evidence=((0, 1), (5, 0))), False, 0.0),
    "grid5x5_clamped": (lambda: grid(5, 5, evidence=((0, 1), (12, 0), (23, 1))), False, 0.5),
    "mixed": (lambda: pcd.learnable(temper.small_mixed(), fixed=(0,)), True, 0.5),
}
# (nsteps, iters_per_step, warm, tol, normalize, reg_param): every value of every setting, each pair of values of two
# neighbouring settings at least once
SETTINGS = ((1, 1, 0, 0.0, 0, 0.0), (1, 6, 1, 1e-6, 1, 0.01), (3, 1, 1, 0.0, 1, 0.0), (3, 6, 0, 1e-6, 0, 0.01),
            (8, 1, 0, 1e-6, 1, 0.01), (8, 6, 1, 0.0, 0, 0.0), (3, 6, 1, 0.0, 1, 0.01), (8, 6, 0, 1e-6, 1, 0.0))


# ------------------------------------------------------------------------------------------------------- the mirror
class Learner(object):
    """a bp.Model with its feature table and the mirror of the moments and of the learning steps"""

    def __init__(self, g, hbv=False, sev=0):
        self.m = m = bp.Model(g, hbv, sev)
        fg = m.fg
        self.nw = len(fg.weight)
        self.wid = fg.factor["weightId"].astype(np.int64)
        self.fixed = fg.weight["isFixed"].astype(bool)
        self.nfac = np.bincount(self.wid, minlength=self.nw).astype(np.int64)
        self.feat = bp.theta_tables(m.og, m.layout, m.x, np.ones(self.nw))
        self.entry_wid = np.repeat(self.wid, np.diff(m.layout["table_off"]))

    def theta(self, w):
        return np.asarray(w, np.float64)[self.entry_wid] * self.feat

    def run(self, w, iters, damping=0.0, tol=0.0, messages=None):
        return bp_iterate(self.m.layout, self.theta(w), iters, damping, tol, exp=orc.exp_det, messages=messages)

    def moments(self, r):
        return bp_moment_counts(self.m.layout, self.feat, r["psi"], r["v2f"], self.wid, self.nw)

    def learn(self, w, target, nsteps, iters, damping, tol, warm, step, decay, reg_param, normalize, messages=None):
        """nsk_bp_learn_steps from the weights ``w`` and the messages given (None: a fresh set-up's)"""
        w = np.array(w, np.float64)
        out = {"gmax": np.zeros(nsteps), "iters": np.zeros(nsteps, np.int64), "residual": np.zeros((nsteps, iters)),
               "moments": np.zeros((nsteps, self.nw), np.int64), "skipped": np.zeros(nsteps, np.int64)}
        st = float(step)
        for t in range(nsteps):
            r = self.run(w, iters, damping, tol, messages if warm else None)
            M, sk = self.moments(r)
            w, out["gmax"][t] = pcd_step(w, self.fixed, M, 1, target, self.nfac, st, reg_param, normalize)
            out["iters"][t], out["residual"][t], out["moments"][t], out["skipped"][t] = r["iters"], r["residual"], M, sk
            messages = (r["f2v"], r["v2f"])
            st = st * decay
        out["w"], out["messages"], out["theta"] = w, messages, self.theta(w)
        return out


@functools.lru_cache(maxsize=None)
def learner(name):
    if name in LEARN:
        build, hbv, _ = LEARN[name]
        return Learner(build(), hbv, 0)
    build, hbv, sev = bp.CASES[name] if name in bp.CASES else EXTRA[name]
    return Learner(build(), hbv, sev)


@functools.lru_cache(maxsize=None)
def moments_mirror(name, iters):
    """(M, skipped, the run) of a case after ``iters`` iterations under its initial weights (computed once, shared)"""
    ln = learner(name)
    r = ln.run(ln.m.w, iters)
    M, sk = ln.moments(r)
    return M, sk, r


def learn_target(name):
    """a target the initial weights do not meet: the Bethe moments under planted weights, 20 iterations"""
    ln = learner(name)
    planted = ln.m.w + 0.5 * np.where(np.arange(ln.nw) % 2 == 0, 1.0, -1.0)
    M, _ = ln.moments(ln.run(planted, 20, 0.5))
    return M.astype(np.float64) * 2.0 ** -32


@functools.lru_cache(maxsize=None)
def learn_mirror(name, setting, step=0.5):
    nsteps, iters, warm, tol, normalize, reg = setting
    ln = learner(name)
    s = step if normalize else step / 8
    return ln.learn(ln.m.w, learn_target(name), nsteps, iters, LEARN[name][2], tol, warm, s, DECAY, reg, normalize)


# ------------------------------------------------------------------------------------------------------- enumeration
def exact_moments(og, w, base, free):
    """(E[S_w] for every weight, log Z) by enumeration over every assignment of the variables ``free`` (a mask), the
    others held at ``base``: every factor's table of eval_factor over its free members, broadcast into the grid of all
    assignments (temper.exact_log_z's construction)"""
    free = [int(v) for v in np.nonzero(free)[0]]
    card = [int(og.variable[v]["cardinality"]) for v in free]
    assert np.prod(card, dtype=np.float64) <= 1 << 22, card
    axis = {v: i for i, v in enumerate(free)}
    logp = np.zeros(card if card else (1,))
    f, vid = og.factor, og.fmap["vid"]
    x = np.ascontiguousarray(base, np.int64).copy()
    tables = []
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
        tables.append(table.reshape(full))
        logp = logp + float(w[int(f[fid]["weightId"])]) * tables[-1]
    mx = logp.max()
    p = np.exp(logp - mx)
    z = p.sum()
    p = p / z
    out = np.zeros(len(w))
    for fid, table in enumerate(tables):
        out[int(f[fid]["weightId"])] += float((p * table).sum())
    return out, float(mx + np.log(z))


def vmax(factor):
    """the bound of a factor's value the range rule of nsk_weight_moments uses"""
    fn, ar = factor["factorFunction"].astype(np.int64), np.maximum(factor["arity"].astype(np.float64), 1.0)
    return np.where(fn == 7, ar, np.where(fn == 8, np.log(ar + 1.0), np.where(fn == 30, 1e6, 1.0)))
