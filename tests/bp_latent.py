"""The host side of the tests of latent-variable learning by belief propagation (nsk_bp_select / nsk_bp_latent_steps,
FactorGraph.learn_bp(latent=True) / bp_log_evidence): the cases and the numpy mirror of a run, shared by
tests/test_bp_latent_cpu.py (the rule against enumeration, the liveliness of every GPU case) and
tests/test_bp_latent_gpu.py (the device against the mirror, bit for bit) so that the two cannot drift apart.

The mirror is two ``bp_learn.Learner``s of one graph -- ``sev=0``: the evidence held, the clamped set-up of slot 0;
``sev=1``: everything free, slot 1 -- stepped together: each runs its own iterations from its own messages with its own
early exit, and ``diagnostics.pcd_latent_step`` with ``K = Rf = 1`` moves the weights both share."""

import functools

import numpy as np

import util  # noqa: F401  (puts the repository on sys.path)
import bp
import bp_learn as bl
import pcd
import temper
from numbskull_amd.diagnostics import bp_factor_beliefs, bethe_log_z, pcd_latent_step
from numbskull_amd.numbskulltypes import Weight, Factor, FactorToVar

DECAY = bl.DECAY
# (nsteps, iters_per_step, warm, tol, normalize, reg_param) of bl.SETTINGS: warm and cold, tol 0 and above, normalize
# both ways, reg_param both ways
SETTINGS = (bl.SETTINGS[1], bl.SETTINGS[3], bl.SETTINGS[2], bl.SETTINGS[6])


# ------------------------------------------------------------------------------------------------------- the graphs
def with_fields(g, ids, value):
    """the graph with one more learnable weight of initial value ``value`` and an ISTRUE factor under it on every variable
    of ``ids``.  A plain Ising grid is symmetric under flipping every variable: with everything free its messages stay
    at 1 / 2 and an edge left out would go unnoticed; the fields break the symmetry, so the free set-up's messages move."""
    w, v, f, fm, dm, edges = g
    ids = np.asarray(ids, np.int64)
    w2, f2, fm2 = np.zeros(len(w) + 1, Weight), np.zeros(len(f) + len(ids), Factor), np.zeros(len(fm) + len(ids), FactorToVar)
    w2[:len(w)], f2[:len(f)], fm2[:len(fm)] = w, f, fm
    w2["initialValue"][-1] = value
    new = f2[len(f):]
    new["factorFunction"], new["featureValue"], new["arity"], new["weightId"] = 4, 1.0, 1, len(w)
    new["ftv_offset"] = len(fm) + np.arange(len(ids))
    f2[len(f):] = new
    fm2["vid"][len(fm):] = ids
    return w2, v, f2, fm2, dm, int(edges) + len(ids)


def chain9_ends():
    """1 x 9 under a strong coupling, evidence at both ends, a field on either end: a forest under either set-up.  The
    clamped set-up's messages travel seven free variables and the free one's nine: they converge iterations apart."""
    return with_fields(bl.grid(1, 9, evidence=((0, 1), (8, 1)), weight=(0.3, 1.2)), [0, 8], -0.5)


def grid5x5_third():
    return with_fields(bl.grid(5, 5, evidence=[(v, (v // 3) % 2) for v in range(0, 25, 3)]), [1, 7, 13, 22], 0.6)


def mixed_cat_evidence():
    """the mixed categorical graph with every variable of cardinality above 2 evidence and every binary one latent: the
    clamped set-up has no non-binary variable to walk, the free one has"""
    g = list(pcd.learnable(temper.small_mixed(), fixed=(0,)))
    var = g[1].copy()
    var["isEvidence"] = np.where(var["cardinality"] > 2, 1, 0)
    g[1] = var
    return tuple(g)


def all_evidence():
    return bl.all_clamped(with_fields(bl.grid(4, 4, evidence=[(v, v % 3 % 2) for v in range(16)]), [3, 4, 10], -0.4))


def no_evidence():
    return with_fields(bl.grid(3, 4), [0, 5, 6], 0.7)


def trips_latent():
    """bp_learn's trips graph (24 x 24, every 7th variable evidence) with every 7th from 3 on evidence too"""
    ids = np.arange(3, 24 * 24, 7)
    g = bp.with_evidence(pcd.learnable(bp.trips_grid()), ids, (np.arange(len(ids)) // 2) % 2)
    return with_fields(g, np.arange(1, 24 * 24, 5), 0.5)


def tree_latent():
    """bp_learn's shared tree under weights away from 0, a binary and a cardinality-3 variable evidence"""
    g = list(bl.shared_tree())
    w = g[0].copy()
    w["initialValue"] = [0.4, -0.3, 0.2]
    g[0] = w
    return bp.with_evidence(tuple(g), [0, 4, 8], [1, 0, 2])


# name -> (graph builder, head_by_vid, damping)
CASES = {
    "chain9_ends": (chain9_ends, False, 0.0),
    "grid5x5_third": (grid5x5_third, False, bl.LEARN["grid5x5_clamped"][2]),
    "mixed_cat": (mixed_cat_evidence, True, bl.LEARN["mixed"][2]),
    "all_evidence": (all_evidence, False, 0.0),
    "no_evidence": (no_evidence, False, 0.0),
    "trips": (trips_latent, False, 0.0),
    "tree": (tree_latent, False, 0.0),
}
STEP_CASES = ("chain9_ends", "grid5x5_third", "mixed_cat", "all_evidence", "no_evidence")      # against every setting
TRIP_SETTING = (2, bp.TRIP_ITERS, 1, 0.0, 1, 0.0)
UNEVEN_ITERS, UNEVEN_TOL = 14, 1e-9         # chain9_ends: both set-ups converge inside a step, iterations apart


# ------------------------------------------------------------------------------------------------------- the mirror
class Pair(object):
    """the clamped and the free Learner of one graph; index 0 of every pair axis is the clamped one"""

    def __init__(self, g, hbv=False):
        self.g, self.hbv = g, hbv
        self.side = (bl.Learner(g, hbv, 0), bl.Learner(g, hbv, 1))
        c = self.side[0]
        self.nw, self.fixed, self.nfac, self.w0 = c.nw, c.fixed, c.nfac, c.m.w.copy()

    def learn(self, w, nsteps, iters, damping, tol, warm, step, decay, reg_param, normalize, messages=None):
        """nsk_bp_latent_steps from the weights ``w`` and the two message sets given (None: fresh set-ups')"""
        w = np.array(w, np.float64)
        messages = list(messages) if messages is not None else [None, None]
        out = {"gmax": np.zeros(nsteps), "iters": np.zeros((nsteps, 2), np.int64), "residual": np.zeros((nsteps, 2, iters)),
               "moments": np.zeros((nsteps, 2, self.nw), np.int64), "skipped": np.zeros((nsteps, 2), np.int64)}
        st = float(step)
        for t in range(nsteps):
            for s, ln in enumerate(self.side):
                r = ln.run(w, iters, damping, tol, messages[s] if warm else None)
                out["moments"][t, s], out["skipped"][t, s] = ln.moments(r)
                out["iters"][t, s], out["residual"][t, s] = r["iters"], r["residual"]
                messages[s] = (r["f2v"], r["v2f"])
            w, out["gmax"][t] = pcd_latent_step(w, self.fixed, out["moments"][t, 0], 1, out["moments"][t, 1], 1, self.nfac, st,
                                                reg_param, normalize)
            st = st * decay
        out["w"], out["messages"], out["theta"] = w, messages, [ln.theta(w) for ln in self.side]
        return out

    def log_z(self, w, iters=100, damping=0.0, tol=1e-9):
        """the host-side rule of bp_log_evidence: bethe_log_z of either set-up's run, the clamped one first"""
        out = []
        for ln in self.side:
            r = ln.run(w, iters, damping, tol)
            fb = bp_factor_beliefs(ln.m.layout, r["psi"], r["v2f"])
            out.append(bethe_log_z(ln.m.layout, ln.theta(w), fb, r["beliefs"]))
        return out

    def exact(self, w):
        """(E[S_w | evidence], E[S_w], log Z clamped, log Z free) by enumeration"""
        c, f = self.side
        mc, zc = bl.exact_moments(c.m.og, w, c.m.x, c.m.free)
        mf, zf = bl.exact_moments(f.m.og, w, f.m.x, f.m.free)
        return mc, mf, zc, zf


@functools.lru_cache(maxsize=None)
def pair(name):
    build, hbv, _ = CASES[name]
    return Pair(build(), hbv)


def step_of(normalize, step=0.5):
    return step if normalize else step / 8


@functools.lru_cache(maxsize=None)
def mirror(name, setting):
    """the mirror's run of a case from its initial weights and fresh messages (computed once, shared, left unchanged)"""
    nsteps, iters, warm, tol, normalize, reg = setting
    p = pair(name)
    return p.learn(p.w0, nsteps, iters, CASES[name][2], tol, warm, step_of(normalize), DECAY, reg, normalize)
