"""The host side of the belief-propagation tests (nsk_bp_setup / nsk_bp_run, FactorGraph.belief_propagation): the cases,
the theta tables from the oracle's eval_factor (as temper.exact_log_z builds its tables) and the numpy mirror
numbskull_amd.diagnostics.bp_iterate with the oracle's exp_det, shared by tests/test_bp_cpu.py (the mirror against
enumeration, the liveliness of every GPU case) and tests/test_bp_gpu.py (the device against the mirror, bit for bit) so
that the two cannot drift apart."""

import functools

import numpy as np

import util  # noqa: F401  (puts the repository on sys.path)
import temper
import pt
from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import bp_layout, bp_iterate, bp_factor_beliefs, bethe_log_z
from numbskull_amd.numbskulltypes import Weight, Variable, Factor, FactorToVar
from oracle import binding as orc
from util import session, oracle_of, exact_marginals

ITERS = (1, 2, 30)
TRIP_ITERS = 4


# ------------------------------------------------------------------------------------------------------- the graphs
def spec_graph(cards, evid, init, factors):
    """a graph from cardinalities, isEvidence, initial values and [(function, members, dense_equal_to, weight)]: one
    weight per factor"""
    nvar, nf = len(cards), len(factors)
    variable = np.zeros(nvar, Variable)
    variable["cardinality"], variable["isEvidence"], variable["initialValue"] = cards, evid, init
    arity = np.array([len(m) for _, m, _, _ in factors], np.int64)
    factor = np.zeros(nf, Factor)
    factor["factorFunction"] = [fn for fn, _, _, _ in factors]
    factor["featureValue"] = 1.0
    factor["arity"] = arity
    factor["ftv_offset"] = np.cumsum(arity) - arity
    factor["weightId"] = np.arange(nf)
    fmap = np.zeros(int(arity.sum()), FactorToVar)
    fmap["vid"] = np.concatenate([np.asarray(m, np.int64) for _, m, _, _ in factors]) if nf else []
    fmap["dense_equal_to"] = np.concatenate([np.asarray(d, np.int64) for _, _, d, _ in factors]) if nf else []
    weight = np.zeros(nf, Weight)
    weight["initialValue"] = [w for _, _, _, w in factors]
    weight["isFixed"] = True
    return weight, variable, factor, fmap, np.zeros(nvar, np.bool_), int(arity.sum())


def with_evidence(g, ids, values):
    g = list(g)
    var = g[1].copy()
    var["isEvidence"][ids] = 1
    var["initialValue"][ids] = values
    g[1] = var
    return tuple(g)


def chain9():
    return with_evidence(graphgen.ising_grid(1, 9, weight=0.8), [0, 5], [1, 0])


def chain17():
    return with_evidence(graphgen.ising_grid(1, 17, weight=0.8), [0], [1])


def star(extra=()):
    """a binary centre, six leaves of cardinality 2 and 3 tied to it by EQUAL / AND_CAT, unary factors on the leaves, one
    leaf evidence: the centre has six edges, as many as the variable phase keeps in registers"""
    cards = [2, 2, 2, 2, 3, 3, 2]
    f = [(3, [0, 1], [0, 0], 0.9), (3, [0, 2], [0, 0], -0.4), (3, [3, 0], [0, 0], 0.3), (12, [0, 4], [1, 2], 1.1),
         (12, [5, 0], [0, 0], -0.7), (3, [0, 6], [0, 0], 0.5), (4, [1], [0], 0.6), (4, [2], [0], -1.2), (15, [4], [1], 0.8),
         (15, [5], [2], -0.5), (4, [3], [0], 0.2)]
    return spec_graph(cards, [0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 1], f + list(extra))


def star7():
    """... and with a unary factor on the centre: seven edges, the walk through memory"""
    return star([(4, [0], [0], -0.45)])


def tree():
    """a tree with one arity-3 AND, one OR_CAT over cardinality-3 members and an evidence member"""
    cards = [2, 2, 2, 3, 3, 2, 3]
    f = [(2, [0, 1, 2], [0, 0, 0], 1.3), (12, [2, 3], [1, 0], 0.9), (14, [3, 4], [1, 2], -0.8), (4, [0], [0], 0.4),
         (15, [4], [0], 0.7), (3, [5, 1], [0, 0], 0.6), (14, [4, 6], [2, 1], 0.5), (4, [5], [0], -0.3)]
    return spec_graph(cards, [0, 0, 0, 0, 0, 0, 1], [0, 1, 0, 2, 0, 1, 1], f)


def hub(n=1200):
    """variable 0 carries n unary ISTRUE factors of weights +1, -1, +1, .. and one EQUAL to variable 1, which has a biased
    unary: without the rescale rule both entries of the hub's product underflow"""
    f = [(4, [0], [0], 1.0 if i % 2 == 0 else -1.0) for i in range(n)] + [(3, [0, 1], [0, 0], 0.8), (4, [1], [0], 0.7)]
    return spec_graph([2, 2], [0, 0], [0, 0], f)


def hub_reduced():
    """the hub's model with the unary factors that cancel taken out"""
    return spec_graph([2, 2], [0, 0], [0, 0], [(3, [0, 1], [0, 0], 0.8), (4, [1], [0], 0.7)])


def trips_grid():
    """24 x 24, every 7th variable evidence at alternating values: 576 variables, 2208 directed edges before clamping"""
    ids = np.arange(0, 24 * 24, 7)
    return with_evidence(graphgen.ising_grid(24, 24, weight=0.4), ids, np.arange(len(ids)) % 2)


def limit_graph(nfree=12, nev=4, fn=2):
    """one factor over nfree free binaries and nev evidence members at 1"""
    n = nfree + nev
    return spec_graph([2] * n, [0] * nfree + [1] * nev, [0] * nfree + [1] * nev,
                      [(fn, list(range(n)), [0] * n, 0.5), (4, [0], [0], 0.3)])


# name -> (graph builder, head_by_vid, sample_evidence); the cases the device is held to the mirror on
CASES = {
    "chain9": (chain9, False, 0),
    "chain17": (chain17, False, 0),
    "clamped_grid": (temper.clamped_grid, False, 0),
    "mixed_clamped": (temper.small_mixed, True, 0),
    "mixed_free": (temper.small_mixed, True, 1),
    "grid_int32": (pt.grid_int32, False, 0),
}
TREES = {"chain9": chain9, "chain17": chain17, "star": star, "star7": star7, "tree": tree}


# ------------------------------------------------------------------------------------------------------- the mirror
def theta_tables(og, layout, x, w):
    """w[weightId] * eval_factor over every factor's table: the free members at the digits of the table index, every
    factor asked as its first member sees it (temper.factor_terms)"""
    f = og.factor
    theta = np.zeros(int(layout["table_off"][-1]))
    x = np.ascontiguousarray(x, np.int64).copy()
    for fid in range(len(f)):
        ax, shape = layout["axes"][fid], layout["shapes"][fid]
        s, a = int(f[fid]["ftv_offset"]), int(f[fid]["arity"])
        vs = int(og.fmap["vid"][s]) if a >= 1 and int(f[fid]["factorFunction"]) != -1 else -1
        keep = x[ax].copy() if ax else None
        for i, idx in enumerate(np.ndindex(*shape)):
            for v, k in zip(ax, idx):
                x[v] = k
            rc, e = og.eval_factor(fid, vs, int(x[vs]) if vs >= 0 else 0, x)
            assert rc == 0, ("the oracle refuses factor", fid)
            theta[layout["table_off"][fid] + i] = w[int(f[fid]["weightId"])] * e
        if ax:
            x[ax] = keep
    return theta


class Model(object):
    """a graph, its oracle, the layout of its initial state and the theta tables under its initial weights"""

    def __init__(self, g, hbv=False, sev=0):
        self.g, self.hbv, self.sev = g, hbv, sev
        _, self.fg = session(g, head_by_vid=hbv)
        fg = self.fg
        self.og = oracle_of(fg, hbv, layout=False)
        self.x = fg.variable["initialValue"].astype(np.int64)
        self.w = fg.weight_value[0].copy()
        self.layout = bp_layout(fg.factor, fg.fmap, fg.variable, self.x, bool(sev))
        self.theta = theta_tables(self.og, self.layout, self.x, self.w)
        self.free = ~self.layout["clamped"]

    def run(self, iters, damping=0.0, tol=0.0, messages=None):
        r = bp_iterate(self.layout, self.theta, iters, damping, tol, exp=orc.exp_det, messages=messages)
        r["factor_beliefs"] = bp_factor_beliefs(self.layout, r["psi"], r["v2f"])
        return r

    def log_z(self, r):
        return bethe_log_z(self.layout, self.theta, r["factor_beliefs"], r["beliefs"])

    def belief(self, r, v):
        off = self.layout["offsets"]
        return r["beliefs"][off[v]:off[v + 1]]

    def exact(self):
        return exact_marginals(self.og, self.w, self.free), temper.exact_log_z(self.og, self.w, self.x, self.free)


@functools.lru_cache(maxsize=None)
def model(name):
    if name in CASES:
        build, hbv, sev = CASES[name]
        return Model(build(), hbv, sev)
    return Model({"star": star, "star7": star7, "tree": tree, "hub": hub, "hub_reduced": hub_reduced, "trips": trips_grid,
                  "limit": limit_graph}[name]())


@functools.lru_cache(maxsize=None)
def mirror(name, iters, damping=0.0, tol=0.0):
    """the mirror's run of a case from the initial messages (computed once, shared, left unchanged)"""
    return model(name).run(iters, damping, tol)


def trips(items, cap, block=_lib.BP_BLOCK):
    return _lib.bp_trips(items, cap, block)
