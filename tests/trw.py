"""The host side of the tree-reweighted BP tests (nsk_bp_trw_run, FactorGraph.reweighted_bp): the cases -- the smallest at
which each path of the kernels can go wrong -- and the numpy mirror diagnostics.trw_iterate in float64 and in
np.longdouble, whose difference is the rule's own rounding noise.  Shared by tests/test_trw_cpu.py and
tests/test_trw_gpu.py; the models and tables are those of tests/bp.py."""

import ctypes as C
import functools

import numpy as np

import bp
from numbskull_amd import _lib
from numbskull_amd.diagnostics import trw_iterate, trw_log_z, edge_appearance

ITERS = (1, 2, 30)
EPS = 2.0 ** -52
WIDER = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def grid3():
    """3 x 3 binary Ising grid, weight 0.8, a unary field on every variable: cycles, degrees 3 to 5, 2 x 2 tables"""
    at = lambda r, c: 3 * r + c                                                  # noqa: E731
    f = [(3, [at(r, c), at(r, c + 1)], [0, 0], 0.8) for r in range(3) for c in range(2)]
    f += [(3, [at(r, c), at(r + 1, c)], [0, 0], 0.8) for r in range(2) for c in range(3)]
    # (fields of -3 .. 3: under weaker ones the damped iteration needs more than 200 iterations for a residual of 1e-12)
    f += [(4, [v], [0], float((v * 5) % 7 - 3)) for v in range(9)]
    return bp.spec_graph([2] * 9, [0] * 9, [0] * 9, f)


_TRI_PAIRS = [(12, [0, 1], [1, 2], 0.9), (14, [1, 2], [1, 2], -0.8), (12, [2, 0], [3, 0], 0.6), (15, [0], [2], 0.5),
              (15, [2], [4], -0.4)]


def tri_pair():
    """a 3-cycle of variables of cardinality 3, 4 and 5, pairwise factors and two unary ones"""
    return bp.spec_graph([3, 4, 5], [0] * 3, [0, 1, 2], _TRI_PAIRS)


def tri(evidence=False):
    """... with a fourth variable of cardinality 4 on the cycle's last, an arity-3 factor over the cycle (60 entries) and
    one over variables 1, 2, 3 (80 entries: past a wave's 64 lanes); with ``evidence`` variable 2 is held, so those
    tables' axes are fewer than their members"""
    f = _TRI_PAIRS + [(14, [2, 3], [0, 3], 0.7), (12, [0, 1, 2], [1, 2, 3], 0.75), (14, [1, 2, 3], [0, 1, 2], -0.65)]
    return bp.spec_graph([3, 4, 5, 4], [0, 0, int(evidence), 0], [0, 1, 2, 3], f)


def big():
    """two variables, one of cardinality NSK_ZLOCAL + 1: the variable phase's walk with its sums in memory"""
    return bp.spec_graph([17, 2], [0, 0], [0, 0], [(12, [0, 1], [5, 1], 0.9), (15, [0], [3], 0.6), (4, [1], [0], -0.3)])


GRAPHS = {"grid3": grid3, "star7": bp.star7, "tri": tri, "tri_ev": lambda: tri(True), "big": big, "tri_pair": tri_pair}
CASES = ("grid3", "star7", "tri", "tri_ev", "big")
BOUND = ("grid3", "tri_pair")           # pairwise with a cycle: the "trees" rho is below 1 somewhere


@functools.lru_cache(maxsize=None)
def model(name):
    return bp.Model(GRAPHS[name]()) if name in GRAPHS else bp.model(name)


def rho_of(name, kind="mixed"):
    """``mixed``: weights between 0.55 and 1 that differ from factor to factor; ``trees``: edge_appearance; ``one``"""
    nf = len(model(name).layout["table_off"]) - 1
    if kind == "trees":
        return edge_appearance(model(name).layout, 16, 3)
    return np.ones(nf) if kind == "one" else 0.55 + 0.45 * ((np.arange(nf) * 7) % 5) / 4.0


@functools.lru_cache(maxsize=None)
def mirror(name, iters, damping=0.0, kind="mixed", tol=0.0, dtype=np.float64):
    """the mirror's cold run of a case with its log_z (computed once, shared, left unchanged)"""
    m = model(name)
    rho = rho_of(name, kind)
    r = trw_iterate(m.layout, m.theta, rho, iters, damping, tol, dtype)
    r["log_z"] = trw_log_z(m.layout, m.theta, rho, r["factor_beliefs"], r["beliefs"], dtype)
    return r


def bound(name, key, iters, damping, kind="mixed", tol=0.0):
    """what the device may differ by from the float64 mirror in array ``key``: 16 x the largest difference between the
    float64 and the extended-precision run of the mirror, plus 16 x 2^-52"""
    if not WIDER:       # np.longdouble is float64 here: no spread to measure
        return 16 * EPS * iters
    a, b = mirror(name, iters, damping, kind, tol)[key], mirror(name, iters, damping, kind, tol, np.longdouble)[key]
    return 16 * float(np.max(np.abs(np.asarray(a, np.longdouble) - b))) + 16 * EPS


def plan(fg, sample_evidence=0):
    """nsk_bp_trw_plan: (counts, route per factor, LDS doubles a wave)"""
    desc, keep = fg._descriptor()
    counts, route, lds = np.zeros(2, np.int64), np.zeros(len(fg.factor), np.int32), C.c_int64(0)
    _lib.check(_lib.lib().nsk_bp_trw_plan(C.byref(desc), int(sample_evidence), _lib.ptr(counts), _lib.ptr(route), C.byref(lds)))
    return counts.tolist(), route, lds.value
