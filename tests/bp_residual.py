"""The host side of the residual-schedule tests: the graphs beyond those of tests/bp.py and the runs of the mirror
diagnostics.rbp_iterate, shared by tests/test_bp_residual_cpu.py and tests/test_bp_residual_gpu.py."""

import functools

import numpy as np

import bp
from numbskull_amd.diagnostics import rbp_iterate, bp_factor_beliefs
from oracle import binding as orc


def spin_grid(rows, cols, seed, J, clamp_every=0):
    """binary grid: EQUAL of weight N(0, J) between neighbours, ISTRUE of N(0, 0.1) a variable; every clamp_every-th clamped"""
    rng = np.random.default_rng(seed)
    n = rows * cols
    f = []
    for r in range(rows):
        for c in range(cols):
            v = r * cols + c
            if c + 1 < cols:
                f.append((3, [v, v + 1], [0, 0], float(rng.normal(0, J))))
            if r + 1 < rows:
                f.append((3, [v, v + cols], [0, 0], float(rng.normal(0, J))))
    f += [(4, [v], [0], float(rng.normal(0, 0.1))) for v in range(n)]
    ev = [1 if clamp_every and v % clamp_every == 0 else 0 for v in range(n)]
    return bp.spec_graph([2] * n, ev, [(v // max(clamp_every, 1)) % 2 if ev[v] else 0 for v in range(n)], f)


def cat17():
    """cardinalities 3 and 17 either side of the lane-private vectors' 16, a ternary AND_CAT, cycles through pairs"""
    cards = [3, 17, 2, 3, 17]
    f = [(12, [0, 1, 2], [1, 5, 1], 0.9), (14, [0, 3], [2, 1], -0.7), (12, [3, 4], [0, 16], 0.8), (14, [4, 1], [3, 3], 0.6),
         (12, [1, 3], [2, 2], -0.5), (15, [0], [1], 0.4), (15, [1], [7], -0.6), (15, [4], [2], 0.5), (4, [2], [0], 0.3),
         (14, [2, 3], [1, 0], 0.45)]
    return bp.spec_graph(cards, [0] * 5, [0] * 5, f)


def hubs():
    """binary variable 0 has seven edges, variable 1 six (either side of the register walk); leaves 2 .. 6 hang on both"""
    f = [(3, [0, v], [0, 0], w) for v, w in zip(range(2, 8), (0.9, -0.6, 0.5, -0.8, 0.7, 0.4))]
    f += [(3, [1, v], [0, 0], w) for v, w in zip(range(2, 7), (-0.5, 0.8, 0.6, -0.9, 0.3))]
    f += [(4, [0], [0], -0.45), (4, [1], [0], 0.35)] + [(4, [v], [0], 0.1 * v - 0.4) for v in range(2, 8)]
    return bp.spec_graph([2] * 8, [0] * 8, [0] * 8, f)


# name -> (graph builder, head_by_vid, sample_evidence): held to the mirror (CASES), to flooding at frac = 0 (FLOOD)
CASES = {
    "grid5": (lambda: spin_grid(5, 5, 3, 1.0), False, 0),
    "cat17": (cat17, False, 0),
    "hubs": (hubs, False, 0),
    "grid_int32": bp.CASES["grid_int32"],
    "trips": (bp.trips_grid, False, 0),
}
FLOOD = {
    "mixed_free": bp.CASES["mixed_free"],
    "grid6": (lambda: spin_grid(6, 6, 5, 0.8, clamp_every=3), False, 0),
}


@functools.lru_cache(maxsize=None)
def model(name):
    if name in bp.CASES or name == "trips":
        return bp.model(name)
    build, hbv, sev = (CASES.get(name) or FLOOD[name])
    return bp.Model(build(), hbv, sev)


def run(m, rounds, frac, damping=0.0, tol=0.0, messages=None):
    r = rbp_iterate(m.layout, m.theta, rounds, frac, damping, tol, exp=orc.exp_det, messages=messages)
    r["factor_beliefs"] = bp_factor_beliefs(m.layout, r["psi"], r["v2f"])
    return r


@functools.lru_cache(maxsize=None)
def mirror(name, rounds, frac, damping=0.0, tol=0.0):
    return run(model(name), rounds, frac, damping, tol)
