"""The host side of the max-product tests: the cases beyond tests/bp.py, the mirror diagnostics.ms_iterate over bp.py's
theta tables and plain enumeration of the trees, shared by tests/test_bp_map_cpu.py and tests/test_bp_map_gpu.py."""

import functools

import numpy as np

import bp
from numbskull_amd.diagnostics import ms_iterate
from numbskull_amd.numbskulltypes import Weight

TREES = ("chain9", "star", "star7", "tree")
CASES = ("chain9", "clamped_grid", "mixed_free", "grid_int32") + TREES[1:] + ("routes",)


def untied(g):
    """a copy with one weight per factor, all different: the stock chain's single weight ties its MAP"""
    g = list(g)
    nf = len(g[2])
    w = np.zeros(nf, Weight)
    w["isFixed"] = True
    w["initialValue"] = [(0.8 + 0.07 * i) * (-1.0 if i % 5 == 3 else 1.0) for i in range(nf)]
    f = g[2].copy()
    f["weightId"] = np.arange(nf)
    g[0], g[2] = w, f
    return tuple(g)


def tree():
    """bp.tree with unary factors on variable 2 and the cardinality-3 members: the stock tree leaves them indifferent"""
    cards = [2, 2, 2, 3, 3, 2, 3]
    f = [(2, [0, 1, 2], [0, 0, 0], 1.3), (12, [2, 3], [1, 0], 0.9), (14, [3, 4], [1, 2], -0.8), (4, [0], [0], 0.4),
         (15, [4], [0], 0.7), (3, [5, 1], [0, 0], 0.6), (14, [4, 6], [2, 1], 0.5), (4, [5], [0], -0.3),
         (15, [3], [2], 0.33), (15, [3], [1], 0.12), (15, [4], [1], 0.21), (4, [2], [0], 0.27)]
    return bp.spec_graph(cards, [0, 0, 0, 0, 0, 0, 1], [0, 1, 0, 2, 0, 1, 1], f)


def routes_graph():
    """T = 4096 over 12 free binaries, 64 = 2^6, 63 = 7 x 9, 81 = 3^4, 68 = 17 x 4 and 34 = 17 x 2 on the wave route; pairwise
    binary, 3 x 3, 7 x 3 and 9 x 4 on the lane route; cardinality 600 alone and beside a binary axis on the edge route"""
    cards = [2] * 16 + [7, 9, 3, 3, 3, 3, 17, 4, 600]
    evid = [0] * 12 + [1] * 4 + [0] * 9
    init = [0] * 12 + [1] * 4 + [0] * 9
    f = [(2, list(range(16)), [0] * 16, 0.5), (2, list(range(6)), [0] * 6, 0.7), (12, [16, 17], [3, 5], 1.1),
         (12, [18, 19, 20, 21], [1, 2, 0, 1], -0.9), (14, [22, 23], [11, 2], 0.6), (12, [22, 3], [7, 1], 0.3),
         (3, [0, 6], [0, 0], 0.8), (3, [1, 7], [0, 0], -0.4), (12, [18, 19], [2, 2], 0.5), (14, [20, 21], [0, 1], 0.9),
         (12, [16, 18], [2, 1], 0.4), (12, [17, 23], [4, 3], -0.6), (15, [24], [377], 1.3), (12, [24, 2], [5, 1], 0.7),
         (4, [4], [0], 0.35), (4, [8], [0], -0.25), (4, [11], [0], 0.15), (15, [16], [2], 0.5), (15, [17], [8], -0.3),
         (15, [22], [16], 0.9), (15, [23], [0], 0.2), (15, [19], [1], 0.35), (15, [24], [0], -0.2), (15, [24], [599], 0.4)]
    return bp.spec_graph(cards, evid, init, f)


def graph(name):
    if name == "routes": return routes_graph(), False, 0     # noqa: E701
    if name == "symmetric":     # two binaries tied by EQUAL and nothing else: the joint maxima are mirror images
        return bp.spec_graph([2, 2], [0, 0], [1, 1], [(3, [0, 1], [0, 0], 0.9)]), False, 0
    if name in TREES:
        return untied(tree() if name == "tree" else bp.TREES[name]()), False, 0
    build, hbv, sev = bp.CASES[name]
    return build(), hbv, sev


@functools.lru_cache(maxsize=None)
def model(name):
    return bp.model("trips") if name == "trips" else bp.Model(*graph(name))


@functools.lru_cache(maxsize=None)
def mirror(name, iters, damping=0.0, tol=0.0):
    m = model(name)
    return ms_iterate(m.layout, m.theta, iters, damping, tol)


@functools.lru_cache(maxsize=None)
def enumerate_map(name):
    """(MAP assignment, best - second best, max-marginals in the "full" layout) from every joint state's summed theta"""
    m = model(name)
    L = m.layout
    free = [v for v in range(len(L["card"])) if not L["clamped"][v]]
    states = np.indices([int(L["card"][v]) for v in free]).reshape(len(free), -1)
    col = {v: states[i] for i, v in enumerate(free)}
    total = np.zeros(states.shape[1])
    for f, (ax, shape) in enumerate(zip(L["axes"], L["shapes"])):
        idx = np.ravel_multi_index([col[v] for v in ax], shape) if ax else 0
        total = total + m.theta[L["table_off"][f] + idx]
    order = np.sort(total)
    x = m.x.copy()
    x[free] = states[:, int(np.argmax(total))]
    mm = np.zeros(int(L["offsets"][-1]))
    for v in range(len(L["card"])):
        for k in range(int(L["card"][v])):
            if L["clamped"][v]:
                mm[L["offsets"][v] + k] = 0.0 if k == m.x[v] else -np.inf
            else:
                mm[L["offsets"][v] + k] = total[col[v] == k].max() - order[-1]
    return x, float(order[-1] - order[-2]), mm
