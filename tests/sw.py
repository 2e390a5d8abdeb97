"""The host side of the Swendsen-Wang tests (nsk_sw_setup / nsk_sw_sweeps, FactorGraph.swendsen_wang): the cases and the
uniforms of streams 4 and 5, shared by tests/test_sw_cpu.py (the plan, the rule against the model) and tests/test_sw_gpu.py
(the device against diagnostics.sw_tables / sw_step, bit for bit)."""

import numpy as np

import bp
from numbskull_amd import _lib
from oracle import binding as orc

EQUAL, ISTRUE, IMPLY, OR, AND = 3, 4, 0, 1, 2
SEED = 41


def pairwise(n, bonds, fields, evid=(), seed=1):
    """binary variables, random initial values; bonds [(function, u, v, weight)], fields [(v, weight)] as ISTRUE,
    evid {variable: value} clamped"""
    f = [(fn, [u, v], [0, 0], w) for fn, u, v, w in bonds] + [(ISTRUE, [v], [0], w) for v, w in fields]
    init = np.random.default_rng(seed).integers(0, 2, n)
    ev = np.zeros(n, np.int64)
    for v, x in dict(evid).items():
        ev[v], init[v] = 1, x
    return bp.spec_graph([2] * n, ev, init, f)


def grid(rows, cols, w, field=0.3, seed=1):
    """EQUAL bonds of weight w to the right and down, an ISTRUE field of N(0, field) on every third variable"""
    rng = np.random.default_rng(seed)
    at = lambda r, c: r * cols + c        # noqa: E731
    bonds = [(EQUAL, at(r, c), at(r, c + 1), w) for r in range(rows) for c in range(cols - 1)]
    bonds += [(EQUAL, at(r, c), at(r + 1, c), w) for r in range(rows - 1) for c in range(cols)]
    return pairwise(rows * cols, bonds, [(v, float(rng.normal(0, field))) for v in range(0, rows * cols, 3)], seed=seed)


def mixed(n=30):
    """IMPLY / AND / OR / EQUAL pairs of either sign, a frustrated triangle (0, 1, 2), evidence members 3 and 7 clamped,
    variable n - 2 with fields only, variable n - 1 in no factor.  Weights are multiples of 1 / 16: H is h exactly."""
    fns, ws = (IMPLY, AND, OR, EQUAL), (0.75, -0.5, 1.25, -0.875, 0.4375)
    bonds = [(EQUAL, 0, 1, -1.0), (EQUAL, 1, 2, -1.0), (EQUAL, 2, 0, -1.0)]
    bonds += [(fns[i % 4], i, (i * 5 + 3) % (n - 2), ws[i % 5]) for i in range(n - 2) if i != (i * 5 + 3) % (n - 2)]
    bonds += [(fns[(i + 1) % 4], i, i + 1, ws[(i + 2) % 5]) for i in range(2, n - 3)]
    return pairwise(n, bonds, [(n - 2, 0.5), (n - 2, -1.25), (4, 0.25), (3, 0.5)], evid={3: 1, 7: 0}, seed=2)


# name -> (graph builder, head_by_vid, sample_evidence, chains)
CASES = {
    "grid5x7": (lambda: grid(5, 7, 0.44), False, 0, 1),
    "grid40": (lambda: grid(40, 40, 0.44), False, 0, 3),
    "path3000": (lambda: grid(1, 3000, 3.0), False, 0, 1),
    "mixed": (mixed, False, 0, 3),
    "grid_int32": bp.CASES["grid_int32"] + (1,),
}


def uniforms(seed, chain, sweep, stream, n, device=False):
    """u(c, stream) for c < n of chain `chain` at sweep index `sweep`: ((x >> 5) << 26 | y >> 6) * 2^-53 from words x, y"""
    key, m32 = seed ^ (chain << 32), 0xffffffff
    w = np.zeros((max(n, 1), 4), np.uint32)
    if device:
        _lib.check(_lib.lib().nsk_selftest_philox(0, key, sweep, stream, n, _lib.ptr(w)))
    else:
        w[:n] = [orc.philox(key & m32, key >> 32, c, stream, sweep & m32, sweep >> 32) for c in range(n)]
    w = w[:n].astype(np.uint64)
    return (((w[:, 0] >> np.uint64(5)) << np.uint64(26)) | (w[:, 1] >> np.uint64(6))).astype(np.float64) * 2.0 ** -53
