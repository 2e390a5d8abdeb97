"""The host side of the dual MAP bound tests (nsk_bp_dual_run, FactorGraph.map_dual): the mirror diagnostics.msd_iterate over
tests/bp_map.py's cases, its classes from the host-only plan, and the enumerated optimum's summed theta.  Shared by
tests/test_map_dual_cpu.py and tests/test_map_dual_gpu.py."""

import ctypes as C
import functools
import math

import numpy as np

import bp
import bp_map
from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import ms_decode, msd_iterate, msd_terms


def grid40():
    """40 x 40 binaries, no evidence: 800 lane items a class, four trips of one block of 256"""
    return graphgen.ising_grid(40, 40, weight=0.4)


@functools.lru_cache(maxsize=None)
def model(name):
    return bp.Model(grid40()) if name == "grid40" else bp_map.model(name)


def plan(name):
    """nsk_bp_dual_plan of a case: (counts, route per variable, class per variable, LDS doubles a wave)"""
    m = model(name)
    desc, keep = m.fg._descriptor()
    nv = len(m.fg.variable)
    counts, route, cls, lds = np.zeros(2, np.int64), np.zeros(nv, np.int32), np.zeros(nv, np.int32), C.c_int64(0)
    _lib.check(_lib.lib().nsk_bp_dual_plan(C.byref(desc), int(m.sev), _lib.ptr(counts), _lib.ptr(route), _lib.ptr(cls), C.byref(lds)))
    return counts.tolist(), route, cls, lds.value


@functools.lru_cache(maxsize=None)
def mirror(name, sweeps, tol=0.0, bounds=False):
    """the mirror's cold run of a case with its terms and decode (computed once, shared, left unchanged)"""
    m = model(name)
    r = msd_iterate(m.layout, m.theta, plan(name)[2], sweeps, tol, bounds)
    r["tf"], r["tv"], r["Bv"] = msd_terms(m.layout, m.theta, r["D"])
    r["decode"] = ms_decode(m.layout, r["Bv"], m.x)
    return r


def best(name):
    """(the enumerated MAP assignment, its summed theta, the margin 1e-9 (1 + |that|)): sums of tens of terms of order
    10 round below 1e-13, so the margin cannot hide a wrong update"""
    m = model(name)
    L = m.layout
    x = bp_map.enumerate_map(name)[0]
    total = math.fsum(m.theta[L["table_off"][f] + (np.ravel_multi_index([x[v] for v in ax], sh) if ax else 0)]
                      for f, (ax, sh) in enumerate(zip(L["axes"], L["shapes"])))
    return x, total, 1e-9 * (1.0 + abs(total))
