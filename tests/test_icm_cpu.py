"""Host side of the greedy MAP search (FactorGraph.icm / map_estimate, nsk_icm): the rule numbskull_amd.diagnostics.icm_choice
on hand-written potentials, the host ICM the GPU tests hold the device to (tests/icm.py: the oracle's potential(), the
colouring of FactorGraph.plan() and icm_choice) on a graph small enough to enumerate, the argument errors raised before a
device is touched, and the export of the entry point (no GPU)."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from numbskull_amd import _lib
from numbskull_amd.diagnostics import icm_choice
from icm import host_icm, joint_exponent
from test_conditionals_cpu import evidence_grid, six_variables
from util import REPO, session, oracle_of

NAN = float("nan")


def test_icm_choice_rule_table():
    #        variable: 0 improves  1 tie with the   2 tie of two     3 NaN never   4 outside its   5 one    6 NaN
    #                  strictly    incumbent        others           wins          domain          value    incumbent
    pot = [[0.1, 0.7], [0.5, 0.5], [0.2, 0.9, 0.9], [0.3, NAN, 0.1], [0.4, 0.4, 0.2], [1.5], [NAN, 2.0]]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pot])])
    flat = np.concatenate(pot)
    cur = np.array([0, 1, 0, 2, 7, 0, 0])
    want = np.array([1, 1, 1, 0, 0, 0, 0])
    got = icm_choice(off, flat, cur)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    # the incumbent decides a tie, whichever it is; a negative value starts from 0 as well
    assert np.array_equal(icm_choice(off, flat, [1, 0, 2, 0, -1, 0, 1]), [1, 0, 2, 0, 0, 0, 1])
    # from value 1 (NaN) of variable 3 nothing compares greater: the incumbent stays
    assert np.array_equal(icm_choice([0, 3], [0.3, NAN, 0.1], [1]), [1])
    # an out-of-domain incumbent starts from 0 and still moves on strict improvement
    assert np.array_equal(icm_choice([0, 3], [0.1, 0.2, 0.9], [5]), [2])
    # a stack of states goes through in one call, and the inputs are left alone
    both = icm_choice(off, np.stack([flat, flat]), np.stack([cur, [1, 0, 2, 0, -1, 0, 1]]))
    assert np.array_equal(both, [want, [1, 0, 2, 0, 0, 0, 1]]) and cur[4] == 7
    assert icm_choice([0], np.zeros(0), np.zeros(0, np.int64)).shape == (0,)
    for bad_off, p, x in (([0, 2, 5], np.zeros(4), [0, 0]), ([0, 2, 5], np.zeros(5), [0]), ([0, 2], np.zeros(2), [0.5])):
        with pytest.raises(ValueError):
            icm_choice(bad_off, p, x)


def _grid():
    _, fg = session(evidence_grid())
    og = oracle_of(fg, layout=False)
    color, _ = fg.plan()
    assert og.check_coloring(color) == (-1, -1)
    w = og.weight["initialValue"].astype(np.float64).copy()
    return fg, og, color, w


def test_host_icm_on_the_evidence_grid_reaches_local_maxima():
    """3 x 4 Ising grid, weight 0.5, variables 0, 5, 11 evidence at 1, 0, 1: every potential is a sum of halves, so the
    comparisons below are exact"""
    fg, og, color, w = _grid()
    base = og.variable["initialValue"].astype(np.int64)
    free = np.nonzero(og.variable["isEvidence"] == 0)[0]
    assert len(free) == 9
    rng = np.random.default_rng(2024)
    for _ in range(20):
        x0 = base.copy()
        x0[free] = rng.integers(0, 2, len(free))
        lps = [joint_exponent(og, x0, w)]
        x, sweeps, changed = host_icm(og, color, x0, w, 50, on_sweep=lambda s: lps.append(joint_exponent(og, s, w)))
        assert 1 <= sweeps <= 50 and changed[sweeps - 1] == 0 and (changed[:sweeps - 1] > 0).all()      # it converges
        assert np.array_equal(x[[0, 5, 11]], [1, 0, 1])                                                   # evidence stays
        assert (np.diff(lps) >= 0).all(), lps                                                             # never downhill
        assert (np.diff(lps)[:sweeps - 1] > 0).all()                                                      # a change is a gain
        for v in free:                                      # no single-variable change of a free variable raises it
            y = x.copy()
            y[v] = 1 - y[v]
            assert joint_exponent(og, y, w) <= lps[-1]
        # a second run from the fixed point changes nothing
        again, s2, c2 = host_icm(og, color, x, w, 5)
        assert s2 == 1 and not c2.any() and np.array_equal(again, x)
    # sample_evidence makes the evidence variables eligible too
    x, sweeps, _ = host_icm(og, color, base, w, 50, sample_evidence=True)
    assert sweeps > 0
    lp = joint_exponent(og, x, w)
    for v in range(len(x)):
        y = x.copy()
        y[v] = 1 - y[v]
        assert joint_exponent(og, y, w) <= lp


def test_host_icm_leaves_the_global_map_alone():
    fg, og, color, w = _grid()
    base = og.variable["initialValue"].astype(np.int64)
    free = np.nonzero(og.variable["isEvidence"] == 0)[0]
    best, best_lp = None, -np.inf
    for s in range(1 << len(free)):
        x = base.copy()
        x[free] = (s >> np.arange(len(free))) & 1
        lp = joint_exponent(og, x, w)
        if lp > best_lp:
            best, best_lp = x, lp
    x, sweeps, changed = host_icm(og, color, best, w, 10)
    assert sweeps == 1 and not changed.any() and np.array_equal(x, best)


def test_host_icm_on_categorical_variables_converges_to_a_fixed_point():
    """cardinalities 2, 3, 4, dataType 0 and 1 (test_conditionals_cpu.six_variables: potential() there is the joint's
    exponent up to a constant, so ICM is coordinate ascent on one energy)"""
    _, fg = session(six_variables())
    og = oracle_of(fg, layout=False)
    color, _ = fg.plan()
    w = og.weight["initialValue"].astype(np.float64).copy()
    card = og.variable["cardinality"].astype(np.int64)
    rng = np.random.default_rng(7)
    for _ in range(10):
        x0 = (rng.random(len(card)) * card).astype(np.int64)
        lps = [joint_exponent(og, x0, w)]
        x, sweeps, changed = host_icm(og, color, x0, w, 50, on_sweep=lambda s: lps.append(joint_exponent(og, s, w)))
        assert sweeps > 0 and (np.diff(lps) >= -1e-12).all()
        for v in range(len(card)):
            for k in range(card[v]):
                y = x.copy()
                y[v] = k
                assert joint_exponent(og, y, w) <= lps[-1] + 1e-12


def test_argument_errors_come_before_the_device():
    _, fg = session(six_variables())
    for bad in (0, -3, 4097):
        with pytest.raises(ValueError):
            fg.icm(max_sweeps=bad)
    with pytest.raises(ValueError):
        fg.icm(var_copy="all", evidence_chain=True)
    with pytest.raises(ValueError):
        fg.map_estimate(10, thin=0)
    with pytest.raises(ValueError):
        fg.map_estimate(3, thin=4)                      # no row would be recorded
    assert fg._handle is None


def test_header_declares_and_library_exports_the_entry_point():
    hdr = open(os.path.join(REPO, "include", "numbskull_amd.h")).read()
    assert re.search(r"\bint nsk_icm\(nsk_graph \*g, int which, int64_t first_chain, int64_t nchains,\s*int64_t max_sweeps, "
                     r"int sample_evidence,\s*int64_t \*sweeps[^,]*, int64_t \*changed", hdr)
    assert "nsk_icm" in _lib.SYMBOLS
    assert hasattr(C.CDLL(_lib.LIB_PATH), "nsk_icm")
    assert _lib.lib().nsk_icm.argtypes == [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
