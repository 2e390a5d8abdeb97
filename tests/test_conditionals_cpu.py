"""Host side of the conditionals (FactorGraph.conditionals / log_pseudo_likelihood / rao_blackwell): what the numpy twin
in numbskull_amd.diagnostics MEANS -- conditional_probabilities on the oracle's potentials against the ratio of joint
probabilities from brute-force eval_factor sums -- log_pseudo_likelihood, tally_layout, and the argument errors of the
three methods, which are raised before a device is touched (no GPU)."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import conditional_probabilities, log_pseudo_likelihood, tally_layout
from numbskull_amd.numbskulltypes import Weight, Variable, Factor, FactorToVar
from util import REPO, orc, session, oracle_of

NEW = ["nsk_conditionals", "nsk_trace_conditionals", "nsk_trace_download_conditionals"]


def evidence_grid():
    """the small graph of the statistical check: a 3 x 4 Ising grid, weight 0.5, variables 0, 5, 11 evidence at 1, 0, 1"""
    g = list(graphgen.ising_grid(3, 4, weight=0.5))
    var = g[1].copy()
    var["isEvidence"][[0, 5, 11]] = 1
    var["initialValue"][[0, 5, 11]] = [1, 0, 1]
    g[1] = var
    return tuple(g)


def six_variables():
    """Cardinalities 2, 3, 4; EQUAL, AND, OR and ISTRUE on the binary members, AND_CAT on the others; dataType 0 and 1; no
    IMPLY head.  (A dataType-1 variable lists under value k only the factors whose edge names k; AND_CAT is 0 wherever
    an edge's value differs, so the listed factors are all that depend on the variable and potential() is the joint's
    exponent up to a constant.)"""
    variable = np.zeros(6, Variable)
    variable["cardinality"] = [2, 2, 2, 3, 4, 3]
    variable["dataType"] = [0, 0, 0, 1, 1, 0]
    variable["initialValue"] = [1, 0, 1, 2, 3, 1]
    spec = [(3, [0, 1], [0, 0]), (2, [0, 1, 2], [0, 0, 0]), (1, [1, 2], [0, 0]), (4, [2], [0]), (4, [0], [0]),
            (12, [3, 4], [2, 3]), (12, [3, 4], [0, 1]), (12, [4, 5], [3, 1]), (12, [3, 5], [1, 2]), (12, [3], [2]),
            (12, [5, 4, 3], [0, 2, 1]), (12, [2, 3], [1, 2]), (12, [4], [0]), (12, [5], [1])]
    nedge = sum(len(m) for _, m, _ in spec)
    factor, fmap = np.zeros(len(spec), Factor), np.zeros(nedge, FactorToVar)
    e = 0
    for i, (fn, members, deos) in enumerate(spec):
        factor[i] = (fn, i % 5, 1.0, len(members), e)
        for m, dq in zip(members, deos):
            fmap[e] = (m, dq)
            e += 1
    weight = np.zeros(5, Weight)
    weight["initialValue"] = [0.7, -0.4, 1.3, 0.25, -0.9]
    return weight, variable, factor, fmap, np.zeros(6, np.bool_), nedge


GRAPHS = {"evidence_grid": evidence_grid, "six_variables": six_variables}


def oracle_potentials(og, x, w):
    card = og.variable["cardinality"].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(card)]).astype(np.int64)
    pot = np.zeros(int(off[-1]))
    for v in range(len(card)):
        for k in range(card[v]):
            rc, pot[off[v] + k] = og.potential(v, k, x, w)
            assert rc == 0
    return off, pot


def joint_exponent(og, x, w):
    e = 0.0
    for fid in range(len(og.factor)):
        rc, val = og.eval_factor(fid, -1, 0, x)
        assert rc == 0
        e += w[int(og.factor[fid]["weightId"])] * val
    return e


def states(og, n=6):
    rng = np.random.default_rng(41)
    card = og.variable["cardinality"].astype(np.int64)
    yield og.variable["initialValue"].astype(np.int64).copy()
    for _ in range(n):
        yield (rng.random(len(card)) * card).astype(np.int64)


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_the_twin_is_the_ratio_of_joint_probabilities(name):
    ns, fg = session(GRAPHS[name]())
    og = oracle_of(fg, layout=False)
    w = og.weight["initialValue"].astype(np.float64).copy()
    card = og.variable["cardinality"].astype(np.int64)
    for x in states(og):
        off, pot = oracle_potentials(og, x, w)
        P = conditional_probabilities(off, pot, exp=orc.exp_det)
        for v in range(len(card)):
            ex = np.zeros(card[v])
            for k in range(card[v]):
                y = x.copy()
                y[v] = k
                ex[k] = joint_exponent(og, y, w)
            joint = np.exp(ex - ex.max())
            assert np.abs(P[off[v]:off[v + 1]] - joint / joint.sum()).max() <= 1e-12, (name, v)
        assert np.abs(np.add.reduceat(P, off[:-1]) - 1.0).max() <= 1e-15 * 8
        # numpy's exp agrees to rounding, and a stack of states goes through in one call
        assert np.abs(conditional_probabilities(off, pot) - P).max() <= 1e-15
        both = conditional_probabilities(off, np.stack([pot, pot[::-1].copy()]), exp=orc.exp_det)
        assert both.shape == (2, len(pot)) and np.array_equal(both[0], P)


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_log_pseudo_likelihood_sums_the_logs_of_the_conditionals(name):
    ns, fg = session(GRAPHS[name]())
    og = oracle_of(fg, layout=False)
    w = og.weight["initialValue"].astype(np.float64).copy()
    sel = np.array([4, 1, 1, 3, 0])                     # any order, repeats
    for x in states(og):
        off, pot = oracle_potentials(og, x, w)
        P = conditional_probabilities(off, pot, exp=orc.exp_det)
        assert abs(log_pseudo_likelihood(off, pot, x) - np.log(P[off[:-1] + x]).sum()) <= 1e-12
        soff = np.concatenate([[0], np.cumsum(np.diff(off)[sel])])
        spot = np.concatenate([pot[off[v]:off[v + 1]] for v in sel])
        assert abs(log_pseudo_likelihood(soff, spot, x[sel]) - np.log(P[off[sel] + x[sel]]).sum()) <= 1e-12
        two = log_pseudo_likelihood(off, np.stack([pot, pot]), np.stack([x, x]))
        assert two.shape == (2,) and two[0] == two[1] == log_pseudo_likelihood(off, pot, x)
    # the shift: potentials beyond exp's range still give a finite score
    assert abs(log_pseudo_likelihood([0, 2], [800.0, 799.0], [0]) - (-np.log1p(np.exp(-1.0)))) <= 1e-12
    assert np.isnan(log_pseudo_likelihood([0, 2, 4], [0.1, 0.2, np.nan, np.nan], [1, 0]))      # a variable without a position


def test_tally_layout_lines_up_with_cstart():
    ns, fg = session(six_variables())
    card = fg.variable["cardinality"].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(card)])
    full = np.arange(int(off[-1]), dtype=np.float64) + 0.5
    toff, t = tally_layout(off, full)
    assert np.array_equal(toff, fg.cstart) and t.shape == fg.count.shape
    for v in range(len(card)):
        want = full[off[v] + 1:off[v + 1]] if card[v] == 2 else full[off[v]:off[v + 1]]
        assert np.array_equal(t[toff[v]:toff[v + 1]], want)
    toff2, t2 = tally_layout(off, np.stack([full, 2 * full]))
    assert np.array_equal(toff2, toff) and np.array_equal(t2[1], 2 * t)
    assert tally_layout([0], np.zeros(0))[1].shape == (0,)


def test_the_twin_refuses_what_is_not_a_full_layout():
    for f in (conditional_probabilities, tally_layout):
        for off, x in (([0, 2, 5], np.zeros(4)), ([1, 3], np.zeros(3)), ([0, 2, 2], np.zeros(2)), ([[0, 2]], np.zeros(2)),
                       ([0.0, 2.0], np.zeros(2))):
            with pytest.raises(ValueError):
                f(off, x)
    with pytest.raises(ValueError):
        log_pseudo_likelihood([0, 2, 5], np.zeros(5), [0, 3])       # a value outside its domain
    with pytest.raises(ValueError):
        log_pseudo_likelihood([0, 2, 5], np.zeros(5), [0])          # one value per selected variable
    with pytest.raises(ValueError):
        log_pseudo_likelihood([0, 2, 5], np.zeros(5), [0.0, 1.0])


def test_argument_errors_come_before_the_device():
    ns, fg = session(six_variables())
    nvar = len(fg.variable)
    for call in (lambda ids: fg.conditionals(ids), lambda ids: fg.log_pseudo_likelihood(ids), lambda ids: fg.rao_blackwell(4, ids)):
        for bad in ([nvar], [0, -1], np.array([2, 10 ** 12])):
            with pytest.raises(IndexError):
                call(bad)
        for bad in ([[0, 1]], [0.5], np.zeros((2, 2), np.int64), 3):
            with pytest.raises(ValueError):
                call(bad)
    for call in (fg.conditionals, fg.log_pseudo_likelihood):
        with pytest.raises(ValueError):
            call(var_copy="all", evidence_chain=True)
    for thin in (0, -2):
        with pytest.raises(ValueError):
            fg.rao_blackwell(4, thin=thin)
    with pytest.raises(ValueError):
        fg.rao_blackwell(-1)
    assert fg._handle is None                           # nothing above reached the device
    # an empty selection needs none either
    off, vals = fg.conditionals([])
    assert off.tolist() == [0] and vals.shape == (0,) and fg._handle is None


def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(REPO, "include", "numbskull_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(nsk_graph \*g" % name, hdr), name
        assert name in _lib.SYMBOLS
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
