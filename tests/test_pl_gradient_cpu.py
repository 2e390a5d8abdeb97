"""Host side of the pseudo-likelihood gradient and MPLE learning (FactorGraph.pl_gradient / learn_mple): what the numpy
twin in numbskull_amd.diagnostics MEANS -- pl_gradient_counts on the oracle's entries against central differences of
log_pseudo_likelihood -- its skips, mple_step, the argument errors of the two methods, which are raised before a device
is touched, and the planted pair model the GPU test learns from (no GPU)."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from numbskull_amd import _lib
from numbskull_amd.diagnostics import log_pseudo_likelihood, mple_step, pl_gradient_counts
from numbskull_amd.numbskulltypes import Weight, Variable, Factor, FactorToVar
from test_conditionals_cpu import GRAPHS, oracle_potentials, states
from util import REPO, session, oracle_of
import plgrad

NEW = ["nsk_pl_gradient", "nsk_mple_steps"]


def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(REPO, "include", "numbskull_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(nsk_graph \*g" % name, hdr), name
        assert name in _lib.SYMBOLS
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_the_twin_is_the_derivative_of_the_log_pseudo_likelihood(name):
    """counts * 2^-32 against central differences of diagnostics.log_pseudo_likelihood over the oracle's potentials, in
    every weight, at h = 1e-4.  The tolerance is the difference quotient's own error estimate, ten times |D(h) - D(2h)|,
    plus the quantisation bound n_terms * 2^-33 -- both from the reference side."""
    ns, fg = session(GRAPHS[name]())
    og = oracle_of(fg, layout=False)
    w = og.weight["initialValue"].astype(np.float64).copy()
    twin = plgrad.Twin(fg, og)
    n_terms = len(twin.s[1])
    h = 1e-4

    def lpl(x, wv):
        off, pot = oracle_potentials(og, x, wv)
        return log_pseudo_likelihood(off, pot, x)

    def quotient(x, i, step):
        up, dn = w.copy(), w.copy()
        up[i] += step
        dn[i] -= step
        return (lpl(x, up) - lpl(x, dn)) / (2 * step)

    for x in states(og):
        counts, skipped = twin.counts(x, w)
        assert skipped == 0 and counts.dtype == np.int64 and counts.shape == (len(w),)
        for i in range(len(w)):
            d1, d2 = quotient(x, i, h), quotient(x, i, 2 * h)
            tol = 10 * abs(d1 - d2) + n_terms * 2.0 ** -33
            assert abs(counts[i] * plgrad.Q - d1) <= tol, (name, i, counts[i] * plgrad.Q, d1, tol)


def _constant_factor_graph():
    """variable 0 with ISTRUE(0) on weight 1 and EQUAL(0, 1, 2) on weight 0; x1 != x2 makes the EQUAL constant in x0"""
    variable = np.zeros(3, Variable)
    variable["cardinality"] = 2
    variable["initialValue"] = [1, 0, 1]
    factor, fmap = np.zeros(2, Factor), np.zeros(4, FactorToVar)
    factor[0] = (3, 0, 1.0, 3, 0)
    factor[1] = (4, 1, 1.0, 1, 3)
    fmap["vid"] = [0, 1, 2, 0]
    weight = np.zeros(2, Weight)
    weight["initialValue"] = [0.8, -0.3]
    return weight, variable, factor, fmap, np.zeros(3, np.bool_), 4


def test_a_weight_whose_factors_do_not_depend_on_the_variable_gets_zero():
    ns, fg = session(_constant_factor_graph())
    og = oracle_of(fg, layout=False)
    w = og.weight["initialValue"].astype(np.float64).copy()
    twin = plgrad.Twin(fg, og, [0])
    for x0 in (0, 1):
        counts, skipped = twin.counts(np.array([x0, 0, 1]), w)
        assert skipped == 0 and counts[0] == 0 and counts[1] != 0         # sum_k c_k e with e constant
    counts, _ = twin.counts(np.array([1, 1, 1]), w)                       # ... and where it does depend on it, it counts
    assert counts[0] != 0


def test_a_value_outside_its_domain_is_skipped_and_counted():
    ns, fg = session(GRAPHS["six_variables"]())
    og = oracle_of(fg, layout=False)
    w = og.weight["initialValue"].astype(np.float64).copy()
    x = og.variable["initialValue"].astype(np.int64).copy()
    off, ev, ek, ef, ew = plgrad.structure(fg, np.arange(6))
    _, prob = plgrad.probabilities(og, np.arange(6), off, x, w)
    ee = plgrad.entry_values(og, np.arange(6), (off, ev, ek, ef, ew), x)
    full, s0 = pl_gradient_counts(off, prob, x, ev, ek, ew, ee, len(w))
    assert s0 == 0
    bad = x.copy()
    bad[3] = 3                                                           # cardinality 3
    got, s1 = pl_gradient_counts(off, prob, bad, ev, ek, ew, ee, len(w))
    keep = ev != 3
    rest, _ = pl_gradient_counts(off, prob, x, ev[keep], ek[keep], ew[keep], ee[keep], len(w))
    assert s1 == 1 and np.array_equal(got, rest) and not np.array_equal(got, full)
    neg = x.copy()
    neg[3] = -1
    assert pl_gradient_counts(off, prob, neg, ev, ek, ew, ee, len(w))[1] == 1
    # a normaliser that is not a finite positive number shows in the probabilities: NaN, or nothing positive
    for p3 in ([np.nan, 0.5, 0.5], [0.0, 0.0, 0.0]):
        pr = prob.copy()
        pr[off[3]:off[4]] = p3
        got, s = pl_gradient_counts(off, pr, x, ev, ek, ew, ee, len(w))
        assert s == 1 and np.array_equal(got, rest)
    with pytest.raises(ValueError):
        pl_gradient_counts(off, np.stack([prob, prob]), x, ev, ek, ew, ee, len(w))
    with pytest.raises(IndexError):
        pl_gradient_counts(off, prob, x, ev, ek, ew + len(w), ee, len(w))
    assert pl_gradient_counts([0], np.zeros(0), np.zeros(0, np.int64), [], [], [], [], 4)[0].tolist() == [0, 0, 0, 0]


def test_mple_step_is_the_update_rule_and_leaves_fixed_weights_alone():
    w = np.array([0.3, -1.25, 2.0, 0.0])
    fixed = np.array([False, True, False, True])
    s = np.array([3 << 32, -(5 << 32), -(1 << 31), 1 << 40], np.int64)
    new = mple_step(w, fixed, s, 4, 0.5, 0.1)
    assert new[1] == w[1] and new[3] == w[3] and new is not w
    assert new[0] == 0.3 + 0.5 * (3.0 / 4 - 0.1 * 0.3)
    assert new[2] == 2.0 + 0.5 * (-0.5 / 4 - 0.1 * 2.0)
    assert np.array_equal(mple_step(w, np.zeros(4, bool), np.zeros(4, np.int64), 7, 0.5, 0.0), w)
    with pytest.raises(ValueError):
        mple_step(w, fixed, s.astype(np.float64), 4, 0.5, 0.1)


def test_argument_errors_come_before_the_device():
    ns, fg = session(GRAPHS["six_variables"]())
    nvar = len(fg.variable)
    for call in (lambda ids: fg.pl_gradient(ids), lambda ids: fg.learn_mple(3, 0.1, var_ids=ids)):
        for bad in ([nvar], [0, -1], np.array([2, 10 ** 12])):
            with pytest.raises(IndexError):
                call(bad)
        for bad in ([[0, 1]], [0.5], np.zeros((2, 2), np.int64), 3, [1, 4, 1], [0, 0]):     # ... the selection is a set
            with pytest.raises(ValueError):
                call(bad)
    for call in (lambda **kw: fg.pl_gradient(**kw), lambda **kw: fg.learn_mple(3, 0.1, **kw)):
        with pytest.raises(ValueError):
            call(var_copy="all", evidence_chain=True)
    for kw in (dict(epochs=0, stepsize=0.1), dict(epochs=65537, stepsize=0.1), dict(epochs=2, stepsize=np.inf),
               dict(epochs=2, stepsize=0.1, decay=np.nan), dict(epochs=2, stepsize=0.1, reg_param=-0.5),
               dict(epochs=2, stepsize=0.1, reg_param=np.inf)):
        with pytest.raises(ValueError):
            fg.learn_mple(**kw)
    assert fg._handle is None                           # nothing above reached the device


def test_planted_pairs_have_a_host_optimum_near_the_planted_weights():
    """The input of the GPU test's learning run.  A condition on the committed seed, not a claim about the device: plain
    gradient ascent of the closed-form twin from weights 0 reaches grad_max <= 1e-9, its optimum lies within 0.1 of
    every planted weight, and scores at least as well as the planted weights."""
    x, y = plgrad.planted_state()
    assert len(x) == plgrad.PLANTED_PAIRS == 2000
    w, gmax = plgrad.pairs_mple([(x, y)])
    print("host optimum", w, "grad_max first / last %.3g / %.3g" % (gmax[0], gmax[-1]))
    assert gmax[-1] <= 1e-9
    assert np.abs(w - np.array(plgrad.PLANTED)).max() <= 0.1
    assert plgrad.pairs_lpl(w, x, y) >= plgrad.pairs_lpl(plgrad.PLANTED, x, y)
    # four chains of 500 pairs are the same examples: the integer sums, hence every step, are the same bits
    parts = [(x[i:i + 500], y[i:i + 500]) for i in range(0, 2000, 500)]
    w4, gmax4 = plgrad.pairs_mple(parts)
    assert np.array_equal(w4.view(np.int64), w.view(np.int64)) and np.array_equal(gmax4, gmax)
    # the closed form is the twin on the oracle's entries
    ns, fg = session(plgrad.planted_graph(500, *parts[1]))
    og = oracle_of(fg, layout=False)
    state = fg.variable["initialValue"].astype(np.int64)
    for wv in (np.zeros(3), np.array(plgrad.PLANTED), w):
        counts, skipped = plgrad.Twin(fg, og).counts(state, wv)
        assert skipped == 0 and np.array_equal(counts, plgrad.pairs_counts(wv, *parts[1]))
