"""The host side of the ICM tests: iterated conditional modes built from the oracle's potential() (pinned to the
reference), a colouring, and the numpy rule numbskull_amd.diagnostics.icm_choice -- the yardstick nsk_icm is held to."""

import numpy as np

from numbskull_amd.diagnostics import icm_choice
from util import phases_from_colors


def joint_exponent(og, x, w):
    """the log-potential of a state as exact_marginals computes it: the sum over all factors of weight x eval_factor"""
    e = 0.0
    for fid in range(len(og.factor)):
        rc, val = og.eval_factor(fid, -1, 0, x)
        assert rc == 0
        e += w[int(og.factor[fid]["weightId"])] * val
    return e


def host_icm(og, color, x, w, max_sweeps, sample_evidence=False, on_sweep=None):
    """ICM from state `x` under weights `w`: a sweep visits the colour classes in colour order and decides the eligible
    variables of a class from the potentials of the state as the class found it (icm_choice).  Returns (the final
    state, sweeps in nsk_icm's convention -- the count up to and including the first sweep without a change, or
    -max_sweeps --, the changes of every sweep).  on_sweep(state) is called after every sweep."""
    x = np.ascontiguousarray(x, np.int64).copy()
    w = np.ascontiguousarray(w, np.float64)
    card = og.variable["cardinality"].astype(np.int64)
    eligible = (np.asarray(color) >= 0) & ((og.variable["isEvidence"] == 0) | bool(sample_evidence))
    order, ps = phases_from_colors(color)
    changed = np.zeros(max_sweeps, np.int64)
    sweeps = -max_sweeps
    for s in range(max_sweeps):
        for c in range(len(ps) - 1):
            vs = order[ps[c]:ps[c + 1]]
            vs = vs[eligible[vs]]
            if not len(vs):
                continue
            off = np.concatenate([[0], np.cumsum(card[vs])]).astype(np.int64)
            pot = np.zeros(int(off[-1]))
            for i, v in enumerate(vs):
                for k in range(card[v]):
                    rc, pot[off[i] + k] = og.potential(int(v), k, x, w)
                    assert rc == 0, ("oracle refuses variable", v)
            new = icm_choice(off, pot, x[vs])
            changed[s] += int((new != x[vs]).sum())
            x[vs] = new
        if on_sweep is not None:
            on_sweep(x)
        if changed[s] == 0:             # the fixed point: later sweeps change nothing
            sweeps = s + 1
            break
    return x, sweeps, changed
