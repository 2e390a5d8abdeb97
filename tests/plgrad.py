"""Shared helpers of the pseudo-likelihood gradient tests (tests/test_pl_gradient_cpu.py, tests/test_pl_gradient_gpu.py):
the per-entry arrays ``numbskull_amd.diagnostics.pl_gradient_counts`` takes, built from the product's index
(``fg.vmap`` / ``fg.factor_index``) and the oracle's ``eval_factor`` / ``potential`` / ``exp_det``; the planted pair model
of the MPLE tests with its closed forms."""

import numpy as np

from numbskull_amd import graphgen
from numbskull_amd.diagnostics import conditional_probabilities, pl_gradient_counts
from util import orc

Q = 2.0 ** -32


def positioned(fg, ids=None):
    """the selected variables (None: all) that have a position in a whole-graph handle's layout: isEvidence != 4"""
    ids = np.arange(len(fg.variable)) if ids is None else np.asarray(ids, np.int64)
    return ids[fg.variable["isEvidence"][ids] != 4]


def structure(fg, ids):
    """The walk of the selection `ids`, independent of the state: (offsets, entry_var, entry_k, entry_factor,
    entry_weight) -- one entry per (selected variable, value k, factor of the list of (variable, k)), in walk order."""
    var, vmap, fi = fg.variable, fg.vmap, np.asarray(fg.factor_index, np.int64)
    card = var["cardinality"].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(card[ids])]).astype(np.int64)
    ev, ek, ef = [], [], []
    for i, v in enumerate(ids):
        for k in range(card[v]):
            vt = vmap[int(var["vtf_offset"][v]) + (k if var["dataType"][v] != 0 else 0)]
            f = fi[int(vt["factor_index_offset"]):int(vt["factor_index_offset"]) + int(vt["factor_index_length"])]
            ev.append(np.full(len(f), i, np.int64))
            ek.append(np.full(len(f), k, np.int64))
            ef.append(f)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)       # noqa: E731
    ev, ek, ef = cat(ev), cat(ek), cat(ef)
    return off, ev, ek, ef, fg.factor["weightId"][ef].astype(np.int64)


def entry_values(og, ids, structure_, state):
    """eval_factor of every entry on `state`, through the oracle"""
    _, ev, ek, ef, _ = structure_
    state = np.ascontiguousarray(state, np.int64)
    out = np.zeros(len(ef))
    for j in range(len(ef)):
        rc, out[j] = og.eval_factor(int(ef[j]), int(ids[ev[j]]), int(ek[j]), state)
        assert rc == 0, ("oracle refuses factor", ef[j])
    return out


def probabilities(og, ids, off, state, weights):
    """the conditionals of the selection: the oracle's potential(), exp_det, the twin's running sum and division"""
    state = np.ascontiguousarray(state, np.int64)
    weights = np.ascontiguousarray(weights, np.float64)
    card = np.diff(off)
    pot = np.zeros(int(off[-1]))
    for i, v in enumerate(ids):
        for k in range(card[i]):
            rc, pot[off[i] + k] = og.potential(int(v), k, state, weights)
            assert rc == 0, ("oracle refuses variable", v)
    return pot, conditional_probabilities(off, pot, exp=orc.exp_det)


class Twin(object):
    """pl_gradient_counts on the oracle's entries for a fixed selection of a graph: the structure is built once"""

    def __init__(self, fg, og, ids=None):
        self.fg, self.og = fg, og
        self.ids = positioned(fg, ids)
        self.s = structure(fg, self.ids)
        self.nweight = len(fg.weight)

    def counts(self, state, weights):
        off, ev, ek, _, ew = self.s
        _, prob = probabilities(self.og, self.ids, off, state, weights)
        ee = entry_values(self.og, self.ids, self.s, state)
        return pl_gradient_counts(off, prob, np.asarray(state, np.int64)[self.ids], ev, ek, ew, ee, self.nweight)


# ------------------------------------------------------------------------------------------------ planted pairs
PLANTED = (0.6, -0.4, 0.5)          # the weights the pairs are drawn from: ISTRUE(x), ISTRUE(y), EQUAL(x, y)
PLANTED_SEED = 7                    # the committed seed (tests/test_pl_gradient_cpu.py checks the condition on it)
PLANTED_PAIRS = 2000
MPLE_STEP, MPLE_STEPS = 0.5, 400    # plain gradient ascent from weights 0 (chosen on the host twin, see the CPU test)


def planted_state(npairs=PLANTED_PAIRS, seed=PLANTED_SEED):
    """(x, y): npairs independent draws from p(x, y) ~ exp(a s(x) + b s(y) + c s(x == y)), s(t) = +1 if t else -1 -- the
    joint table enumerated per pair, a numpy generator for the uniforms"""
    a, b, c = PLANTED
    s = lambda t: 1.0 if t else -1.0                                                    # noqa: E731
    z = np.array([np.exp(a * s(x) + b * s(y) + c * s(x == y)) for x in (0, 1) for y in (0, 1)])
    u = np.random.default_rng(seed).random(npairs)
    idx = np.searchsorted(np.cumsum(z) / z.sum(), u, side="left").clip(0, 3)
    return (idx >= 2).astype(np.int64), (idx % 2).astype(np.int64)


def planted_graph(npairs, x, y):
    """graphgen.ising_pairs with the given state as initial (and evidence) values, free weights 0"""
    g = list(graphgen.ising_pairs(npairs, *PLANTED, seed=0))
    var = g[1].copy()
    var["initialValue"][0::2] = x
    var["initialValue"][1::2] = y
    g[1] = var
    return tuple(g)


def pairs_counts(w, x, y):
    """pl_gradient_counts of the pair model in closed form, vectorised over the pairs (one state): per variable the
    list [ISTRUE(self), EQUAL(x, y)], both values k; ISTRUE is +1 at 1 and -1 at 0, EQUAL +1 when equal else -1.  The
    operations are the device's: rounded products added in list order, exp, the running sum, one division, and per entry
    one subtraction, one product, one rounding to int64."""
    w = np.asarray(w, np.float64)
    counts = np.zeros(3, np.int64)
    other = np.array([0, 1])                                            # a variable's terms depend on (own value, other's value)
    for self_w, me_, other_ in ((0, x, y), (1, y, x)):
        n = np.zeros((2, 2), np.int64)                                  # pairs with (own value, other's value)
        np.add.at(n, (me_, other_), 1)
        e_is = np.array([-1.0, 1.0])                                    # ISTRUE with the variable at k
        e_eq = [np.where(other == k, 1.0, -1.0) for k in (0, 1)]        # EQUAL with the variable at k, by the other's value
        p = [(0.0 + w[self_w] * e_is[k]) + w[2] * e_eq[k] for k in (0, 1)]
        e = [orc.exp_det(pk) for pk in p]
        z = e[0] + e[1]
        for k in (0, 1):
            for me in (0, 1):
                c = (1.0 if me == k else 0.0) - e[k] / z               # by the other's value
                counts[self_w] += (n[me] * np.rint((c * e_is[k]) * 2.0 ** 32).astype(np.int64)).sum()
                counts[2] += (n[me] * np.rint((c * e_eq[k]) * 2.0 ** 32).astype(np.int64)).sum()
    return counts


def pairs_mple(examples, steps=MPLE_STEPS, step=MPLE_STEP, decay=1.0, reg_param=0.0, w0=(0.0, 0.0, 0.0), fixed=(0, 0, 0)):
    """The host twin of learn_mple on the pair model: `examples` is a list of (x, y) states, each a training example.
    Returns (weights, grad_max per step)."""
    from numbskull_amd.diagnostics import mple_step
    w, fixed = np.array(w0, np.float64), np.asarray(fixed, bool)
    n = sum(2 * len(x) for x, _ in examples)
    gmax, st = np.zeros(steps), float(step)
    for t in range(steps):
        s = np.sum([pairs_counts(w, x, y) for x, y in examples], axis=0).astype(np.int64)
        gmax[t] = np.abs(s[~fixed]).max() * Q / n
        w = mple_step(w, fixed, s, n, st, reg_param)
        st = st * decay
    return w, gmax


def pairs_lpl(w, x, y):
    """log-pseudo-likelihood of the pair model's state under w (numpy's exp / log)"""
    w = np.asarray(w, np.float64)
    out = 0.0
    for self_w, me, other in ((0, x, y), (1, y, x)):
        p = np.stack([w[self_w] * (2.0 * k - 1.0) + w[2] * np.where(other == k, 1.0, -1.0) for k in (0, 1)])
        m = p.max(axis=0)
        out += (np.take_along_axis(p, me[None, :], axis=0)[0] - m - np.log(np.exp(p - m).sum(axis=0))).sum()
    return float(out)
