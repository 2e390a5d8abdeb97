"""Flip pairs: two ADJACENT float64 weights at which one chosen draw of the oracle's device mode comes out 0 and 1.

The table kernels decide a draw from the top 27 bits of the generator's 53-bit integer k and look at the low 26 bits
only when the top bits equal the threshold's (probability 2^-27 per update; nsk_device.h quad_block).  The weights are
the caller's, so that branch can be forced: on a graph with one shared weight w, bisect w over the doubles with the
oracle until two neighbouring doubles w_a, w_b give variable v the values 0 and 1.  With K(w) the largest k for which
the decision function gives 0 at v's neighbourhood, v's draw k then satisfies K(w_b) < k <= K(w_a); when both
thresholds have the same top 27 bits, k has them too, and the library meets a tie at both weights that must resolve
to 0 at w_a and to 1 at w_b.  gap = K(w_a) - K(w_b) == 1 pins k == K(w_a): the inclusive boundary itself.

Nothing here re-implements the generator: the oracle draws, this module only moves the weight.
"""

import struct
from collections import namedtuple

import numpy as np

from oracle import binding as orc

TOP = (1 << 53) - 1

FlipPair = namedtuple("FlipPair", "v w_a w_b K_a K_b gap state_a state_b steps")


# ---- doubles in their numerical order (-0.0 and +0.0 share key 0) ----
def _key(x):
    b = struct.unpack("<q", struct.pack("<d", float(x)))[0]
    return b if b >= 0 else -(b & 0x7FFFFFFFFFFFFFFF)


def _unkey(k):
    return struct.unpack("<d", struct.pack("<q", k if k >= 0 else (-k) | -0x8000000000000000))[0]


def adjacent(a, b):
    """True when no double lies strictly between a and b."""
    return abs(_key(a) - _key(b)) == 1


# ---- the decision function (inference.py:49-52 for a binary variable) in float64, as the oracle's pick() ----
def draw_from_z(z0, z1, k):
    z = (float(k) * 2.0 ** -53) * z1            # k * 2^-53 is exact for k < 2^53
    return 0 if z0 >= z else (1 if z1 >= z else 0)


def z_pair(og, v, state, weights):
    """(z0, z1) of variable v in ``state``: float64 sums in factor-list order (Graph.potential), the oracle's exp."""
    state = np.ascontiguousarray(state, np.int64)
    weights = np.ascontiguousarray(weights, np.float64)
    rc0, p0 = og.potential(int(v), 0, state, weights)
    rc1, p1 = og.potential(int(v), 1, state, weights)
    assert rc0 == 0 and rc1 == 0
    z0 = float(orc.lib().orc_exp_det(float(p0)))
    z1 = z0 + float(orc.lib().orc_exp_det(float(p1)))
    return z0, z1


def threshold_from_z(z0, z1):
    """Largest k in [0, 2^53) with draw_from_z(z0, z1, k) == 0.  fl(k * 2^-53 * z1) is non-decreasing in k, so those k
    are a prefix; k = 0 always gives 0 (z = +0, or NaN and both comparisons false)."""
    assert draw_from_z(z0, z1, 0) == 0
    lo, hi = 0, TOP + 1                          # draw(lo) == 0, draw(hi) == 1 (or hi past the end)
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if draw_from_z(z0, z1, mid) == 0:
            lo = mid
        else:
            hi = mid
    return lo


def threshold_K(og, v, state, weights):
    return threshold_from_z(*z_pair(og, v, state, weights))


def unbalanced(og, v, state):
    """v's neighbourhood gives the two candidates different potentials at a non-zero weight (else z0 / z1 = 1/2
    whatever the weight, and no weight moves the draw)."""
    w = np.ones(len(og.weight), np.float64)
    state = np.ascontiguousarray(state, np.int64)
    return og.potential(int(v), 0, state, w)[1] != og.potential(int(v), 1, state, w)[1]


# ---- oracle runs up to and including v's class of sweep `sweep` ----
def gibbs_runner(og, order, ps, seed, sweep, cls, sample_evidence=True):
    """run(w) -> (values,) after sweeps 0 .. sweep - 1 and classes 0 .. cls of sweep `sweep`, every weight = w."""
    order = np.ascontiguousarray(order, np.int64)
    ps = np.ascontiguousarray(ps, np.int64)
    head = np.ascontiguousarray(ps[:cls + 2])

    def run(w):
        vv, _, wv, cnt = og.initial_state()
        wv[:] = w
        for s in range(sweep):
            assert og.gibbs_dev(order, ps, vv, wv, cnt, seed, s, sample_evidence, burnin=True) == 0
        assert og.gibbs_dev(order, head, vv, wv, cnt, seed, sweep, sample_evidence, burnin=True) == 0
        return (vv,)
    return run


def learn_runner(og, order, ps, seed, sweep, cls):
    """run(w) -> (free chain, evidence chain) of a learning call of fixed weights, up to class cls of sweep `sweep`."""
    order = np.ascontiguousarray(order, np.int64)
    ps = np.ascontiguousarray(ps, np.int64)
    head = np.ascontiguousarray(ps[:cls + 2])

    def run(w):
        vv, ve, wv, _ = og.initial_state()
        wv[:] = w
        assert og.weight["isFixed"].all()
        if sweep:
            assert og.learn_call(order, ps, vv, ve, wv, sweep, 0.01, 1.0, 0, 0.0, 1, False, seed, 0) == 0
        lag = wv.copy() if (og.device_lag if og.device_lag is not None else len(wv) <= 256) else None
        assert og.learn_dev(order, head, vv, ve, wv, 0.01, 0, 0.0, 1, False, seed, sweep, lag=lag) == 0
        return (vv, ve)
    return run


def find_flip_pair(og, order, ps, seed, sweep, v, cls=0, run=None, chain=0, sample_evidence=True, why=None):
    """Bisect the shared weight over float64 until two adjacent doubles give v the values 0 (w_a) and 1 (w_b) in
    array ``chain`` of what ``run`` returns (default: gibbs_runner).  None when v cannot serve: its draw is too
    extreme for the bracket +-20 / neighbours, its neighbourhood is balanced, the two thresholds differ in their top
    27 bits (no certain tie), or something other than v differs between the two runs.  ``why``: a list that receives
    the reason."""
    def no(reason):
        if why is not None:
            why.append((int(v), reason))
        return None
    v = int(v)
    if run is None:
        run = gibbs_runner(og, order, ps, seed, sweep, cls, sample_evidence)
    nnb = max(1, int(og.vmap["factor_index_length"][int(og.variable["vtf_offset"][v])]))
    lo, hi = _key(-20.0 / nnb), _key(20.0 / nnb)
    s_lo, s_hi = run(_unkey(lo)), run(_unkey(hi))
    if s_lo[chain][v] == s_hi[chain][v]:
        return no("both ends of the bracket agree")
    steps = 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        s_mid = run(_unkey(mid))
        steps += 1
        if s_mid[chain][v] == s_lo[chain][v]:
            lo, s_lo = mid, s_mid
        else:
            hi, s_hi = mid, s_mid
    (ka, sa), (kb, sb) = ((lo, s_lo), (hi, s_hi)) if s_lo[chain][v] == 0 else ((hi, s_hi), (lo, s_lo))
    w_a, w_b = _unkey(ka), _unkey(kb)
    assert adjacent(w_a, w_b) and sa[chain][v] == 0 and sb[chain][v] == 1
    # (2) the flip is v's own
    for c, (xa, xb) in enumerate(zip(sa, sb)):
        diff = np.nonzero(xa != xb)[0]
        if not (len(diff) == 0 or (c == chain and list(diff) == [v])):
            return no("another variable differs: %s" % diff[:4])
    # thresholds of v's neighbourhood (v's own value does not enter its potentials)
    nw = len(og.weight)
    K_a = threshold_K(og, v, sa[chain], np.full(nw, w_a))
    K_b = threshold_K(og, v, sb[chain], np.full(nw, w_b))
    assert K_b < K_a, (K_a, K_b)                  # v flipped: K_b < k <= K_a
    # (1) equal top 27 bits: K_b < k <= K_a has them too -- a certain tie at both weights
    if K_a >> 26 != K_b >> 26:
        return no("thresholds differ in their top 27 bits")
    return FlipPair(v, w_a, w_b, K_a, K_b, K_a - K_b, sa, sb, steps)


def first_flip_pair(cands, find):
    """The first candidate (of at most 16) that yields a flip pair; a case whose list is exhausted FAILS."""
    cands = [int(c) for c in cands]
    assert 0 < len(cands) <= 16, len(cands)
    why = []
    for v in cands:
        fp = find(v, why)
        if fp is not None:
            return fp
    raise AssertionError("no flip pair among %d candidates: %s" % (len(cands), why))


def candidates_by_position(ids, colors, cls, pred, limit=16, gen=None):
    """At most ``limit`` variables of colour class ``cls`` whose layout position q (and generator word, when ``gen``
    is given) satisfies pred(q[, gen]), in the order of their positions, spread evenly over the matches."""
    ids, colors = np.asarray(ids, np.int64), np.asarray(colors)
    vs = np.nonzero(colors == cls)[0]
    vs = vs[np.argsort(ids[vs], kind="stable")]
    ok = [int(v) for v in vs if (pred(int(ids[v]), int(gen[v])) if gen is not None else pred(int(ids[v])))]
    if len(ok) <= limit:
        return ok
    step = len(ok) / float(limit)
    return [ok[int(i * step)] for i in range(limit)]
