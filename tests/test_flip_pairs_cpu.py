"""tests/flip_pairs.py on the host: the oracle alone (generator ids = variable ids, ``oracle_of(..., layout=False)``)
finds flip pairs on small grids; every pair found must satisfy what the GPU cases (tests/test_draw_ties_gpu.py) rest on,
and its thresholds are checked once more in exact rational arithmetic."""

import math
from fractions import Fraction

import numpy as np
import pytest

from numbskull_amd import graphgen
from util import session, oracle_of, phases_from_colors
import flip_pairs as fp

SEED = 77


def _setup(rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    g = graphgen.ising_grid(rows, cols, weight=0.3, initial=rng.integers(0, 2, rows * cols))
    ns, fg = session(g, seed=SEED)
    og = oracle_of(fg, layout=False)
    color, _ = fg.plan()
    order, ps = phases_from_colors(color)
    return og, color, order, ps


def _fl_product(k, z1):
    """fl(k * 2^-53 * z1) by exact rational arithmetic (int / int true division rounds correctly)."""
    return float(Fraction(k, 1 << 53) * Fraction(z1))


def _check_pair(og, pair, chain=0):
    assert fp.adjacent(pair.w_a, pair.w_b)
    assert pair.state_a[chain][pair.v] == 0 and pair.state_b[chain][pair.v] == 1
    assert pair.K_a >> 26 == pair.K_b >> 26                                  # (1) a certain tie at both weights
    for c, (a, b) in enumerate(zip(pair.state_a, pair.state_b)):             # (2) the flip is v's own
        d = np.nonzero(a != b)[0]
        assert len(d) == 0 or (c == chain and list(d) == [pair.v])
    assert pair.gap == pair.K_a - pair.K_b >= 1
    nw = len(og.weight)
    for w, st, K in ((pair.w_a, pair.state_a, pair.K_a), (pair.w_b, pair.state_b, pair.K_b)):
        z0, z1 = fp.z_pair(og, pair.v, st[chain], np.full(nw, w))
        assert math.isfinite(z0) and math.isfinite(z1) and 0 < K < fp.TOP
        assert Fraction(z0) >= Fraction(_fl_product(K, z1))                  # 0 at k = K ...
        assert not Fraction(z0) >= Fraction(_fl_product(K + 1, z1))          # ... and 1 at K + 1


GAPS = {}


@pytest.mark.parametrize("rows,cols,sweep,cls", [(16, 16, 0, 0), (16, 16, 0, 1), (16, 16, 3, 0),
                                                 (57, 33, 0, 0), (57, 33, 0, 1), (57, 33, 2, 1)])
def test_flip_pairs_hold_what_the_gpu_cases_rest_on(rows, cols, sweep, cls):
    og, color, order, ps = _setup(rows, cols)
    ids = np.arange(rows * cols)
    for part in range(4):                       # four candidate lists: positions q with (q // 2) % 4 == part
        cands = fp.candidates_by_position(ids, color, cls, lambda q: (q // 2) % 4 == part)
        pair = fp.first_flip_pair(cands, lambda v, why: fp.find_flip_pair(og, order, ps, SEED, sweep, v, cls=cls, why=why))
        assert pair.steps <= 70
        _check_pair(og, pair)
        GAPS[(rows, cols, sweep, cls, part)] = pair.gap


def test_flip_pairs_of_a_learning_sweep_on_either_chain():
    rows, cols = 16, 16
    rng = np.random.default_rng(4)
    g = graphgen.ising_grid(rows, cols, weight=0.3, fixed=True, evidence=rng.integers(0, 2, rows * cols))
    g[1]["isEvidence"] = ((np.arange(rows * cols) % cols) >= cols // 2).astype(g[1]["isEvidence"].dtype)
    ns, fg = session(g, seed=SEED)
    og = oracle_of(fg, layout=False)
    color, _ = fg.plan()
    order, ps = phases_from_colors(color)
    free = np.nonzero(g[1]["isEvidence"] == 0)[0]
    for chain in (0, 1):
        cands = [v for v in fp.candidates_by_position(np.arange(rows * cols), color, 0, lambda q: True, limit=64)
                 if chain == 0 or v in free][:16]
        run = fp.learn_runner(og, order, ps, SEED, 0, 0)
        pair = fp.first_flip_pair(cands, lambda v, why: fp.find_flip_pair(og, order, ps, SEED, 0, v, run=run, chain=chain, why=why))
        _check_pair(og, pair, chain)
        GAPS[("learn", chain)] = pair.gap


def test_adjacent_doubles_nearly_always_pin_the_boundary():
    """|w| in [0.25, 1): an ulp of w moves K by less than 1, so the pairs above mostly have gap == 1 (the GPU file asks
    for three such cases at least)."""
    assert len(GAPS) >= 20
    assert sum(1 for g in GAPS.values() if g == 1) >= 3, GAPS


def test_double_keys_and_thresholds_at_the_edges():
    xs = [-math.inf, -1e308, -1.0, -5e-324, 0.0, 5e-324, 1.0, 1e308, math.inf]
    ks = [fp._key(x) for x in xs]
    assert ks == sorted(ks) and len(set(ks)) == len(ks)
    assert all(fp._unkey(k) == x for k, x in zip(ks, xs)) and fp._key(-0.0) == fp._key(0.0)
    assert fp.adjacent(0.0, 5e-324) and fp.adjacent(-5e-324, 0.0) and not fp.adjacent(1.0, 1.0)
    assert fp.adjacent(1.0, np.nextafter(1.0, 2.0)) and not fp.adjacent(1.0, 1.0 + 2 ** -51)
    assert fp.threshold_from_z(1.0, 2.0) == 1 << 52                          # z0 >= k 2^-53 2  <=>  k <= 2^52
    assert fp.threshold_from_z(1.0, math.inf) == 0                          # z1 = inf: 0 at k = 0 only
    assert fp.threshold_from_z(math.inf, math.inf) == fp.TOP                 # z0 = inf >= everything
    assert fp.threshold_from_z(math.nan, math.nan) == fp.TOP                 # NaN: both comparisons false -> 0
    assert fp.threshold_from_z(1.0, math.nan) == fp.TOP
    assert fp.threshold_from_z(2.0 ** -60, 1.0) == 0                         # K >> 26 == 0


def test_candidates_by_position():
    ids = np.array([5, 3, 9, 1, 7, 0])
    col = np.array([0, 0, 1, 0, 0, -1])
    assert fp.candidates_by_position(ids, col, 0, lambda q: True) == [3, 1, 0, 4]
    assert fp.candidates_by_position(ids, col, 0, lambda q: q > 3) == [0, 4]
    assert fp.candidates_by_position(ids, col, 0, lambda q, g: g == 2, gen=np.array([2, 0, 2, 0, 2, 2])) == [0, 4]
    assert len(fp.candidates_by_position(np.arange(100), np.zeros(100, int), 0, lambda q: True)) == 16
