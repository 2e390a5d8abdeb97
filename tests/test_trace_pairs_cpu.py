"""The numpy side of the pairwise joint marginals (diagnostics.pair_counts, pair_tables, factor_pairs; what
FactorGraph.pairwise counts on the device from a bit-packed trace): the counts against a plain loop, the tables against
numpy's own statistics and against tables whose figures are known in closed form."""

import numpy as np
import pytest

from numbskull_amd import graphgen
from numbskull_amd.diagnostics import Pairwise, factor_pairs, pair_counts, pair_tables


def _trace(rows, chains, ncol, seed, p=None):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, ncol) if p is None else p
    return (rng.random((rows, chains, ncol)) < p).astype(np.int8)


def _loop(x, pairs):
    out = np.zeros((len(pairs), x.shape[1], 3), np.int64)
    for j, (a, b) in enumerate(pairs):
        for r in range(x.shape[1]):
            for t in range(x.shape[0]):
                out[j, r, 0] += int(x[t, r, a]) * int(x[t, r, b])
                out[j, r, 1] += int(x[t, r, a])
                out[j, r, 2] += int(x[t, r, b])
    return out


@pytest.mark.parametrize("chains", [1, 3])
def test_counts_equal_a_plain_loop(chains):
    x = _trace(37, chains, 9, seed=chains)
    pairs = [(0, 1), (1, 0), (8, 8), (3, 7), (3, 7), (7, 3), (0, 8), (4, 4), (2, 5)]
    got = pair_counts(x, np.array(pairs))
    assert got.dtype == np.int64 and got.shape == (len(pairs), chains, 3)
    assert np.array_equal(got, _loop(x, pairs))
    assert np.array_equal(got[0, :, 0], got[1, :, 0]) and np.array_equal(got[0, :, 1], got[1, :, 2])       # the reverse swaps n1a and n1b
    assert np.array_equal(got[2, :, 0], got[2, :, 1]) and np.array_equal(got[2, :, 0], got[2, :, 2])       # a == b
    assert np.array_equal(got[3], got[4])                                                                  # a repeat
    # more pairs than one batch of the implementation, and no pairs
    rng = np.random.default_rng(5)
    many = rng.integers(0, 9, (700, 2))
    assert np.array_equal(pair_counts(x, many), _loop(x, many))
    assert pair_counts(x, np.zeros((0, 2), np.int64)).shape == (0, chains, 3)
    assert pair_counts(x.astype(bool), many[:5]).tolist() == pair_counts(x, many[:5]).tolist()


def test_tables_against_numpy_statistics():
    rows, chains, ncol = 400, 3, 7
    x = _trace(rows, chains, ncol, seed=11)
    x[:, :, 5] = x[:, :, 2] ^ (np.random.default_rng(1).random((rows, chains)) < 0.1)      # a correlated pair
    pairs = np.array([(a, b) for a in range(ncol) for b in range(ncol)])
    t = pair_tables(pair_counts(x, pairs), rows)
    assert isinstance(t, Pairwise) and t.samples == rows * chains
    assert t.joint.shape == (len(pairs), 2, 2) and t.counts.shape == (len(pairs), chains, 3)
    flat = x.reshape(-1, ncol).astype(np.float64)
    mean = flat.mean(axis=0)
    np.testing.assert_allclose(t.joint.sum(axis=(1, 2)), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(t.joint[:, 1, :].sum(axis=1), mean[pairs[:, 0]], rtol=0, atol=1e-15)       # margin of a
    np.testing.assert_allclose(t.joint[:, :, 1].sum(axis=1), mean[pairs[:, 1]], rtol=0, atol=1e-15)       # margin of b
    want = np.corrcoef(flat.T)
    np.testing.assert_allclose(t.corr, want[pairs[:, 0], pairs[:, 1]], rtol=0, atol=1e-12)
    cov = np.cov(flat.T, bias=True)
    np.testing.assert_allclose(t.cov, cov[pairs[:, 0], pairs[:, 1]], rtol=0, atol=1e-12)
    assert t.corr[2 * ncol + 5] > 0.5 and t.mi[2 * ncol + 5] > 10 * t.mi[0 * ncol + 1]
    # every cell by counting
    for j in (1, 19, 37):
        a, b = pairs[j]
        for va in (0, 1):
            for vb in (0, 1):
                assert t.joint[j, va, vb] == ((flat[:, a] == va) & (flat[:, b] == vb)).sum() / (rows * chains)
    # (b, a) is the transposed table, with equal cov, corr and mi
    rev = pair_tables(pair_counts(x, pairs[:, ::-1]), rows)
    assert np.array_equal(rev.joint, t.joint.transpose(0, 2, 1))
    assert np.array_equal(rev.cov, t.cov) and np.array_equal(rev.corr, t.corr)
    np.testing.assert_allclose(rev.mi, t.mi, rtol=0, atol=1e-15)
    # a == b: correlation 1, the mutual information is the column's entropy
    diag = np.arange(ncol) * (ncol + 1)
    assert (t.corr[diag] == 1.0).all()
    ent = -(mean * np.log(mean) + (1 - mean) * np.log(1 - mean))
    np.testing.assert_allclose(t.mi[diag], ent, rtol=0, atol=1e-12)
    assert (t.joint[diag, 0, 1] == 0).all() and (t.joint[diag, 1, 0] == 0).all()


def test_a_constant_column():
    x = _trace(50, 2, 4, seed=3)
    x[:, :, 1] = 1
    x[:, :, 3] = 0
    t = pair_tables(pair_counts(x, [(0, 1), (1, 0), (3, 2), (1, 3), (1, 1), (3, 3)]), 50)
    assert np.isnan(t.corr).all()
    assert (t.mi == 0.0).all() and (t.cov == 0.0).all()
    assert t.joint[0, 0, 0] == 0 and t.joint[0, 1, 0] == 0 and abs(t.joint[0, :, 1].sum() - 1.0) < 1e-15
    assert np.array_equal(t.counts[0, :, 0], t.counts[0, :, 1])        # n11 against a column of ones: the other's n1
    assert (t.counts[2, :, 0] == 0).all()                              # ... against a column of zeros


def test_an_independent_table_has_zero_covariance_and_information_exactly():
    """N = 60, na = 20, nb = 15, n11 = na nb / N = 5: every cell is row total x column total / N"""
    a = np.zeros(60, np.int8)
    b = np.zeros(60, np.int8)
    a[:20] = 1
    b[:5] = 1
    b[20:30] = 1
    x = np.stack([a, b], axis=1).reshape(30, 2, 2)                     # two chains of 30 rows
    t = pair_tables(pair_counts(x, [(0, 1)]), 30)
    assert t.samples == 60 and t.counts.sum(axis=1).tolist() == [[5, 20, 15]]
    assert t.cov[0] == 0.0 and t.mi[0] == 0.0 and t.corr[0] == 0.0
    assert np.array_equal(t.joint[0], np.array([[30, 10], [15, 5]]) / 60.0)


def test_no_rows_and_no_pairs():
    t = pair_tables(np.zeros((3, 2, 3), np.int64), 0)
    assert t.samples == 0 and np.isnan(t.joint).all() and np.isnan(t.cov).all() and np.isnan(t.corr).all() and np.isnan(t.mi).all()
    t = pair_tables(np.zeros((0, 2, 3), np.int64), 10)
    assert t.joint.shape == (0, 2, 2) and t.cov.shape == t.corr.shape == t.mi.shape == (0,) and t.samples == 20


def test_factor_pairs_of_a_grid():
    w, v, f, fm, dm, e = graphgen.ising_grid(4, 5)
    p = factor_pairs(f, fm)
    two = np.flatnonzero(f["arity"] == 2)
    assert p.dtype == np.int64 and p.shape == (len(two), 2) and len(two) == 4 * 4 + 3 * 5
    for row, fid in zip(p, two):
        off = int(f["ftv_offset"][fid])
        assert row.tolist() == [int(fm["vid"][off]), int(fm["vid"][off + 1])]
    assert len({tuple(sorted(r)) for r in p.tolist()}) == len(p) and (p[:, 0] != p[:, 1]).all()
    assert factor_pairs(f[f["arity"] != 2], fm).shape == (0, 2)


def test_value_errors():
    x = _trace(10, 2, 3, seed=1)
    ok = np.array([(0, 1)])
    with pytest.raises(ValueError):
        pair_counts(x * 2, ok)
    with pytest.raises(ValueError):
        pair_counts(x[0], ok)
    with pytest.raises(ValueError):
        pair_counts(x, np.array([0, 1, 2]))
    with pytest.raises(ValueError):
        pair_counts(x, np.array([(0, 1, 2)]))
    with pytest.raises(ValueError):
        pair_counts(x, np.array([(0.0, 1.0)]))
    with pytest.raises(ValueError):
        pair_counts(x, np.array([(0, 3)]))
    with pytest.raises(ValueError):
        pair_counts(x, np.array([(-1, 0)]))
    c = pair_counts(x, ok)
    with pytest.raises(ValueError):
        pair_tables(c[0], 10)
    with pytest.raises(ValueError):
        pair_tables(c[:, :, :2], 10)
    with pytest.raises(ValueError):
        pair_tables(c.astype(np.float64), 10)
    with pytest.raises(ValueError):
        pair_tables(c, 1)                                  # more ones than rows
    with pytest.raises(ValueError):
        pair_tables(np.zeros((1, 2, 3), np.int64), 2 ** 30)        # N = 2^31
    assert pair_tables(np.zeros((1, 2, 3), np.int64), 2 ** 30 - 1).samples == 2 ** 31 - 2
