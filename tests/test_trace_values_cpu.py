"""The numpy side of the trace statistics for categorical variables: diagnostics.indicators (the 0 / 1 series
x == value of (column, value) pairs) against a plain loop, and diagnostics.contingency_tables on hand-made counts."""

import numpy as np
import pytest

from numbskull_amd.diagnostics import Contingency, autocov_counts, contingency_tables, indicators, pair_counts


@pytest.mark.parametrize("dtype,top", [(np.int8, 7), (np.int32, 200)])
def test_indicators_equal_a_plain_loop(dtype, top):
    rng = np.random.default_rng(int(top))
    trace = rng.integers(0, top, (11, 3, 9)).astype(dtype)
    sel = np.array([(8, 0), (0, top - 1), (3, 2), (3, 2), (8, 0), (5, 1), (0, 0), (4, 3), (3, 1), (8, top), (2, -1)])
    got = indicators(trace, sel)
    assert got.dtype == np.uint8 and got.shape == (11, 3, len(sel))
    want = np.zeros_like(got)
    for t in range(11):
        for r in range(3):
            for i, (c, v) in enumerate(sel):
                want[t, r, i] = 1 if int(trace[t, r, c]) == v else 0
    assert np.array_equal(got, want)
    assert got[:, :, :9].any() and not got[:, :, 9:].any()             # a value no row holds: zeros
    assert np.array_equal(got[:, :, 2], got[:, :, 3])
    # all values of a column partition the rows, and the 0 / 1 estimators take the result as it is
    full = indicators(trace, [(4, v) for v in range(top)])
    assert (full.sum(axis=2) == 1).all()
    n, H, A, S1, S2 = autocov_counts(full, 3)
    assert (n, H) == (5, 6) and S1.sum() == n * H
    assert pair_counts(full, [(0, 1), (1, 1)])[0, :, 0].sum() == 0
    empty = indicators(trace, np.zeros((0, 2), np.int64))
    assert empty.shape == (11, 3, 0) and empty.dtype == np.uint8


def test_indicators_argument_errors():
    trace = np.zeros((4, 2, 3), np.int8)
    with pytest.raises(ValueError):
        indicators(trace[0], [(0, 0)])
    with pytest.raises(ValueError):
        indicators(trace.astype(np.float64), [(0, 0)])
    with pytest.raises(ValueError):
        indicators(trace, [0, 1, 2])
    with pytest.raises(ValueError):
        indicators(trace, [(0, 0, 0)])
    with pytest.raises(ValueError):
        indicators(trace, np.array([(0.0, 1.0)]))
    with pytest.raises(IndexError):
        indicators(trace, [(3, 0)])
    with pytest.raises(IndexError):
        indicators(trace, [(1, 0), (-1, 0)])


def test_contingency_tables_on_hand_made_counts():
    nrows, chains = 60, 2
    # pair 0: a 2 x 3 product table in both chains; pair 1: a diagonal 3 x 3; pair 2: a 1 x 1 table
    product = np.outer([20, 40], [15, 15, 30]) // 60                   # row total x column total / nrows, every cell whole
    assert product.sum() == nrows
    diagonal = np.diag([20, 20, 20])
    counts = np.concatenate([product.reshape(-1), diagonal.reshape(-1), [nrows]])
    counts = np.stack([counts, counts], axis=1)
    t = contingency_tables(counts, [(2, 3), (3, 3), (1, 1)], nrows)
    assert isinstance(t, Contingency) and t.samples == nrows * chains and len(t.joint) == 3
    assert [j.shape for j in t.joint] == [(2, 3), (3, 3), (1, 1)] and [c.shape for c in t.counts] == [(2, 2, 3), (2, 3, 3), (2, 1, 1)]
    for j in t.joint:
        assert j.dtype == np.float64 and abs(j.sum() - 1.0) < 1e-15
    assert np.array_equal(t.joint[0], product * 2 / 120.0) and np.array_equal(t.counts[0][1], product)
    assert t.mi.shape == (3,) and t.mi[0] == 0.0 and t.mi[2] == 0.0    # log(1) terms: exactly 0
    assert abs(t.mi[1] - np.log(3.0)) < 1e-15
    # chains pooled: unequal chains, one cell empty in one of them
    a = np.array([[30, 0], [10, 20]])
    b = np.array([[0, 30], [30, 0]])
    t = contingency_tables(np.stack([a.reshape(-1), b.reshape(-1)], axis=1), [(2, 2)], nrows)
    assert np.array_equal(t.joint[0], (a + b) / 120.0) and np.array_equal(t.counts[0], np.stack([a, b]))
    p = (a + b) / 120.0
    want = sum(p[i, k] * np.log(p[i, k] / (p[i].sum() * p[:, k].sum())) for i in range(2) for k in range(2) if p[i, k] > 0)
    assert abs(t.mi[0] - want) < 1e-14
    # nothing counted
    t = contingency_tables(np.zeros((4, 3), np.int64), [(2, 2)], 0)
    assert t.samples == 0 and np.isnan(t.joint[0]).all() and np.isnan(t.mi).all()
    t = contingency_tables(np.zeros((0, 3), np.int64), np.zeros((0, 2), np.int64), 5)
    assert t.samples == 15 and t.joint == [] and t.counts == [] and t.mi.shape == (0,)


def test_contingency_tables_argument_errors():
    ok = np.array([[3], [1], [0], [2]])
    contingency_tables(ok, [(2, 2)], 6)
    with pytest.raises(ValueError):
        contingency_tables(ok, [(2, 2)], 7)                            # the cells do not sum to the rows
    with pytest.raises(ValueError):
        contingency_tables(ok, [(2, 3)], 6)                            # not the number of cells
    with pytest.raises(ValueError):
        contingency_tables(ok.reshape(-1), [(2, 2)], 6)
    with pytest.raises(ValueError):
        contingency_tables(ok.astype(np.float64), [(2, 2)], 6)
    with pytest.raises(ValueError):
        contingency_tables(ok, [2, 2], 6)
    with pytest.raises(ValueError):
        contingency_tables(ok, [(2, 0)], 6)
    with pytest.raises(ValueError):
        contingency_tables(np.array([[7], [1], [0], [-2]]), [(2, 2)], 6)
    with pytest.raises(ValueError):
        contingency_tables(ok, [(2, 2)], -1)
    with pytest.raises(ValueError):
        contingency_tables(np.array([[2 ** 31]]), [(1, 1)], 2 ** 31)
