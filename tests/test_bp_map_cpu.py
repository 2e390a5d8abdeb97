"""diagnostics.ms_iterate / ms_decode against plain enumeration on trees, and the signed-zero argument that lets the
device take its maxima in any order, on every case of tests/test_bp_map_gpu.py."""

import numpy as np
import pytest

import bp_map
from numbskull_amd.diagnostics import ms_decode


@pytest.mark.parametrize("name", bp_map.TREES)
def test_a_converged_tree_decodes_to_the_enumerated_map(name):
    m = bp_map.model(name)
    best, gap, mm = bp_map.enumerate_map(name)
    assert gap >= 1e-6, "the enumerated MAP is unique"
    r = bp_map.mirror(name, 40, 0.0, 0.0)
    assert 1 < r["iters"] < 40 and r["residual"][r["iters"] - 1] == 0.0
    x, ties = ms_decode(m.layout, r["max_marginals"], m.x)
    assert ties == 0 and np.array_equal(x, best)
    assert not np.array_equal(x, m.x), "the decode moves the initial state"
    fin = np.isfinite(mm)
    assert np.array_equal(fin, np.isfinite(r["max_marginals"]))
    assert np.abs(r["max_marginals"][fin] - mm[fin]).max() <= 1e-12
    assert (r["max_marginals"][fin] < 0).any()


@pytest.mark.parametrize("name", bp_map.CASES + ("trips", "symmetric"))
def test_no_maximum_over_several_entries_meets_a_negative_zero(name):
    for damping in (0.0, 0.5):
        r = bp_map.mirror(name, 8 if name != "trips" else 4, damping, 0.0)
        assert r["negzero_maxima"] == 0
        for key in ("F", "V"):
            assert not (np.signbit(r[key]) & (r[key] == 0.0)).any(), key
            assert np.isfinite(r[key]).all() and (r[key] <= 0.0).all()


def test_a_symmetric_graph_ties():
    m = bp_map.model("symmetric")
    r = bp_map.mirror("symmetric", 8, 0.0, 0.0)
    x, ties = ms_decode(m.layout, r["max_marginals"], m.x)
    assert ties == 2 and x.tolist() == [0, 0] and m.x.tolist() == [1, 1]
