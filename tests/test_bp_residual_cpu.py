"""The residual schedule's numpy mirror (diagnostics.rbp_iterate) without a GPU; the liveliness of every GPU case."""

import numpy as np
import pytest

import bp
import bp_residual as br


def _same(a, b, keys=("f2v", "v2f", "beliefs", "residual")):
    return all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in keys)


@pytest.mark.parametrize("name", ["chain9", "star"])
def test_the_mirror_is_exact_on_trees(name):
    """the bounds of tests/test_bp_cpu.py for flooding: beliefs within 1e-12 of enumeration, log Z within 1e-10"""
    m = bp.model(name)
    r = br.run(m, 200, 0.5)
    ex, lz = m.exact()
    err = max(float(np.abs(m.belief(r, v) - p).max()) for v, p in ex.items())
    assert 1 < r["rounds"] < 200 and r["residual"][r["rounds"] - 1] == 0.0
    assert err <= 1e-12 and abs(m.log_z(r) - lz) <= 1e-10


@pytest.mark.parametrize("damping", [0.0, 0.5])
@pytest.mark.parametrize("name", sorted(br.FLOOD))
def test_frac_zero_is_the_flooding_schedule(name, damping):
    m = br.model(name)
    for n, tol in ((1, 0.0), (2, 0.0), (7, 0.0), (30, 1e-3)):
        a, b = br.run(m, n, 0.0, damping, tol), m.run(n, damping, tol)
        assert _same(a, b) and a["rounds"] == b["iters"], (name, damping, n, tol)


@pytest.mark.parametrize("damping", [0.0, 0.5])
def test_a_warm_call_continues_where_a_longer_one_would_be(damping):
    m = br.model("grid5")
    whole, a = br.mirror("grid5", 7, 0.5, damping), br.mirror("grid5", 3, 0.5, damping)
    b = br.run(m, 4, 0.5, damping, messages=(a["f2v"], a["v2f"]))
    assert _same(whole, b, ("f2v", "v2f", "beliefs", "cand", "r"))
    for k in ("residual", "updates"):
        assert np.array_equal(whole[k], np.concatenate([a[k], b[k]])), k
    assert np.array_equal(whole["recomputed"][4:], b["recomputed"][1:]) and b["recomputed"][0] == len(m.layout["edge_var"])


def test_fewer_candidates_than_flooding_on_a_frustrated_grid():
    """8 x 8, couplings N(0, 1), seed 2, tol 1e-9: the totals are in DESIGN.md section 4"""
    m = bp.Model(br.spin_grid(8, 8, 2, 1.0))
    nedge = len(m.layout["edge_var"])
    flood, res = m.run(1000, 0.0, 1e-9), br.run(m, 1000, 0.5, 0.0, 1e-9)
    print("flooding: %d iterations x %d edges = %d; residual: %d rounds, %d candidates, %d commits"
          % (flood["iters"], nedge, flood["iters"] * nedge, res["rounds"], res["recomputed"].sum(), res["updates"].sum()))
    assert flood["iters"] > 0 and res["rounds"] > 0
    assert res["recomputed"].sum() < flood["iters"] * nedge


@pytest.mark.parametrize("name", sorted(br.CASES))
def test_every_gpu_case_is_lively(name):
    nedge = len(br.model(name).layout["edge_var"])
    rounds = 4 if name == "trips" else 40
    for frac in (0.1, 0.5):
        r = br.mirror(name, rounds, frac)
        assert ((r["updates"] > 0) & (r["updates"] < nedge)).any(), (name, frac)
