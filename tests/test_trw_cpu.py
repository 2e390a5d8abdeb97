"""diagnostics.trw_iterate / trw_log_z / edge_appearance against plain enumeration, and the routing plan of the factor
phase (nsk_bp_trw_plan, host only), on the cases of tests/trw.py."""

import numpy as np
import pytest

import bp
import trw
from numbskull_amd import _lib
from numbskull_amd.diagnostics import edge_appearance, trw_iterate, trw_log_z


@pytest.mark.parametrize("name", sorted(bp.TREES))
def test_rho_one_on_a_forest_is_exact(name):
    m = bp.model(name)
    exact, log_z = m.exact()
    r = trw.mirror(name, 40, 0.0, "one")
    assert 1 < r["iters"] < 40 or r["residual"][-1] <= 1e-12
    for v, p in exact.items():
        assert np.abs(m.belief(r, v) - p).max() <= 1e-12, v
    assert abs(r["log_z"] - log_z) <= 1e-11


@pytest.mark.parametrize("name", trw.BOUND)
def test_tree_weights_converge_to_a_strict_upper_bound(name):
    m = trw.model(name)
    rho = trw.rho_of(name, "trees")
    assert rho.min() < 1.0
    r = trw_iterate(m.layout, m.theta, rho, 200, 0.5, 1e-12)
    assert 0 < r["iters"] <= 200
    log_z = trw_log_z(m.layout, m.theta, rho, r["factor_beliefs"], r["beliefs"])
    assert log_z - m.exact()[1] > 1e-6


@pytest.mark.parametrize("name", trw.BOUND + ("star7",))
def test_edge_appearance_lies_in_the_spanning_tree_polytope(name):
    layout = trw.model(name).layout
    rho = edge_appearance(layout, 16, 3)
    assert ((rho > 0) & (rho <= 1)).all()
    pair = np.array([len(ax) == 2 for ax in layout["axes"]])
    nfree = len({v for ax in np.array(layout["axes"], object)[pair] for v in ax})      # (each case's edges connect them)
    assert abs(rho[pair].sum() - (nfree - 1)) <= 1e-12 and (rho[~pair] == 1).all()
    with pytest.raises(ValueError, match="pass rho explicitly"):
        edge_appearance(trw.model("tri").layout, 16, 3)


@pytest.mark.parametrize("name", trw.CASES)
def test_the_plan_routes_by_table_size_and_cardinalities(name, monkeypatch):
    m = trw.model(name)
    shapes = [s for s in m.layout["shapes"]]
    want = [-1 if not s else int(not (int(np.prod(s)) <= _lib.BP_TRW_LANE_TABLE and sum(s) <= _lib.BP_MAP_LANE_CARDS)) for s in shapes]
    monkeypatch.delenv("NSK_DIAG", raising=False)
    monkeypatch.setenv("NSK_TRW_LANE_MAX", "0")                 # ignored without NSK_DIAG
    counts, route, lds = trw.plan(m.fg, m.sev)
    assert route.tolist() == want and counts == [want.count(0), want.count(1)]
    assert lds == max([int(np.prod(s)) + 2 * sum(s) for s, w in zip(shapes, want) if w == 1], default=0)
    assert {"tri": [7, 1], "big": [1, 2]}.get(name, counts) == counts
    monkeypatch.setenv("NSK_DIAG", "1")
    for knob, to in (("0", 1), ("4096", 0)):
        monkeypatch.setenv("NSK_TRW_LANE_MAX", knob)
        counts, route, _ = trw.plan(m.fg, m.sev)
        assert route.tolist() == [-1 if not s else to for s in shapes] and counts[1 - to] == 0
