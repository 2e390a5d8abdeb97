"""diagnostics.msd_iterate / msd_terms against plain enumeration on the cases of tests/bp_map.py, the classes and routes from
the host-only plan (nsk_bp_dual_plan).  No GPU."""

import math

import numpy as np
import pytest

import bp_map
import map_dual
from numbskull_amd import _lib


@pytest.mark.parametrize("name", bp_map.TREES + ("clamped_grid", "mixed_free"))
def test_every_class_step_keeps_the_bound_above_the_map_and_never_raises_it(name):
    x, best, margin = map_dual.best(name)
    m = bp_map.model(name)
    b = map_dual.mirror(name, 8, 0.0, True)["bounds"]
    start = math.fsum(map_dual.msd_terms(m.layout, m.theta, np.zeros(int(m.layout["msg_off"][-1])))[0].tolist())
    assert len(b) >= 8 and (b >= best - margin).all()
    assert (np.diff(np.concatenate([[start], b])) <= margin).all()


@pytest.mark.parametrize("name", bp_map.TREES)
def test_on_a_tree_the_bound_is_tight_and_the_decode_is_the_map(name):
    x, best, margin = map_dual.best(name)
    r = map_dual.mirror(name, 4096, 1e-12)
    assert 0 < r["sweeps"] <= 4096
    assert math.fsum(r["tf"].tolist() + r["tv"].tolist()) - best <= margin
    assert (r["decode"][0].tolist(), r["decode"][1]) == (x.tolist(), 0)


def test_the_plan_routes_by_cardinality_table_size_and_degree(monkeypatch):
    m = bp_map.model("routes")
    L = m.layout
    monkeypatch.delenv("NSK_DIAG", raising=False)
    monkeypatch.setenv("NSK_DUAL_LANE_MAX", "0")                # ignored without NSK_DIAG
    counts, route, cls, lds = map_dual.plan("routes")
    tmax = [max([int(np.prod(L["shapes"][f])) for f, ax in enumerate(L["axes"]) if v in ax], default=0) for v in range(len(route))]
    want = [-1 if L["clamped"][v] or not L["var_edges"][v] else
            int(not (L["card"][v] <= _lib.BP_MAP_LANE_CARDS and tmax[v] <= _lib.BP_DUAL_LANE_TABLE and
                     len(L["var_edges"][v]) <= _lib.BP_DUAL_LANE_EDGES)) for v in range(len(route))]
    assert route.tolist() == want and counts == [want.count(0), want.count(1)] and min(counts) > 0
    assert ((cls >= 0) == (np.array(want) >= 0)).all()
    for ax in L["axes"]:                                         # no factor has two free members of one class
        assert len({int(cls[v]) for v in ax}) == len(ax)
    assert lds == max(2 * int(L["card"][v]) + max(sum(L["shapes"][f]) for f, ax in enumerate(L["axes"]) if v in ax)
                      for v in range(len(route)) if want[v] == 1)
    monkeypatch.setenv("NSK_DIAG", "1")
    assert map_dual.plan("routes")[0][0] == 0
    monkeypatch.setenv("NSK_DUAL_LANE_MAX", "4096")
    assert map_dual.plan("routes")[0][1] == int((L["card"][np.array(want) >= 0] > _lib.BP_MAP_LANE_CARDS).sum())
