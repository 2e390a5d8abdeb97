"""Host-only plans of the star graphs (tests/hubs.py): the hub route each GPU case of tests/test_hubs_gpu.py relies on,
read from the plan's hub counters (nsk_graph_info.hubs / hubs_ep / hubs_block); the same counters of the parity tests'
graphs with hubs, so that what those cover cannot drift unseen; and the liveliness of every case in the oracle's own
run -- a hub that never moved, or weights that never changed, would let a parity test pass for nothing."""

import numpy as np
import pytest

from conftest import graph_from  # noqa: F401
from util import session, oracle_of, phases_from_colors
from hubs import (CASES, LEARN_CASES, LEARN_CFG, HubSpec, build_case, check_route, general_hubs, hub_entries, nhubs,
                  oracle_inference, oracle_learning, set_switches, star_graph)


def _plan(g, hbv=True):
    ns, fg = session(g, head_by_vid=hbv)
    color, info = fg.plan()
    return fg, color, info


@pytest.mark.parametrize("name", sorted(CASES))
def test_star_graph_plans_take_the_intended_route(monkeypatch, name):
    set_switches(monkeypatch, name)
    g = build_case(name)
    assert [hub_entries(g, h) for h in range(nhubs(name))] == [h.entries for h in CASES[name].hubs]
    fg, color, info = _plan(g)
    check_route(name, info)
    assert info["value_bytes"] == (4 if CASES[name].wide else 1)
    # hubs 0 and 1 share a factor: hubs in two colours at least
    assert color[0] != color[1] and len(set(color[:nhubs(name)].tolist())) >= 2


def test_every_route_has_its_cases_on_both_sides_of_every_boundary():
    """What the table must keep: the four routes, and the list lengths next to each routing boundary."""
    by_route = {}
    for name, cs in CASES.items():
        by_route.setdefault(cs.route, set()).update(h.entries for h in cs.hubs)
    assert {31, 32, 33, 64, 65, 128, 129, 256} <= by_route["wave"]
    assert {129, 257, 1024, 1025, 2100, 16384} <= by_route["block"]
    assert {33, 129, 130, 257, 16385} <= by_route["walk"]
    assert {33, 130} <= by_route["lane"]
    cards = lambda r: {(h.card, h.dtype) for n, cs in CASES.items() if cs.route == r for h in cs.hubs}
    assert {(c, d) for c in (9, 16, 17, 64, 65) for d in (0, 1)} | {(2, 1)} <= cards("walk")
    assert {2, 3, 16, 17} <= {c for c, _ in cards("lane")}
    assert {(2, 0), (2, 1), (3, 1), (5, 0), (8, 0), (8, 1)} <= cards("wave") & cards("block")


def test_one_factor_off_the_tile_form_takes_the_hub_off_the_entry_parallel_routes():
    """Cardinality 9, a LINEAR or RATIO factor, a factor with 7 others: each alone sends the hub to the generic walk,
    while its general-form neighbour keeps its entry-parallel stream.  The leaves of the LINEAR factor are off the
    tile form too and, being few, become hubs themselves (every generic-path variable of a colour with few of them)."""
    for odd, extra in ((HubSpec(65, 9, 0), 0), (HubSpec(65, 5, 0, "linear"), 2), (HubSpec(65, 5, 1, "ratio"), 2),
                       (HubSpec(65, 2, 1, "seven"), 7)):
        g = star_graph([HubSpec(65, 5, 0), odd], seed=3)
        _, _, info = _plan(g)
        assert (info["hubs"], info["hubs_ep"], info["hubs_block"]) == (2 + extra, 1, 0), (odd, info)
    g = star_graph([HubSpec(65, 5, 0), HubSpec(65, 5, 0, "general", 6)], seed=3)       # 6 others: still of the form
    assert _plan(g)[2]["hubs_ep"] == 2


def test_no_heavy_puts_every_hub_on_the_one_lane_kernel(monkeypatch):
    g = build_case("wave65")
    base = _plan(g)[2]
    monkeypatch.setenv("NSK_DIAG", "1")
    monkeypatch.setenv("NSK_NO_HEAVY", "1")
    info = _plan(g)[2]
    assert base["hubs"] == 6 and info["hubs"] == info["hubs_ep"] == info["hubs_block"] == 0
    assert info["ngeneric"] == base["ngeneric"] == 6


def test_hub_counters_of_the_parity_graphs(golden):
    """tests/test_hip_parity.py's graphs with hubs: `hubs` tests the generic walk only (its hubs of 300 and 400 entries
    exceed the 256-entry cap of their colours, the third is a labelling-function factor's), the clipped-window ends
    of the LR graphs the workgroup route in a single chunk.  The other routes and edges: tests/test_hubs_gpu.py."""
    import test_hip_parity as thp
    graphs = thp._small_graphs(golden)
    want = {"hubs": (203, 0, 0), "lr3000": None, "lr_bigcard": None, "lr_manyw": None}
    got = {}
    for name in want:
        g, hbv = graphs[name]
        info = _plan(g, hbv)[2]
        got[name] = (info["hubs"], info["hubs_ep"], info["hubs_block"])
    assert got["hubs"] == (203, 0, 0), got
    assert got["lr3000"][1:] == (2, 2) and got["lr_manyw"][1:] == (2, 2) and got["lr_bigcard"][1:] == (1, 1), got


def _oracle(g, color):
    ns, fg = session(g, head_by_vid=True)
    og = oracle_of(fg, True, layout=False)
    assert og.check_coloring(color) == (-1, -1)
    return og, phases_from_colors(color)


@pytest.mark.parametrize("se", [True, False], ids=["sample_evidence", "no_sample_evidence"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_inference_cases_are_lively_in_the_oracle(monkeypatch, name, se):
    set_switches(monkeypatch, name)
    g = build_case(name)
    og, (order, ps) = _oracle(g, _plan(g)[1])
    vv, cnt, live = oracle_inference(og, order, ps, 41, se, nhubs(name))
    live.check(g[1], se)


@pytest.mark.parametrize("name,cfg", LEARN_CASES)
def test_learning_cases_move_their_weights_in_the_oracle(monkeypatch, name, cfg):
    set_switches(monkeypatch, name)
    nweight, hubs_evidence = LEARN_CFG[cfg][4], LEARN_CFG[cfg][3]
    g = build_case(name, nweight=nweight, hubs_evidence=hubs_evidence)
    _, color, info = _plan(g)
    check_route(name, info)
    assert (info["direct_weights"] > 0) == (nweight == "per_factor") and info["learn_lag"] == (nweight == 7), info
    og, (order, ps) = _oracle(g, color)
    og.device_lag = bool(info["learn_lag"])
    oracle_learning(og, order, ps, 43, cfg)
