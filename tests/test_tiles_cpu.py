"""Host-only plans of the edge graphs of tests/tiles.py: the route of EVERY target of every case, read from the plan's
route words (nsk_graph_plan_routes) and checked against the plan's tile / group counters; the same counters of the
parity tests' graphs, so that what those cover cannot drift unseen; and the liveliness of every case in the oracle's
own run -- lanes that never moved, or weights that never changed, would let a parity test pass for nothing."""

import numpy as np
import pytest

from conftest import graph_from  # noqa: F401
from util import session, oracle_of, phases_from_colors
from numbskull_amd import _lib
import tiles
from tiles import CASES, LEARN_CASES, LEARN_CFG, GENERAL, GROUP, SHAPE, LANE, HUB, build_case, check_case, set_switches


def _plan(name, **kw):
    g, targets = build_case(name, **kw)
    ns, fg = session(g, head_by_vid=CASES[name].hbv)
    color, info = fg.plan()
    return g, targets, fg, color, fg.plan_routes(), info


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_target_takes_the_intended_route(monkeypatch, name):
    set_switches(monkeypatch, name)
    g, targets, fg, color, routes, info = _plan(name)
    check_case(name, g, targets, color, routes, info)
    # the builder made the lists it was asked for
    for (size, spec, expect), fam in zip(CASES[name].families, targets):
        if "own_entries" in expect:
            assert tiles.entries_of(g, int(fam[0])) == tiles.entries_of(g, int(fam[-1])) == expect["own_entries"]
    assert len(g[1]) <= 4200


def _families(pred):
    """(case, size, spec, expect) of every family whose expectation satisfies pred."""
    return [(n, s, t, e) for n, cs in CASES.items() for s, t, e in cs.families if pred(e)]


def test_every_route_has_its_cases_on_both_sides_of_every_boundary():
    """What the table must keep: each tile family at the sizes next to each routing boundary, and the cases just
    past every boundary on the route that takes over."""
    gens = _families(lambda e: e.get("kind") == GENERAL and e.get("tile_width") is not None)
    grps = _families(lambda e: e.get("kind") == GROUP)
    shps = _families(lambda e: e.get("kind") == SHAPE)
    offs = {n for n, s, t, e in _families(lambda e: e.get("kind") == HUB)}
    # general tiles: every member width, on both walks; E = 1, 16 and an E the compiler has to pad, per width M <= 3
    assert {e["tile_width"] for _, _, _, e in gens} == {0, 1, 2, 3, 4, 5, 6}
    for M in (0, 1, 2, 3):
        own = {e["own_entries"] for _, _, _, e in gens if e["tile_width"] == M}
        assert {1, 16} <= own, (M, own)
        assert any(e["own_entries"] != e["tile_entries"] for _, _, _, e in gens if e["tile_width"] == M) or M == 2, M
    assert {"gen_m7_off", "gen_e17_off", "gen_w121_off", "gen_card9_dt0_off", "gen_card9_dt1_off", "gen_deo32_off",
            "gen_or_two_of_three_off", "gen_three_own_off", "ep_beside_e17"} <= offs
    assert {"gen_w120", "gen_card8_dt0", "gen_card8_dt1", "gen_deo31", "gen_card2_dt1", "gen_pad_null", "gen_literal_heads",
            "gen_self_dt0", "gen_self_binary", "gen_self_partner7"} <= {n for n, _, _, _ in gens}
    # lanes narrower and shorter than their tile: padding entries and empty member slots
    assert any(e["own_width"] < e["tile_width"] and e["own_entries"] < e["tile_entries"] for _, _, _, e in gens)
    assert {1, 256, 257} <= {s for n, s, _, _ in gens if n.startswith("gen_tiles_")}
    assert any(CASES[n].env == () for n, _, _, e in gens if e["tile_width"] == 3), "a colour kept off the groups without NSK_NO_EP"
    assert any("NSK_NO_EP" in CASES[n].env for n, _, _, e in gens)
    # groups: 8 entries (one pass), 9 and 16 (two); a class row of 64 and of 65 entries; 1, 4 and 5 tiles
    assert {8, 9, 16} <= {e["tile_entries"] for _, _, _, e in grps}
    assert {0, 1} == {e["two_pass"] for _, _, _, e in grps}
    assert {(64, 1), (65, 1)} <= {(s, e["own_entries"]) for n, s, _, e in grps if n.startswith("ep_row")}
    assert {1, 63, 256, 257} <= {s for n, s, _, _ in grps if n.startswith("ep_tiles_")}
    assert any(e["own_width"] == 0 and n == "ep_m0_only" for n, _, _, e in grps)
    assert any(t.card == 8 and t.dtype == 1 and e["tile_entries"] == 16 for _, _, t, e in grps)
    assert any(CASES[n].wide for n, _, _, _ in grps) and any(CASES[n].wide for n, _, _, _ in gens)
    assert any(t.card == 2 for n, _, t, _ in grps if n == "ep_binary_only") and any(t.card > 2 for _, _, t, _ in grps)
    # shape tiles: 16 against 17 words, 4 against 5, 64 against 63 members, null words under each function, the switches
    words = lambda t: sum(1 + e.others for e in t.entries)
    assert {4, 16} <= {words(t) for _, _, t, _ in shps}
    assert words(CASES["shape_w17_off"].families[0][1]) == 17 and words(CASES["shape_ep_w5_off"].families[0][1]) == 5
    assert CASES["shape_w17_off"].families[0][2]["kind"] == GENERAL and CASES["shape_ep_w5_off"].families[0][2]["kind"] == GROUP
    assert {0, 1} == {e["null_word"] for _, _, _, e in shps}
    for fn, n in ((1, "or"), (2, "and"), (3, "equal"), (0, "imply")):
        fams = CASES["shape_pad_" + n].families
        assert {e["null_word"] for _, _, e in fams} == {0, 1} and all(x.fn == fn for _, t, _ in fams for x in t.entries)
        assert all(e["kind"] == GENERAL for _, _, e in CASES["shape_pad_%s_nopad" % n].families)
    assert CASES["shape_exact64"].families[0][0] == 64 and CASES["shape_exact63_general"].families[0][0] == 63
    assert CASES["shape_w16_noshape"].families[0][2]["kind"] == LANE
    assert CASES["sliver_keeps"].families[0][2]["kind"] == SHAPE and CASES["sliver_gives_up"].families[0][2]["kind"] == GENERAL
    # learning: each family on both sides of its main boundaries, and enough factors that one weight per factor means
    # weights updated in place (more than 256; the two class-row cases have 64 and 65 entries by definition)
    assert {"gen_m3_e16", "gen_m4", "ep_e8", "ep_e9", "ep_m3_e16", "ep_row64", "ep_row65", "shape_w16", "shape_pad_or"} <= set(LEARN_CASES)
    assert all(tiles.nfactors(n) > 256 for n in LEARN_CASES if not n.startswith("ep_row"))
    assert {c for _, c in tiles.LEARN_PARAMS} == set(LEARN_CFG)
    sizes = {s for cs in CASES.values() for s, _, _ in cs.families}
    assert set(tiles.SIZES) <= sizes


def test_a_literal_head_that_names_an_unrelated_variable_keeps_the_colours_valid(monkeypatch):
    """gen_literal_heads: every positional factor reads its head at the edge index, which names one of the isolated
    variables in front -- a read that is not mutual and that greedy colouring in id order satisfies by accident (the
    variable read comes first).  The recolouring and balancing passes used to put reader and read into one class."""
    set_switches(monkeypatch, "gen_literal_heads")
    g, targets, fg, color, routes, info = _plan("gen_literal_heads")
    og = oracle_of(fg, False, layout=False)
    assert og.check_coloring(color) == (-1, -1)
    heads = g[2]["ftv_offset"] + g[2]["arity"] - 1              # the variables the heads are read at: isolated ones
    assert (heads < CASES["gen_literal_heads"].pad_front).all()
    assert (color[heads] != color[np.repeat(targets[0], 3)]).all()      # (factor 3 t + i is target t's)


def test_the_mixed_graph_holds_every_route():
    g, targets, fg, color, routes, info = _plan("mixed_routes")
    f = _lib.route_fields(routes.astype(np.int64))
    leaves = np.ones(len(routes), bool)
    leaves[np.concatenate(targets)] = False
    assert tiles.MIXED_KINDS <= set(np.unique(f["kind"]).tolist())
    assert {GROUP, HUB} <= set(np.unique(f["kind"][leaves]).tolist())
    assert info["tiles_shape_padded"] >= 1 and info["ep_groups"] >= 1 and info["tiles_general_roles"] >= 1
    assert info["tiles_general"] > info["tiles_general_roles"] and info["hubs"] > info["hubs_ep"] >= 1


def test_the_sliver_rule_is_a_count_of_the_colour(monkeypatch):
    """nfast * 20 < ngt: 64 classed variables keep their shape tile beside 1280 general ones and lose it beside 1281."""
    set_switches(monkeypatch, "sliver_keeps")
    for n, kind in ((1280, SHAPE), (1281, GENERAL)):
        fam = [(64, CASES["sliver_keeps"].families[0][1]), (n, CASES["sliver_keeps"].families[1][1])]
        g, targets = tiles.tile_graph(fam, nweight="per_factor", seed=n)
        ns, fg = session(g, head_by_vid=True)
        color, info = fg.plan()
        assert len(set(color[np.concatenate(targets)].tolist())) == 1
        assert (_lib.route_fields(fg.plan_routes().astype(np.int64))["kind"][targets[0]] == kind).all(), n


def test_tile_counters_of_the_parity_graphs(golden):
    """tests/test_hip_parity.py's random graphs: which of the tile families each of them reaches at all.  Relations
    that hold by the way the graphs are drawn; the edges themselves are tests/test_tiles_gpu.py's."""
    import test_hip_parity as thp
    graphs = thp._small_graphs(golden)
    got = {}
    for name in ("gencat", "gencat4", "lr3000", "lr_selfdup", "boolw"):
        g, hbv = graphs[name]
        ns, fg = session(g, head_by_vid=hbv)
        color, info = fg.plan()
        tiles.check_counters(color, fg.plan_routes(), info)
        got[name] = info
    # arity up to 5: entries of 4 others, so no colour of gencat is laid out as groups and some tiles take the role walk
    assert got["gencat"]["ep_groups"] == 0 and got["gencat"]["tiles_general_roles"] > 0
    assert got["gencat"]["tiles_general"] > got["gencat"]["tiles_general_roles"]
    # arity up to 4: every colour on the groups -- but 1700 factors over 2000 variables make no list longer than 8
    # entries: gencat4 never takes a group's second pass (ep_e9, ep_m3_e16, ep_e16_dt1_card8 do)
    assert got["gencat4"]["tiles_general"] == 0 and got["gencat4"]["ep_groups"] > 0 and got["gencat4"]["ep_groups_two_pass"] == 0
    # the LR graphs: groups only, two-pass ones among them
    for name in ("lr3000", "lr_selfdup"):
        assert got[name]["ep_groups"] > 0 and got[name]["tiles_general"] == 0, (name, got[name])
        assert 0 < got[name]["ep_groups_two_pass"] < got[name]["ep_groups"], (name, got[name])
    # one weight per factor on 6000 variables: no shape of boolw has 64 members in a colour, so every variable ends on
    # the general tiles (most of them on the role walk) and NONE on a shape tile -- the shape tiles' parity cover is
    # test_shape_classes_per_id_range and the shape_* cases of tests/tiles.py
    assert got["boolw"]["tiles_shape"] == 0 and got["boolw"]["ep_groups"] == 0
    assert 0 < got["boolw"]["tiles_general_roles"] < got["boolw"]["tiles_general"]
    assert all(got[n]["tiles_shape"] == 0 and got[n]["tiles_lane"] == 0 for n in got)


# ------------------------------------------------------------------------------------------------------ liveliness
def _oracle(fg, color, hbv):
    og = oracle_of(fg, hbv, layout=False)
    assert og.check_coloring(color) == (-1, -1)
    return og, phases_from_colors(color)


@pytest.mark.parametrize("se", [True, False], ids=["sample_evidence", "no_sample_evidence"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_inference_cases_are_lively_in_the_oracle(monkeypatch, name, se):
    """After 41 sweeps, of every 64 consecutive targets of a family that are sampled at all at least half have
    changed their value; with cardinality 8 every value is taken by some target."""
    set_switches(monkeypatch, name)
    g, targets, fg, color, routes, info = _plan(name)
    og, (order, ps) = _oracle(fg, color, CASES[name].hbv)
    changes, seen = tiles.oracle_live_inference(og, order, ps, 41, se)
    for (size, spec, expect), fam in zip(CASES[name].families, targets):
        for i in range(0, size, 64):
            lanes = fam[i:i + 64]
            lanes = lanes[(g[1]["isEvidence"][lanes] == 0) | se]
            assert 2 * int((changes[lanes] > 0).sum()) >= len(lanes), (name, i, int((changes[lanes] > 0).sum()), len(lanes))
        held = fam[(g[1]["isEvidence"][fam] != 0) & (not se)]
        assert (changes[held] == 0).all()
        if spec.card == 8 and (se or not spec.evidence):
            assert set(np.unique(seen[:, fam]).tolist()) == set(range(8)), name


@pytest.mark.parametrize("name,cfg", tiles.LEARN_PARAMS)
def test_learning_cases_move_their_weights_in_the_oracle(monkeypatch, name, cfg):
    reg, trunc, lne, nweight, extra = LEARN_CFG[cfg]
    set_switches(monkeypatch, name, extra)
    g, targets, fg, color, routes, info = _plan(name, nweight=nweight, learn=lne)
    check_case(name, g, targets, color, routes, info)
    og, (order, ps) = _oracle(fg, color, CASES[name].hbv)
    og.device_lag = bool(info["learn_lag"])
    vv, ve, wv, _ = og.initial_state()
    step, sweep = 0.02, 0
    for chunk in (1, 3):
        assert og.learn_call(order, ps, vv, ve, wv, chunk, step, 0.9, reg, 0.05, trunc, lne, 43, sweep) == 0
        step *= 0.9 ** chunk
        sweep += chunk
    free = og.weight["isFixed"] == 0
    moved = wv[free] != og.weight["initialValue"][free]
    assert 2 * int(moved.sum()) >= int(free.sum()), (name, cfg, int(moved.sum()), int(free.sum()))
