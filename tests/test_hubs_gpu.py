"""The hub kernels at their list-length and cardinality edges, bit-exact against the oracle (tests/hubs.py builds the
star graphs and holds the case table; tests/test_hubs_cpu.py plans every case on the host and checks its liveliness).

A hub -- a variable a whole wave or workgroup samples -- has four implementations, each with a learning twin:

- entry-parallel, one wave (heavy_update_ep / hub_potentials, learn_heavy_variable_ep): rounds of 64 entries --
  31, 32, 33, 64, 65, 128 entries, 129 and 256 under NSK_NO_EP, 256 in a colour that is no entry-parallel colour;
- entry-parallel, one workgroup (block_hub_update / block_hub_potentials, block_hub_learn): chunks of 1024 entries
  summed 16 at a time -- 129, 257, 1024, 1025 (one entry in the second chunk), 2100, 16384;
- the generic wave walk (heavy_update / wave_draw_sample, learn_heavy_variable): cardinality 9, 16, 17, 64, 65
  (the 64-lane draw against the two-pass draw), hubs with one LINEAR / RATIO factor or one factor of 7 others,
  general-form hubs past the caps or under NSK_NO_HUB_EP / NSK_NO_EP;
- one lane (draw_sample, k_learn_phase) under NSK_NO_HEAVY: cardinality 2, 3, 16, 17 (registers against two passes).

Every graph holds the six (cardinality, dataType) of general-tile form -- or the cardinalities of its route -- at one
list length, hubs 0 and 1 in different colours, hub 3 evidence; the factors that name a hub twice (role 3, partner
entries, codes 10 and 11) are part of every general-form hub.  Every test re-asserts its route from the handle's
counters, so that a change of the routing rules breaks it instead of hollowing it out."""

import numpy as np
import pytest

from util import session, oracle_of, phases_from_colors
from hubs import (CASES, EPOCHS, INFER, LEARN_CASES, LEARN_CFG, build_case, check_route, nhubs, oracle_inference,
                  oracle_learning, set_switches)

pytestmark = pytest.mark.gpu


def _session(monkeypatch, name, seed, **kw):
    set_switches(monkeypatch, name)
    g = build_case(name, **kw)
    ns, fg = session(g, seed=seed, head_by_vid=True)
    info = fg.info()
    check_route(name, info)
    assert info["value_bytes"] == (4 if CASES[name].wide else 1)
    color = fg.colors()
    assert color[0] != color[1]                              # hubs of a second colour: the base offsets of its hubs
    return g, fg, info, oracle_of(fg, True), phases_from_colors(color)


@pytest.mark.parametrize("se", [True, False], ids=["sample_evidence", "no_sample_evidence"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_hub_inference_equals_oracle(monkeypatch, name, se):
    g, fg, info, og, (order, ps) = _session(monkeypatch, name, 41)
    vv, cnt, live = oracle_inference(og, order, ps, 41, se, nhubs(name))
    fg.inference(INFER[0], INFER[1], se)
    n = nhubs(name)
    bad = np.nonzero(fg.var_value[0] != vv)[0]
    assert len(bad) == 0, (name, "differing variables (ids below %d are hubs)" % n, bad[:12], len(bad))
    assert np.array_equal(fg.count, cnt), name
    # the run was no still life (the hub-by-hub condition is tests/test_hubs_cpu.py's, on the oracle's own layout)
    sampled = sum(1 for h in range(n) if se or g[1][h]["isEvidence"] == 0)
    assert int(live.changes.sum()) >= 5 * sampled, live.changes


@pytest.mark.parametrize("name,cfg", LEARN_CASES)
def test_hub_learning_equals_oracle(monkeypatch, name, cfg):
    reg, trunc, lne, hubs_evidence, nweight = LEARN_CFG[cfg]
    g, fg, info, og, (order, ps) = _session(monkeypatch, name, 43, nweight=nweight, hubs_evidence=hubs_evidence)
    assert (info["direct_weights"] > 0) == (nweight == "per_factor") and info["learn_lag"] == (nweight == 7), info
    if nweight != "per_factor":
        assert (info["acc_copies"] & 15) == (8 if nweight == 300 else 1), info    # global XCD-private accumulators / LDS
    # (that half of the free weights move is tests/test_hubs_cpu.py's condition, on the oracle's own layout; here,
    # on the handle's layout, a quarter says the run was no still life)
    vv, ve, wv, vv2, cnt = oracle_learning(og, order, ps, 43, cfg, need=0.25)
    fg.learn(0, EPOCHS, 0.02, 0.9, reg, 0.05, trunc, learn_non_evidence=lne)
    assert np.array_equal(fg.var_value[0], vv), (name, np.nonzero(fg.var_value[0] != vv)[0][:12])
    assert np.array_equal(fg.var_value_evid[0], ve), (name, np.nonzero(fg.var_value_evid[0] != ve)[0][:12])
    bad = np.nonzero(fg.weight_value[0].view(np.uint64) != wv.view(np.uint64))[0]
    assert len(bad) == 0, (name, cfg, bad[:8], fg.weight_value[0][bad[:8]], wv[bad[:8]])
    fg.inference(0, 3, True)                                  # three sweeps from the learnt state
    assert np.array_equal(fg.var_value[0], vv2) and np.array_equal(fg.count, cnt), name


def test_one_graph_four_routes(monkeypatch):
    """The same six hubs of 200 entries through the workgroup kernels, the one-wave kernels (NSK_NO_EP), the generic
    wave walk (NSK_NO_HUB_EP) and the one-lane kernels (NSK_NO_HEAVY): four different routings by the counters, each
    equal to the oracle (which follows each handle's own layout and colours) in inference and in learning."""
    seen = set()
    for route in ("block", "wave", "walk", "lane"):
        name = "four200_" + route
        with monkeypatch.context() as mp:
            g, fg, info, og, (order, ps) = _session(mp, name, 47, hubs_evidence=True)
            seen.add((info["hubs"] > 0, info["hubs_ep"], info["hubs_block"]))
            vv, ve, wv, vv2, cnt = oracle_learning(og, order, ps, 47, "C", need=0.25)
            fg.learn(0, EPOCHS, 0.02, 0.9, 2, 0.05, 1, learn_non_evidence=True)
            assert np.array_equal(fg.var_value[0], vv) and np.array_equal(fg.var_value_evid[0], ve), route
            assert np.array_equal(fg.weight_value[0].view(np.uint64), wv.view(np.uint64)), route
            fg.inference(0, 3, True)
            assert np.array_equal(fg.var_value[0], vv2) and np.array_equal(fg.count, cnt), route
            fg.close()
    assert seen == {(True, 6, 6), (True, 6, 0), (True, 0, 0), (False, 0, 0)}
