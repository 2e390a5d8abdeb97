"""The tile families at their routing edges, bit-exact against the oracle (tests/tiles.py builds the graphs and holds
the case table; tests/test_tiles_cpu.py plans every case on the host and checks its liveliness in the oracle).

- general tiles walked one lane per variable (k_gibbs_general / k_learn_general): member widths 0 .. 3 on the walks
  specialised on the width, each at 1 entry, 16 entries and an entry count the compiler pads to the super-group;
  widths 4 .. 6 on the role walk; lanes shorter and narrower than their tile (padding entries, empty member slots whose
  gather reads internal id 0 -- which holds a non-zero categorical value there); 16 entries and 120 words a lane;
  cardinality 8 and dataType 1; dense_equal_to 31; the entries that name their variable twice (role 3, codes 10 and
  11, partner lists); literal heads; 1, 4 and 5 tiles a colour; int32 values;
- entry-parallel groups (k_gibbs_ep / k_learn_ep and their wide variants): 8 entries (one LDS pass), 9 and 16 (two);
  a class row of 64 and of 65 entries; member-less entries only; 1 part-filled tile, 4 tiles, 5; all-binary and
  categorical colours; int32 values; hubs of 40 and 130 entries and a shape tile in the same launch;
- shape tiles (the shape walks of k_gibbs_fast / k_learn_fast, k_refresh_shape_weights): 16 and 4 words a lane, exact
  shapes and padded ones whose null words stand in for members under OR, AND, EQUAL and IMPLY_NATURAL; the same
  graphs under NSK_NO_PAD_SHAPE and NSK_NO_SHAPE; both sides of the sliver rule.

Every test re-asserts the route of every target from the HANDLE's route words (nsk_graph_get_routes), so that a change
of a routing rule breaks it instead of hollowing it out."""

import numpy as np
import pytest

from util import session, oracle_of, phases_from_colors
from numbskull_amd import _lib
from tiles import CASES, LEARN_CFG, LEARN_PARAMS, MIXED_KINDS, build_case, check_case, set_switches

pytestmark = pytest.mark.gpu


def _session(monkeypatch, name, seed, extra=None, **kw):
    set_switches(monkeypatch, name, extra)
    g, targets = build_case(name, **kw)
    hbv = CASES[name].hbv
    ns, fg = session(g, seed=seed, head_by_vid=hbv)
    info, color = fg.info(), fg.colors()
    check_case(name, g, targets, color, fg.routes(), info, layout=fg.layout())
    return g, fg, info, oracle_of(fg, hbv), phases_from_colors(color)


def _inference(fg, og, order, ps, seed, se):
    """3 sweeps of burn-in, then 1 + 4: values after each call, tallies at the end."""
    vv, _, wv, cnt = og.initial_state()
    sweep = 0
    fg.burnIn(3, se)
    for _ in range(3):
        assert og.gibbs_dev(order, ps, vv, wv, cnt, seed, sweep, se, burnin=True) == 0
        sweep += 1
    assert np.array_equal(fg.var_value[0], vv), np.nonzero(fg.var_value[0] != vv)[0][:12]
    for rounds in (1, 4):
        fg.inference(0, rounds, se)
        for _ in range(rounds):
            assert og.gibbs_dev(order, ps, vv, wv, cnt, seed, sweep, se) == 0
            sweep += 1
        bad = np.nonzero(fg.var_value[0] != vv)[0]
        assert len(bad) == 0, ("differing variables", bad[:12], len(bad))
        assert np.array_equal(fg.count, cnt)


def _learning(fg, og, order, ps, seed, reg, trunc, lne):
    """Chunks of 1 + 3 epochs: both chains and the weights after each."""
    vv, ve, wv, _ = og.initial_state()
    step, sweep = 0.02, 0
    for chunk in (1, 3):
        fg.learn(0, chunk, step, 0.9, reg, 0.05, trunc, learn_non_evidence=lne)
        assert og.learn_call(order, ps, vv, ve, wv, chunk, step, 0.9, reg, 0.05, trunc, lne, seed, sweep) == 0
        step *= 0.9 ** chunk
        sweep += chunk
        assert np.array_equal(fg.var_value[0], vv), np.nonzero(fg.var_value[0] != vv)[0][:12]
        assert np.array_equal(fg.var_value_evid[0], ve), np.nonzero(fg.var_value_evid[0] != ve)[0][:12]
        bad = np.nonzero(fg.weight_value[0].view(np.uint64) != wv.view(np.uint64))[0]
        assert len(bad) == 0, (bad[:8], fg.weight_value[0][bad[:8]], wv[bad[:8]])
    assert np.any(wv != og.weight["initialValue"])


@pytest.mark.parametrize("se", [True, False], ids=["sample_evidence", "no_sample_evidence"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_tile_inference_equals_oracle(monkeypatch, name, se):
    g, fg, info, og, (order, ps) = _session(monkeypatch, name, 41)
    _inference(fg, og, order, ps, 41, se)


@pytest.mark.parametrize("name,cfg", LEARN_PARAMS)
def test_tile_learning_equals_oracle(monkeypatch, name, cfg):
    reg, trunc, lne, nweight, extra = LEARN_CFG[cfg]
    g, fg, info, og, (order, ps) = _session(monkeypatch, name, 43, extra, nweight=nweight, learn=lne)
    nw = len(g[0])
    assert info["learn_lag"] == int(nw <= 256), info
    if nw == len(g[2]) and nw > 256:                              # one weight per factor: updated in place, in layout order
        assert info["direct_weights"] > 0 and info["weight_slots"] == 1, info     # (ep_row64 / ep_row65 alone have too few)
    else:
        assert info["direct_weights"] == 0, info
        assert (info["acc_copies"] & 15) == (1 if nw <= 256 or extra == "NSK_ONE_ACC" else 8), info
    _learning(fg, og, order, ps, 43, reg, trunc, lne)


def test_one_graph_every_route(monkeypatch):
    """tests/tiles.py "mixed_routes": a padded shape tile, general tiles on both walks and a hub in the targets' colour,
    entry-parallel groups beside a shape tile in the leaves' colours, generic-path leaves on the wave walk -- learning,
    then inference from the learnt state, on one handle."""
    g, fg, info, og, (order, ps) = _session(monkeypatch, "mixed_routes", 47, learn=True)
    f = _lib.route_fields(fg.routes().astype(np.int64))
    assert MIXED_KINDS <= set(np.unique(f["kind"]).tolist())
    assert info["tiles_shape_padded"] >= 1 and info["ep_groups"] >= 1 and info["tiles_general_roles"] >= 1
    assert info["tiles_general"] > info["tiles_general_roles"] and info["hubs_ep"] >= 1 and info["hubs"] > info["hubs_ep"]
    vv, ve, wv, cnt = og.initial_state()
    fg.learn(0, 4, 0.02, 0.9, 2, 0.05, 1, learn_non_evidence=True)
    assert og.learn_call(order, ps, vv, ve, wv, 4, 0.02, 0.9, 2, 0.05, 1, True, 47, 0) == 0
    assert np.array_equal(fg.var_value[0], vv) and np.array_equal(fg.var_value_evid[0], ve)
    assert np.array_equal(fg.weight_value[0].view(np.uint64), wv.view(np.uint64)) and np.any(wv != og.weight["initialValue"])
    fg.inference(0, 3, True)
    for s in range(4, 7):
        assert og.gibbs_dev(order, ps, vv, wv, cnt, 47, s, True) == 0
    assert np.array_equal(fg.var_value[0], vv) and np.array_equal(fg.count, cnt)
