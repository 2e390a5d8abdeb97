"""The later trips of the class launches' persistent grids, bit-exact against the oracle (tests/class_trips.py builds the
graphs and restates the kernels' index arithmetic; tests/test_class_trips_cpu.py shows from the host-only plans that
under the cap each case's waves make a third trip, and that the oracle's run is lively).

Every case runs under NSK_DIAG=1 NSK_CLASS_GRID_CAP=1 -- one workgroup, or one round of 8 for the tile and group
launches --, four of them also at 3 (12 waves: no power of two), and once more with the cap unset: values of both
chains and weights equal the oracle's after every chunk, the sums being order-independent fixed point, and so the capped
and the uncapped handle equal each other -- the grid is no part of the semantics.  What a wrong stride, a wrong `per`
or a wrong chunk row would do -- skip tiles, sample them twice, apply an in-place weight update twice -- shows in the
first compared state: every run of 64 positions of the class under test holds a variable that has left its initial
value by then.

- generic_range / dyn_list: k_learn_phase in range and in list mode; hubs_alone: k_learn_heavy;
- general_tiles (7 weights: LDS tables accumulated over the trips; 300: per-XCD global copies; one weight per factor:
  updated in place; int32 values), general_binary: the tile walk of k_learn_general<8> / <2>; general_hubs_rest: its hub
  blocks (the first tile block off XCD 0) and the run of learn-rest tiles per wave;
- fast_rest: k_learn_fast; ep_rest: the rest walk of learn_ep_body behind the groups;
- ep_two_rows: ep_walk / ep_group over two chunk rows -- k_learn_ep_w4 and, in inference, k_gibbs_ep_w5.

Slowest on an MI355X, each with its two or three handles and the oracle's run (all 87 tests of the module: 26 s):
  test_learning_trips_equal_the_oracle[ep_two_rows-w7-l1_trunc2]       1.90 s
  test_learning_trips_equal_the_oracle[ep_rest-wper_factor-l1_trunc2]  1.78 s
  test_learning_trips_equal_the_oracle[ep_two_rows-w7-l2]              1.73 s"""

import numpy as np
import pytest

from util import session, oracle_of, phases_from_colors
import class_trips as ct
from class_trips import CASES, PARAMS, SETTINGS

pytestmark = pytest.mark.gpu


def _handle(monkeypatch, name, g, marks, cap):
    """A fresh handle under the case's switches and the cap (None: unset), its class under test checked."""
    ct.set_switches(monkeypatch, name, cap)
    cs = CASES[name]
    ns, fg = session(g, seed=ct.SEED, head_by_vid=cs.hbv)
    info, color = fg.info(), fg.colors()
    nw = len(g[0])
    assert info["value_bytes"] == (4 if cs.wide else 1)
    assert info["learn_lag"] == int(nw <= 256), info
    if info["direct_weights"] == 0:
        assert (info["acc_copies"] & 15) == (1 if nw <= 256 else 8), info
    plan = fg.plan()[1]
    for key in ("direct_weights", "weight_slots", "hubs", "hubs_ep", "hubs_block", "tiles_shape", "tiles_lane", "tiles_general", "ep_groups",
                "ep_groups_two_pass", "ncolors", "nfast", "ngeneric"):
        assert info[key] == plan[key], (key, info[key], plan[key])
    if nw == len(g[2]) and nw > 256:
        assert info["direct_weights"] > 0 and info["weight_slots"] == 1, info        # one weight per factor: updated in place
    return fg, info, color


def _oracle_learning(og, order, ps, reg, trunc, lne):
    """The states the device is compared with: (values, evidence-chain values, weights) after each chunk."""
    vv, ve, wv, _ = og.initial_state()
    step, sweep, out = ct.STEP, 0, []
    for chunk in ct.CHUNKS:
        assert og.learn_call(order, ps, vv, ve, wv, chunk, step, ct.DECAY, reg, ct.REG_PARAM, trunc, lne, ct.SEED, sweep) == 0
        step *= ct.DECAY ** chunk
        sweep += chunk
        out.append((vv.copy(), ve.copy(), wv.copy()))
    return out


def _learn_and_compare(fg, want, reg, trunc, lne, tag):
    step = ct.STEP
    for chunk, (vv, ve, wv) in zip(ct.CHUNKS, want):
        fg.learn(0, chunk, step, ct.DECAY, reg, ct.REG_PARAM, trunc, learn_non_evidence=lne)
        step *= ct.DECAY ** chunk
        bad = np.nonzero(fg.var_value[0] != vv)[0]
        assert len(bad) == 0, (tag, "values", bad[:12], len(bad))
        bad = np.nonzero(fg.var_value_evid[0] != ve)[0]
        assert len(bad) == 0, (tag, "evidence-chain values", bad[:12], len(bad))
        bad = np.nonzero(fg.weight_value[0].view(np.uint64) != wv.view(np.uint64))[0]
        assert len(bad) == 0, (tag, "weights", bad[:8], fg.weight_value[0][bad[:8]], wv[bad[:8]])
    return fg.var_value[0].copy(), fg.var_value_evid[0].copy(), fg.weight_value[0].copy()


def _every_run_of_64_is_lively(name, r, ids, color, k, init, first):
    """Positions of the class under test that its launch samples, in runs of 64: each holds a variable whose value
    after the first epoch differs from its initial one in one of the two chains."""
    p0, p1 = ct.positions(r, CASES[name].launch)
    here = np.nonzero((np.asarray(color) == k) & (ids >= p0) & (ids < p1))[0]
    assert len(here) > 0
    moved = (first[0][here] != init[here]) | (first[1][here] != init[here])
    run = (ids[here] - p0) // 64
    live = np.bincount(run[moved], minlength=int(run.max()) + 1) > 0
    held = np.bincount(run, minlength=int(run.max()) + 1) > 0
    assert (live | ~held).all(), (name, "runs of 64 positions where nothing moved", np.nonzero(held & ~live)[0][:8])


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("name,w", PARAMS, ids=ct.ids(PARAMS))
def test_learning_trips_equal_the_oracle(monkeypatch, name, w, setting):
    reg, trunc, lne = SETTINGS[setting]
    cs = CASES[name]
    g, marks = cs.build(w, lne)
    want, ends = None, {}
    for cap in cs.caps + (None,):
        fg, info, color = _handle(monkeypatch, name, g, marks, cap)
        if cap:
            k, r = ct.check_class(name, cap, color, fg.routes(), fg.plan_classes(True, reg, cap), marks)
        if want is None:                                   # the oracle's run, once: the layout does not depend on the cap
            og = oracle_of(fg, cs.hbv)
            order, ps = phases_from_colors(color)
            want = _oracle_learning(og, order, ps, reg, trunc, lne)
            init = og.initial_state()[0]
            layout = fg.layout()
            _every_run_of_64_is_lively(name, r, layout, color, k, init, want[0])
            assert np.any(want[-1][2] != og.weight["initialValue"])
        else:
            assert np.array_equal(fg.layout(), layout)
        ends[cap] = _learn_and_compare(fg, want, reg, trunc, lne, (name, w, setting, "cap", cap))
    for cap in cs.caps:                                    # the twin without the cap: bit-identical
        for a, b in zip(ends[cap], ends[None]):
            assert a.tobytes() == b.tobytes(), (name, w, setting, "capped and uncapped runs differ", cap)


@pytest.mark.parametrize("se", [True, False], ids=["sample_evidence", "no_sample_evidence"])
def test_group_walk_inference_equals_the_oracle(monkeypatch, se):
    """ep_two_rows in inference: 3 sweeps of burn-in and 4 tallied ones under the cap and without it."""
    name, w = "ep_two_rows", 2000
    cs = CASES[name]
    g, marks = cs.build(w, True)
    want, ends = None, {}
    for cap in (1, None):
        fg, info, color = _handle(monkeypatch, name, g, marks, cap)
        if cap:
            k, r = ct.class_under_test(fg.plan_classes(False, 0, cap), "ep", color, marks)
            assert r["gen_ep"] and r["gen_gblocks"] == 8 and r["ngroups"] >= 129 + 5
        if want is None:
            og = oracle_of(fg, cs.hbv)
            order, ps = phases_from_colors(color)
            vv, _, wv, cnt = og.initial_state()
            want = []
            for s in range(7):
                assert og.gibbs_dev(order, ps, vv, wv, cnt, ct.SEED, s, se, burnin=s < 3) == 0
                if s in (2, 6):
                    want.append((vv.copy(), cnt.copy()))
            assert want[1][1].any()
        fg.burnIn(3, se)
        bad = np.nonzero(fg.var_value[0] != want[0][0])[0]
        assert len(bad) == 0, ("cap", cap, "values after burn-in", bad[:12], len(bad))
        fg.inference(0, 4, se)
        bad = np.nonzero(fg.var_value[0] != want[1][0])[0]
        assert len(bad) == 0, ("cap", cap, "values", bad[:12], len(bad))
        assert np.array_equal(fg.count, want[1][1]), ("cap", cap, "tallies")
        ends[cap] = (fg.var_value[0].copy(), np.asarray(fg.count).copy())
    assert np.array_equal(ends[1][0], ends[None][0]) and np.array_equal(ends[1][1], ends[None][1])
