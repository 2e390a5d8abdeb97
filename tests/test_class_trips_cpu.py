"""What the host-only plans say about the cases of tests/class_trips.py -- the conditions that make each of them worth
running on the device under NSK_CLASS_GRID_CAP (tests/test_class_trips_gpu.py):

- the class under test routes where the case says (nsk_graph_plan_routes) and gets the launch the case names
  (nsk_graph_plan_classes with the cap as its argument);
- with the kernels' index arithmetic restated in numpy (class_trips.WALKS), every item of the launch falls to exactly
  one wave -- which checks the restatement against the plan's counts --, some wave makes three trips or more and some
  wave one fewer; a launch that gives each wave a contiguous run gives runs of two or more with a last one short or
  empty; a general launch behind hub blocks starts its tiles off XCD 0; the groups of the two-row case fill a second
  chunk row and one workgroup walks both;
- liveliness in the oracle alone, over the epochs the device test compares: nine in ten of the class's free variables
  leave their initial value in some compared state, and every free weight a factor of the class reads changes.

And, with the cap unset, the plans of three of tests/test_hip_parity.py's graphs against grids derived by hand from the
launch rules as they stood before the cap existed."""

import numpy as np
import pytest

from util import session, oracle_of, phases_from_colors
from numbskull_amd import _lib
import class_trips as ct
from class_trips import CASES, PARAMS, WALKS, ALSO


def _plan(monkeypatch, name, w, lne=True):
    ct.set_switches(monkeypatch, name, None)
    g, marks = CASES[name].build(w, lne)
    ns, fg = session(g, head_by_vid=CASES[name].hbv)
    color, info = fg.plan()
    return g, marks, fg, color, info


def check_trips(launch, r, cap):
    """The walk of one launch of a class: every item exactly once, and the later trips the case is there for."""
    walk, field, runs = WALKS[launch]
    waves = walk(r, cap)
    items = np.concatenate(waves)
    assert np.array_equal(np.sort(items), np.arange(r[field])), (launch, "an item is skipped or taken twice")
    trips = np.array([len(x) for x in waves])
    if runs:
        per = int(trips.max())
        assert per >= 2 and (trips < per).any(), (launch, trips.tolist())
        assert all(len(x) == 0 or np.array_equal(x, np.arange(x[0], x[0] + len(x))) for x in waves)
    else:
        assert trips.max() >= 3, (launch, trips.tolist())
        if launch != "ep":                                      # (a workgroup's groups: whole chunks of 16)
            assert (trips == trips.max() - 1).any(), (launch, trips.tolist())
    return waves


@pytest.mark.parametrize("name,w", PARAMS, ids=ct.ids(PARAMS))
def test_the_class_under_test_makes_later_trips(monkeypatch, name, w):
    cs = CASES[name]
    g, marks, fg, color, info = _plan(monkeypatch, name, w)
    routes = fg.plan_routes()
    assert info["value_bytes"] == (4 if cs.wide else 1)
    for cap in cs.caps:
        k, r = ct.check_class(name, cap, color, routes, fg.plan_classes(True, 2, cap), marks)
        for launch in (cs.launch,) + ALSO.get(name, ()):
            waves = check_trips(launch, r, cap)
            if launch == "ep" and name == "ep_two_rows":
                assert any((x < 128).any() and (x >= 128).any() for x in waves), "no workgroup walks both chunk rows"
        # uncapped, every wave of these launches makes one trip or none -- what every other parity graph gives -- (a
        # workgroup of the group walk two at most: chunks of 16 groups go to an XCD whole)
        k0, r0 = ct.class_under_test(fg.plan_classes(True, 2, 0), cs.launch, color, marks)
        assert k0 == k
        for launch in (cs.launch,) + ALSO.get(name, ()):
            assert max(len(x) for x in WALKS[launch][0](r0, 0)) <= (2 if launch == "ep" else 1), (name, launch)
    # the inference group walk shares ep_walk: capped to one round as well
    if name == "ep_two_rows":
        k, r = ct.class_under_test(fg.plan_classes(False, 0, 1), "ep", color, marks)
        assert r["gen_gblocks"] == 8 and r["gen_rblocks"] == -(-r["gen_nrest"] // 4)
        check_trips("ep", r, 1)


@pytest.mark.parametrize("setting", sorted(ct.SETTINGS))
@pytest.mark.parametrize("name,w", PARAMS, ids=ct.ids(PARAMS))
def test_cases_are_lively_in_the_oracle(monkeypatch, name, w, setting):
    """The oracle's own run over CHUNKS, from the host-only plan (the device test hands the oracle the handle's layout:
    other draws, the same distribution)."""
    reg, trunc, lne = ct.SETTINGS[setting]
    cs = CASES[name]
    g, marks, fg, color, info = _plan(monkeypatch, name, w, lne)
    k, r = ct.class_under_test(fg.plan_classes(True, reg, 1), cs.launch, color, marks)
    og = oracle_of(fg, cs.hbv, layout=False)
    assert og.check_coloring(color) == (-1, -1)
    og.device_lag = bool(info["learn_lag"])
    order, ps = phases_from_colors(color)
    vv, ve, wv, _ = og.initial_state()
    init = vv.copy()
    moved = np.zeros(len(vv), bool)
    step, sweep = ct.STEP, 0
    for chunk in ct.CHUNKS:
        assert og.learn_call(order, ps, vv, ve, wv, chunk, step, ct.DECAY, reg, ct.REG_PARAM, trunc, lne, ct.SEED, sweep) == 0
        step *= ct.DECAY ** chunk
        sweep += chunk
        moved |= (vv != init) | (ve != init)
    var = g[1]
    here = color == k
    free = here & (var["isEvidence"] == 0)
    if lne:
        assert free.sum() >= 64, (name, "no free variables in the class under test")
    if free.any():
        assert 10 * int(moved[free].sum()) >= 9 * int(free.sum()), (name, int(moved[free].sum()), int(free.sum()))
    assert 2 * int(moved[here].sum()) >= int(here.sum())
    # the free weights of the factors the class visits every epoch: those with a member in it that takes part (evidence,
    # or any under learn_non_evidence) and is of dataType 0 -- a dataType-1 variable visits the lists of its two
    # chains' values only
    fac, fm = g[2], g[3]
    fid = np.repeat(np.arange(len(fac)), fac["arity"])
    mem = fm["vid"]
    visited = here[mem] & ((var["isEvidence"][mem] != 0) | lne) & (var["dataType"][mem] == 0)
    nvisit = np.bincount(fac["weightId"][fid[visited]], minlength=len(g[0]))
    free_w = g[0]["isFixed"] == 0
    reads = (nvisit > 0) & free_w
    changed = wv != g[0]["initialValue"]
    assert reads.any() and (g[0]["initialValue"][reads] != 0).all()
    if reg == 2:
        # L2: a visited weight that is not 0 shrinks at every update, whatever its gradient -- every one of them changes
        assert changed[reads].all(), (name, int(changed[reads].sum()), int(reads.sum()))
    else:
        # L1 with truncation 2 shrinks a weight at a visit with probability 1 / 2, no regulariser never: a weight with
        # one factor keeps its value while that factor has the same value in both chains (and no coin falls).  The
        # weights many factors share (64 or more visits an epoch) all change but for exact cancellation: nine in ten
        shared = reads & (nvisit >= 64)
        assert changed[reads].any()
        assert 10 * int(changed[shared].sum()) >= 9 * int(shared.sum()), (name, int(changed[shared].sum()), int(shared.sum()))


def test_uncapped_plans_of_three_parity_graphs():
    """grid_cap = 0: the grids the sweep drivers launched before the cap existed, by hand from the launch rules.
    generic_lanes: 32832 positions of one colour -- 513 items of 64, ceil(513 / 4) = 129 blocks (learning); 32832 / 256
    = 128.25, 129 blocks (inference).  pairs_manyw: 300 variables a colour, 5 tiles -- ceil(5 / 4) = 2 blocks of
    k_learn_fast, one round of 8 of k_gibbs_fast.  boolw_hub: 11 all-binary general tiles a colour, 3 blocks in one
    round of 8; the last colour's hub rides in front: 1 + 8."""
    import test_hip_parity as thp
    S1, M = 1, -1

    def plans(g, hbv, learning):
        ns, fg = session(g, head_by_vid=hbv)
        recs = fg.plan_classes(learning, 2, 0)
        f = _lib.class_fields(recs)
        return [{x: int(v[k]) for x, v in f.items() if v[k]} for k in range(len(recs))]

    g = thp._generic_lane_graph()
    assert plans(g, False, True) == [dict(generic_on=1, generic_n=513, generic_grid=129, generic_stream=S1, ngeneric=32832, e=32832, update=1)]
    assert plans(g, False, False) == [dict(generic_on=1, generic_n=32832, generic_grid=129, generic_stream=S1, ngeneric=32832, e=32832)]
    g = thp._pairs_many_weights()
    for learning, grid in ((True, 2), (False, 8)):
        p = plans(g, False, learning)
        assert len(p) == 2
        for k, fb in enumerate((0, 384)):
            assert (p[k]["fast_on"], p[k]["fast_n"], p[k]["fast_grid"], p[k]["fast_stream"]) == (1, 5, grid, M)
            assert p[k].get("fb", 0) == fb and p[k]["fe"] == p[k]["e"] == fb + 320 and "gen_on" not in p[k] and "dyn_on" not in p[k]
    g = thp._boolw_hub()
    for learning in (True, False):
        p = plans(g, True, learning)
        assert len(p) == 9
        for k in range(9):
            hub = int(k == 8)
            assert (p[k]["gen_on"], p[k]["gen_maxc"], p[k]["gen_ntiles"], p[k]["gen_nblocks"], p[k]["gen_stream"]) == (1, 2, 11, 3, M)
            assert (p[k].get("gen_hblocks", 0), p[k]["gen_gblocks"], p[k]["gen_grid"], p[k].get("nhub", 0)) == (hub, 8, 8 + hub, hub)
            assert p[k].get("gen_behind", 0) == int(not learning) and "heavy_on" not in p[k] and "fast_on" not in p[k]
