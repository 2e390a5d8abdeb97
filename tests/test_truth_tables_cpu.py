"""The truth-table graphs of tests/truth_tables.py on the host alone: plan and oracle.

(a) ROUTES: which functions each kind of route holds, per variant, read from the plan's route words; and that the union
    over the variants puts every function on every family that supports it (SUPPORT).
(b) COMPLETENESS: the indices into the general tiles' 2048-entry table (gen_lut_entry) that the cells of a graph visit,
    per function code, are EXACTLY those any tuple of other-member values can reach -- computed by brute force over
    all tuples, independently of the builder's loops.  No reachable table entry is left out.
(c) DECISIVE WEIGHTS: with |w| = W = 40 a target whose factor separates its candidates is drawn at the argmax of
    sign * f(c).  Two candidates' potentials differ by at least W (every function's values differ by at least 1 where
    they differ; RATIO's weights are scaled so that the same holds), so a draw leaves the argmax set with probability
    at most (cardinality - 1) * exp(-W) <= 2 e^-40 = 8.5e-18: below the generator's resolution 2^-53.  The oracle's own
    device-mode sampler must put EVERY unique-argmax target on its argmax in EVERY one of 12 sweeps: no tolerance.
(d) LIVELINESS: with |w| = 0.7 the targets move, and learning moves every free weight."""

import functools
from itertools import product

import numpy as np
import pytest

from util import session, oracle_of, phases_from_colors
from numbskull_amd import _lib
import truth_tables as tt
from truth_tables import ALL, FAST, TILE, OFF_TILE
from tiles import TABLE, UNIFORM, SHAPE, LANE, GENERAL, GROUP, HUB, GENERIC, check_counters

# what each family evaluates: the fast path's tiles the six symmetric boolean functions of binary
# dataType-0 variables, the general tiles and the groups those and IMPLY_MLN and the *_CAT functions, the generic
# kernels (a wave or a lane per variable) everything
SUPPORT = {TABLE: set(FAST), UNIFORM: set(FAST), SHAPE: set(FAST), LANE: set(FAST), GENERAL: set(TILE), GROUP: set(TILE),
           HUB: set(ALL), GENERIC: set(ALL)}
_B = set(FAST) - {-1}
# variant -> kind -> the functions whose targets take that kind of route
ROUTES = {
    "main": {TABLE: {-1}, UNIFORM: _B, SHAPE: _B, GROUP: set(TILE), HUB: set(OFF_TILE)},
    "tables": {TABLE: set(FAST), SHAPE: _B, GROUP: set(TILE), HUB: set(OFF_TILE)},
    "no_ztab": {UNIFORM: set(FAST), GROUP: set(FAST)},
    "per_factor": {SHAPE: set(FAST), GROUP: set(TILE), HUB: set(OFF_TILE)},
    "lane": {LANE: set(FAST), GROUP: set(TILE), HUB: set(OFF_TILE)},
    "general": {TABLE: {-1}, UNIFORM: _B, SHAPE: _B, GENERAL: set(TILE), HUB: set(OFF_TILE)},
    "roles": {TABLE: set(FAST), GENERAL: set(TILE)},
    "one_lane": {TABLE: {-1}, UNIFORM: _B, SHAPE: _B, GROUP: set(TILE), GENERIC: set(OFF_TILE)},
    "generic": {HUB: set(ALL)},
    "generic_lane": {GENERIC: set(ALL)},
    "self": {GENERAL: {0, 1, 2, 3, 12, 13, 14, 16, 17}, HUB: {12, 14, 17}},
    "literal": {GENERAL: {13, 16, 17}},
}
# the table kinds hold binary targets only
BINARY_ONLY = (TABLE, UNIFORM, SHAPE, LANE)


def routes_of(cells, routes):
    """kind -> functions, over the targets of the cells."""
    kind = _lib.route_fields(np.asarray(routes, np.int64))["kind"]
    out = {}
    for c in cells:
        out.setdefault(int(kind[c.target]), set()).add(c.fn)
    return out


def check_routes(name, g, cells, color, routes, info):
    """The plan (or the handle) took the targets of the variant where the variant was built to take them."""
    got = routes_of(cells, routes)
    assert got == ROUTES[name], (name, got)
    kind = _lib.route_fields(np.asarray(routes, np.int64))["kind"]
    for c in cells:
        assert c.card == 2 or int(kind[c.target]) not in BINARY_ONLY
    check_counters(color, routes, info)
    if name in ("general", "literal"):
        assert info["tiles_general"] > 0 and info["tiles_general_roles"] == 0 and info["ep_groups"] == 0, info
    if name == "roles":
        assert info["tiles_general_roles"] > 0, info
    if name in ("main", "per_factor", "tables"):
        assert info["ep_groups"] > 0 and info["tiles_general"] == 0 and info["hubs"] > 0, info
    if name in ("one_lane", "generic_lane"):
        assert info["hubs"] == 0 and info["ngeneric"] > 0, info
    if name == "lane":
        assert info["tiles_lane"] > 0 and info["tiles_shape"] == 0, info
    assert len(g[1]) <= 200000


@functools.lru_cache(maxsize=None)
def _planned(name, W=tt.W_DECISIVE):
    """(graph, cells, FactorGraph, colours, route words, info) of a variant; the caller has set its switches."""
    g, cells = tt.build_variant(name, W=W)
    ns, fg = session(g, head_by_vid=tt.VARIANTS[name].hbv)
    color, info = fg.plan()
    return g, cells, fg, color, fg.plan_routes(), info


def _oracle(name, fg, color):
    og = oracle_of(fg, tt.VARIANTS[name].hbv, layout=False)
    assert og.check_coloring(color) == (-1, -1)
    return og, phases_from_colors(color)


# ---------------------------------------------------------------------------------------------------------- (a) routes
@pytest.mark.parametrize("name", sorted(tt.VARIANTS))
def test_every_function_takes_the_routes_of_its_variant(monkeypatch, name):
    tt.set_switches(monkeypatch, name)
    g, cells, fg, color, routes, info = _planned(name)
    check_routes(name, g, cells, color, routes, info)


def test_the_variants_put_every_function_on_every_family_that_supports_it():
    union = {}
    for name, kinds in ROUTES.items():
        for k, fns in kinds.items():
            assert fns <= SUPPORT[k], (name, k, fns - SUPPORT[k])
            union.setdefault(k, set()).update(fns)
    assert union == SUPPORT, {k: SUPPORT[k] - union.get(k, set()) for k in SUPPORT}
    assert set(ROUTES) == set(tt.VARIANTS)


def test_the_main_enumeration_is_what_the_builder_says():
    g, cells = tt.truth_graph()
    assert (len(cells), len(g[1])) == (18360, 68208)
    assert {c.fn for c in cells} == set(ALL) and {c.card for c in cells} == {2, 3} and {c.sign for c in cells} == {1, -1}
    # one factor per target, private leaves: every variable is a member of exactly one factor
    assert np.array_equal(np.sort(g[3]["vid"]), np.arange(len(g[1])))
    ev = g[1]["isEvidence"]
    t = np.array([c.target for c in cells])
    assert (ev[t] == 0).all() and ev.sum() == len(ev) - len(t)
    for c in cells[::97]:
        s = int(g[2][c.factor]["ftv_offset"])
        m = g[3]["vid"][s:s + c.arity]
        assert m[c.j] == c.target and tuple(g[1]["initialValue"][np.delete(m, c.j)]) == c.leaves
    gw, cw = tt.truth_graph(wide=True)
    assert len(gw[1]) == len(g[1]) + 1 and gw[1][-1]["cardinality"] == 200 and len(cw) == len(cells)
    gl, cl = tt.truth_graph(learn=True, reps="card", W=tt.W_LIVELY)
    assert len(cl) == sum(c.card for c in cells) and len(gl[1]) <= 200000
    tl = np.array([c.target for c in cl])
    assert (gl[1]["isEvidence"][tl] == 1).all()
    # the copies of a cell hold every value of the target once
    for card in (2, 3):
        n = np.bincount(gl[1]["initialValue"][tl][[c.card == card for c in cl]])
        assert len(n) == card and (n == n[0]).all(), n


# ---------------------------------------------------------------------------------------------------- (b) completeness
def _reachable(fn, widths, values):
    """Brute force: every table index an entry of function fn can reach with ``widths`` other members holding ``values``."""
    out = set()
    for n in widths:
        for xs in product(values, repeat=n):
            # (the target is head or body member of a positional function; alone in its factor it is the head)
            for head in (((True,) if n == 0 else (False, True)) if fn in tt.POSITIONAL else (False,)):
                out.add(tt.lut_index(fn, xs, head))
    return out


def test_the_chain_facts_restate_the_device_code():
    """chain_facts / lut_index against hand-worked entries (GenChain::member, GenChain::close)."""
    assert tt.chain_facts(2, ()) == (True, True, False, True, False)
    assert tt.chain_facts(2, (2,)) == (True, True, False, True, True)              # OR: non-zero, not 1
    assert tt.chain_facts(2, (0, 2, 1)) == (False, False, True, False, True)
    assert tt.chain_facts(8, (1, 1, 0)) == (False, True, True, False, False)       # *_CAT: matching = equal to 1
    assert tt.chain_facts(8, (2, 1)) == (False, False, True, False, True)
    # IMPLY_NATURAL_CAT (code 8), the target a body member, body true, head false: allnz 0, prevall 1, any1 1
    assert tt.lut_index(16, (1, 1, 0), False) == 8 | 1 << 4 | 1 << 7 | 1 << 8
    assert tt.lut_index(16, (1, 1, 0), True) == 8 | 1 << 7 | 1 << 8
    assert tt.lut_index(4, (), False) == 3 | 1 << 5 | 1 << 6 | 1 << 7 | 1 << 9       # ISTRUE over the target alone
    assert tt.lut_index(-1, (1, 2), False) == 0 | 1 << 5 | 1 << 6 | 1 << 7 | 1 << 9


def test_no_reachable_table_entry_is_left_out():
    """Main enumeration: <= 3 other members with values 0 .. 2.  Arity 5 .. 7: 4 .. 6 binary other members."""
    for cells, widths, values in ((tt.truth_graph(fns=TILE)[1], (0, 1, 2, 3), (0, 1, 2)),
                                  (tt.wide_family()[1], (4, 5, 6), (0, 1))):
        visited = {}
        for c in cells:
            visited.setdefault(c.fn, set()).add(tt.cell_lut_index(c))
        assert set(visited) == set(TILE)
        for fn in TILE:
            want = _reachable(fn, widths, values)
            assert visited[fn] == want, (fn, sorted(want - visited[fn]), sorted(visited[fn] - want))
            assert all(i & 15 == tt.general_code(fn) for i in want) and len(want) > (0 if fn == -1 else 3)


# ------------------------------------------------------------------------------------------------ (c) decisive weights
CENSUS = {           # variant -> (cells, unique-argmax targets, partial ties, constant in the candidate)
    "main": (18360, 3988, 1336, 13036), "tables": (50416, 12312, 4008, 34096), "no_ztab": (9408, 1392, 464, 7552),
    "roles": (17472, 357, 141, 16974), "self": (4680, 485, 291, 3904), "literal": (10224, 1086, 438, 8700),
}
for _n in ("per_factor", "lane", "general", "one_lane", "generic", "generic_lane"):         # the main enumeration again
    CENSUS[_n] = CENSUS["main"]


@pytest.mark.parametrize("name", sorted(tt.VARIANTS))
def test_the_oracle_draws_every_decisive_target_at_its_argmax(monkeypatch, name):
    tt.set_switches(monkeypatch, name)
    g, cells, fg, color, routes, info = _planned(name)
    og, (order, ps) = _oracle(name, fg, color)
    vv, _, wv, cnt = og.initial_state()
    cls = tt.classify(og, cells, vv)
    cen = tt.census(cells, cls)
    assert cen[1] > 0 and cen[0] == sum(cen[1:])
    assert cen == CENSUS[name], cen
    # the gap the bound rests on: where two candidates differ, |w| * |f(c) - f(c')| >= W
    for c, (f, _) in zip(cells, cls):
        w = abs(float(g[0]["initialValue"][g[2]["weightId"][c.factor]]))
        gaps = [abs(a - b) for a in f for b in f if a != b]
        assert not gaps or w * min(gaps) >= tt.W_DECISIVE, (c, f, w)
    held = g[1]["isEvidence"] != 0
    start = vv.copy()
    for s in range(12):
        assert og.gibbs_dev(order, ps, vv, wv, cnt, 7, s, False) == 0
        tt.check_decisive(cells, cls, vv)
        assert np.array_equal(vv[held], start[held]), "a leaf moved"
    # (the initial values are not all on the argmax: the sampler had something to do)
    assert any(int(start[c.target]) not in a for c, (_, a) in zip(cells, cls))


# ------------------------------------------------------------------------------------------------------ (d) liveliness
def test_lively_weights_move_the_targets():
    g, cells, fg, color, routes, info = _planned("main", tt.W_LIVELY)
    og, (order, ps) = _oracle("main", fg, color)
    vv, _, wv, cnt = og.initial_state()
    seen = np.zeros((len(vv), 3), bool)
    for s in range(24):
        assert og.gibbs_dev(order, ps, vv, wv, cnt, 7, s, False) == 0
        seen[np.arange(len(vv)), vv] = True
    whole = sum(int(seen[c.target].sum()) == c.card for c in cells)
    assert whole >= 0.99 * len(cells), (whole, len(cells))


@pytest.mark.parametrize("per_factor", [False, True], ids=["shared", "per_factor"])
def test_learning_moves_the_weights(per_factor):
    g, cells = tt.truth_graph(W=tt.W_LIVELY, learn=True, reps="card", per_factor=per_factor)
    ns, fg = session(g, head_by_vid=True)
    color, info = fg.plan()
    og, (order, ps) = _oracle("main", fg, color)
    og.device_lag = bool(info["learn_lag"])
    vv, ve, wv, _ = og.initial_state()
    assert og.learn_call(order, ps, vv, ve, wv, 4, 0.02, 0.9, 0, 0.05, 1, True, 43, 0) == 0
    free = og.weight["isFixed"] == 0
    moved = wv[free] != og.weight["initialValue"][free]
    assert np.array_equal(ve, og.variable["initialValue"])
    if per_factor:          # a weight with one factor moves when its factor's value differs between the chains
        assert 2 * int(moved.sum()) >= int(free.sum()), (int(moved.sum()), int(free.sum()))
    else:
        assert moved.all() and int(free.sum()) == 2 * (len(ALL) - 1), (int(moved.sum()), int(free.sum()))


# --------------------------------------------------------------------------------------------------------------- hubs
def test_the_truth_table_hubs_take_every_hub_route_and_are_lively():
    g, cells, hubs = tt.hub_family()
    ns, fg = session(g, head_by_vid=True)
    color, info = fg.plan()
    f = _lib.route_fields(fg.plan_routes().astype(np.int64))
    assert info["hubs_ep"] > info["hubs_block"] > 0 and info["hubs"] > info["hubs_ep"], info
    ids = np.array([h for h, _, _ in hubs])
    assert (f["kind"][ids] == HUB).all()
    form = np.array([x for _, _, x in hubs])
    assert (f["hub_ep"][ids][form] == 1).all() and (f["hub_ep"][ids][~form] == 0).any()
    assert {(int(g[1][h]["cardinality"]), int(g[1][h]["dataType"]), int(f["hub_ep"][h]), int(f["hub_block"][h])) for h in ids} >= \
        {(c, d, e, b) for c, d in tt.HUB_KINDS for e, b in ((1, 1), (1, 0), (0, 0))}
    assert all(33 <= L <= 300 for _, L, _ in hubs)
    # the functions of the hubs on each route
    on = {}
    for c in cells:
        on.setdefault((int(f["hub_ep"][c.target]), int(f["hub_block"][c.target])), set()).add(c.fn)
    assert on[(1, 1)] == set(TILE) and on[(1, 0)] == set(TILE) and on[(0, 0)] == set(ALL), on
    og, (order, ps) = _oracle("main", fg, color)
    vv, _, wv, cnt = og.initial_state()
    seen = [set() for _ in ids]
    for s in range(24):
        assert og.gibbs_dev(order, ps, vv, wv, cnt, 5, s, False) == 0
        for i, h in enumerate(ids):
            seen[i].add(int(vv[h]))
    # (potentials of size 2 .. 3 |w| leave a binary hub on one value through 24 sweeps now and then)
    assert 8 * sum(len(s) >= 2 for s in seen) >= 7 * len(seen), [len(s) for s in seen]
