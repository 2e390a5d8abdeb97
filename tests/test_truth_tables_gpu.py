"""The truth tables of every factor function through every kernel family (tests/truth_tables.py builds the cells;
tests/test_truth_tables_cpu.py checks routes, completeness and the decisive condition on the oracle alone).

A. READ-BACK, no sampler involved: factor_values() and conditionals(potentials=True) of the main enumeration EQUAL
   oracle.eval_factor and w * eval_factor per candidate -- the generic eval_factor of the device (k_factor_values,
   k_cond), on both chains after a learning epoch, by id and with literal heads, int8 and int32 values.
B. DECISIVE INFERENCE, every sampling family as an evaluator: with |w| = 40 the argmax of sign * f(c) is drawn with
   failure probability <= 2 e^-40 per update (derivation: test_truth_tables_cpu.py (c)).  After EVERY one of 12
   one-sweep calls every unique-argmax target holds its argmax and every partial-tie target a member of its argmax
   set -- asserted directly from oracle.eval_factor, no sampler in between -- and values and tallies equal the
   oracle's device mode bit for bit.  A wrong table byte, chain fact or satisfied bit of a reachable cell moves an
   argmax and fails here with certainty.
C. LIVELY INFERENCE AND LEARNING, bit for bit: |w| = 0.7, 24 sweeps; then 4 learning epochs for every regulariser and
   learn_non_evidence both ways, with the targets as evidence holding every value of their domain once.  The
   truth-table HUBS run here: a wrong hub entry shifts one potential by |w| (scaled with the list length: 0.04 .. 0.37),
   which changes a draw -- and from there values, tallies and weights -- with high probability over the 24 sweeps and
   the learning runs, not with certainty; this is unlike B."""

import functools

import numpy as np
import pytest

from util import session, oracle_of, phases_from_colors
import truth_tables as tt
from test_truth_tables_cpu import check_routes, routes_of, ROUTES
from tiles import TABLE, SHAPE, GENERAL, GROUP, GENERIC

pytestmark = pytest.mark.gpu

SAMPLED = sorted(tt.VARIANTS)
# learning: (regularization, truncation, learn_non_evidence)
LEARN_CFG = [(reg, 2 if reg == 1 else 1, lne) for reg in (0, 1, 2) for lne in (False, True)]
# variant -> the arguments of its learning graph beyond learn=True and W_LIVELY ("card": one copy of a cell per value of
# its target).  The table kernels' learning variant is lcard 2 with shared weights; one weight per factor (weights
# updated in place) on the shape, group and general variants
LEARN_VARIANTS = {
    "main": dict(reps="card"), "tables": dict(fns=tt.FAST, reps=8), "no_ztab": dict(reps=8),
    "per_factor": dict(reps="card"), "lane": dict(reps="card"), "general": dict(reps="card"),
    "general_per_factor": dict(reps="card", per_factor=True, fns=tt.TILE),
    "roles": dict(reps="card", arities=(5, 6)), "one_lane": dict(reps="card"), "generic": dict(reps="card"),
    "self": dict(reps="card"), "literal": dict(reps="card", arities=(1, 2, 3)),
}
# where the learning graph's targets take other routes than the variant's inference graph: fewer functions; a generic
# colour of more than 32768 variables is sampled by one lane per variable, not by a wave each
LEARN_ROUTES = {
    "tables": {TABLE: set(tt.FAST), GROUP: set(tt.FAST)},
    "general_per_factor": {GENERAL: set(tt.TILE), SHAPE: set(tt.FAST)},
    "generic": {GENERIC: set(tt.ALL)},
}


def _variant(name):
    return "general" if name == "general_per_factor" else name


@functools.lru_cache(maxsize=2)
def _graph(v, kw):
    """Built once for the tests that share it (the learning configurations of a variant); session() copies the arrays."""
    return tt.build_variant(v, **dict(kw))


def _session(monkeypatch, name, seed, routes=True, **kw):
    v = _variant(name)
    tt.set_switches(monkeypatch, v)
    g, cells = _graph(v, tuple(sorted(kw.items())))
    hbv = tt.VARIANTS[v].hbv
    ns, fg = session(g, seed=seed, head_by_vid=hbv)
    if routes:
        check_routes(v, g, cells, fg.colors(), fg.routes(), fg.info())
    return g, cells, fg, oracle_of(fg, hbv), phases_from_colors(fg.colors())


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------- A. read-back
def _read_back(fg, og, g, cells, state, weights, evidence_chain):
    state = np.ascontiguousarray(state, np.int64)
    # a factor's value "on the state as it is" is the value its FIRST member sees at its own value (nsk_factor_values:
    # with literal heads a factor whose head is its first member reads the head from the variable, not at the edge index)
    first = g[3]["vid"][np.minimum(g[2]["ftv_offset"], len(g[3]) - 1)]
    want = np.array([og.eval_factor(f, int(first[f]), int(state[first[f]]), state)[1] for f in range(len(g[2]))])
    got = fg.factor_values(evidence_chain=evidence_chain)
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert len(bad) == 0, (len(bad), [(cells[i], got[i], want[i]) for i in bad[:6]])
    ids = np.array([c.target for c in cells], np.int64)
    off, pot = fg.conditionals(ids, evidence_chain=evidence_chain, potentials=True)
    wid = g[2]["weightId"]
    for i, c in enumerate(cells):            # one factor per target: no summation order to argue about
        w = float(weights[wid[c.factor]])
        p = np.array([w * og.eval_factor(c.factor, c.target, v, state)[1] for v in range(c.card)])
        # (a dataType-0 target's potential is 0.0 + w * f: the sum's first term)
        assert np.array_equal(_bits(pot[off[i]:off[i + 1]]), _bits(0.0 + p)), (c, pot[off[i]:off[i + 1]], p)


@pytest.mark.parametrize("name,wide", [("main", False), ("main", True), ("literal", False)],
                         ids=["by_vid", "by_vid_int32", "literal_heads"])
def test_factor_values_and_potentials_equal_the_oracle_cell_by_cell(monkeypatch, name, wide):
    kw = dict(wide=True) if wide else {}
    g, cells, fg, og, (order, ps) = _session(monkeypatch, name, 3, W=tt.W_LIVELY, **kw)
    assert fg.info()["value_bytes"] == (4 if wide else 1)
    vv, ve, wv, _ = og.initial_state()
    _read_back(fg, og, g, cells, vv, wv, False)
    # one learning epoch: both chains move on (the evidence chain where a variable is no evidence), the weights too
    fg.learn(0, 1, 0.02, 0.9, 0, 0.05, 1, learn_non_evidence=True)
    assert og.learn_call(order, ps, vv, ve, wv, 1, 0.02, 0.9, 0, 0.05, 1, True, 3, 0) == 0
    assert np.array_equal(fg.var_value[0], vv) and np.array_equal(fg.var_value_evid[0], ve)
    assert np.array_equal(_bits(fg.weight_value[0]), _bits(wv))
    assert np.any(vv != ve) and np.any(vv != og.variable["initialValue"])
    _read_back(fg, og, g, cells, vv, wv, False)
    _read_back(fg, og, g, cells, ve, wv, True)


# ----------------------------------------------------------------------------------------------- B. decisive inference
@pytest.mark.parametrize("name", SAMPLED)
def test_every_family_draws_every_decisive_target_at_its_argmax(monkeypatch, name):
    g, cells, fg, og, (order, ps) = _session(monkeypatch, name, 7)
    vv, _, wv, cnt = og.initial_state()
    cls = tt.classify(og, cells, vv)
    held = g[1]["isEvidence"] != 0
    for s in range(12):
        fg.inference(0, 1, False)
        got = np.asarray(fg.var_value[0])
        tt.check_decisive(cells, cls, got)                       # directly: no sampler in between
        assert np.array_equal(got[held], vv[held]), "a leaf moved"
        assert og.gibbs_dev(order, ps, vv, wv, cnt, 7, s, False) == 0
        bad = np.nonzero(got != vv)[0]
        assert len(bad) == 0, ("differing variables", s, bad[:12], len(bad))
    assert np.array_equal(fg.count, cnt)


def test_the_draw_tables_reach_both_ends_of_their_range(monkeypatch):
    """The lcard-2 variant at |w| = 40: a decisive cell's threshold K -- value 0 iff the generator's 53-bit integer
    k <= K -- is 2^53 - 1 (always 0) or at the lower end of its range (always 1), so no draw of 12 sweeps leaves the
    argmax; a cell constant in the candidate keeps K in the middle and takes both values."""
    g, cells, fg, og, (order, ps) = _session(monkeypatch, "tables", 7)
    from numbskull_amd import _lib
    kind = _lib.route_fields(fg.routes().astype(np.int64))["kind"]
    vv, _, wv, cnt = og.initial_state()
    cls = tt.classify(og, cells, vv)
    on = [(c, a) for c, (_, a) in zip(cells, cls) if kind[c.target] == TABLE]
    assert {len(a) for _, a in on} == {1, 2} and {min(a) for _, a in on if len(a) == 1} == {0, 1}
    seen = np.zeros((len(vv), 2), bool)
    for s in range(12):
        fg.inference(0, 1, False)
        got = np.asarray(fg.var_value[0])
        seen[np.arange(len(got)), np.minimum(got, 1)] = True
    for c, a in on:
        if len(a) == 1:
            assert seen[c.target].tolist() == [0 in a, 1 in a], c
    flat = [c for c, a in on if len(a) == 2]
    assert sum(seen[c.target].all() for c in flat) >= 0.99 * len(flat)      # (2 * 2^-12 of them see one value only)


# ---------------------------------------------------------------------------------------------- C. lively, bit for bit
@pytest.mark.parametrize("name", SAMPLED)
def test_lively_inference_equals_the_oracle(monkeypatch, name):
    g, cells, fg, og, (order, ps) = _session(monkeypatch, name, 11, W=tt.W_LIVELY)
    vv, _, wv, cnt = og.initial_state()
    start = vv.copy()
    sweep = 0
    for rounds in (1, 23):
        fg.inference(0, rounds, False)
        for _ in range(rounds):
            assert og.gibbs_dev(order, ps, vv, wv, cnt, 11, sweep, False) == 0
            sweep += 1
        bad = np.nonzero(fg.var_value[0] != vv)[0]
        assert len(bad) == 0, ("differing variables", bad[:12], len(bad))
        assert np.array_equal(fg.count, cnt)
    t = np.array([c.target for c in cells])
    assert np.any(vv[t] != start[t])


def _learning(fg, og, order, ps, seed, reg, trunc, lne):
    vv, ve, wv, _ = og.initial_state()
    fg.learn(0, 4, 0.02, 0.9, reg, 0.05, trunc, learn_non_evidence=lne)
    assert og.learn_call(order, ps, vv, ve, wv, 4, 0.02, 0.9, reg, 0.05, trunc, lne, seed, 0) == 0
    assert np.array_equal(fg.var_value[0], vv), np.nonzero(fg.var_value[0] != vv)[0][:12]
    assert np.array_equal(fg.var_value_evid[0], ve), np.nonzero(fg.var_value_evid[0] != ve)[0][:12]
    bad = np.nonzero(_bits(fg.weight_value[0]) != _bits(wv))[0]
    assert len(bad) == 0, (bad[:8], fg.weight_value[0][bad[:8]], wv[bad[:8]])
    assert np.any(wv != og.weight["initialValue"])
    return vv, ve, wv


@pytest.mark.parametrize("name,reg,trunc,lne", [(n,) + c for n in sorted(LEARN_VARIANTS) for c in LEARN_CFG])
def test_learning_equals_the_oracle(monkeypatch, name, reg, trunc, lne):
    kw = dict(LEARN_VARIANTS[name], learn=True, W=tt.W_LIVELY)
    g, cells, fg, og, (order, ps) = _session(monkeypatch, name, 13, routes=False, **kw)
    info = fg.info()
    assert routes_of(cells, fg.routes()) == LEARN_ROUTES.get(name, ROUTES[_variant(name)])
    if kw.get("per_factor") or tt.VARIANTS[_variant(name)].kw.get("per_factor"):
        assert info["direct_weights"] > 0, info                   # one weight per factor: updated in place
    else:
        assert info["direct_weights"] == 0, info
    vv, ve, wv = _learning(fg, og, order, ps, 13, reg, trunc, lne)
    t = np.array([c.target for c in cells])
    assert np.array_equal(ve[t], g[1]["initialValue"][t])         # the targets are evidence: every own value, once a copy


# --------------------------------------------------------------------------------------------------------------- hubs
@functools.lru_cache(maxsize=2)
def _hub_graph(kw):
    return tt.hub_family(**dict(kw))


def _hub_session(monkeypatch, seed, env=(), **kw):
    for k in env:
        monkeypatch.setenv("NSK_DIAG", "1")
        monkeypatch.setenv(k, "1")
    g, cells, hubs = _hub_graph(tuple(sorted(kw.items())))
    ns, fg = session(g, seed=seed, head_by_vid=True)
    info = fg.info()
    if env:
        assert info["hubs_ep"] > 0 and info["hubs_block"] == 0 and info["hubs"] > info["hubs_ep"], info
    else:
        assert info["hubs_ep"] > info["hubs_block"] > 0 and info["hubs"] > info["hubs_ep"], info
    return g, cells, hubs, fg, oracle_of(fg, True), phases_from_colors(fg.colors())


@pytest.mark.parametrize("env", [(), ("NSK_NO_EP",)], ids=["block_wave_walk", "no_ep"])
def test_truth_table_hubs_inference_equals_the_oracle(monkeypatch, env):
    """Hubs of 33 .. 300 entries whose lists walk through the cells: a workgroup, a wave with one lane per entry and the
    generic wave walk in one graph (under NSK_NO_EP the wave takes the lists of up to 256 entries in rounds)."""
    g, cells, hubs, fg, og, (order, ps) = _hub_session(monkeypatch, 17, env)
    vv, _, wv, cnt = og.initial_state()
    seen = [set() for _ in hubs]
    for s in range(24):
        fg.inference(0, 1, False)
        assert og.gibbs_dev(order, ps, vv, wv, cnt, 17, s, False) == 0
        bad = np.nonzero(fg.var_value[0] != vv)[0]
        assert len(bad) == 0, ("differing variables", s, bad[:12], len(bad))
        for i, (h, _, _) in enumerate(hubs):
            seen[i].add(int(vv[h]))
    assert np.array_equal(fg.count, cnt)
    assert 8 * sum(len(s) >= 2 for s in seen) >= 7 * len(seen), [len(s) for s in seen]


@pytest.mark.parametrize("per_factor,reg,trunc,lne", [(p,) + c for p in (False, True) for c in LEARN_CFG])
def test_truth_table_hubs_learning_equals_the_oracle(monkeypatch, per_factor, reg, trunc, lne):
    g, cells, hubs, fg, og, (order, ps) = _hub_session(monkeypatch, 19, learn=True, per_factor=per_factor)
    assert (fg.info()["direct_weights"] > 0) == per_factor
    _learning(fg, og, order, ps, 19, reg, trunc, lne)
