"""Belief propagation, the host side: numbskull_amd.diagnostics.bp_layout / bp_iterate / bp_factor_beliefs / bethe_log_z
(the rule nsk_bp_run is held to bit for bit in tests/test_bp_gpu.py) against enumeration -- exact on trees, sane on
loopy graphs --, hand-written small cases, and the liveliness of every case the GPU tests use.  No GPU needed."""

import numpy as np
import pytest

import bp
import temper
from numbskull_amd import _lib
from numbskull_amd.diagnostics import bp_layout, bethe_log_z, bp_factor_beliefs, bp_iterate


def _max_error(m, r, ex):
    return max(float(np.abs(m.belief(r, v) - p).max()) for v, p in ex.items())


# ---------------------------------------------------------------------------------------------- exact on trees
@pytest.mark.parametrize("name,zero_at", [("chain9", 5), ("chain17", 17), ("star", None), ("star7", None), ("tree", None)])
def test_the_mirror_is_exact_on_trees(name, zero_at):
    """fewer than 1e4 roundings of 1.1e-16 enter any belief at these sizes: 1e-12 absolute; log Z within 1e-10"""
    m = bp.model(name)
    r = bp.mirror(name, 40, 0.0, 0.0)
    ex, lz = m.exact()
    err, got = _max_error(m, r, ex), m.log_z(r)
    zero = int(np.nonzero(r["residual"] == 0.0)[0][0]) + 1
    print("%s: belief error %.3g, Bethe %.12f exact %.12f, residual exactly 0 in iteration %d" % (name, err, got, lz, zero))
    assert err <= 1e-12
    assert abs(got - lz) <= 1e-10
    assert r["iters"] == zero and r["iters"] > 1
    if zero_at is not None:
        assert r["iters"] == zero_at
    assert not r["residual"][zero:].any() and (r["residual"][:zero - 1] > 0).all()


# ---------------------------------------------------------------------------------------------- loopy sanity
@pytest.mark.parametrize("name,bound", [("clamped_grid", 0.05), ("mixed_clamped", 0.2)])
@pytest.mark.parametrize("damping", [0.0, 0.5])
def test_loopy_runs_converge_near_the_enumeration(name, bound, damping):
    """the bounds catch a broken rule; they are no accuracy claim (prototype: 0.022 and 0.13)"""
    m = bp.model(name)
    r = bp.mirror(name, 200, damping, 1e-12)
    ex, lz = m.exact()
    err = _max_error(m, r, ex)
    print("%s damping %.1f: %d iterations, belief error %.4f, Bethe %.6f exact %.6f" % (name, damping, r["iters"], err, m.log_z(r), lz))
    assert 0 < r["iters"] <= 200
    assert err <= bound
    assert np.isfinite(m.log_z(r))


# ---------------------------------------------------------------------------------------------- liveliness of the GPU cases
@pytest.mark.parametrize("name", sorted(bp.CASES) + ["hub", "trips", "star", "star7", "tree"])
def test_every_gpu_case_is_lively(name):
    iters = bp.TRIP_ITERS if name == "trips" else 30
    r = bp.mirror(name, iters, 0.0, 0.0)
    assert r["residual"][0] > 0
    assert len(set(r["residual"][:iters].tolist())) >= 3, "at least three iterations differ from one another"
    assert (r["rescaled"] > 0) == (name == "hub"), (name, r["rescaled"])
    if name in ("star", "star7"):                   # either side of the edges the variable phase keeps in registers
        assert len(bp.model(name).layout["var_edges"][0]) == (_lib.BP_VAR_REG if name == "star" else _lib.BP_VAR_REG + 1)
    assert np.isfinite(r["beliefs"]).all() and np.isfinite(r["f2v"]).all() and np.isfinite(r["v2f"]).all()


def test_the_capped_case_makes_three_trips_in_every_kernel():
    """grid = min(ceil(items / block), cap) blocks: restated here (256 lanes a block, 128 in the variable phase)"""
    L = bp.model("trips").layout
    nvl = sum(1 for e in L["var_edges"] if e)
    for items, block in ((int(L["table_off"][-1]), 256), (len(L["edge_var"]), 256), (nvl, 128)):
        blocks = max(1, min(-(-items // block), 1))
        assert -(-items // (blocks * block)) >= 3 and bp.trips(items, 1, block) == -(-items // block) >= 3, items
        assert bp.trips(items, 0, block) == 1                   # ... and one trip as is
    assert len(L["edge_var"]) > 1500 and nvl > 3 * 128 and (_lib.BP_BLOCK, _lib.BP_VAR_BLOCK) == (256, 128)


def test_the_hub_matches_the_reduced_model():
    m, red = bp.model("hub"), bp.model("hub_reduced")
    r = bp.mirror("hub", 30, 0.0, 0.0)
    ex, _ = red.exact()
    for v in (0, 1):
        assert np.abs(m.belief(r, v) - ex[v]).max() <= 1e-12, v
    # without the rule the product of the 1200 messages underflows in both entries
    f2v, mo = r["f2v"], m.layout["msg_off"]
    p = np.ones(2)
    for e in m.layout["var_edges"][0]:
        p = p * f2v[mo[e]:mo[e] + 2]
    assert (p == 0).all()


def test_every_refusal_case_breaks_exactly_the_rule_it_names():
    def shape(g, hbv=True):
        w, var, f, fm, _, _ = g
        L = bp_layout(f, fm, var, var["initialValue"])
        return max(len(m) for m in L["members"]), int(np.diff(L["table_off"]).max())
    assert shape(bp.limit_graph(12, 4)) == (16, 4096) == (_lib.BP_MAX_MEMBERS, _lib.BP_MAX_TABLE)     # accepted: at both caps
    assert shape(bp.limit_graph(13, 0)) == (13, 8192)               # the table alone
    assert shape(bp.limit_graph(12, 5)) == (17, 4096)               # the members alone
    for fn in (30, 13):                                             # UFO; the literal head: small otherwise
        assert shape(bp.limit_graph(2, 1, fn=fn))[0] == 3


# ---------------------------------------------------------------------------------------------- hand-written small cases
def test_layout_of_a_repeated_member_and_of_a_clamped_factor():
    # EQUAL(x, x) ; EQUAL(y, z) with y, z evidence ; AND(x, y, x, u) ; NOOP(x)
    g = bp.spec_graph([2, 3, 2, 3], [0, 1, 1, 0], [0, 2, 1, 0],
                      [(3, [0, 0], [0, 0], 0.5), (3, [1, 2], [0, 0], 0.25), (2, [0, 1, 0, 3], [0, 0, 0, 0], 1.0), (-1, [0], [0], 1.0)])
    w, var, f, fm, _, _ = g
    L = bp_layout(f, fm, var, var["initialValue"])
    assert L["members"] == [[0], [1, 2], [0, 1, 3], []] and L["slots"] == [[0, 0], [0, 1], [0, 1, 0, 2], []]
    assert L["axes"] == [[0], [], [0, 3], []] and L["shapes"] == [[2], [], [2, 3], []]
    assert L["table_off"].tolist() == [0, 2, 3, 9, 10] and L["edge_off"].tolist() == [0, 1, 1, 3, 3]
    assert L["edge_var"].tolist() == [0, 0, 3] and L["msg_off"].tolist() == [0, 2, 4, 7]
    assert L["var_edges"] == [[0, 1], [], [], [2]] and L["clamped"].tolist() == [False, True, True, False]
    assert L["offsets"].tolist() == [0, 2, 5, 7, 10]
    free = bp_layout(f, fm, var, var["initialValue"], sample_evidence=True)
    assert free["axes"] == [[0], [1, 2], [0, 1, 3], []] and free["table_off"].tolist() == [0, 2, 8, 26, 27]
    # the tables of that graph, by hand: EQUAL(x, x) = 1; EQUAL(2, 1) = -1; AND(x, 2, x, u) = 1 iff x and u non-zero
    m = bp.Model(g)
    assert m.theta.tolist() == [0.5, 0.5, -0.25, -1.0, -1.0, -1.0, -1.0, 1.0, 1.0, 0.0]
    r = m.run(10)
    ex, lz = m.exact()
    assert r["iters"] == 2 and abs(m.log_z(r) - lz) <= 1e-12
    assert max(np.abs(m.belief(r, v) - ex[v]).max() for v in ex) <= 1e-15
    assert m.belief(r, 1).tolist() == [0, 0, 1] and m.belief(r, 2).tolist() == [0, 1]


def test_bethe_log_z_by_hand():
    # two independent binary variables, one with a unary factor of theta (0.3, -0.3), one with no factor at all;
    # a clamped third
    g = bp.spec_graph([2, 2, 2], [0, 0, 1], [0, 0, 1], [(4, [0], [0], 0.3), (4, [2], [0], 5.0)])
    m = bp.Model(g)
    assert m.theta.tolist() == [-0.3, 0.3, 5.0]
    r = m.run(3)
    want = np.log(np.exp(0.3) + np.exp(-0.3)) + np.log(2.0) + 5.0
    assert abs(m.log_z(r) - want) <= 1e-14
    # 0 log 0 = 0: a hard table
    L = {"card": np.array([2]), "clamped": np.array([False]), "edge_var": np.array([0])}
    assert bethe_log_z(L, np.array([0.0, 1.5]), np.array([0.0, 1.0]), np.array([0.0, 1.0])) == 1.5
    # a pair with a known partition function, by the formula itself
    g = bp.spec_graph([2, 2], [0, 0], [0, 0], [(3, [0, 1], [0, 0], 0.7)])
    m = bp.Model(g)
    r = m.run(5)
    assert abs(m.log_z(r) - np.log(2 * np.exp(0.7) + 2 * np.exp(-0.7))) <= 1e-14
    assert np.allclose(bp_factor_beliefs(m.layout, r["psi"], r["v2f"]).sum(), 1.0)


def test_damping_and_continuation_of_the_mirror():
    m = bp.model("clamped_grid")
    a = m.run(7, 0.5)
    b = m.run(3, 0.5)
    c = m.run(4, 0.5, messages=(b["f2v"], b["v2f"]))
    assert np.array_equal(a["f2v"], c["f2v"]) and np.array_equal(a["v2f"], c["v2f"]) and np.array_equal(a["beliefs"], c["beliefs"])
    assert np.array_equal(a["residual"], np.concatenate([b["residual"], c["residual"]]))
    und = m.run(7)
    assert not np.array_equal(und["f2v"], a["f2v"]) and abs(a["residual"][0] - 0.5 * und["residual"][0]) <= 1e-15
    # tol stops the run behind the first iteration at or below it
    r = m.run(30, 0.0, 1e-3)
    k = r["iters"]
    assert 1 < k < 30 and r["residual"][k - 1] <= 1e-3 < r["residual"][k - 2] and not r["residual"][k:].any()
    assert m.run(2, 0.0, 1e-12)["iters"] == -2
    with np.errstate(all="ignore"):                  # two hard constraints that contradict each other: NaN, as IEEE gives
        g = bp.spec_graph([2], [0], [0], [(4, [0], [0], 800.0), (4, [0], [0], -800.0)])
        r = bp.Model(g).run(2)
    assert np.isnan(r["beliefs"]).all()
