"""Several chains on one handle (nsk_set_chains, FactorGraph.inference(..., var_copy="all")): chain r of a handle seeded s
must be, bit for bit, a one-chain handle seeded s ^ (r << 32) driven through the same calls -- values, per-chain tallies,
and ``count`` the sum of them -- on every kind of graph: the parity graphs (every kernel family, chains sampled one launch
per chain), grids whose sweep is table launches (every chain in one launch, eager and captured, wide quads and front
workgroups), and under the table kernels' diagnostic switches.  Pooled marginals of a tiny grid against enumeration."""

import ctypes as C

import numpy as np
import pytest

from numbskull_amd import _lib, graphgen
from test_hip_parity import _small_graphs, GRAPHS
from perturbed import build_case
from util import session, oracle_of, exact_marginals

pytestmark = pytest.mark.gpu

SEED = 77


def _calls(fg, se, calls, var_copy):
    """burn-in / inference calls: (sweeps, burnin)"""
    for n, burn in calls:
        if burn:
            fg.burnIn(n, se, var_copy=var_copy)
        else:
            fg.inference(0, n, se, var_copy=var_copy)
        yield


def _compare_chains(g, nchains, se, calls=((3, True), (1, False), (4, False)), hbv=False, seed=SEED, edit=None):
    ns, fg = session(g, seed=seed, head_by_vid=hbv, chains=nchains)
    assert fg.var_value.shape[0] == nchains
    singles = [session(g, seed=seed ^ (r << 32), head_by_vid=hbv)[1] for r in range(nchains)]
    steps = [_calls(fg, se, calls, "all")] + [_calls(f, se, calls, 0) for f in singles]
    for k in range(len(calls)):
        for it in steps:
            next(it)
        for r, f in enumerate(singles):
            assert np.array_equal(fg.var_value[r], f.var_value[0]), ("values", r, k)
            assert np.array_equal(fg.chain_count[r], f.count), ("tally", r, k)
        assert np.array_equal(fg.count, sum(f.count for f in singles))
        if edit is not None and k == 0:       # host edits of the rows between calls reach their chains
            edit(fg.var_value, [f.var_value[0] for f in singles])
    return fg, singles


@pytest.mark.parametrize("name", GRAPHS)
@pytest.mark.parametrize("sample_evidence", [True, False])
def test_chains_equal_single_chain_handles(golden, name, sample_evidence):
    g, hbv = _small_graphs(golden)[name]
    _compare_chains(g, 3, sample_evidence, hbv=hbv)


def test_chains_of_the_million_grid_in_one_launch():
    """1000 x 1000 grid (wide quads), 8 chains: 85 tallied sweeps replay both captured sequence sizes (64 + 16) and end
    eagerly; every class launch serves all chains (launches counted once)."""
    g = graphgen.ising_grid(1000, 1000, weight=0.3)
    fg, singles = _compare_chains(g, 8, False, calls=((3, True), (85, False)))
    L = _lib.lib()

    def launches(f, var_copy):
        ms, n = C.c_double(), C.c_int64()
        _lib.check(L.nsk_profile_begin(f._engine()))
        f.inference(0, 16, False, var_copy=var_copy)
        _lib.check(L.nsk_profile_end(f._engine(), C.byref(ms), C.byref(n)))
        return n.value
    assert fg.info()["wide_quads"] > 0
    assert launches(fg, "all") == launches(singles[0], 0)      # one launch per class serves all 8 chains


def test_chains_on_a_perturbed_grid(monkeypatch):
    """Quads that are not wide (front workgroups, replicated per chain) next to wide ones."""
    monkeypatch.setenv("NSK_DIAG", "1")
    monkeypatch.setenv("NSK_WIDE_MIN", "0")
    _, graph = build_case("exc8")
    _compare_chains(graph, 3, True, calls=((3, True), (85, False)), seed=31)


@pytest.mark.parametrize("switch", [None, ("NSK_NO_WIDE", "1")])
def test_chains_on_two_chunk_tiles(monkeypatch, switch):
    """4 x 8 x 1000 grid (5- and 6-slot classes: two-chunk tiles and quads), 3 chains in one launch per class: the
    wide-quad chain kernel and, with wide quads switched off, the tile-pair one; 85 tallied sweeps replay both captured
    sequence sizes and end eagerly."""
    monkeypatch.setenv("NSK_DIAG", "1")
    monkeypatch.setenv("NSK_WIDE_MIN", "0")
    if switch:
        monkeypatch.setenv(*switch)
    fg, _ = _compare_chains(build_case("slots45_3d")[1], 3, True, calls=((3, True), (85, False)), seed=31)
    if switch:
        assert fg.info()["wide_quads"] == 0
    else:
        assert fg.info()["wide_quads"] > 0


def test_chains_of_an_lr_graph_one_launch_per_chain():
    g = graphgen.mixed_lr_graph(200_000, seed=5)
    _compare_chains(g, 2, True, hbv=True)


@pytest.mark.parametrize("switch", [("NSK_NO_WIDE", "1"), ("NSK_NO_GRAPH", "1"), ("NSK_TAB_GRID_CAP", "8")])
def test_chains_under_table_kernel_switches(monkeypatch, switch):
    monkeypatch.setenv("NSK_DIAG", "1")
    monkeypatch.setenv(*switch)
    g = graphgen.ising_grid(300, 300, weight=0.4)
    _compare_chains(g, 3, False, calls=((3, True), (85, False)))


def test_one_chain_all_equals_copy_zero():
    g = graphgen.ising_grid(57, 33, weight=0.3)
    _, a = session(g, seed=SEED)
    _, b = session(g, seed=SEED)
    a.burnIn(3, False)
    b.burnIn(3, False, var_copy="all")
    a.inference(0, 20, False)
    b.inference(0, 20, False, var_copy="all")
    assert np.array_equal(a.var_value, b.var_value)
    assert np.array_equal(a.count, b.count) and np.array_equal(b.chain_count[0], b.count)
    assert np.allclose(a.marginals, b.marginals)


def test_edits_between_calls_reach_their_chain():
    def edit(rows, singles):
        rows[1][::3] = 1
        singles[1][::3] = 1
        rows[2][:] = 0
        singles[2][:] = 0
    g = graphgen.ising_grid(200, 200, weight=0.3)
    _compare_chains(g, 3, False, calls=((3, True), (20, False)), edit=edit)
    g = graphgen.mixed_lr_graph(3000, seed=5, nweights=40)
    _compare_chains(g, 3, True, calls=((3, True), (4, False)), hbv=True, edit=edit)


def test_several_chains_refuse_learning_sequential_and_own_range():
    g = graphgen.ising_grid(40, 40, weight=0.3, fixed=False)
    ns, fg = session(g, seed=SEED, chains=3)
    fg.inference(0, 2, False, var_copy="all")
    with pytest.raises(ValueError):
        fg.learn(0, 1, 0.01, 1.0, 0, 0.0, 1, var_copy="all")
    L, h = _lib.lib(), fg._engine()
    assert L.nsk_get_chains(h) == 3
    assert L.nsk_learn_sweeps(h, 1, 0.01, 1.0, 0, 0.0, 1, 0) == _lib.E_INVALID
    assert L.nsk_set_scan(h, _lib.SCAN_SEQUENTIAL) == _lib.E_INVALID
    assert L.nsk_set_chains(h, 0) == _lib.E_INVALID and L.nsk_set_chains(h, 1025) == _lib.E_INVALID
    fg.learn(0, 1, 0.01, 1.0, 0, 0.0, 1)        # an integer var_copy takes the handle back to one chain
    assert L.nsk_get_chains(h) == 1
    ns, fg = session(g, seed=SEED, chains=3, scan="sequential")
    with pytest.raises(ValueError):
        fg.inference(0, 2, False, var_copy="all")
    ns, fg = session(g, seed=SEED, chains=3)
    fg.own_range = (0, 800)
    with pytest.raises(ValueError):
        fg.inference(0, 2, False, var_copy="all")


def test_pooled_marginals_of_64_chains_match_enumeration():
    g = graphgen.ising_grid(4, 3, weight=0.5)
    ns, fg = session(g, seed=123, chains=64)
    og = oracle_of(fg)
    fg.inference(100, 4000, True, var_copy="all")
    exact = exact_marginals(og, og.weight["initialValue"].astype(float))
    for v, p in exact.items():
        got = fg.marginals[int(fg.cstart[v])]
        assert abs(got - p[1]) < 5e-3, (v, got, p[1])
    assert fg.count.sum() == fg.chain_count.sum()
    rh = fg.rhat[np.isfinite(fg.rhat)]
    assert len(rh) > 0 and rh.max() < 1.05
