"""Table segments and wide quads just past the grid pattern (tests/perturbed.py): chosen numbers of exceptions in a
quad (up to and past NSK_WIDE_MAXEXC), exceptions at the candidate bases and in the four positions of one lane,
exceptions in every slot, two-chunk (5- and 6-slot) tiles and quads of 3-D grids, more than NSK_TABW_REST_MAX quads
that are not wide in one launch, more than NSK_SEG_MAX segments per colour, removed edges and evidence islands --
inference and learning bit-exact against the oracle, with wide quads and without (NSK_NO_WIDE)."""

import numpy as np
import pytest

from util import session, oracle_of, phases_from_colors
from perturbed import CASES, EXPECTED, LEARN_CASES, ROW, Grid, build_case, run_cells

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _wide_quads_on_small_graphs(monkeypatch):
    monkeypatch.setenv("NSK_DIAG", "1")
    monkeypatch.setenv("NSK_WIDE_MIN", "0")
    monkeypatch.setenv("NSK_WIDE_LEARN_MIN", "0")


def _infer_and_compare(fg, og, seed, burn, sweeps, se):
    """A burn-in call, then one call of `sweeps` (64 + 16 + 5: both captured sequences and an eager remainder)."""
    order, ps = phases_from_colors(fg.colors())
    vv, _, wv, cnt = og.initial_state()
    fg.inference(burn, 0, se)
    fg.inference(0, sweeps, se)
    for s in range(burn + sweeps):
        assert og.gibbs_dev(order, ps, vv, wv, cnt, seed, s, se, burnin=s < burn) == 0
    assert np.array_equal(fg.var_value[0], vv), int((fg.var_value[0] != vv).sum())
    assert np.array_equal(fg.count, cnt), int((fg.count != cnt).sum())


def _check_placement(g, fg, name):
    """The quad the 2-D swap cases perturb is where the cases put it: row 6's run of colour 0 fills one quad, and
    every perturbed cell sits where it sits in the perfect grid."""
    if name in ("removed_island", "many_segments", "rest_many"):       # (these move cells between classes or runs)
        return
    ids = fg.layout()
    if len(g.dims) == 2 and g.dims[1] == 1000:
        q = np.array([ids[v] for v in run_cells(g, ROW, 0, range(256))])
        assert q[0] % 256 == 0 and np.array_equal(q, q[0] + np.arange(256)), name
    ns0, fg0 = session(Grid(g.dims).graph(), seed=1)
    ids0 = fg0.layout()
    moved = [v for v in g.exceptions() if ids[v] != ids0[v]]
    assert not moved, (name, moved[:8])
    fg0.close()


@pytest.mark.parametrize("se", [True, False], ids=["sample_evidence", "no_sample_evidence"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_perturbed_grid_inference(name, se):
    g, graph = build_case(name)
    ns, fg = session(graph, seed=31)
    info = fg.info()
    assert {k: info[k] for k in EXPECTED[name]} == EXPECTED[name], info
    _check_placement(g, fg, name)
    og = oracle_of(fg)
    sweeps = 150 if name == "exc8" else 85          # 150 tallied sweeps: the packed tally is unpacked mid-call
    _infer_and_compare(fg, og, 31, 3, sweeps, se)


@pytest.mark.parametrize("name", sorted(CASES))
def test_perturbed_grid_inference_without_wide_quads(monkeypatch, name):
    """The same graphs on the tile-by-tile table kernel (seg_aff where a tile is affine)."""
    monkeypatch.setenv("NSK_NO_WIDE", "1")
    g, graph = build_case(name)
    ns, fg = session(graph, seed=32)
    assert fg.info()["wide_quads"] == 0
    og = oracle_of(fg)
    _infer_and_compare(fg, og, 32, 2, 85, True)


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "no_wide"])
@pytest.mark.parametrize("name", LEARN_CASES)
def test_perturbed_grid_learning(monkeypatch, name, wide):
    """Two weights, every variable evidence: k_learn_seg_tabw (learn bound 0) or k_learn_seg_tab (NSK_NO_WIDE).
    Whether a learning launch takes the wide kernel is decided per launch when it is planned (at least one wide
    quad per 8 tiles of the launch, nsk_learn.hip); no figure reports that choice, so the test asserts what it
    follows from on the whole graph: at least half of the table quads wide (without NSK_NO_WIDE), none with it."""
    if not wide:
        monkeypatch.setenv("NSK_NO_WIDE", "1")
    g, graph = build_case(name, two_weights=True, fixed=False, evidence_seed=7)
    ns, fg = session(graph, seed=5)
    info = fg.info()
    if wide:
        assert 2 * info["wide_quads"] >= info["tab_quads"] > 0, info
    else:
        assert info["wide_quads"] == 0, info
    og = oracle_of(fg)
    order, ps = phases_from_colors(fg.colors())
    vv, ve, wv, _ = og.initial_state()
    fg.learn(0, 3, 1e-3, 0.9, 2, 0.01, 1)
    assert og.learn_call(order, ps, vv, ve, wv, 3, 1e-3, 0.9, 2, 0.01, 1, False, 5, 0) == 0
    assert np.array_equal(fg.var_value[0], vv) and np.array_equal(fg.var_value_evid[0], ve)
    assert np.array_equal(fg.weight_value[0], wv), (fg.weight_value[0], wv)


def random_case(seed):
    """A seeded shape (2-D or 3-D, odd or even width) with a random mix of swaps, removed edges and an evidence
    island."""
    rng = np.random.default_rng(seed)
    dims = [(16, 1000), (13, 1001), (20, 999), (4, 6, 1000), (4, 7, 801)][rng.integers(0, 5)]
    g = Grid(dims)
    nd = len(dims)
    done = tries = 0
    want = int(rng.integers(4, 40))
    while done < want and tries < 2000:
        tries += 1
        row = tuple(int(rng.integers(1, d - 1)) for d in dims[:-1])
        k1, k2 = sorted(int(x) for x in rng.integers(1, dims[-1] - 1, 2))
        if k1 == k2 or (k2 - k1) % 2:
            continue
        ax2 = int(rng.integers(0, nd - 1))                     # y2 = the earlier cell, along a slower axis
        ax1 = int(rng.integers(ax2, nd))
        try:
            g.swap(g.cell(*row, k2), ax1, g.cell(*row, k1), ax2)
            done += 1
        except (AssertionError, IndexError):
            continue
    for _ in range(int(rng.integers(0, 3))):
        v = g.cell(*(int(rng.integers(1, d - 1)) for d in dims))
        try:
            g.remove(v, int(rng.integers(0, nd)))
        except AssertionError:
            pass
    ev = np.zeros(g.nvar, np.int8)
    if rng.integers(0, 2):
        a = int(rng.integers(0, g.nvar - 300))
        ev[a:a + int(rng.integers(20, 300))] = 1
    return g, g.graph(evidence=rng.integers(0, 2, g.nvar), is_evidence=ev), done


@pytest.mark.parametrize("seed", range(10), ids=lambda s: "seed%d" % s)
def test_random_perturbed_grids(seed):
    g, graph, nswaps = random_case(seed)
    assert nswaps > 0
    for se in (True, False):
        ns, fg = session(graph, seed=100 + seed)
        assert fg.info()["wide_quads"] > 0, (seed, g.dims)
        og = oracle_of(fg)
        _infer_and_compare(fg, og, 100 + seed, 2, 85, se)
        fg.close()
