"""Forced 27-bit draw ties and table entries at the edge of float64, bit for bit against the oracle.

The table kernels decide a draw from the top 27 bits of a Philox block and evaluate a second block only when some
lane's top bits equal the threshold's (nsk_kernels_gibbs.h tab_tiles / tab_tiles_x / wide_finish; 2^-27 per update).
tests/flip_pairs.py finds, with the oracle, two adjacent doubles w_a, w_b of the grid's one weight at which a chosen
variable v comes out 0 and 1 while the two thresholds share their top 27 bits: v's draw then ties at BOTH weights
and must resolve to 0 at w_a and to 1 at w_b.  Each case first asserts that v lies where the case says (generator
scheme bits 40 / 41 of FactorGraph.generators(), position in FactorGraph.layout(), figures of FactorGraph.info()),
then runs the library on fresh handles at w_a and at w_b and compares the whole state and the tallies with the oracle's
run at that weight (np.array_equal: no tolerance anywhere).  gap = K(w_a) - K(w_b); gap == 1 pins v's draw to the
threshold itself (lo == e.y, the inclusive boundary); the last test of the file asks for three such cases.

Cases: (1) the tile-by-tile kernel, the four words of a quad's blocks; (2) the second tile pair of a quad in a launch
dealt in pairs, and a quad of a later trip of a grid-capped launch; (3) wide quads, the lane's four words, packed tally,
plain tally and burn-in; (4) quads of a wide launch that are not wide, in front workgroups and in line; (5) wide-scheme
positions sampled tile by tile (ds_bpermute of the second block); (6) chain-batched launches; (7) a tie at sweep 20 of a
captured 64-sweep call; (9) learning sweeps (53-bit compares against the same tables), free and evidence chain, tile by
tile and wide; (8) the fused peer-to-peer copy of the branch (tab_tiles_x): two shards of a grid on one device through
tests/test_config5_shards_gpu.py's harness, v in a border tile of shard 0's first class.

Then the tables at weights where z1 overflows or the potentials are NaN, and a learning run whose weights run through
overflow, both bit-exact (float64 patterns compared as integers, so that NaN equals NaN).
"""

import numpy as np
import pytest

from numbskull_amd import graphgen
from util import session, oracle_of, phases_from_colors
import flip_pairs as fp

pytestmark = pytest.mark.gpu

SEED = 77
GAPS = {}              # case -> gap, for the closing test and the printed record
WIDE = {"NSK_DIAG": "1", "NSK_WIDE_MIN": "0"}


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _grid(rows, cols, **kw):
    """One shared weight; a seeded random start, so that the first class of sweep 0 meets every neighbourhood."""
    rng = np.random.default_rng(rows * 10000 + cols)
    return graphgen.ising_grid(rows, cols, weight=0.3, initial=rng.integers(0, 2, rows * cols), **kw)


def _half_evidence(rows, cols):
    """Fixed weight, seeded values, the right half of every row evidence (learning: the weights cannot move)."""
    rng = np.random.default_rng(rows * 10000 + cols + 1)
    g = graphgen.ising_grid(rows, cols, weight=0.3, fixed=True, evidence=rng.integers(0, 2, rows * cols))
    g[1]["isEvidence"] = ((np.arange(rows * cols) % cols) >= cols // 2).astype(g[1]["isEvidence"].dtype)
    return g


def _quad(gen):
    return (gen >> 40) & 1 == 1 and (gen >> 41) & 1 == 0      # quad scheme: word (q >> 6) & 3 of the quad's blocks


def _wide(gen):
    return (gen >> 41) & 1 == 1                              # wide scheme: word q & 3 of the lane's blocks


def _placement(fg):
    return fg.layout(), fg.colors(), fg.generators()


def _infer_at(graph, seed, w, order, ps, ids, burn, sweeps, v, sweep, expect):
    """A fresh handle at weight w against the oracle at w: whole state and tallies."""
    ns, fg = session(graph, seed=seed)
    fg.weight_value[0][:] = w                      # uploaded at call entry
    og = oracle_of(fg)
    assert np.array_equal(fg.layout(), ids)
    vv, _, wv, cnt = og.initial_state()
    wv[:] = w
    fg.inference(burn, sweeps, True)
    for s in range(burn + sweeps):
        assert og.gibbs_dev(order, ps, vv, wv, cnt, seed, s, True, burnin=s < burn) == 0
        if s == sweep:
            assert vv[v] == expect                 # the oracle's own flip, in the full run too
    same = np.array_equal(fg.var_value[0], vv) and np.array_equal(fg.count, cnt)
    at_v = (int(fg.var_value[0][v]), int(vv[v]))
    fg.close()
    return same, at_v


def _tie_case(monkeypatch, name, graph, env, pred, check, cls=0, sweep=0, burn=0, sweeps=2, seed=SEED, where=None,
              prepare=None):
    _setenv(monkeypatch, env)
    ns, fg = session(graph, seed=seed)
    info = fg.info()
    check(info)
    ids, col, gen = _placement(fg)
    if prepare is not None:
        pred = prepare(fg, ids, col, gen)
    og = oracle_of(fg)
    order, ps = phases_from_colors(col)
    cands = fp.candidates_by_position(ids, col, cls, pred, gen=gen)
    pair = fp.first_flip_pair(cands, lambda v, why: fp.find_flip_pair(og, order, ps, seed, sweep, v, cls=cls, why=why))
    v = pair.v
    assert col[v] == cls and pred(int(ids[v]), int(gen[v]))                 # v sits where the case says
    if where is not None:
        where(fg, ids, col, gen, v)
    assert pair.K_a >> 26 == pair.K_b >> 26 and pair.gap >= 1
    GAPS[name] = pair.gap
    print("%s: v=%d q=%d w_a=%r w_b=%r K_a=%d gap=%d" % (name, v, ids[v], pair.w_a, pair.w_b, pair.K_a, pair.gap))
    fg.close()
    for w, expect in ((pair.w_a, 0), (pair.w_b, 1)):
        same, at_v = _infer_at(graph, seed, w, order, ps, ids, burn, sweeps, v, sweep, expect)
        assert same, (name, "w_a" if expect == 0 else "w_b", at_v)
    return pair


def _dealt_in_pairs(fg, ids, col, gen, v):
    """The class launch of v runs in tile pairs (split = 1).  nsk_tab_grid gives a launch of `vt` virtual tiles
    need = 8 ceil(ceil(vt / 8) / 8) workgroups when need <= 2048, i.e. wpx = need / 2 >= 4 ceil(quads / 16) waves per XCD
    against per = ceil(quads / 8) quads per XCD: per < wpx for every count, so no whole round of quads is dealt and every
    unit is a pair (k_gibbs_seg_tab's h >= 0 branch, tab_tiles<.., 2>).  vt is bounded from the layout: the class's
    tiles in at most that many segments, each padded by at most 6 dead tiles."""
    tiles = len(np.unique(ids[col == col[v]] >> 6))
    vt = 7 * tiles
    need = max(8, 8 * (((vt // 2 + 3) // 4 + 7) // 8))
    assert need <= 2048, (tiles, need)


# ---- 1 + 2a: the tile-by-tile kernel (no wide quads), word (q >> 6) & 3 = 0 .. 3.  A launch this small is dealt in tile
# pairs (_dealt_in_pairs): words 2 and 3 are the SECOND pair of their quad (tab_tiles<.., 2> with w0 = 2), sampled by a
# wave of its own that evaluates its own second block -- nothing is shared between the pairs here; a second block that
# must be started afresh for the next quad of the SAME wave is the capped case's below.
@pytest.mark.parametrize("word", [0, 1, 2, 3])
def test_tie_in_the_tile_by_tile_kernel(monkeypatch, word):
    def check(info):
        assert info["wide_quads"] == 0 and info["ztab_entries"] > 0 and info["nfast"] == info["nvar"] == 64 * 300, info
    _tie_case(monkeypatch, "tile_word%d" % word, _grid(64, 300), {},
              lambda q, g: _quad(g) and (q >> 6) & 3 == word, check, where=_dealt_in_pairs)


# ---- 2b: a grid-capped launch (8 workgroups: 4 waves per XCD), v in a quad that its wave reaches on a later trip.
# XCD x walks quads [x per, (x + 1) per) of the launch's virtual quads, per = ceil(quads / 8): quad r of that eighth is
# trip r / 4 of wave r % 4 when it belongs to the whole rounds, and a pair unit behind them otherwise -- either way
# r >= 4 is a trip after the wave's first, on which have_b must start false again.  The interior cells (four slots) are
# one run of positions and the class's largest segment, which the launch numbers first (tile_start 0, `lead` dead
# tiles in front); the few other tiles add between 1 and 2 quads each, so `per` is 5 or 6 and quad 4 is a later trip
# under both.
def test_tie_on_a_later_trip_of_a_capped_launch(monkeypatch):
    def interior_run(fg, ids, col):
        nb = fg.vmap["factor_index_length"][fg.variable["vtf_offset"]]
        inner = (col == 0) & (nb == 4)
        pos = np.sort(ids[inner])
        assert np.array_equal(pos, pos[0] + np.arange(len(pos))) and pos[0] % 64 == 0      # one run of whole tiles
        return inner, int(pos[0]), len(pos)

    def prepare(fg, ids, col, gen):
        inner, pos0, n = interior_run(fg, ids, col)
        lead = (pos0 >> 6) & 3
        return lambda q, g: _quad(g) and q >= pos0 and (lead + ((q - pos0) >> 6)) >> 2 == 4

    def where(fg, ids, col, gen, v):
        inner, pos0, n = interior_run(fg, ids, col)
        assert inner[v] and 2 * n > (col == 0).sum()                  # the largest segment: first in the launch
        lead = (pos0 >> 6) & 3
        quads0 = (((n + 63) >> 6) + lead + 3) >> 2
        others = len(np.unique(ids[(col == 0) & ~inner] >> 6))        # tiles of the class's other segments
        assert others >= 1
        Q = (lead + ((int(ids[v]) - pos0) >> 6)) >> 2
        for nquads in range(quads0 + 1, quads0 + 2 * others + 1):
            per = (nquads + 7) >> 3
            assert per >= 5 and Q < per and (Q // per + 1) * per <= nquads and Q % per >= 4, (Q, per, nquads)

    _tie_case(monkeypatch, "capped_trip", _grid(128, 128), {"NSK_DIAG": "1", "NSK_TAB_GRID_CAP": "8"}, None,
              lambda info: None, where=where, prepare=prepare)


# ---- 3: wide quads (generator bit 41), the lane's word q & 3.  A one-chain handle whose every launch is the wide
# kernel's keeps its tally in the value bytes (MODE 2: the tie store must keep tally & 0xFE and write 3 nv): word 0 ties
# in the third sweep of a burn-in sweep and three tallied ones.  Words 1 and 3 switch the packing off (MODE 0, the
# position tally), word 2 ties in a burn-in sweep (MODE 1) that is the whole run: a burn-in flip leaves no tally, and a
# later sweep would resample v and could wash it out.  (Whether a handle packs is decided in nsk_gibbs.hip -- every
# launch plan wide, no NSK_NO_PACK_TALLY -- and no figure of info() reports it: word 0 asserts what packing follows
# from, a layout of wide quads whose few other quads the wide launches list for their front workgroups, and would run
# MODE 0 unnoticed if a later layout left one launch to the tile-by-tile kernel.)
@pytest.mark.parametrize("word,env,burn,sweeps,sweep", [(0, {}, 1, 3, 2), (1, {"NSK_NO_PACK_TALLY": "1"}, 0, 2, 0),
                                                        (2, {}, 1, 0, 0), (3, {"NSK_NO_PACK_TALLY": "1"}, 1, 2, 1)])
def test_tie_in_a_wide_quad(monkeypatch, word, env, burn, sweeps, sweep):
    def check(info):
        assert info["wide_quads"] * 10 >= info["tab_quads"] * 9 > 0, info
        assert info["tab_quads"] - info["wide_quads"] <= 64 and info["nfast"] == info["nvar"], info
    _tie_case(monkeypatch, "wide_word%d" % word, _grid(16, 1000), dict(WIDE, **env),
              lambda q, g: _wide(g) and q & 3 == word, check, burn=burn, sweeps=sweeps, sweep=sweep)


# ---- 4: the quads of a wide launch that are not wide (the grid's border columns: quad scheme, bit 41 clear): front
# workgroups (tab_tiles<.., 1, MODE>, a wave per tile) at the defaults, in line with NSK_NO_TABW_REST.
@pytest.mark.parametrize("inline", [False, True], ids=["front_workgroups", "in_line"])
def test_tie_in_a_quad_of_a_wide_launch_that_is_not_wide(monkeypatch, inline):
    def check(info):
        assert info["wide_quads"] * 10 >= info["tab_quads"] * 9 > 0 and info["wide_quads"] < info["tab_quads"], info
        # (every launch has at least half of its quads wide: the wide kernel takes it, nsk_gibbs.hip; and at most 5 of
        #  them are not: fewer than NSK_TABW_REST_MAX, so they are listed for the front workgroups)
        assert info["tab_quads"] - info["wide_quads"] <= 64, info
    env = dict(WIDE, NSK_NO_TABW_REST="1") if inline else WIDE
    _tie_case(monkeypatch, "rest_%s" % ("inline" if inline else "front"), _grid(16, 1000), env,
              lambda q, g: _quad(g), check)


# ---- 5: wide-scheme positions sampled tile by tile (ws = true: wide_word_of_tile on BOTH blocks).  The smallest
# set-up that produces it: the 16 x 1000 grid's wide layout with NSK_NO_WIDE_KERNEL, which hands every launch to
# k_gibbs_seg_tab; v at offset 64 k + l of its quad with k >= 1 and l & 3 != 0.
@pytest.mark.parametrize("word", [1, 3])
def test_tie_at_a_wide_scheme_position_sampled_tile_by_tile(monkeypatch, word):
    def check(info):
        assert info["wide_quads"] * 10 >= info["tab_quads"] * 9 > 0, info
    _tie_case(monkeypatch, "wide_scheme_tile%d" % word, _grid(16, 1000), dict(WIDE, NSK_NO_WIDE_KERNEL="1"),
              lambda q, g: _wide(g) and (q & 255) >> 6 >= 1 and q & 3 == word, check)


# ---- 6: chain-batched launches: three chains, the tie in chain 1 (seed ^ 1 << 32); all chains against one-chain oracles
def test_tie_in_a_chain_batched_launch(monkeypatch):
    graph, nch = _grid(57, 33), 3
    ns, fg = session(graph, seed=SEED, chains=nch)
    assert fg.info()["ztab_entries"] > 0 and fg.info()["nfast"] == 57 * 33
    ids, col, gen = _placement(fg)
    og = oracle_of(fg)
    order, ps = phases_from_colors(col)
    s1 = SEED ^ (1 << 32)
    cands = fp.candidates_by_position(ids, col, 0, lambda q, g: _quad(g), gen=gen)
    pair = fp.first_flip_pair(cands, lambda v, why: fp.find_flip_pair(og, order, ps, s1, 0, v, why=why))
    GAPS["chains"] = pair.gap
    print("chains: v=%d q=%d w_a=%r w_b=%r gap=%d" % (pair.v, ids[pair.v], pair.w_a, pair.w_b, pair.gap))
    fg.close()
    for w, expect in ((pair.w_a, 0), (pair.w_b, 1)):
        ns, fg = session(graph, seed=SEED, chains=nch)
        fg.weight_value[0][:] = w
        fg.inference(0, 2, True, var_copy="all")
        total = 0
        for r in range(nch):
            vv, _, wv, cnt = og.initial_state()
            wv[:] = w
            for s in range(2):
                assert og.gibbs_dev(order, ps, vv, wv, cnt, SEED ^ (r << 32), s, True) == 0
                if r == 1 and s == 0:
                    assert vv[pair.v] == expect
            assert np.array_equal(fg.var_value[r], vv), (r, expect)
            assert np.array_equal(fg.chain_count[r], cnt), (r, expect)
            total = total + cnt
        assert np.array_equal(fg.count, total)
        fg.close()


# ---- 7: sweep 20 of one 64-sweep call (a captured sequence: the replayed launches must hand the sweep index to the
# second block too).  The bisection runs the oracle's sweeps 0 .. 20; a pair whose flip is a neighbour's is refused.
def test_tie_inside_a_captured_sequence(monkeypatch):
    def check(info):
        assert info["wide_quads"] > 0, info
    _tie_case(monkeypatch, "captured_sweep20", _grid(16, 1000), WIDE, lambda q, g: _wide(g), check,
              sweep=20, burn=0, sweeps=64)


# ---- 8: the fused peer-to-peer copy of the branch (tab_tiles_x): a 64 x 300 grid in two range shards on one device,
# their boundary exchanged inside the table launches.  v is a cell of shard 0's last row in the shard's first class: it
# reads a ghost (the cell below it belongs to shard 1), so its tile is a border tile (nsk_exchange.hip p2p_fuse_plan) and the
# fused launch samples it with tab_tiles_x.  Sweep 0 reads the ghosts' initial values, so shard 0's own oracle IS the
# emulation there; the comparison at w_a and w_b is the harness's (owned values, ghosts and tallies of both shards).
def test_tie_in_the_fused_peer_to_peer_launch(monkeypatch):
    import test_config5_shards_gpu as shards
    monkeypatch.setattr(shards, "WORLD", 2)
    rows, cols, seed = 64, 300, 20240601                                    # (run_case's seed)
    parts, _, _ = shards.make_parts("grid", (rows, cols), False, seed)
    fg = parts[0].fg
    ids, col, gen = _placement(fg)
    lo, hi = fg.own_range
    gids = np.asarray(fg.global_ids)
    cls = int(col[lo:hi][col[lo:hi] >= 0].min())
    og = oracle_of(fg)
    order, ps = phases_from_colors(col)
    last_row = np.zeros(len(ids), bool)
    last_row[lo:hi] = gids[lo:hi] // cols == rows // 2 - 1                   # the cell below is shard 1's
    at = np.full(int(ids.max()) + 1, -1, np.int64)
    at[ids] = np.arange(len(ids))
    cands = fp.candidates_by_position(ids, col, cls, lambda q, g: _quad(g) and bool(last_row[at[q]]), gen=gen)
    pair = fp.first_flip_pair(cands, lambda v, why: fp.find_flip_pair(og, order, ps, seed, 0, v, cls=cls, why=why))
    v, gv = pair.v, int(gids[pair.v])
    assert lo <= v < hi and col[v] == cls and gv // cols == rows // 2 - 1 and _quad(int(gen[v]))
    GAPS["fused_p2p"] = pair.gap
    print("fused_p2p: v=%d (global %d) q=%d w_a=%r w_b=%r gap=%d" % (v, gv, ids[v], pair.w_a, pair.w_b, pair.gap))
    for p in parts:
        p.fg.close()

    def probe(parts, needs):
        assert all(p.fg.info()["p2p_fused"] == 1 for p in parts)
        assert gv + cols in set(int(x) for x in needs[0])                    # v's tile reads a ghost: a border tile
        assert np.array_equal(parts[0].fg.layout(), ids)
    for w in (pair.w_a, pair.w_b):
        shards.run_case("grid", (rows, cols), False, "tie2shards (64x300 grid, two shards)", nsweeps=2, fused=True,
                        probe=probe, weight=w)


# ---- 9: learning compares all 53 bits with the same table entries: an off-by-one K moves these draws.
def _learn_case(monkeypatch, name, graph, env, chain, check, scheme):
    _setenv(monkeypatch, env)
    ns, fg = session(graph, seed=SEED)
    check(fg.info())
    ids, col, gen = _placement(fg)
    og = oracle_of(fg)
    order, ps = phases_from_colors(col)
    free = graph[1]["isEvidence"] == 0
    run = fp.learn_runner(og, order, ps, SEED, 0, 0)
    at = np.full(int(ids.max()) + 1, -1, np.int64)
    at[ids] = np.arange(len(ids))                                            # position -> variable
    cands = fp.candidates_by_position(ids, col, 0, lambda q, g: scheme(g) and (chain == 0 or bool(free[at[q]])), gen=gen)
    pair = fp.first_flip_pair(cands, lambda v, why: fp.find_flip_pair(og, order, ps, SEED, 0, v, run=run, chain=chain, why=why))
    assert col[pair.v] == 0 and scheme(int(gen[pair.v])) and (chain == 0 or free[pair.v])    # v sits where the case says
    GAPS[name] = pair.gap
    print("%s: v=%d q=%d w_a=%r w_b=%r gap=%d" % (name, pair.v, ids[pair.v], pair.w_a, pair.w_b, pair.gap))
    fg.close()
    for w, expect in ((pair.w_a, 0), (pair.w_b, 1)):
        ns, fg = session(graph, seed=SEED)
        fg.weight_value[0][:] = w
        og = oracle_of(fg)
        vv, ve, wv, _ = og.initial_state()
        wv[:] = w
        fg.learn(0, 1, 0.01, 1.0, 0, 0.0, 1)
        assert og.learn_call(order, ps, vv, ve, wv, 1, 0.01, 1.0, 0, 0.0, 1, False, SEED, 0) == 0
        assert np.array_equal(fg.var_value[0], vv), (name, expect, int(fg.var_value[0][pair.v]))
        assert np.array_equal(fg.var_value_evid[0], ve), (name, expect, int(fg.var_value_evid[0][pair.v]))
        assert np.array_equal(fg.weight_value[0].view(np.int64), wv.view(np.int64))
        fg.close()


@pytest.mark.parametrize("chain", [0, 1], ids=["free_chain", "evidence_chain"])
def test_learning_draw_at_the_threshold(monkeypatch, chain):
    def check(info):
        assert info["wide_quads"] == 0 and info["ztab_entries"] > 0, info
    _learn_case(monkeypatch, "learn_chain%d" % chain, _half_evidence(64, 300), {}, chain, check, _quad)


def test_learning_draw_at_the_threshold_wide_kernel(monkeypatch):
    """k_learn_seg_tabw (NSK_WIDE_LEARN_MIN=0), the free chain's draw of a variable inside a wide quad (bit 41)."""
    def check(info):
        assert 2 * info["wide_quads"] >= info["tab_quads"] > 0, info
    _learn_case(monkeypatch, "learn_wide", _half_evidence(16, 1000), dict(WIDE, NSK_WIDE_LEARN_MIN="0"), 0, check, _wide)


# ---- table entries at the edge of float64 ----
# 4 neighbours x 177.5 = 710: past nsk_exp's overflow bound, z1 = inf (the rule gives 0 at k = 0 and, for a finite z0, 1
# elsewhere); inf and NaN weights make NaN potentials (0 * inf) -- both comparisons false, value 0; 8.75 x 4 = 35:
# z0 / z1 2^53 near 1, K >> 26 == 0; 5e-324 and 1e-300: products that underflow to 0 or stay denormal.
EDGE_WEIGHTS = [0.0, -0.0, 5e-324, 1e-300, -1e-300, 8.75, -8.75, 40.0, -40.0, 177.5, -177.5, 1e308, -1e308,
                float("inf"), float("-inf"), float("nan")]


@pytest.mark.parametrize("shape", [(57, 33), (16, 1000)], ids=["57x33", "16x1000_wide"])
@pytest.mark.parametrize("w", EDGE_WEIGHTS, ids=[repr(w) for w in EDGE_WEIGHTS])
def test_table_entries_at_the_edge_of_float64(monkeypatch, shape, w):
    if shape == (16, 1000):
        _setenv(monkeypatch, WIDE)
    graph = _grid(*shape)
    ns, fg = session(graph, seed=SEED)
    info = fg.info()
    assert info["ztab_entries"] > 0 and (info["wide_quads"] > 0) == (shape == (16, 1000)), info
    fg.weight_value[0][:] = w
    og = oracle_of(fg)
    order, ps = phases_from_colors(fg.colors())
    vv, _, wv, cnt = og.initial_state()
    wv[:] = w
    fg.inference(1, 4, True)
    for s in range(5):
        assert og.gibbs_dev(order, ps, vv, wv, cnt, SEED, s, True, burnin=s < 1) == 0
    assert np.array_equal(fg.var_value[0], vv), int((fg.var_value[0] != vv).sum())
    assert np.array_equal(fg.count, cnt), int((fg.count != cnt).sum())


def test_learning_through_overflowing_weights():
    """learn_cap = 0, step 50, no regulariser: the two weights run through overflow within 6 sweeps and k_apply_bins
    rebuilds the tables from them.  Both chains and the weights' float64 patterns equal the oracle's."""
    rng = np.random.default_rng(12)
    graph = graphgen.ising_grid(64, 300, weight=0.0, fixed=False, two_weights=True, evidence=rng.integers(0, 2, 64 * 300))
    ns, fg = session(graph, seed=SEED, learn_cap=0.0)
    og = oracle_of(fg)
    order, ps = phases_from_colors(fg.colors())
    vv, ve, wv, _ = og.initial_state()
    fg.learn(0, 6, 50.0, 1.0, 0, 0.0, 1)
    assert og.learn_call(order, ps, vv, ve, wv, 6, 50.0, 1.0, 0, 0.0, 1, False, SEED, 0, cap=0.0) == 0
    print("weights after 6 sweeps:", fg.weight_value[0], wv)
    assert np.abs(wv).min() > 177.5, wv            # 4 neighbours: |potential| > 710, nsk_exp overflows in every rebuilt entry
    assert np.array_equal(fg.weight_value[0].view(np.int64), wv.view(np.int64)), (fg.weight_value[0], wv)
    assert np.array_equal(fg.var_value[0], vv), int((fg.var_value[0] != vv).sum())
    assert np.array_equal(fg.var_value_evid[0], ve), int((fg.var_value_evid[0] != ve).sum())


def test_three_cases_hit_the_boundary_itself():
    """gap == 1: v's draw IS the threshold (lo == e.y), resolved from both sides.  In file order, after every case."""
    print("gaps:", GAPS)
    assert sum(1 for g in GAPS.values() if g == 1) >= 3, GAPS
