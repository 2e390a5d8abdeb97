"""The trip loops of the wide-quad table kernels (k_gibbs_seg_tabw, k_gibbs_seg_tabw_chains, k_learn_seg_tabw) at small
shapes, bit for bit against the oracle's device mode.

These kernels run on a resident grid: a launch of T virtual quads gets min(cap, need) workgroups (nsk_internal.h
nsk_tabw_grid / nsk_learn_tabw_grid; the cap is 1536 / 1024 or 2048 workgroups), and only a launch that needs more than
the cap makes its waves loop.  Every other wide-quad test of the suite stays below the cap -- one trip per wave -- so the
code that only a later trip runs (the descriptor loaded a trip ahead, the segment scalars re-read on the way into a
later segment, the thresholds' LDS copy rebuilt there, the keys fetched once, the learning counters carried from trip to
trip) was reached by the full-size runs alone.  NSK_TABW_GRID_CAP and NSK_LEARN_TABW_GRID_CAP (NSK_DIAG=1) lower the
cap, and here they do so far enough for grids the oracle walks in seconds.

The arithmetic, for a cap of c workgroups (a multiple of 8) of four waves each:

- workgroup b of the grid serves XCD b & 7, so an XCD has c / 8 workgroups and wpx = c / 2 waves, numbered
  wx = (b >> 3) * 4 + wave;
- XCD x walks the quads [x per, (x + 1) per) of the launch, per = ceil(T / 8), clipped to T;
- wave wx samples Q = x per + wx, + wpx, + 2 wpx, ...: quad r of an XCD's share is trip r // wpx of wave r % wpx.

So a wave makes a second trip only if per > wpx, that is T > 4 c, and a third only if T > 8 c; with T > 4 c the launch
also needs more than c workgroups (need = 8 ceil(ceil((T + 8) / 4) / 8) > c), so the cap is what sizes the grid.  Under
cap 8 (wpx = 4) the quads 4 .. 7 of every XCD's share are second trips, 8 .. 11 third ones; under cap 16 (wpx = 8, two
workgroups per XCD: wx has a non-zero workgroup term) the quads 8 .. 15 are second trips.

T is not a figure the library reports, so every case bounds it from below from the device layout before it compares
anything: the cells of a colour class lie in at least len(unique(position >> 8)) quads of 256 positions, each of them at
least one virtual quad of the class's launch -- and a sweep is one launch per colour on these grids, which every
inference case counts (nsk_profile_begin / nsk_profile_end).  Three graphs give a colour more segments than one launch
takes, or segments of both chunk counts; their cases count two launches per colour and bound the first from the cells of
its largest segments alone.  The grids (tests/wide_trips.py, shared with the host-only
tests/test_wide_trips_cpu.py) are the smallest of their kind with more than 4 c quads per class: a row of 1000 cells
gives each colour a run of 500, padded to two quads, so 16 rows make 32 quads and the border columns' quads the 33rd.
The evidence grid has 60 rows and the learning grids 28 where tests/test_wide_quads_gpu.py has 48 and 24: at those row
counts 88 % and 89.5 % of the table quads are wide, short of the nine tenths every case here asks of its layout.

Whether a case depends on its later trips was checked once with a build whose waves leave the loop after their first
trip (the three kernels' `Q += wpx` replaced by `Q = q1`): every case of this module fails on it, and
tests/test_wide_quads_gpu.py passes.
"""

import ctypes as C

import numpy as np
import pytest

from numbskull_amd import _lib

from util import session, oracle_of, phases_from_colors
import wide_trips as wt

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _wide_quads_on_small_graphs(monkeypatch):
    """As tests/test_wide_quads_gpu.py: wide quads and wide learning launches on graphs the oracle walks in seconds."""
    for k, v in wt.ENV.items():
        monkeypatch.setenv(k, v)


def _capped(monkeypatch, name, cap, learn=False, **env):
    """The handle of shape `name` under the grid cap `cap` (one the shape is listed with) and further switches."""
    assert cap in wt.SHAPES[name][1] and cap % 8 == 0
    monkeypatch.setenv("NSK_LEARN_TABW_GRID_CAP" if learn else "NSK_TABW_GRID_CAP", str(cap))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return wt.graph(name)


def _assert_multi_trip(fg, cap, trips=2, cells=None):
    """Every table launch is the wide kernel's, and every colour class holds enough quads for `trips` trips under
    `cap`.  `cells`: the cells to count (all of them unless a case names those of one launch)."""
    info = fg.info()
    assert info["wide_quads"] * 10 >= info["tab_quads"] * 9 > 0, info
    # (tests/test_draw_ties_gpu.py's wide cases: all variables in table segments, and so few quads that are not wide that
    #  every launch lists them for its front workgroups -- or samples them in line with NSK_NO_TABW_REST)
    assert info["tab_quads"] - info["wide_quads"] <= 64 and info["nfast"] == info["nvar"], info
    ids, col = fg.layout(), fg.colors()
    assert info["ncolors"] == int(col.max()) + 1 >= 2
    for k in range(info["ncolors"]):
        mine = (col == k) if cells is None else (col == k) & cells
        quads = len(np.unique(ids[mine] >> 8))                 # a lower bound on the launch's virtual quads T
        assert quads > 4 * cap * (trips - 1), (k, quads, cap, trips)
    return info


def _launches(fg, call):
    ms, n = C.c_double(), C.c_int64()
    _lib.check(_lib.lib().nsk_profile_begin(fg._engine()))
    call()
    _lib.check(_lib.lib().nsk_profile_end(fg._engine(), C.byref(ms), C.byref(n)))
    return n.value


def _infer(fg, og, state, seed, s0, burn, sweeps, se, per_sweep):
    """One inference call from sweep index s0 on, counted (`per_sweep` launches a sweep) and walked by the oracle."""
    order, ps, vv, wv, cnt = state
    n = _launches(fg, lambda: fg.inference(burn, sweeps, se))
    assert n == (burn + sweeps) * per_sweep, (n, burn, sweeps, per_sweep)
    for s in range(s0, s0 + burn + sweeps):
        assert og.gibbs_dev(order, ps, vv, wv, cnt, seed, s, se, burnin=s - s0 < burn) == 0
    assert np.array_equal(fg.var_value[0], vv), int((fg.var_value[0] != vv).sum())
    assert np.array_equal(fg.count, cnt), int((fg.count != cnt).sum())


def _run_and_compare(graph, cap, seed, burn, sweeps, se=True, trips=2, more=(), cells=None, per_colour=1):
    """A fresh handle: the multi-trip condition, then `burn` burn-in and `sweeps` tallied sweeps in one call (and the
    calls of `more`, tallied sweeps each) against the oracle -- values and tallies after every call.  `cells`, `per_colour`:
    a graph whose colours take `per_colour` launches each names the cells that bound its first launches."""
    ns, fg = session(graph, seed=seed)
    info = _assert_multi_trip(fg, cap, trips, cells)
    per_sweep = per_colour * info["ncolors"]
    og = oracle_of(fg)
    order, ps = phases_from_colors(fg.colors())
    vv, _, wv, cnt = og.initial_state()
    state = (order, ps, vv, wv, cnt)
    _infer(fg, og, state, seed, 0, burn, sweeps, se, per_sweep)
    s0 = burn + sweeps
    for n in more:
        _infer(fg, og, state, seed, s0, 0, n, se, per_sweep)
        s0 += n
    fg.close()


# ---- 1: one chain.  A burn-in launch is MODE 1, a tallied one of a handle whose every launch is wide MODE 2 (the tally
# inside the value bytes) and, with NSK_NO_PACK_TALLY, MODE 0 (the position tally).  33 x 1537: the two colours' rows
# differ in length.  9 x 4099: the three-slot border rows are wide segments of nine quads each, so a wave walks from one
# wide segment into the next on a later trip (the segment scalars re-read, the LDS thresholds rebuilt).  Cap 16: a second
# workgroup per XCD.
@pytest.mark.parametrize("name,cap,trips", [("grid40x1000", 8, 3), ("grid33x1537", 8, 2), ("grid9x4099", 8, 2),
                                            ("grid40x1000", 16, 2)])
def test_later_trips_of_burn_in_and_packed_tally_launches(monkeypatch, name, cap, trips):
    _run_and_compare(_capped(monkeypatch, name, cap), cap, 5, 2, 5, trips=trips)


def test_later_trips_of_position_tally_launches(monkeypatch):
    _run_and_compare(_capped(monkeypatch, "grid16x1000", 8, NSK_NO_PACK_TALLY="1"), 8, 13, 2, 20)


# ---- 2: 37 + 300 sweeps in one call replay the captured sequences of 64 and 16 sweeps, end eagerly and cross the
# 127-sweep unpack of the packed tally; a second call continues from plain values (the shape of
# tests/test_wide_quads_gpu.py test_wide_quads_in_captured_sequences_and_tally_folds, every wave on several trips)
def test_captured_sequences_and_tally_unpacks_on_later_trips(monkeypatch):
    _run_and_compare(_capped(monkeypatch, "grid16x1000", 8), 8, 9, 37, 300, more=(21,))


# ---- 3: evidence columns split every class by evidence flag: runs of mixed length, several segments per launch, and
# with sample_evidence = False launches over the free cells alone.  With the evidence sampled a colour has more segments
# than the NSK_SEG_MAX = 8 of a launch -- interior, top row, bottom row, border column and corner, free and evidence -- and
# takes two launches, so the colour's quads do not bound a launch.  The launches are filled with the segments largest
# first (nsk_gibbs.hip nsk_ensure_seg_plans): the free interior cells, one class and most of their colour, are in the
# first launch whichever way, and they alone are the bound here.
@pytest.mark.parametrize("se", [True, False], ids=["sample_evidence", "no_sample_evidence"])
def test_later_trips_across_evidence_segments(monkeypatch, se):
    graph = _capped(monkeypatch, "evidence60x1200", 8)
    rows, cols = 60, 1200
    assert len(graph[1]) == rows * cols
    r, c = np.divmod(np.arange(rows * cols), cols)
    interior = (r > 0) & (r < rows - 1) & (c > 0) & (graph[1]["isEvidence"] == 0)
    assert 2 * interior.sum() > rows * cols                                    # ... most of the grid
    _run_and_compare(graph, 8, 21, 1, 4, se=se, cells=interior, per_colour=2 if se else 1)


# ---- 4: the quads that are not wide (border columns, class ends).  In line (NSK_NO_TABW_REST): the tile-by-tile
# fall-back inside the trip loop, reached by waves that have their keys already.  Listed for front workgroups: the capped
# grid sits behind them (bid = blockIdx.x - nfront).
@pytest.mark.parametrize("inline", [True, False], ids=["in_line", "front_workgroups"])
def test_later_trips_beside_quads_that_are_not_wide(monkeypatch, inline):
    env = {"NSK_NO_TABW_REST": "1"} if inline else {}
    graph = _capped(monkeypatch, "grid24x1000", 8, **env)
    ns, fg = session(graph, seed=5)
    info = fg.info()
    assert info["wide_quads"] < info["tab_quads"], info          # there ARE quads that are not wide
    fg.close()
    _run_and_compare(graph, 8, 5, 1, 3)


# ---- 5: exception cells in capped launches.  exc8: eight exceptions in one quad, wide_finish's scalar loop (16 x 1000: 33
# quads per class or more, enough for cap 8).  slots45_3d: 5- and 6-slot classes, two-chunk quads (NCH = 2) -- a launch of
# their own beside the one of the box's edges (four slots and fewer), so a colour takes two launches and the bound is on
# the cells of five and six slots, 28 of the box's 32 rows.
@pytest.mark.parametrize("name", ["exc8", "slots45_3d"])
def test_later_trips_of_quads_with_exceptions(monkeypatch, name):
    graph = _capped(monkeypatch, name, 8)
    if name == "exc8":
        _run_and_compare(graph, 8, 31, 3, 5)
        return
    slots = np.bincount(graph[3]["vid"], minlength=len(graph[1]))          # factors per variable
    assert slots.max() == 6
    _run_and_compare(graph, 8, 31, 3, 5, cells=slots >= 5, per_colour=2)


def test_exceptions_on_a_second_trip(monkeypatch):
    """exc8's quad sits where a wave meets it on its first trip (quad 10 of its launch: XCD 2's first under per = 5).  The
    same eight exceptions in quad 0 of row 3 are quad 4 of their launch: the interior cells of a colour are its largest
    segment, numbered first, with two quads per row and no dead tiles in front.  Every launch here has T > 32 quads, so
    per >= 5 > 4: quad 4 belongs to XCD 0 and is the second trip of its wave 0, whatever T is."""
    _capped(monkeypatch, "exc8_row3", 8)
    g, graph = wt.later_trip_exceptions()
    ns, fg = session(graph, seed=31)
    ids, col = fg.layout(), fg.colors()
    r, c = np.divmod(np.arange(16 * 1000), 1000)
    interior = (r > 0) & (r < 15) & (c > 0) & (c < 999)
    exc = g.exceptions()
    row3 = [v for v in exc if v // 1000 == 3]
    assert sorted(sum(len(exc[v]) for v in row3 if col[v] == k) for k in (0, 1)) == [4, 8]     # in one quad per colour
    for v in row3:
        mine = interior & (col == col[v])
        pos0 = int(ids[mine].min())
        assert 2 * mine.sum() > (col == col[v]).sum() and pos0 % 256 == 0          # the largest segment, no lead tiles
        assert (int(ids[v]) - pos0) >> 8 == 4, (v, int(ids[v]), pos0)
    fg.close()
    _run_and_compare(graph, 8, 31, 3, 5)


# ---- 6: k_gibbs_seg_tabw_chains: three chains in one launch per class (three copies of the capped grid), chain r
# against the oracle seeded seed ^ (r << 32) -- not against one-chain handles under the same cap, where a fault common to
# both kernels would cancel
def test_later_trips_of_chain_batched_launches(monkeypatch):
    graph, seed, nch, burn, sweeps = _capped(monkeypatch, "grid16x1000", 8), 77, 3, 3, 20
    ns, fg = session(graph, seed=seed, chains=nch)
    info = _assert_multi_trip(fg, 8)
    og = oracle_of(fg)
    order, ps = phases_from_colors(fg.colors())

    def run():
        fg.burnIn(burn, True, var_copy="all")
        fg.inference(0, sweeps, True, var_copy="all")
    assert _launches(fg, run) == (burn + sweeps) * info["ncolors"]       # every class launch serves all chains
    total = 0
    for r in range(nch):
        vv, _, wv, cnt = og.initial_state()
        for s in range(burn + sweeps):
            assert og.gibbs_dev(order, ps, vv, wv, cnt, seed ^ (r << 32), s, True, burnin=s < burn) == 0
        assert np.array_equal(fg.var_value[r], vv), (r, int((fg.var_value[r] != vv).sum()))
        assert np.array_equal(fg.chain_count[r], cnt), (r, int((fg.chain_count[r] != cnt).sum()))
        total = total + cnt
    assert np.array_equal(fg.count, total)
    fg.close()


# ---- 7: k_learn_seg_tabw under NSK_LEARN_TABW_GRID_CAP.  Every variable evidence: the free chain's draw alone.  Half
# of them (whole rows) with learn_non_evidence: the evidence chain's own draw and segments of both evidence flags, so the
# gradient counters live across trips and across changes of the slot program.  Regularization 1 with truncation 3 counts
# the truncation coins too (accT / accTv).  NSK_ONE_ACC: bins shared across XCDs (agent-scope adds).  NSK_NO_TABW_REST:
# the ballot counters of the tiles sampled in line (acc) and the per-lane ones of the wide quads (accv) within one wave's
# trips.  (A learning sweep's launches are not counted here -- the updates ride along --, and the half-evidence grid has
# more segments per colour than one launch takes: the bound is on the interior cells, the colour's two largest segments
# at most, which the first launch holds whichever way.)
LEARN = [("all", 2, 1, {}), ("all", 1, 3, {}), ("half", 2, 1, {}), ("half", 1, 3, {}),
         ("half", 2, 1, {"NSK_ONE_ACC": "1"}), ("half", 1, 3, {"NSK_NO_TABW_REST": "1"})]


@pytest.mark.parametrize("evidence,reg,trunc,env", LEARN,
                         ids=["%s-reg%d%s" % (e, r, "".join("-" + k for k in v)) for e, r, t, v in LEARN])
def test_later_trips_of_learning_launches(monkeypatch, evidence, reg, trunc, env):
    half = evidence == "half"
    graph = _capped(monkeypatch, "learn28x1000_half" if half else "learn28x1000", 8, learn=True, **env)
    ns, fg = session(graph, seed=5)
    rows, cols = 28, 1000
    assert len(graph[1]) == rows * cols
    r, c = np.divmod(np.arange(rows * cols), cols)
    info = _assert_multi_trip(fg, 8, cells=(r > 0) & (r < rows - 1) & (c > 0) & (c < cols - 1))
    assert info["acc_copies"] == (1 if "NSK_ONE_ACC" in env else 17), info
    og = oracle_of(fg)
    order, ps = phases_from_colors(fg.colors())
    vv, ve, wv, _ = og.initial_state()
    w0 = wv.copy()
    fg.learn(0, 3, 1e-3, 0.9, reg, 0.01, trunc, learn_non_evidence=half)
    assert og.learn_call(order, ps, vv, ve, wv, 3, 1e-3, 0.9, reg, 0.01, trunc, half, 5, 0) == 0
    assert np.array_equal(fg.var_value[0], vv), int((fg.var_value[0] != vv).sum())
    assert np.array_equal(fg.var_value_evid[0], ve), int((fg.var_value_evid[0] != ve).sum())
    assert np.array_equal(fg.weight_value[0], wv), (fg.weight_value[0], wv)
    assert (wv != w0).all(), (w0, wv)                                    # the weights moved
    fg.close()
