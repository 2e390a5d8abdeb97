"""Graphs whose colour classes are large enough that, under the diagnostic cap of the class plans' persistent grids
(NSK_DIAG=1 NSK_CLASS_GRID_CAP, numbskull_amd/csrc/nsk_class_plan.h), the waves of the learning kernels -- and of the
inference group walk -- make a second and a third trip: one table for tests/test_class_trips_cpu.py (what the host-only
plan says about each case: routes, trips per wave, liveliness in the oracle) and tests/test_class_trips_gpu.py (the runs
against the oracle), so that the two cannot drift apart.

Uncapped, a wave of these launches walks more than one item only in classes of several hundred thousand variables (the
table in DESIGN.md "Later trips of the class launches"); every other oracle-parity graph of the suite gives each wave
exactly one.  With the cap at 1 the tile and group launches have 8 workgroups (one per XCD, whole rounds), the others 1.

CASES: name -> Case.  ``launch`` names the launch under test, ``walk(rec, cap)`` (WALKS) restates its kernel's index
arithmetic: the items -- tiles, hubs, groups, items of 64 positions, by their index in the launch -- every wave takes,
in order.  A builder returns (graph, marks): ``marks`` are variables of the class under test -- all of one colour, which
is asserted -- or None: the class with the most items of the launch."""

from collections import namedtuple

import numpy as np

import util  # noqa: F401  (puts the repository on sys.path)
from numbskull_amd import _lib, graphgen
from numbskull_amd.numbskulltypes import Weight, Variable, Factor, FactorToVar
import hubs
import tiles
from tiles import Target, cyc, gen, shp, GENERAL, GROUP, SHAPE, LANE, HUB, GENERIC

SWITCH = "NSK_CLASS_GRID_CAP"
# learning: (regularization, truncation, learn_non_evidence); step, decay, reg_param; epochs in chunks
SETTINGS = {"l2": (2, 1, True), "l1_trunc2": (1, 2, True), "noreg_evid": (0, 1, False)}
STEP, DECAY, REG_PARAM = 0.02, 0.9, 0.05
CHUNKS = (1, 2)
SEED = 53
WAVES = 4           # per workgroup

Case = namedtuple("Case", "build weights caps env hbv launch kind wide")


# ------------------------------------------------------------------------------------------------------- the graphs
def generic_lanes(nweight, lne=True, npos=41 * 64 + 7):
    """tests/test_hip_parity.py's generic-lane graph -- cardinality 12, every variable under one EQUAL-to-a-value prior,
    one colour -- at 41 items of 64 positions and one of 7.  (NSK_NO_HEAVY: below 32768 such variables each would get a
    wave.)"""
    rng = np.random.default_rng(31)
    variable = np.zeros(npos, Variable)
    variable["cardinality"] = 12
    variable["isEvidence"] = rng.random(npos) < 0.5
    variable["initialValue"] = rng.integers(0, 12, npos)
    factor = np.zeros(npos, Factor)
    factor["factorFunction"] = 4
    factor["weightId"] = np.arange(npos) % nweight
    factor["featureValue"] = 1.0
    factor["arity"] = 1
    factor["ftv_offset"] = np.arange(npos)
    fmap = np.zeros(npos, FactorToVar)
    fmap["vid"] = np.arange(npos)
    fmap["dense_equal_to"] = rng.integers(0, 12, npos)
    weight = np.zeros(nweight, Weight)
    weight["initialValue"] = rng.normal(0, 0.3, nweight)
    return (weight, variable, factor, fmap, np.zeros(npos, np.bool_), npos), np.arange(npos)


def pairs_many_weights(share, lne=True, npairs=25 * 64 + 5):
    """graphgen.ising_pairs with a weight per pair (``share`` = 1) or per two neighbouring pairs (2) under the EQUAL
    factors: no two lanes of a tile share a weight id, so the tiles carry per-lane headers.  Every other pair is free
    (ising_pairs makes all of them evidence: nothing would move in the evidence chain)."""
    g = list(graphgen.ising_pairs(npairs, seed=2))
    fac = g[2].copy()
    eq = np.nonzero(fac["factorFunction"] == 3)[0]
    fac["weightId"][eq] = 3 + np.arange(len(eq)) // share
    g[0] = np.zeros(3 + (len(eq) + share - 1) // share, Weight)
    g[0]["initialValue"] = np.random.default_rng(5).normal(0, 0.3, len(g[0]))
    var = g[1].copy()
    var["isEvidence"] = np.repeat(np.arange(npairs) % 2 == 0, 2) if lne else 1
    g[1], g[2] = var, fac
    return tuple(g), np.arange(0, 2 * npairs, 2)


def many_hubs(nweight, lne=True, n=27):
    """tests/hubs.py's star graph with 27 hubs of 70 .. 130 entries, every factor over the hub alone (boolean functions,
    cardinalities 2 .. 8) and no filler: whatever variable a hub read would share a colour with other hubs and bring
    its general tile -- and the hubs would ride in that tile's launch.  Hub 1 is joined to hub 0 and takes another
    colour; the other 26 share one."""
    cds = ((2, 1), (3, 0), (3, 1), (5, 0), (8, 0), (8, 1))
    spec = [hubs.HubSpec(70 + (i * 37) % 61, cds[i % 6][0], cds[i % 6][1], "boolean", 0, (i % 2 == 0) if lne else True)
            for i in range(n)]
    return hubs.star_graph(spec, filler=None, nweight=nweight, seed=17), np.arange(2, n)


_TILES = {
    # 75 categorical general tiles: per8 = 10 against 4 waves of an XCD -- three trips, two for the last two waves; the
    # last XCD has 5 tiles
    "general_tiles": tiles._case([(74 * 64 + 9, Target(cyc(2, 2)), gen(2, 2))], env=tiles.NOEP),
    "general_tiles_i32": tiles._case([(74 * 64 + 9, Target(cyc(2, 2)), gen(2, 2))], env=tiles.NOEP, wide=True),
    "general_binary": tiles._case([(74 * 64 + 9, Target(cyc(3, 2, card=2, fns=tiles._BCAT), 2, 0), gen(3, 2))], env=tiles.NOEP),
    # ... behind 9 hubs (one hub block: the first tile block sits on XCD 1) and in front of 37 shape tiles (a run of two
    # per wave, the last waves' short or empty)
    "general_hubs_rest": tiles._case([(37 * 64, tiles._sh([4, 2]), shp()), (74 * 64 + 9, Target(cyc(2, 2)), gen(2, 2)),
                                     (9, Target(cyc(40, 2)), tiles.OFF_EP)], env=tiles.NOEP, nweight="per_factor"),
    # 13 shape tiles and nothing else in their class
    "fast_rest": tiles._case([(13 * 64, tiles._sh([4, 2]), shp())], nweight="per_factor"),
}


def tile_case(name):
    def build(nweight, lne=True):
        g, targets = tiles.build_case(name, nweight=nweight, learn=lne, case=_TILES[name], max_vars=60000)
        return g, np.concatenate(targets)
    return build


def lr_groups(nweight, lne=True, nvar=275000):
    """graphgen.mixed_lr_graph: the smallest (in steps of 5 000 variables) whose classes have 129 + 5 groups -- 135 each:
    an XCD's workgroup walks chunk row 0, that of XCD 0 the 7 groups of row 1 as well.  Initial weights drawn, not 0 (a
    weight at 0 that L1 keeps at 0 would not show whether it was visited)."""
    g = list(graphgen.mixed_lr_graph(nvar, seed=7, nweights=nweight))
    g[0] = g[0].copy()
    g[0]["initialValue"] = np.random.default_rng(9).normal(0, 0.2, len(g[0]))
    return tuple(g), None


def boolw_groups(nweight, lne=True, nvar=160000):
    """graphgen.boolean_weighted_graph (arity up to 3: groups, and shape tiles for the rest), free weights, half of the
    variables evidence with drawn values -- as tests/test_hip_parity.py's "boolw" --, the weights halved (at N(0, 0.3) one
    free variable in nine keeps its initial value through both chains of both compared states).  160 000 variables: the
    first class has 82 groups and 36 shape tiles outside segments, 5 to an XCD -- a run of two per wave."""
    g = list(graphgen.boolean_weighted_graph(nvar, seed=4))
    w = g[0].copy()
    w["isFixed"] = False
    w["initialValue"] *= 0.5
    var = g[1].copy()
    rng = np.random.default_rng(8)
    var["isEvidence"] = rng.random(len(var)) < 0.5
    var["initialValue"] = rng.integers(0, 2, len(var))
    g[0], g[1] = w, var
    if nweight != "per_factor":
        g[2] = g[2].copy()
        g[2]["weightId"] = g[2]["weightId"] % nweight
        g[0] = w[:nweight].copy()
    return tuple(g), None


CASES = {
    "generic_range": Case(generic_lanes, (3, 300), (1, 3), ("NSK_NO_HEAVY",), False, "generic", GENERIC, False),
    "dyn_list": Case(pairs_many_weights, (1, 2), (1, 3), ("NSK_NO_SHAPE",), False, "dyn", LANE, False),
    "hubs_alone": Case(many_hubs, (7, "per_factor"), (1, 3), (), True, "heavy", HUB, False),
    "general_tiles": Case(tile_case("general_tiles"), (7, 300, "per_factor"), (1,), tiles.NOEP, True, "general", GENERAL, False),
    "general_tiles_i32": Case(tile_case("general_tiles_i32"), (300,), (1,), tiles.NOEP, True, "general", GENERAL, True),
    "general_binary": Case(tile_case("general_binary"), (7, "per_factor"), (1,), tiles.NOEP, True, "general", GENERAL, False),
    "general_hubs_rest": Case(tile_case("general_hubs_rest"), (300, "per_factor"), (1,), tiles.NOEP, True, "general", GENERAL, False),
    "fast_rest": Case(tile_case("fast_rest"), (300, "per_factor"), (1, 3), (), True, "fast", SHAPE, False),
    "ep_two_rows": Case(lr_groups, (7, 2000), (1,), (), True, "ep", GROUP, False),
    "ep_rest": Case(boolw_groups, (300, "per_factor"), (1,), (), True, "ep_rest", SHAPE, False),
}
# what else a case's class under test must hold: launch -> walks checked beside the main one
ALSO = {"general_hubs_rest": ("general_hubs", "general_rest"), "ep_rest": ("ep",)}
PARAMS = [(n, w) for n, cs in CASES.items() for w in cs.weights]


def ids(params):
    return ["%s-w%s" % (n, w) for n, w in params]


def set_switches(monkeypatch, name, cap):
    """The case's switches; ``cap`` None: NSK_CLASS_GRID_CAP unset."""
    monkeypatch.setenv("NSK_DIAG", "1")
    for k in CASES[name].env:
        monkeypatch.setenv(k, "1")
    if cap is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, str(cap))


# ------------------------------------------------------------------------------------------ the kernels' arithmetic
def _strided(n, nwaves):
    """k_learn_phase, k_learn_heavy, the hub blocks: wave w takes w, w + nwaves, ..."""
    return [np.arange(w, n, nwaves) for w in range(nwaves)]


def _runs(n, nwaves, base=0):
    """k_learn_fast, the rest walk of k_learn_general: a contiguous run of per = ceil(n / nwaves) per wave"""
    per = -(-n // nwaves)
    return [base + np.arange(min(n, w * per), min(n, (w + 1) * per)) for w in range(nwaves)]


def _xcd_blocks(hblocks, end):
    """(block, xcd, first block of the kind on that XCD, blocks of the kind on that XCD) for the blocks [hblocks, end)"""
    for b in range(hblocks, end):
        xcd = b & 7
        first = hblocks + ((xcd - (hblocks & 7) + 8) & 7)
        nbx = (end - 1 - first) // 8 + 1 if first < end else 0
        yield b, xcd, first, nbx


def walk_generic(r, cap):
    return _strided(int(r["generic_n"]), WAVES * int(r["generic_grid"]))


def walk_dyn(r, cap):
    return _strided(int(r["dyn_n"]), WAVES * int(r["dyn_grid"]))


def walk_heavy(r, cap):
    return _strided(int(r["heavy_n"]), WAVES * int(r["heavy_grid"]))


def walk_fast(r, cap):
    return _runs(int(r["fast_n"]), WAVES * int(r["fast_grid"]))


def walk_general(r, cap):
    """k_learn_general: XCD x walks the x-th eighth of the tiles, its waves strided"""
    n, hb, grid = int(r["gen_ntiles"]), int(r["gen_hblocks"]), int(r["gen_grid"])
    assert not r["gen_ep"] and r["gen_rblocks"] == 0
    per8 = (n + 7) >> 3
    out = []
    for b, xcd, first, nbx in _xcd_blocks(hb, grid):
        for w in range(WAVES):
            wx = ((b - first) >> 3) * WAVES + w
            out.append(np.arange(xcd * per8 + wx, min(n, (xcd + 1) * per8), nbx * WAVES))
    return out


def walk_general_hubs(r, cap):
    hubs_ = int(r["gen_hblocks"]) - (int(r["nbh"]) if r["gen_ep"] else 0)
    return _strided(int(r["nhub"]), WAVES * hubs_)


def walk_general_rest(r, cap):
    return _runs(int(r["gen_nrest"]), WAVES * (int(r["gen_grid"]) - int(r["gen_hblocks"])))


def walk_ep(r, cap):
    """ep_walk / ep_group, per workgroup: chunks of 16 consecutive groups dealt to the XCDs in turn"""
    n, hb, gb = int(r["ngroups"]), int(r["gen_hblocks"]), int(r["gen_gblocks"])
    assert r["gen_ep"]
    lend = -(-n // 128) * 16
    out = []
    for b, xcd, first, nbx in _xcd_blocks(hb, hb + gb):
        li = np.arange((b - first) >> 3, lend, nbx)
        gi = ((li // 16) * 8 + xcd) * 16 + li % 16
        out.append(gi[gi < n])
    return out


def walk_ep_rest(r, cap):
    """the rest walk of learn_ep_body: an eighth per XCD, a run per wave of the group and rest blocks"""
    n, hb, grid = int(r["gen_nrest"]), int(r["gen_hblocks"]), int(r["gen_grid"])
    assert r["gen_ep"] and grid - hb >= 8
    per8 = (n + 7) >> 3
    out = []
    for b, xcd, first, nbx in _xcd_blocks(hb, grid):
        t0 = min(n, xcd * per8)
        tend = min(n, t0 + per8)
        per = -(-(tend - t0) // (nbx * WAVES))
        for w in range(WAVES):
            r0 = min(tend, t0 + (((b - first) >> 3) * WAVES + w) * per)
            out.append(np.arange(r0, min(tend, r0 + per)))
    return out


# launch -> (walk, record field with its items, contiguous runs)
WALKS = {"generic": (walk_generic, "generic_n", False), "dyn": (walk_dyn, "dyn_n", False), "heavy": (walk_heavy, "heavy_n", False),
         "fast": (walk_fast, "fast_n", True), "general": (walk_general, "gen_ntiles", False),
         "general_hubs": (walk_general_hubs, "nhub", False), "general_rest": (walk_general_rest, "gen_nrest", True),
         "ep": (walk_ep, "ngroups", False), "ep_rest": (walk_ep_rest, "gen_nrest", True)}
ON = {"generic": "generic_on", "dyn": "dyn_on", "heavy": "heavy_on", "fast": "fast_on", "general": "gen_on",
      "general_hubs": "gen_on", "general_rest": "gen_on", "ep": "gen_ep", "ep_rest": "gen_ep"}


def class_under_test(recs, launch, color=None, marks=None):
    """(class index, its record by name): the colour of the marks, or the class with the most items of the launch"""
    f = _lib.class_fields(recs)
    n = np.where(f[ON[launch]] != 0, f[WALKS[launch][1]], 0)
    if marks is None:
        k = int(np.argmax(n))
    else:
        ks = set(np.asarray(color)[marks].tolist())
        assert len(ks) == 1, ("the marked variables are spread over colours", ks)
        k = ks.pop()
    assert n[k] > 0, (launch, "the class has no such launch", k)
    return k, {name: int(v[k]) for name, v in f.items()}


def positions(r, launch):
    """[first, last) positions of the items the launch samples in its class, where they are a range"""
    if launch in ("generic",):
        return r["he"], r["e"]
    if launch in ("heavy", "general_hubs"):
        return r["fe"], r["he"]
    if launch in ("general", "ep"):
        return r["fb"] + 64 * r["gen_tile0"], r["fb"] + 64 * (r["gen_tile0"] + r["gen_ntiles"])
    return r["fb"], r["fe"]             # lists of tiles: somewhere among the class's tiles


def check_class(name, cap, color, routes, recs, marks):
    """The class under test of a plan (or of a handle: its colours and route words) routes where the case says and
    gets the launch the case names; returns (class, record)."""
    cs = CASES[name]
    kind = _lib.route_fields(np.asarray(routes, np.int64))["kind"]
    k, r = class_under_test(recs, cs.launch, color, marks)
    # the route: as many variables of the case's kind as the launch has room for (shape tiles need not be full)
    n = int(((np.asarray(color) == k) & (kind == cs.kind)).sum())
    per_item = {"heavy": 1, "ep": 256}.get(cs.launch, 64)
    items = r[WALKS[cs.launch][1]]
    if cs.launch in ("fast", "ep_rest"):
        assert 0 < n <= 64 * items, (name, n, items)
    else:
        assert per_item * (items - 1) < n <= per_item * items, (name, n, items)
    if cs.launch == "generic":
        assert r["generic_grid"] == min(cap, -(-items // 4)) and r["ngeneric"] == n
    if cs.launch == "dyn":
        assert r["dyn_grid"] == min(cap, -(-items // 4))
    if cs.launch == "heavy":
        assert not r["gen_on"] and r["heavy_grid"] == min(cap, -(-r["nhub"] // 4))
    if cs.launch == "general":
        assert not r["gen_ep"] and r["gen_maxc"] == (2 if name == "general_binary" else 8) and r["gen_gblocks"] == 8
        assert r["gen_grid"] == r["gen_hblocks"] + 8
    if cs.launch in ("ep", "ep_rest"):
        assert r["gen_ep"] and r["gen_gblocks"] == 8 and r["gen_rblocks"] == 0
    if cs.launch == "fast":
        assert not r["gen_on"] and r["ntiles"] == r["nlrest"] and r["fast_grid"] == min(cap, -(-items // 4))
    if name == "general_hubs_rest":
        assert r["gen_hblocks"] & 7 != 0 and r["nhub"] >= 9 and r["gen_nrest"] > 32
    if name == "ep_two_rows":
        assert r["ngroups"] >= 129 + 5
    return k, r
