"""Graphs built for a routing edge of the tile families -- general tiles walked per lane, entry-parallel groups, shape
tiles -- as tests/hubs.py builds them for the hubs (tests/test_tiles_cpu.py plans every case and checks the route of
every target and its liveliness in the oracle, tests/test_tiles_gpu.py runs them against the oracle).

``tile_graph(families, ...)`` returns ((weight, variable, factor, fmap, domain_mask, edges), targets): TARGET variables
whose factor lists are given exactly, entry by entry, and LEAF variables -- the other members of those factors, each
private to its factor.  Two targets never share a factor, so nothing keeps the colouring from giving a whole case's
targets one colour; whether it did is read back (check_case), never assumed.  A FAMILY is ``size`` targets of one
spec -- 1, 63, 64, 65, 256, 257: a tile filled, one short, spilling into the next tile or group.

A target's spec: Target(entries, card, dtype, evidence); an entry: ent(fn, others, own, form, ldeo, lcard) --
- ``fn`` the factor function, ``others`` the number of leaves;
- ``own`` the target's own dense_equal_to (None: entry index modulo the cardinality; a tuple with the forms that name
  the target more than once);
- ``form``: "a" the target is the first member, "z" the last (the head of the positional functions 13 / 16 / 17),
  "az" first and last (role 3), "aa" first and second (own edges that disagree: codes 10 / 11), "aaa" the first
  three; None: "a" for even entries, "z" for odd ones;
- ``ldeo`` / ``lcard``: dense_equal_to and cardinality of the leaves (None: cardinality 2 .. 4 drawn per entry of the
  spec, a valid dense_equal_to under the *_CAT functions, 0 otherwise).
The ENTRIES the compiler counts (nsk_compile_words.cpp) are one per factor of a dataType-0 target and one per factor
and named own value of a dataType-1 target.

Weights: ``nweight`` = 30 (the default), 7 or 300 shared weights handed out in turn, or "per_factor"; initial values
normal(0, 0.3), every fifth fixed -- as test_hip_parity._general_tile_graph.  Leaves: 40 % evidence.

CASES: name -> Case; a family = (size, Target, expect), ``expect`` the fields of the route word
(numbskull_amd._lib.route_fields) every target of the family must show (None: not the same for all of them)."""

from collections import namedtuple

import numpy as np

import util  # noqa: F401  (puts the repository on sys.path)
from numbskull_amd import _lib
from numbskull_amd.numbskulltypes import Weight, Variable, Factor, FactorToVar

TABLE, UNIFORM, SHAPE, LANE, GENERAL, GROUP, HUB, GENERIC = (_lib.ROUTE_TABLE, _lib.ROUTE_UNIFORM, _lib.ROUTE_SHAPE,
                                                             _lib.ROUTE_LANE, _lib.ROUTE_GENERAL, _lib.ROUTE_GROUP,
                                                             _lib.ROUTE_HUB, _lib.ROUTE_GENERIC)
CAT = (12, 14, 15, 16, 17)
VALUED = (12, 14, 3, 16, 15, 17)               # defined over values: what a categorical target's entries cycle through
BINARY = (1, 13, 12, 0, 14, 3, 17, 2, 16, 15)  # ... and a binary target's
SIZES = (1, 63, 64, 65, 256, 257)

Target = namedtuple("Target", "entries card dtype evidence")
Target.__new__.__defaults__ = (3, 0, False)
Ent = namedtuple("Ent", "fn others own form ldeo lcard")


def ent(fn, others, own=None, form=None, ldeo=None, lcard=None):
    return Ent(fn, others, own, form, ldeo, lcard)


def cyc(n, others, card=3, fns=None, **kw):
    """n entries of ``others`` leaves each (an int, or one per entry), the functions in turn."""
    fns = fns or (VALUED if card > 2 else BINARY)
    oth = [others] * n if isinstance(others, int) else list(others)
    return tuple(ent(fns[i % len(fns)], oth[i], **kw) for i in range(n))


def tile_graph(families, nweight=30, wide=False, pad_front=0, seed=0, max_vars=4200):
    """families: [(size, Target)].  ``pad_front``: isolated binary evidence variables in front of everything (the
    literal head lookup reads var_value[edge index]: the case that uses it keeps every edge index among them).
    ``max_vars``: what the graph may not outgrow -- the cases of this module stay small; tests/class_trips.py builds
    whole colour classes of tiles with the same builder."""
    rng = np.random.default_rng(seed)
    cards, dtypes, evid = [2] * pad_front, [0] * pad_front, [1] * pad_front
    fn_, members_, deos_ = [], [], []
    targets = []
    for size, spec in families:
        # what the family shares: the leaves' cardinalities and dense_equal_to per entry
        shared = []
        for e in spec.entries:
            lc = [int(e.lcard) if e.lcard is not None else int(rng.integers(2, 5)) for _ in range(e.others)]
            ld = [int(e.ldeo) if e.ldeo is not None else (int(rng.integers(0, c)) if e.fn in CAT else 0) for c in lc]
            shared.append((lc, ld))
        fam = []
        for _ in range(size):
            t = len(cards)
            fam.append(t)
            cards.append(spec.card); dtypes.append(spec.dtype); evid.append(int(spec.evidence))
            for i, e in enumerate(spec.entries):
                lc, ld = shared[i]
                leaves = list(range(len(cards), len(cards) + e.others))
                cards.extend(lc); dtypes.extend([0] * e.others); evid.extend(int(x) for x in rng.random(e.others) < 0.4)
                form = e.form or ("a" if i % 2 == 0 else "z")
                own = e.own if e.own is not None else i % spec.card
                own = (own,) * 3 if isinstance(own, int) else tuple(own)
                if form == "a": m, d = [t] + leaves, [own[0]] + ld
                elif form == "z": m, d = leaves + [t], ld + [own[0]]
                elif form == "az": m, d = [t] + leaves + [t], [own[0]] + ld + [own[1]]
                elif form == "aa": m, d = [t, t] + leaves, [own[0], own[1]] + ld
                else:
                    assert form == "aaa", form
                    m, d = [t, t, t] + leaves, list(own[:3]) + ld
                fn_.append(e.fn); members_.append(m); deos_.append(d)
        targets.append(np.asarray(fam, np.int64))
    if wide:
        cards.append(200); dtypes.append(0); evid.append(0)          # values no longer fit int8: the int32 kernels
    nvar, nfactor = len(cards), len(fn_)
    variable = np.zeros(nvar, Variable)
    variable["cardinality"] = cards
    variable["dataType"] = dtypes
    variable["isEvidence"] = evid
    variable["initialValue"] = (rng.random(nvar) * np.asarray(cards)).astype(np.int64)
    arity = np.array([len(m) for m in members_], np.int64)
    nedge = int(arity.sum())
    factor = np.zeros(nfactor, Factor)
    factor["factorFunction"] = fn_
    factor["featureValue"] = 1.0
    factor["arity"] = arity
    factor["ftv_offset"] = np.cumsum(arity) - arity
    fmap = np.zeros(nedge, FactorToVar)
    fmap["vid"] = np.concatenate([np.asarray(m, np.int64) for m in members_])
    fmap["dense_equal_to"] = np.concatenate([np.asarray(d, np.int64) for d in deos_])
    if nweight == "per_factor":
        nw = nfactor
        factor["weightId"] = np.arange(nfactor)
    else:
        nw = int(nweight)
        factor["weightId"] = (rng.permutation(nfactor) + int(rng.integers(0, nw))) % nw      # in turn: every weight is used
    weight = np.zeros(nw, Weight)
    weight["initialValue"] = rng.normal(0, 0.3, nw)
    weight["isFixed"][::5] = True
    assert nvar <= max_vars, nvar
    assert pad_front == 0 or nedge <= pad_front, (nedge, pad_front)
    return (weight, variable, factor, fmap, np.zeros(nvar, np.bool_), nedge), targets


def entries_of(g, v):
    """Entries of variable v as the compiler counts them."""
    _, variable, factor, fmap = g[:4]
    keyed = int(variable[v]["dataType"]) != 0
    own = np.nonzero(fmap["vid"] == v)[0]
    fid = np.searchsorted(factor["ftv_offset"], own, side="right") - 1
    return len(set(zip(fid.tolist(), fmap["dense_equal_to"][own].tolist() if keyed else [0] * len(own))))


# ---------------------------------------------------------------------------------------------------------- the cases
Case = namedtuple("Case", "families env hbv wide nweight colours learn pad_front")


def _case(families, env=(), hbv=True, wide=False, nweight=30, colours=1, learn=False, pad_front=0):
    """``colours``: 1 -- every target of the case shares one colour (asserted); None -- not asserted."""
    return Case(tuple(families), tuple(env), hbv, wide, nweight, colours, learn, pad_front)


def _eg(M):
    """Entries per super-group of the per-lane walk (nsk_compile_tiles.cpp): a lane's words are eaten in 16-byte chunks."""
    return 1 if (2 + M) % 4 == 0 else 2 if (2 + M) % 2 == 0 else 4


AUTO = "auto"


def gen(E, M, tE=AUTO, tM=AUTO):
    """Route of a target on a general tile walked per lane: own entries / width, then the tile's width (default: the
    target's) and entries (default: the target's, padded to the super-group of the tile's width); None: not asserted."""
    tM = M if tM == AUTO else tM
    if tE == AUTO:
        tE = None if tM is None else (E + _eg(tM) - 1) // _eg(tM) * _eg(tM)
    return dict(kind=GENERAL, own_entries=E, own_width=M, tile_entries=tE, tile_width=tM)


def grp(E, M, emax=None):
    emax = E if emax is None else emax
    return dict(kind=GROUP, own_entries=E, own_width=M, tile_entries=emax, two_pass=int(emax > 8))


def shp(null=0):
    return dict(kind=SHAPE, null_word=null)


OFF = dict(kind=HUB, hub_ep=0)          # not of the general-tile form: the generic wave walk
OFF_EP = dict(kind=HUB, hub_ep=1, hub_block=0)     # of the form but too long for a lane: a wave, one lane per entry
NOEP = ("NSK_NO_EP",)

CASES = {}
# ---- general tiles, per-lane walk.  Categorical (cardinality 3) targets unless the case says otherwise.
for _M in (0, 1, 2, 3):
    for _E in sorted({1, 16, 3 if _M in (1, 3) else 1}):
        _fns = (4, 3) if _M == 0 else None                 # M = 0: ISTRUE / EQUAL over the target alone
        CASES["gen_m%d_e%d" % (_M, _E)] = _case(
            [(65, Target(cyc(_E, _M, fns=_fns), 3, int(_E == 3), _E == 3), gen(_E, _M))], env=NOEP,
            learn=(_M == 3 and _E == 16))
for _M in (4, 5, 6):
    CASES["gen_m%d" % _M] = _case([(65, Target(cyc(4, _M)), gen(4, _M))], learn=_M == 4)
CASES["gen_m7_off"] = _case([(65, Target(cyc(2, (7, 1))), OFF)])
# the blocker: one binary variable with an entry of 4 others (it sorts behind the categorical lanes, into a tile of
# its own) keeps the colour off the groups without any switch
CASES["gen_m3_blocker"] = _case([(64, Target(cyc(16, 3)), gen(16, 3)),
                                 (1, Target(cyc(1, 4, card=2), 2, 1), gen(1, 4))], learn=True)
# padding entries and NSK_GEN_NULL member words: tile 0 = 64 lanes of 3 entries x 6 others, tile 1 = the 65th of them
# beside 63 lanes of 1 entry x 1 other.  The first family is evidence with non-zero values and sorts first: internal
# id 0 -- what an empty slot's gather reads -- holds a categorical 1 or 2 (check_case with a layout)
CASES["gen_pad_null"] = _case([(65, Target(cyc(3, 6), 3, 0, True), gen(3, 6)),
                               (63, Target(cyc(1, 1), 3, 0, False), gen(1, 1, 3, 6))], learn=True,
                              env=("NSK_NO_RECOLOUR", "NSK_NO_BALANCE"))       # greedy colours: the targets' colour is colour 0
CASES["gen_e17_off"] = _case([(65, Target(cyc(17, 1)), OFF_EP)], env=NOEP)
# (40 lanes, not 65: 89 variables a target, and no graph here is to have more than about 4 000)
CASES["gen_w120"] = _case([(40, Target(cyc(16, [6] * 14 + [2] * 2)), gen(16, 6))])
CASES["gen_w121_off"] = _case([(40, Target(cyc(16, [6] * 14 + [3, 2])), OFF_EP)])
for _d in (0, 1):
    CASES["gen_card8_dt%d" % _d] = _case([(65, Target(cyc(8, 2, card=8), 8, _d), gen(8, 2))], env=NOEP, learn=_d == 1)
    CASES["gen_card9_dt%d_off" % _d] = _case([(65, Target(cyc(8, 2, card=9), 9, _d), OFF)], env=NOEP)
CASES["gen_card2_dt1"] = _case([(65, Target(cyc(4, 2, card=2), 2, 1), gen(4, 2))], env=NOEP)
CASES["gen_deo31"] = _case([(65, Target((ent(12, 1, ldeo=31, lcard=33), ent(14, 2))), gen(2, 2))], env=NOEP)
CASES["gen_deo32_off"] = _case([(65, Target((ent(12, 1, ldeo=32, lcard=33), ent(14, 2))), OFF)], env=NOEP)
# the entries that name the target twice
_SELF0 = (ent(13, 1, form="az"), ent(17, 1, own=(1, 1), form="az"), ent(17, 2, own=(1, 2), form="az"),     # role 3
          ent(12, 1, own=(0, 2), form="aa"), ent(16, 1, own=(0, 1), form="aa"),                            # code 10
          ent(17, 1, own=(2, 1), form="aa"), ent(3, 1))                                                    # code 11
CASES["gen_self_dt0"] = _case([(65, Target(_SELF0, 3, 0), gen(7, 2))], env=NOEP, learn=True)
_SELFB = (ent(13, 2, form="az"), ent(14, 1, own=(0, 1), form="aa"), ent(17, 1, own=(0, 1), form="aa"),     # binary: code 11
          ent(12, 1, own=(1, 0), form="aa"), ent(1, 1))
CASES["gen_self_binary"] = _case([(65, Target(_SELFB, 2, 1), gen(8, 2))], env=NOEP)    # dataType 1: two lists each
# dataType 1, cardinality 8: AND_CAT over own values 6 and 7 -- the entry in list 7 names list 6 as its partner
_SELF8 = (ent(12, 1, own=(6, 7), form="aa"), ent(17, 1, own=(7, 7), form="az"), ent(14, 2, own=7), ent(15, 1, own=6))
CASES["gen_self_partner7"] = _case([(65, Target(_SELF8, 8, 1), gen(5, 2))], env=NOEP, learn=True)
CASES["gen_or_two_of_three_off"] = _case([(65, Target((ent(14, 1, own=(0, 1), form="aa"), ent(3, 1))), OFF)], env=NOEP)
CASES["gen_three_own_off"] = _case([(65, Target((ent(12, 1, own=(0, 1, 2), form="aaa"), ent(3, 1))), OFF)], env=NOEP)
CASES["gen_literal_heads"] = _case([(65, Target((ent(17, 1, form="a"), ent(16, 1, form="z"), ent(13, 2, form="a")), 3, 0), gen(3, 2))],
                                   env=NOEP, hbv=False, pad_front=700, colours=None)
for _n in (1, 256, 257):                       # 1, 4 and 5 general tiles in the colour: a workgroup takes four
    CASES["gen_tiles_%d" % _n] = _case([(_n, Target(cyc(2, 2)), gen(2, 2))], env=NOEP, learn=_n == 257)
_BCAT = (12, 14, 17)
CASES["gen_binary_only"] = _case([(65, Target(cyc(3, 2, card=2, fns=_BCAT), 2, 0), gen(3, 2))], env=NOEP)
CASES["gen_cat_and_binary"] = _case([(65, Target(cyc(3, 2)), gen(3, 2)),
                                     (65, Target(cyc(2, 1, card=2, fns=_BCAT), 2, 0), gen(2, 1, None, None))], env=NOEP)
CASES["gen_i32"] = _case([(65, Target(cyc(3, 3)), gen(3, 3))], env=NOEP, wide=True)
# ---- entry-parallel groups
CASES["ep_m3_e16"] = _case([(65, Target(cyc(16, 3)), grp(16, 3))], learn=True)
CASES["ep_off_m4"] = _case([(65, Target(cyc(16, 3)), gen(16, 3, 16, None)), (1, Target(cyc(1, 4)), gen(1, 4, 16, 4))])
# (17 entries: the variable is no general-tile variable at all -- gen_max_entries -- so the colour keeps its groups
# and the variable takes a wave of its own)
CASES["ep_beside_e17"] = _case([(65, Target(cyc(16, 3)), grp(16, 3)), (1, Target(cyc(17, 1)), OFF_EP)])
for _E in (8, 9):
    CASES["ep_e%d" % _E] = _case([(65, Target(cyc(_E, [0, 1, 2, 3] * 3)), grp(_E, 3))], learn=True)
CASES["ep_e16_dt1_card8"] = _case([(65, Target(cyc(16, [1, 2] * 8, card=8), 8, 1), grp(16, 2))], learn=True)
CASES["ep_row64"] = _case([(64, Target(cyc(1, 2)), grp(1, 2))], learn=True)
CASES["ep_row65"] = _case([(65, Target(cyc(1, 2)), grp(1, 2))], learn=True)
CASES["ep_m0_only"] = _case([(65, Target((ent(4, 0), ent(-1, 0), ent(3, 0)), 3, 0), grp(3, 0))])
for _n in (1, 63, 256, 257):
    CASES["ep_tiles_%d" % _n] = _case([(_n, Target(cyc(3, [3, 0, 2])), grp(3, 3))], learn=_n == 257)
CASES["ep_binary_only"] = _case([(65, Target(cyc(3, 2, card=2, fns=_BCAT), 2, 0), grp(3, 2))])
CASES["ep_i32"] = _case([(65, Target(cyc(9, 2)), grp(9, 2))], wide=True)
# ---- shape tiles: binary dataType-0 targets under the boolean functions over binary leaves, one weight per factor
_B = (1, 2, 3, 0, 4)


def _sh(others, fns=_B, form=None):
    return Target(tuple(ent(fns[i % len(fns)] if o else 4, o, form=form, lcard=2) for i, o in enumerate(others)), 2, 0, False)


CASES["shape_w16"] = _case([(64, _sh([4, 4, 4, 0]), shp()), (64, _sh([4, 4, 4, 0], (3, 0, 1)), shp())], nweight="per_factor", learn=True)
CASES["shape_w17_off"] = _case([(64, _sh([4, 4, 4, 1]), gen(4, 4))], nweight="per_factor")
CASES["shape_ep_w4"] = _case([(64, _sh([3]), shp())], nweight="per_factor")
CASES["shape_ep_w5_off"] = _case([(64, _sh([3, 0]), grp(2, 3))], nweight="per_factor")
CASES["shape_exact64"] = _case([(64, _sh([4, 2]), shp())], nweight="per_factor")
# 63 of a shape fill no tile: alone they take the general tiles; with one lane of a near shape (1 other where they have
# 2) the PADDED shape has 64 members
CASES["shape_exact63_general"] = _case([(63, _sh([4, 2]), gen(2, 4))], nweight="per_factor")
CASES["shape_exact63_padded"] = _case([(63, _sh([4, 2]), shp(0)), (1, _sh([4, 1]), shp(1))], nweight="per_factor")
# lanes of 1, 3 and 4 others beside lanes of 2, 4 and 4: one padded shape, null words in the first half of each of
# its two tiles (positions inside a class go by id)
for _f, _n in ((1, "or"), (2, "and"), (3, "equal"), (0, "imply")):
    _fam = [(32, _sh([1, 3, 4], (_f,), "a"), shp(1)), (32, _sh([2, 4, 4], (_f,), "z"), shp(0)),
            (32, _sh([1, 4, 4], (_f,), "z"), shp(1)), (32, _sh([2, 3, 4], (_f,), "a"), shp(1))]     # (four exact shapes, none of 64)
    CASES["shape_pad_%s" % _n] = _case(_fam, nweight="per_factor", learn=_n in ("or", "imply"))
    CASES["shape_pad_%s_nopad" % _n] = _case([(s, t, gen(3, 4)) for s, t, _ in _fam], env=("NSK_NO_PAD_SHAPE",), nweight="per_factor")
CASES["shape_w16_noshape"] = _case([(64, _sh([4, 4, 4, 0]), dict(kind=LANE))], env=("NSK_NO_SHAPE",), nweight="per_factor")
CASES["shape_pad_or_noshape"] = _case([(s, t, gen(3, 4)) for s, t, _ in CASES["shape_pad_or"].families], env=("NSK_NO_SHAPE",),
                                      nweight="per_factor")
# the sliver rule: 64 classed variables beside 1280 / 1344 general ones (greedy colours: the later passes deal the
# general ones, which have no neighbours, out over the colours or renumber the classes)
_GREEDY = NOEP + ("NSK_NO_BALANCE", "NSK_NO_RECOLOUR")
CASES["sliver_keeps"] = _case([(64, _sh([4, 2]), shp()), (1280, Target(cyc(1, 0, fns=(4,))), gen(1, 0))], env=_GREEDY, nweight="per_factor")
CASES["sliver_gives_up"] = _case([(64, _sh([4, 2]), gen(2, 4)), (1344, Target(cyc(1, 0, fns=(4,))), gen(1, 0))], env=_GREEDY,
                                 nweight="per_factor")
# ---- hubs, rest tiles and tiles / groups in one launch
CASES["gen_rest_hub"] = _case([(64, _sh([4, 2]), shp()), (65, Target(cyc(3, 4)), gen(3, 4)), (1, Target(cyc(40, 2)), OFF_EP)],
                              nweight="per_factor")
CASES["ep_rest_hubs"] = _case([(64, _sh([3]), shp()), (65, Target(cyc(3, 3)), grp(3, 3)), (1, Target(cyc(40, 2)), OFF_EP),
                               (1, Target(cyc(130, 2)), dict(kind=HUB, hub_ep=1, hub_block=1))], nweight="per_factor", learn=True)
# ---- one graph, every route.  Colour 0 (the targets): a padded shape tile, general tiles on both walks (the entries of
# 4 others keep the colour off the groups), a hub.  The leaves of those entries have cardinality 9 -- generic-path
# variables, a wave each -- so that the colours of the OTHER leaves hold general variables of at most 3 others only:
# entry-parallel groups, beside the padded shape tile the shape families' own leaves make there.
CASES["mixed_routes"] = _case([(32, _sh([1]), shp(1)), (32, _sh([2]), shp(0)),
                               (65, Target(cyc(9, [3, 2, 1] * 3)), gen(9, 3, None, None)),
                               (65, Target(cyc(3, 4, lcard=9)), gen(3, 4, None, 4)),
                               (1, Target(cyc(40, 2)), OFF_EP)], nweight="per_factor", learn=True)
MIXED_KINDS = {SHAPE, GENERAL, GROUP, HUB}

LEARN_CASES = sorted(k for k in CASES if CASES[k].learn)
# learning configurations: (regularization, truncation, learn_non_evidence, nweight, extra switch)
LEARN_CFG = {
    "A": (0, 1, False, 7, None), "B": (1, 3, True, 300, None), "C": (2, 1, True, "per_factor", None),
    "D": (1, 1, False, 300, "NSK_NO_KSTAT"), "E": (2, 1, True, 300, "NSK_ONE_ACC"), "F": (1, 1, True, 7, None),
}
SALT = 0


def ntargets(name):
    return sum(s for s, _, _ in CASES[name].families)


def nfactors(name):
    return sum(s * len(t.entries) for s, t, _ in CASES[name].families)


def learn_cfgs(name):
    """The learning configurations of a case: three of the six, in turn.  A case of fewer than 600 factors gets none
    with 300 weights (most of them would have no factor to move them)."""
    if name in ("ep_rest_hubs", "mixed_routes"):
        return "CDE"       # (their shape lanes have one entry: 7 shared weights would make exact classes, uniform tiles, of them)
    if nfactors(name) < 600:
        return "ACF"
    return "ABCDEF"


def build_case(name, nweight=None, learn=None, case=None, max_vars=4200):
    """((weight, ...), targets per family).  ``nweight``: overrides the case's weights (shared weights drawn in turn
    make no exact class of 64 either, so a shape case keeps its shape tiles: check_case says so each time).  ``learn``: None, or the learn_non_evidence flag of a learning test -- every other
    target of a family becomes evidence (both halves of the structural visit counts; without learn_non_evidence only
    the evidence half is visited).  A shape class is keyed by the evidence flag, so a case with shape tiles makes every
    target evidence without learn_non_evidence and none with it.  ``case``: a Case of the caller's own, seeded by
    ``name`` (tests/class_trips.py)."""
    cs = CASES[name] if case is None else case
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + SALT
    nw = cs.nweight if nweight is None else nweight
    g, targets = tile_graph([(s, t) for s, t, _ in cs.families], nweight=nw, wide=cs.wide, pad_front=cs.pad_front, seed=seed,
                            max_vars=max_vars)
    if learn is not None:
        shapes = any(e.get("kind") == SHAPE for _, _, e in cs.families)
        for fam in targets:
            g[1]["isEvidence"][fam] = int(not learn) if shapes else (np.arange(len(fam)) % 2 == 0)
    if name == "gen_pad_null":                                 # evidence, and never 0
        g[1]["isEvidence"][targets[0]] = 1
        g[1]["initialValue"][targets[0]] = 1 + (targets[0] % 2)
    return g, targets


LEARN_PARAMS = [(n, c) for n in LEARN_CASES for c in learn_cfgs(n)]


def set_switches(monkeypatch, name, extra=None):
    for k in CASES[name].env + ((extra,) if extra else ()):
        monkeypatch.setenv("NSK_DIAG", "1")
        monkeypatch.setenv(k, "1")


def check_case(name, g, targets, color, routes, info, layout=None):
    """The plan (or the handle) took every target of the case where the case was built to go."""
    cs = CASES[name]
    f = _lib.route_fields(np.asarray(routes, np.int64))
    for (size, spec, expect), fam in zip(cs.families, targets):
        assert len(fam) == size
        for k, want in expect.items():
            if want is None:
                continue
            got = f[k][fam]
            assert (got == want).all(), (name, k, want, np.unique(got, return_counts=True))
    if cs.colours == 1:
        allt = np.concatenate(targets)
        assert len(set(np.asarray(color)[allt].tolist())) == 1, (name, "the targets are spread over colours")
    assert info["value_bytes"] == (4 if cs.wide else 1)
    check_counters(color, routes, info)
    if name == "gen_pad_null":           # colour 0 holds the targets and nothing else: its first position is one of theirs
        assert set(np.nonzero(np.asarray(color) == 0)[0].tolist()) == set(np.concatenate(targets).tolist())
    if name == "gen_pad_null" and layout is not None:
        at0 = np.nonzero(np.asarray(layout) == 0)[0]
        assert len(at0) == 1 and at0[0] in targets[0], at0
        v = g[1][int(at0[0])]
        assert v["cardinality"] == 3 and v["isEvidence"] == 1 and v["initialValue"] != 0, v


def check_counters(color, routes, info):
    """What the counters must be given the routes: general tiles and groups are cut from one sorted run per colour."""
    color = np.asarray(color)
    f = _lib.route_fields(np.asarray(routes, np.int64))
    want = dict(tiles_general=0, tiles_general_roles=0, ep_groups=0, ep_groups_two_pass=0)
    nshape = nshape_null = nlane = 0
    for k in range(int(color.max()) + 1):
        here = color == k
        ng = int((here & (f["kind"] == GENERAL)).sum())
        ne = int((here & (f["kind"] == GROUP)).sum())
        assert ng == 0 or ne == 0, "a colour is laid out as groups or as general tiles, not both"
        want["tiles_general"] += -(-ng // 64)
        want["tiles_general_roles"] += -(-int((here & (f["kind"] == GENERAL) & (f["tile_width"] >= 4)).sum()) // 64)
        want["ep_groups"] += -(-ne // 256)
        want["ep_groups_two_pass"] += -(-int((here & (f["kind"] == GROUP) & (f["two_pass"] == 1)).sum()) // 256)
        nshape += -(-int((here & (f["kind"] == SHAPE)).sum()) // 64)
        nshape_null += int((here & (f["kind"] == SHAPE) & (f["null_word"] == 1)).any())
        nlane += int((here & (f["kind"] == LANE)).any())
    assert {k: info[k] for k in want} == want, ({k: info[k] for k in want}, want)
    # (shape classes start tiles of their own: lower bounds)
    assert info["tiles_shape"] >= nshape and info["tiles_shape_padded"] >= nshape_null and info["tiles_lane"] >= nlane
    assert info["tiles_shape_padded"] <= info["tiles_shape"] and info["tiles_general_roles"] <= info["tiles_general"]
    assert (info["tiles_shape"] > 0) == bool((f["kind"] == SHAPE).any()) and (info["tiles_lane"] > 0) == bool((f["kind"] == LANE).any())
    assert (info["tiles_shape_padded"] > 0) == bool(((f["kind"] == SHAPE) & (f["null_word"] == 1)).any())
    # a general lane lies inside its tile, a group's variable inside its group
    gl = f["kind"] == GENERAL
    assert (f["own_entries"][gl] <= f["tile_entries"][gl]).all() and (f["own_width"][gl] <= f["tile_width"][gl]).all()
    gr = f["kind"] == GROUP
    assert (f["own_entries"][gr] <= f["tile_entries"][gr]).all() and (f["own_width"][gr] <= 3).all() and (f["tile_entries"][gr] <= 16).all()
    assert ((f["tile_entries"][gr] > 8) == (f["two_pass"][gr] == 1)).all()
    assert ((f["kind"] != 0) == (color >= 0)).all()


# ------------------------------------------------------------------------------------------------------- the oracle
def oracle_live_inference(og, order, ps, seed, sample_evidence, sweeps=41):
    """``sweeps`` sweeps of the oracle's device mode from the initial state: (sweeps in which each variable changed its
    value, the values after every sweep)."""
    vv, _, wv, cnt = og.initial_state()
    changes = np.zeros(len(vv), np.int64)
    seen = [vv.copy()]
    for s in range(sweeps):
        last = vv.copy()
        assert og.gibbs_dev(order, ps, vv, wv, cnt, seed, s, sample_evidence, burnin=s < 3) == 0
        changes += vv != last
        seen.append(vv.copy())
    return changes, np.asarray(seen)
