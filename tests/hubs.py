"""Star graphs: hubs -- variables a whole wave or a whole workgroup samples -- with a chosen number of list entries,
cardinality, dataType and kind of factors, for the tests that take the four hub routes at their list-length and
cardinality edges (tests/test_hubs_cpu.py plans every case and checks the route, tests/test_hubs_gpu.py runs them
against the oracle).

``star_graph(hubs=[HubSpec, ...], filler=..., nweight=..., wide_values=..., seed=...)`` returns (weight, variable,
factor, fmap, domain_mask, edges); load it with ``head_by_vid=True`` (the positional functions read their head by id).

A hub's ENTRIES are what the compiler counts (nsk_compile_words.cpp): one per factor in the single list of a
dataType-0 variable, one per factor and named value over the value lists of a dataType-1 variable.  Every hub gets
exactly ``entries`` of them:

- plain factors: the hub once -- first member in the even ones, last in the odd ones, so that it is body and head of
  the positional functions 13 / 16 / 17 -- and 0 .. ``max_others`` private leaves (cardinality 2 .. 4, 40 % evidence;
  a hub's leaves are handed out in turn, each to a few of its factors);
- on hubs of general-tile form with room for them, the factors that name the hub TWICE: body and head of a positional
  function (role 3), AND_CAT with two different values (code 10; on a dataType-1 hub the second list's entry names
  the first as its partner), and OR_CAT with both values of a binary hub (code 11);
- hub 0 and hub 1 share one OR_CAT factor, which puts them in different colours (base offsets of a second colour's
  hubs: phase_hub_base, phase_bighub_base);
- function set ``"boolean"``: functions 0 .. 4 over binary leaves, whatever the hub's cardinality (leaves of the
  fast-path form);
- function set ``"linear"`` / ``"ratio"``: one LINEAR / RATIO factor of featureValue 0.5, ``"seven"``: one factor with
  7 others -- each alone takes the hub off the entry-parallel routes.

Function set "general" is -1, 0 .. 4, 12 .. 17 on a binary hub; a hub of more than two values keeps the functions that
are defined over values (-1, EQUAL, the *_CAT ones), not the boolean ones.

Filler (40 % evidence, as the leaves): ``"cat"`` -- 200 cardinality-3 variables, each joined to its neighbours at distance 1, 3
and 5 under EQUAL / AND_CAT / OR_CAT (general tiles of at most six entries with one other member; enough factors that
300 weights have two factors each on the smallest graphs); ``"binary"`` -- the same over binary variables under
EQUAL (fast path); None.  A
colour is laid out as entry-parallel groups when it holds general tiles whose entries all have at most 3 others: with
``max_others`` <= 3 the leaves alone see to that, with more the hubs' colours are not entry-parallel colours.

Weights: ``nweight`` = 7 (LDS accumulators, lagged learning), 300 (global accumulators) or ``"per_factor"`` (direct
weights); every fifth is fixed; initial values N(0, 1) * WSCALE / sqrt(L), L = entries of the largest hub -- beyond 256
entries * 16 / sqrt(L) again: with weights shared by many factors a hub's log-odds grow like sqrt(L) otherwise --, so
that a hub's conditional neither degenerates nor goes flat (the liveliness condition of tests/test_hubs_cpu.py).  The
SPIKES -- the last three plain factors of every hub, which name its last value and so stand at the end of its last
list, and the factor that joins hubs 0 and 1 -- read weights of their own of size SPIKE, signs alternating (the
last weight and the last but two; with "per_factor" each its own): a sum that loses the end of a list is then wrong by a visible amount.
"""

from collections import namedtuple

import numpy as np

import util  # noqa: F401  (puts the repository on sys.path)
from numbskull_amd.numbskulltypes import Weight, Variable, Factor, FactorToVar

GENERAL = (-1, 0, 1, 2, 3, 4, 12, 13, 14, 15, 16, 17)
VALUED = (-1, 3, 12, 14, 15, 16, 17)          # defined over values, not truth values
BOOLEAN = (0, 1, 2, 3, 4)                     # the fast path's functions
POSITIONAL = (13, 16, 17)
CAT = (12, 14, 15, 16, 17)
WSCALE = 0.45
SPIKE = 0.4

HubSpec = namedtuple("HubSpec", "entries card dtype fset max_others evidence")
HubSpec.__new__.__defaults__ = ("general", 3, False)


class _Build:
    def __init__(self):
        self.fn, self.members, self.deos, self.feat, self.spike = [], [], [], [], []

    def add(self, fn, members, deos, feat=1.0, spike=False):
        self.spike.append(spike)
        self.fn.append(fn)
        self.members.append([int(m) for m in members])
        self.deos.append([int(d) for d in deos])
        self.feat.append(feat)


def hub_entries(g, v):
    """Entries of variable v as the compiler counts them: (factor, named value) pairs of a dataType-1 variable,
    factors of a dataType-0 one."""
    _, variable, factor, fmap = g[:4]
    keyed = int(variable[v]["dataType"]) != 0
    own = np.nonzero(fmap["vid"] == v)[0]
    fid = np.searchsorted(factor["ftv_offset"], own, side="right") - 1
    return len(set(zip(fid.tolist(), fmap["dense_equal_to"][own].tolist() if keyed else [0] * len(own))))


def star_graph(hubs, filler="cat", nweight=7, wide_values=False, seed=0):
    rng = np.random.default_rng(seed)
    hubs = [HubSpec(*h) for h in hubs]
    nh = len(hubs)
    b = _Build()
    cards, dtypes, evid = [h.card for h in hubs], [h.dtype for h in hubs], [int(h.evidence) for h in hubs]

    def new_vars(n, card, dtype=0, ev=0):
        first = len(cards)
        cards.extend(int(c) for c in np.broadcast_to(card, n))
        dtypes.extend([dtype] * n)
        evid.extend(int(e) for e in np.broadcast_to(ev, n))
        return first

    for h, s in enumerate(hubs):
        general = s.card <= 8
        keyed = s.dtype != 0
        funcs = BOOLEAN if s.fset == "boolean" else GENERAL if s.card == 2 else VALUED
        left = s.entries - (1 if nh > 1 and h < 2 else 0)        # the factor that joins hubs 0 and 1
        # leaves, handed out in turn: about two uses each, at most 3000 leaves a hub
        npool = int(max(8, min(3000, left * max(1, s.max_others) // 4)))
        pool = new_vars(npool, 2 if s.fset == "boolean" else rng.integers(2, 5, npool), 0, rng.random(npool) < 0.4)
        at = [0]

        def leaves(n):
            out = [pool + (at[0] + j) % npool for j in range(n)]
            at[0] += n
            return out

        def ldeo(ms):
            return [int(rng.integers(0, cards[m])) for m in ms]

        def own():
            return int(rng.integers(0, s.card))

        # ---- the factors that name the hub twice (general-tile form only; every one of them is of that form)
        if general and s.fset == "general" and left >= 12:
            a, c = own(), own()
            while c == a:
                c = own()
            pos = 13 if s.card == 2 else 17
            ms = leaves(1)
            b.add(pos, [h] + ms + [h], [a] + ldeo(ms) + [a])              # role 3, head test true
            left -= 1
            if not keyed:                                                 # role 3 with another head value (dataType 0:
                ms = leaves(2)                                            # the list is not keyed by the value)
                b.add(16, [h] + ms + [h], [a] + ldeo(ms) + [c])
                left -= 1
            ms = leaves(1)
            b.add(12, [h] + ms + [h], [a] + ldeo(ms) + [c])               # AND_CAT, own edges disagree: code 10
            left -= 2 if keyed else 1                                     # (dataType 1: lists a and c, partner entry)
            if s.card == 2:
                ms = leaves(2)
                b.add(14, [h, ms[0], h, ms[1]], [0, 1, 1, 0])             # OR_CAT names 0 and 1: code 11
                left -= 2 if keyed else 1
                if keyed:                                                 # two different dense_equal_to, body and head
                    ms = leaves(1)
                    b.add(17, [h] + ms + [h], [0] + ldeo(ms) + [1])
                    left -= 2
        if s.fset in ("linear", "ratio"):
            ms = leaves(2)
            b.add(7 if s.fset == "linear" else 8, ms + [h], ldeo(ms) + [own()], feat=0.5)
            left -= 1
        elif s.fset == "seven":
            ms = leaves(7)
            b.add(12 if s.card > 2 else 1, [h] + ms, [own()] + ldeo(ms))
            left -= 1
        else:
            assert s.fset in ("general", "boolean"), s.fset
        assert left >= 0, "too few entries for the hub's special factors"
        # ---- plain factors: one entry each
        # (the last three, SPIKES, name the hub's last value and so close its last list: a round or a chunk that
        # holds nothing but the end of the list still carries weight)
        for i in range(left):
            spike = i >= left - 3
            fn = int(funcs[rng.integers(0 if not spike else 1, len(funcs))])
            ms = leaves(int(rng.integers(0, s.max_others + 1)))
            d = ldeo(ms)
            o = s.card - 1 if spike else own()
            if i % 2 == 0:
                b.add(fn, [h] + ms, [o] + d, spike=spike)
            else:
                b.add(fn, ms + [h], d + [o], spike=spike)
    if nh > 1:
        # (values below 4: a cardinality-65 neighbour must not push a general-form hub's member word past 5 bits)
        b.add(14, [0, 1], [min(3, hubs[0].card - 1), min(3, hubs[1].card - 1)], spike=True)

    if filler == "cat":
        f0 = new_vars(200, 3, 0, rng.random(200) < 0.4)
        for st in (1, 3, 5):                               # (odd strides: the filler stays 2-colourable)
            for i in range(200 - st):
                b.add((3, 12, 14)[i % 3], [f0 + i, f0 + i + st], [int(rng.integers(0, 3)), int(rng.integers(0, 3))])
    elif filler == "binary":
        f0 = new_vars(200, 2, 0, rng.random(200) < 0.4)
        for st in (1, 3, 5):
            for i in range(200 - st):
                b.add(3, [f0 + i, f0 + i + st], [0, 0])
    else:
        assert filler is None, filler
    if wide_values:
        new_vars(1, 200)                                   # values no longer fit int8: the int32 kernels

    nvar, nfactor = len(cards), len(b.fn)
    variable = np.zeros(nvar, Variable)
    variable["cardinality"] = cards
    variable["dataType"] = dtypes
    variable["isEvidence"] = evid
    variable["initialValue"] = (rng.random(nvar) * np.asarray(cards)).astype(np.int64)
    arity = np.array([len(m) for m in b.members], np.int64)
    nedge = int(arity.sum())
    factor = np.zeros(nfactor, Factor)
    factor["factorFunction"] = b.fn
    factor["featureValue"] = b.feat
    factor["arity"] = arity
    factor["ftv_offset"] = np.cumsum(arity) - arity
    fmap = np.zeros(nedge, FactorToVar)
    fmap["vid"] = np.concatenate([np.asarray(m, np.int64) for m in b.members])
    fmap["dense_equal_to"] = np.concatenate([np.asarray(d, np.int64) for d in b.deos])
    if nweight == "per_factor":
        nw = nfactor
        factor["weightId"] = np.arange(nfactor)
    else:
        nw = int(nweight)
        regular = np.array([w for w in range(nw) if w not in (nw - 1, nw - 3)])      # (the other two: the spikes')
        # in turn, from a shuffled start: every weight has a factor once there are as many factors as weights
        factor["weightId"] = regular[(rng.permutation(nfactor) + int(rng.integers(0, nw))) % len(regular)]
    lmax = max(h.entries for h in hubs)
    weight = np.zeros(nw, Weight)
    weight["initialValue"] = rng.normal(0, 1, nw) * WSCALE / max(np.sqrt(lmax), lmax / 16.0)
    if nweight != "per_factor":
        # opposite pairs: most functions grow with the hub's value, so a weight shared by many of a binary hub's
        # factors pushes it one way by its whole sum; two weights of opposite sign on equal shares cancel on average
        weight["initialValue"][regular[1::2]] = -weight["initialValue"][regular[0:2 * len(regular[1::2]):2]]
    spikes = np.nonzero(b.spike)[0]
    sign = np.where(np.arange(len(spikes)) % 2 == 0, 1.0, -1.0)
    if nweight == "per_factor":
        weight["initialValue"][spikes] = sign * SPIKE
    else:
        factor["weightId"][spikes] = np.where(sign > 0, nw - 1, nw - 3)
        weight["initialValue"][nw - 1], weight["initialValue"][nw - 3] = SPIKE, -SPIKE
    weight["isFixed"][::5] = True
    g = (weight, variable, factor, fmap, np.zeros(nvar, np.bool_), nedge)
    for h, s in enumerate(hubs):
        assert hub_entries(g, h) == s.entries, (h, hub_entries(g, h), s.entries)
    return g


# ---------------------------------------------------------------------------------------------------------- the cases
ROT = ((2, 0), (2, 1), (3, 1), (5, 0), (8, 0), (8, 1))         # the (cardinality, dataType) of general-tile form
BIG = tuple((c, d) for c in (9, 16, 17, 64, 65) for d in (0, 1))    # too many values for a general tile
# general-tile (cardinality, dataType) with one factor that is not: LINEAR, 7 others, RATIO
OFF_FORM = ((2, 0, "linear"), (2, 1, "seven"), (5, 0, "ratio"), (8, 1, "linear"), (3, 1, "seven"), (2, 1, "linear"))
# the one-lane draw: card 2 / registers up to 16 / two passes above
LANE = ((2, 0, "linear"), (2, 1, "seven"), (3, 0, "linear"), (3, 1, "ratio"), (16, 0, "general"), (16, 1, "general"),
        (17, 0, "general"), (17, 1, "general"))


def general_hubs(L, mo=3, cds=ROT, fset="general"):
    return [HubSpec(L, c, d, fset, mo) for c, d in cds]


def formed_hubs(L, cdf):
    return [HubSpec(L, c, d, f, 3) for c, d, f in cdf]


Case = namedtuple("Case", "hubs filler wide env route expect learn")


def _case(hubs, route, expect, filler="cat", wide=False, env=(), learn=True):
    return Case(hubs, filler, wide, tuple(env), route, expect, learn)


# name -> Case.  ``route``: "wave" (entry-parallel, one wave), "block" (entry-parallel, one workgroup), "walk" (generic
# wave walk), "lane" (one lane per variable).  ``expect`` = (hubs_ep, hubs_block) of the plan, which follow from the
# routing rules for the case's hubs (nsk_compile_groups.cpp build_hub_streams): the hubs of general-tile form up to the
# cap of their colour -- 16384 entries in a colour laid out as entry-parallel groups, 256 elsewhere -- and of those
# the ones with more than 128 entries in an entry-parallel colour.  ``env``: diagnostic switches (with NSK_DIAG=1).
CASES = {}
for _L in (31, 32, 33, 64, 65, 128):
    CASES["wave%d" % _L] = _case(general_hubs(_L), "wave", (6, 0))
for _L in (129, 256):                                      # 3 and 4 rounds of 64 entries
    CASES["wave%d_noep" % _L] = _case(general_hubs(_L), "wave", (6, 0), env=["NSK_NO_EP"])
# entries of 4 .. 6 others: the leaves' colours are no entry-parallel colours, the cap is 256 without any switch
CASES["wave65_mo6"] = _case(general_hubs(65, mo=6), "wave", (6, 0), learn=False)
CASES["wave256_mo6"] = _case(general_hubs(256, mo=6), "wave", (6, 0))
CASES["walk257_mo6"] = _case(general_hubs(257, mo=6), "walk", (0, 0))
CASES["wave65_i32"] = _case(general_hubs(65), "wave", (6, 0), wide=True)
# boolean functions over binary leaves, with each kind of filler.  (On graphs this small the compiler moves fast-path
# variables without a class of their own to the general tiles, so the leaves make the hubs' colours entry-parallel
# colours whatever the filler is; what takes a colour off that layout here is an entry of more than 3 others.)
_BOOL = ((2, 1), (3, 0), (3, 1), (5, 0), (8, 0), (8, 1))
for _f in ("cat", "binary", None):
    CASES["wave65_bool_%s" % _f] = _case(general_hubs(65, cds=_BOOL, fset="boolean"), "wave", (6, 0), filler=_f, learn=False)
    CASES["block129_bool_%s" % _f] = _case(general_hubs(129, cds=_BOOL, fset="boolean"), "block", (6, 6), filler=_f,
                                           learn=_f is None)
for _L in (129, 257, 1024, 1025, 2100):                    # 1025: the second chunk of 1024 entries holds one entry
    CASES["block%d" % _L] = _case(general_hubs(_L), "block", (6, 6))
CASES["block16384"] = _case(general_hubs(16384), "block", (6, 6), learn=False)
CASES["walk16385"] = _case(general_hubs(16385), "walk", (0, 0), learn=False)
CASES["block1025_i32"] = _case(general_hubs(1025), "block", (6, 6), wide=True)
for _L in (33, 130):
    CASES["walk%d_big" % _L] = _case(general_hubs(_L, cds=BIG), "walk", (0, 0))        # (65, dataType 1) at 33: empty lists
    CASES["walk%d_form" % _L] = _case(formed_hubs(_L, OFF_FORM), "walk", (0, 0))
    CASES["lane%d" % _L] = _case(formed_hubs(_L, LANE), "lane", (0, 0), env=["NSK_NO_HEAVY"])
CASES["walk129_nohubep"] = _case(general_hubs(129), "walk", (0, 0), env=["NSK_NO_HUB_EP"])
CASES["walk257_noep"] = _case(general_hubs(257), "walk", (0, 0), env=["NSK_NO_EP"])
CASES["walk33_i32"] = _case(general_hubs(33, cds=BIG), "walk", (0, 0), wide=True, learn=False)
CASES["lane33_i32"] = _case(formed_hubs(33, LANE), "lane", (0, 0), wide=True, env=["NSK_NO_HEAVY"], learn=False)
# one graph, four routes
for _r, _e, _x in (("block", (), (6, 6)), ("wave", ("NSK_NO_EP",), (6, 0)), ("walk", ("NSK_NO_HUB_EP",), (0, 0)),
                   ("lane", ("NSK_NO_HEAVY",), (0, 0))):
    CASES["four200_%s" % _r] = _case(general_hubs(200), _r, _x, env=_e, learn=_r != "block")

# learning configurations: (regularization, truncation, learn_non_evidence, hubs are evidence, nweight).  Without
# learn_non_evidence only evidence variables are visited, so those configurations make the hubs evidence.
LEARN_CFG = {
    "A": (0, 1, False, True, 7), "B": (1, 3, True, False, 300), "C": (2, 1, True, True, "per_factor"),
    "D": (0, 1, False, True, 300), "E": (2, 1, True, False, 7), "F": (1, 3, True, False, "per_factor"),
}
LEARN_CASES = [(n, c) for i, n in enumerate(k for k in CASES if CASES[k].learn) for c in ("ABC", "DEF")[i % 2]]

SALT = 0                # added to every case's seed: chosen so that every case is lively in the oracle
INFER = (3, 40)         # burn-in and tallied sweeps of the inference tests
EPOCHS = 6


def nhubs(name):
    return len(CASES[name].hubs)


def build_case(name, nweight=7, hubs_evidence=None):
    """Graph of a case.  ``hubs_evidence``: None -- hub 3 alone is evidence (sampled with sample_evidence, held
    otherwise); True / False -- every hub / none (the learning configurations)."""
    cs = CASES[name]
    hubs = [h._replace(evidence=(i == 3) if hubs_evidence is None else bool(hubs_evidence)) for i, h in enumerate(cs.hubs)]
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + SALT
    return star_graph(hubs, filler=cs.filler, nweight=nweight, wide_values=cs.wide, seed=seed)


def set_switches(monkeypatch, name):
    for k in CASES[name].env:
        monkeypatch.setenv("NSK_DIAG", "1")
        monkeypatch.setenv(k, "1")


def check_route(name, info):
    """The counters of a plan / a handle say the case took its route."""
    cs, n = CASES[name], nhubs(name)
    assert (info["hubs_ep"], info["hubs_block"]) == cs.expect, (name, info)
    if cs.route == "lane":
        assert info["hubs"] == 0 and info["ngeneric"] >= n, (name, info)
    else:
        assert info["hubs"] >= n and info["ngeneric"] >= n, (name, info)       # (a leaf off the tile form is a hub too)


# ------------------------------------------------------------------------------------------------------- the oracle
class Live:
    """What the oracle's own run did to the hubs: changes of value and distinct values per hub."""

    def __init__(self, vv, n):
        self.n = n
        self.last = vv[:n].copy()
        self.changes = np.zeros(n, np.int64)
        self.seen = [{int(x)} for x in vv[:n]]

    def note(self, vv):
        self.changes += vv[:self.n] != self.last
        self.last = vv[:self.n].copy()
        for h in range(self.n):
            self.seen[h].add(int(vv[h]))

    def check(self, variable, sample_evidence):
        """Every sampled hub changed value at least 5 times and took 2 values, 3 above cardinality 4."""
        for h in range(self.n):
            if int(variable[h]["isEvidence"]) != 0 and not sample_evidence:
                assert self.changes[h] == 0
                continue
            need = 3 if int(variable[h]["cardinality"]) > 4 else 2
            assert self.changes[h] >= 5 and len(self.seen[h]) >= need, (h, int(self.changes[h]), sorted(self.seen[h]))


def oracle_inference(og, order, ps, seed, sample_evidence, n):
    """INFER sweeps of the oracle's device mode from the initial state: (values, tallies, Live)."""
    vv, _, wv, cnt = og.initial_state()
    live = Live(vv, n)
    for s in range(sum(INFER)):
        assert og.gibbs_dev(order, ps, vv, wv, cnt, seed, s, sample_evidence, burnin=s < INFER[0]) == 0
        live.note(vv)
    return vv, cnt, live


def oracle_learning(og, order, ps, seed, cfg, step=0.02, decay=0.9, need=0.5):
    """EPOCHS learning epochs in one call, then 3 inference sweeps from the learnt state:
    (values, evidence-chain values, weights, values after inference, tallies).  At least ``need`` of the free weights
    must have moved."""
    reg, trunc, lne = LEARN_CFG[cfg][:3]
    vv, ve, wv, cnt = og.initial_state()
    assert og.learn_call(order, ps, vv, ve, wv, EPOCHS, step, decay, reg, 0.05, trunc, lne, seed, 0) == 0
    learnt = (vv.copy(), ve.copy(), wv.copy())
    for s in range(EPOCHS, EPOCHS + 3):
        assert og.gibbs_dev(order, ps, vv, wv, cnt, seed, s, True) == 0
    free = og.weight["isFixed"] == 0
    moved = learnt[2][free] != og.weight["initialValue"][free]
    assert int(moved.sum()) >= need * int(free.sum()), ("too few of the free weights moved", int(moved.sum()), int(free.sum()))
    return learnt + (vv, cnt)
