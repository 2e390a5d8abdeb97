"""Truth tables of the factor functions, cell by cell, as graphs (tests/test_truth_tables_cpu.py plans them and checks
routes, completeness and decisiveness on the oracle; tests/test_truth_tables_gpu.py runs them on every kernel family).

A CELL is one TARGET variable, its private LEAF variables and ONE factor over them; nothing else touches them.  Leaves
are evidence, so with ``sample_evidence=False`` they keep their enumerated values through an inference run, and the
target's conditional is the truth table of its factor in the target's own value.

``truth_graph(...)`` enumerates, per function: the arity (from the function's minimum arity on), the target's position
``j`` among the members (every one), the target's cardinality (2 and 3), its own dense_equal_to (its whole domain under
the *_CAT functions, 0 otherwise), EVERY combination of leaf values (``lcard ** (arity - 1)``; leaves have dense_equal_to
1 under the *_CAT functions, 0 otherwise) and the sign of the weight.  It returns the graph tuple and one Cell per cell.

Weights: two per function, +W and -W (lanes then share slot programs: uniform tiles, draw tables), or one per factor
(``per_factor``: shape tiles, weights updated in place).  NOOP's weights are fixed: no state gives them a gradient.
W is the same for every function but RATIO, whose values log(k + 1), k <= 3, lie closer together than 1: its weights
are RATIO_SCALE times as large, so that W times the smallest gap between two of its values is >= W again.

``learn=True``: the targets are evidence and every cell is repeated once per value of its target (``reps`` = "card"),
the repeat's number being the target's initial value: the evidence chain's term of the gradient then visits every
(cell, own value) exactly once per epoch.

The smaller families: ``wide_family`` (arity 5 .. 7 over binary leaves: the role walk M = 4 .. 6, 4 .. 6 other members
on the fast path), ``self_family`` (the target named two or three times: forms "az", "aa", "aaa" of tests/tiles.py),
``literal_family`` (head_by_vid=False under functions 13 / 16 / 17: the head is read at the factor's last EDGE INDEX,
which names an isolated evidence variable in front holding the enumerated head value) and ``hub_family`` (targets whose
factor LIST walks through the cells: 33 .. 300 entries each)."""

from collections import namedtuple
from itertools import product

import numpy as np

import util  # noqa: F401  (puts the repository on sys.path)
from numbskull_amd.numbskulltypes import Weight, Variable, Factor, FactorToVar

ALL = (-1, 0, 1, 2, 3, 4, 7, 8, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 30)
FAST = (-1, 0, 1, 2, 3, 4)                      # the fast path's functions (binary dataType-0 targets)
TILE = FAST + (12, 13, 14, 15, 16, 17)          # the general tiles', the groups' and the entry-parallel hubs'
OFF_TILE = tuple(f for f in ALL if f not in TILE)
CAT = (12, 14, 15, 16, 17)
POSITIONAL = (13, 16, 17)
RATIO = 8
RATIO_SCALE = 4.0        # 1 / (log 4 - log 3) = 3.48: the smallest gap between two values of RATIO at arity <= 4
W_DECISIVE = 40.0
W_LIVELY = 0.7

Cell = namedtuple("Cell", "fn arity j card own sign leaves target factor")


def min_arity(fn, card, lcard):
    """The data-programming functions read fixed member positions; UFO reads member (value of the first member) - 1,
    and the first member is the target or a leaf."""
    if fn in (21, 22, 25, 26):
        return 2
    if fn in (23, 24):
        return 3
    if fn == 30:
        return max(card, lcard)
    return 1


class _Build:
    def __init__(self, W, per_factor, pad_front=0):
        self.W, self.per_factor = float(W), per_factor
        self.cards, self.dtypes, self.evid, self.init = [3] * pad_front, [0] * pad_front, [1] * pad_front, [0] * pad_front
        self.pad_front = pad_front
        self.fn, self.members, self.deos, self.wid = [], [], [], []
        self.wval, self.wfixed, self.shared = [], [], {}
        self.nedge = 0
        self.cells = []
        self.scale = 1.0                 # of the weights handed out from here on (hub_family)

    def var(self, card, evidence, init, dtype=0):
        self.cards.append(int(card)); self.dtypes.append(int(dtype)); self.evid.append(int(evidence)); self.init.append(int(init))
        return len(self.cards) - 1

    def weight(self, fn, sign):
        key = len(self.fn) if self.per_factor else (fn, sign, self.scale)
        if key not in self.shared:
            self.shared[key] = len(self.wval)
            self.wval.append(sign * self.W * self.scale * (RATIO_SCALE if fn == RATIO else 1.0))
            self.wfixed.append(fn == -1)
        return self.shared[key]

    def factor(self, fn, members, deos, sign):
        assert len(members) == len(deos)
        self.wid.append(self.weight(fn, sign))
        self.fn.append(int(fn)); self.members.append([int(m) for m in members]); self.deos.append([int(d) for d in deos])
        self.nedge += len(members)
        return len(self.fn) - 1

    def cell(self, fn, arity, j, card, own, sign, leaves, target=None, learn=False, init=0, ldeo=None, lcard=3, dtype=0):
        """One cell: a new target (or ``target``, a hub) at position j, new leaves around it."""
        ldeo = (1 if fn in CAT else 0) if ldeo is None else ldeo
        t = self.var(card, learn, init % card, dtype) if target is None else target
        ids = [self.var(lcard, 1, x) for x in leaves]
        f = self.factor(fn, ids[:j] + [t] + ids[j:], [ldeo] * j + [own] + [ldeo] * (arity - 1 - j), sign)
        self.cells.append(Cell(fn, arity, j, card, own, sign, tuple(leaves), t, f))
        return t, ids, f

    def graph(self, wide=False):
        if wide:
            self.var(200, 0, 0)              # values no longer fit int8: the int32 kernels
        nvar, nfactor, nw = len(self.cards), len(self.fn), len(self.wval)
        variable = np.zeros(nvar, Variable)
        variable["cardinality"] = self.cards
        variable["dataType"] = self.dtypes
        variable["isEvidence"] = self.evid
        variable["initialValue"] = self.init
        arity = np.array([len(m) for m in self.members], np.int64)
        factor = np.zeros(nfactor, Factor)
        factor["factorFunction"] = self.fn
        factor["featureValue"] = 1.0
        factor["arity"] = arity
        factor["ftv_offset"] = np.cumsum(arity) - arity
        factor["weightId"] = self.wid
        fmap = np.zeros(self.nedge, FactorToVar)
        fmap["vid"] = np.concatenate([np.asarray(m, np.int64) for m in self.members])
        fmap["dense_equal_to"] = np.concatenate([np.asarray(d, np.int64) for d in self.deos])
        weight = np.zeros(nw, Weight)
        weight["initialValue"] = self.wval
        weight["isFixed"] = self.wfixed
        assert nvar <= 200000, nvar
        return (weight, variable, factor, fmap, np.zeros(nvar, np.bool_), self.nedge), self.cells


def owns(fn, card):
    return range(card) if fn in CAT else (0,)


def truth_graph(fns=ALL, lcard=3, W=W_DECISIVE, per_factor=False, reps=1, wide=False, learn=False, arities=(1, 2, 3, 4)):
    """The main enumeration.  ``reps``: copies of every cell ("card": one per value of the target); a copy's number
    modulo the cardinality is its target's initial value."""
    b = _Build(W, per_factor)
    for fn in fns:
        for card in (2, 3):
            for arity in arities:
                if arity < min_arity(fn, card, lcard):
                    continue
                for j in range(arity):
                    for own in owns(fn, card):
                        for leaves in product(range(lcard), repeat=arity - 1):
                            for sign in (1, -1):
                                for r in range(card if reps == "card" else reps):
                                    b.cell(fn, arity, j, card, own, sign, leaves, learn=learn, init=r + (0 if learn else 1), lcard=lcard)
    return b.graph(wide)


def wide_family(fns=TILE, W=W_DECISIVE, per_factor=False, reps=1, learn=False, arities=(5, 6, 7)):
    """Arity 5 .. 7: 4 .. 6 other members, binary leaves (all 2 ** (arity - 1) combinations of matching / not matching),
    the target first (a body member of the positional functions) and last (their head)."""
    b = _Build(W, per_factor)
    for fn in fns:
        for card in (2, 3):
            for arity in arities:
                for j in (0, arity - 1):
                    for own in owns(fn, card):
                        for leaves in product(range(2), repeat=arity - 1):
                            for sign in (1, -1):
                                for r in range(card if reps == "card" else reps):
                                    b.cell(fn, arity, j, card, own, sign, leaves, learn=learn, init=r + (0 if learn else 1), lcard=2)
    return b.graph()


# the forms that name the target more than once: (form, functions, number of own edges)
SELF_FORMS = (("az", POSITIONAL, 2), ("aa", (0, 1, 2, 3, 12, 13, 14, 16, 17), 2), ("aaa", (12, 14, 17), 3))


def self_family(W=W_DECISIVE, per_factor=False, reps=1, learn=False, lcard=3):
    """The target first and last ("az": role 3 of the positional functions), first and second ("aa": own edges that
    disagree, codes 10 / 11) or the first three members ("aaa"), every combination of own dense_equal_to under the *_CAT
    functions, 1 and 2 leaves, all their values.  Cell.j is the form, Cell.own the tuple of own dense_equal_to."""
    b = _Build(W, per_factor)
    for form, fns, nown in SELF_FORMS:
        for fn in fns:
            for card in (2, 3):
                for own in (product(range(card), repeat=nown) if fn in CAT else [(0,) * nown]):
                    for nl in (1, 2):
                        for leaves in product(range(lcard), repeat=nl):
                            for sign in (1, -1):
                                for r in range(card if reps == "card" else reps):
                                    ld = 1 if fn in CAT else 0
                                    t = b.var(card, learn, (r + (0 if learn else 1)) % card)
                                    ids = [b.var(lcard, 1, x) for x in leaves]
                                    if form == "az":
                                        m, d = [t] + ids + [t], [own[0]] + [ld] * nl + [own[1]]
                                    else:
                                        m, d = [t] * nown + ids, list(own) + [ld] * nl
                                    f = b.factor(fn, m, d, sign)
                                    b.cells.append(Cell(fn, len(m), form, card, tuple(own), sign, tuple(leaves), t, f))
    return b.graph()


def literal_family(W=W_DECISIVE, per_factor=False, reps=1, learn=False, lcard=3, arities=(1, 2, 3, 4), pad_front=None):
    """head_by_vid=False: functions 13 / 16 / 17 read their head at var_value[last edge index] unless the head is the
    sampled variable itself.  ``pad_front`` isolated evidence variables (cardinality 3) come first; the one at each
    factor's last edge index holds the enumerated head value -- the LAST entry of Cell.leaves, behind the values of
    the arity - 1 leaves (when the target is not the last member, the last leaf is the head by id and is never read)."""
    if pad_front is None:                     # as many as there are edges
        pad_front = sum(arity * arity * len(owns(fn, card)) * lcard ** arity * 2 * (card if reps == "card" else reps)
                        for fn in POSITIONAL for card in (2, 3) for arity in arities)
    b = _Build(W, per_factor, pad_front)
    for fn in POSITIONAL:
        for card in (2, 3):
            for arity in arities:
                for j in range(arity):
                    for own in owns(fn, card):
                        for leaves in product(range(lcard), repeat=arity - 1):
                            for head in range(lcard):
                                for sign in (1, -1):
                                    for r in range(card if reps == "card" else reps):
                                        t, ids, f = b.cell(fn, arity, j, card, own, sign, leaves, learn=learn,
                                                           init=r + (0 if learn else 1), lcard=lcard)
                                        b.cells[-1] = b.cells[-1]._replace(leaves=tuple(leaves) + (head,))
                                        b.init[b.nedge - 1] = head
    assert b.nedge <= pad_front, (b.nedge, pad_front)
    return b.graph()


HUB_KINDS = ((2, 0), (3, 1), (2, 1), (3, 0))             # (cardinality, dataType) of the hubs, in turn


def hub_entries(g, v):
    """Entries of variable v as the compiler counts them (tests/hubs.py)."""
    import hubs
    return hubs.hub_entries(g, v)


def hub_family(W=W_LIVELY, per_factor=False, learn=False, lcard=3, lengths=(300, 150, 100, 33), fns=TILE, off_fns=ALL):
    """Truth-table hubs: every hub's factor list walks through cells -- (function, position of the hub, own
    dense_equal_to, leaf values, sign) in enumeration order, each with private leaves -- until it has its length in
    ENTRIES (one per factor of a dataType-0 hub, one per factor and named value of a dataType-1 hub).  The hubs of the
    functions ``fns`` are of general-tile form (the entry-parallel routes: a wave up to 128 entries, a workgroup
    beyond); those of ``off_fns`` hold a function that is not (the generic wave walk).  Returns (graph, cells, hubs)."""
    b = _Build(W, per_factor)
    hubs_ = []

    def cells_of(fset, card):
        for arity in (1, 2, 3, 4):
            for fn in fset:
                if arity < min_arity(fn, card, lcard):
                    continue
                for j in sorted({0, arity - 1}):
                    for own in owns(fn, card):
                        for leaves in product(range(lcard), repeat=arity - 1):
                            for sign in (1, -1):
                                yield fn, arity, j, own, sign, leaves

    for fset in (fns, off_fns):
        for k, (card, dtype) in enumerate(HUB_KINDS):
            # a dataType-1 hub finds a factor in the list of the value its own edge names: for the functions that ignore
            # dense_equal_to the own value cycles, so that every list is filled
            stream = list(cells_of(fset, card))
            at = 0
            stride = next(p for p in (11, 13, 17, 19, 23) if len(stream) % p)      # a stride through the whole enumeration
            for L in lengths:
                h = b.var(card, learn, len(hubs_) % card, dtype)
                # a sum of L terms of either sign: potentials of size 3 |w| (2 |w| where every value has a list of its
                # own, whose sums do not share terms)
                b.scale = (2.0 if dtype else 3.0) / float(np.sqrt(L))
                for i in range(L):
                    fn, arity, j, own, sign, leaves = stream[(at + i * stride) % len(stream)]
                    if dtype == 1 and fn not in CAT:
                        own = i % card
                    b.cell(fn, arity, j, card, own, sign, leaves, target=h, lcard=lcard)
                at += L * stride
                hubs_.append((h, L, fset is fns))
    g, cells = b.graph()
    for h, L, _ in hubs_:
        assert hub_entries(g, h) == L, (h, hub_entries(g, h), L)
    return g, cells, hubs_


# ------------------------------------------------------------------------------------------------------------ the facts
def general_code(fn):
    """nsk_compile_words.cpp general_code: the function code of a general-tile entry."""
    return {-1: 0, 0: 1, 1: 2, 2: 3, 4: 3, 3: 4, 13: 5, 12: 6, 15: 6, 14: 7, 16: 8, 17: 9}[fn]


def chain_facts(code, xs, deo=1):
    """GenChain::member over the values ``xs`` of the other members, in member order: (allnz, prevall, any1, alleq,
    lastnz).  Facts about leaf values, not function values: under a *_CAT code a member is "non-zero" and "one" when it
    equals its dense_equal_to, otherwise when it is != 0 / == 1."""
    cat = code >= 6
    allnz, prevall, any1, alleq, lastnz, first = True, True, False, True, False, 0
    for m, x in enumerate(xs):
        nz = (x == deo) if cat else (x != 0)
        one = (x == deo) if cat else (x == 1)
        alleq = True if m == 0 else (alleq and x == first)
        first = x if m == 0 else first
        prevall = allnz
        allnz = allnz and nz
        any1 = any1 or one
        lastnz = nz
    return allnz, prevall, any1, alleq, lastnz


def lut_index(fn, xs, head, deo=1):
    """The index into the 2048-entry table (gen_lut_entry) an entry of function ``fn`` reaches whose OTHER members hold
    ``xs``; ``head``: the target is the last member (own role 2 under a positional function, else role 1; role 0 under
    the others)."""
    code = general_code(fn)
    if code == 0:
        xs = ()                                     # NOOP keeps no member words
    allnz, prevall, any1, alleq, lastnz = chain_facts(code, xs, deo)
    role1 = int(fn in POSITIONAL and not head)
    return (code | role1 << 4 | int(len(xs) == 0) << 5 | int(allnz) << 6 | int(prevall) << 7 | int(any1) << 8 |
            int(alleq) << 9 | int(lastnz) << 10)


def cell_lut_index(c):
    return lut_index(c.fn, c.leaves, c.j == c.arity - 1)


# ------------------------------------------------------------------------------------------------------- the argmax sets
def classify(og, cells, state):
    """Per cell: (values f(c) of the factor per candidate c, argmax set of sign * f).  ``og``: the oracle's view."""
    out = []
    state = np.ascontiguousarray(state, np.int64)
    for c in cells:
        f = []
        for v in range(c.card):
            rc, val = og.eval_factor(c.factor, c.target, v, state)
            assert rc == 0, (c, rc)
            f.append(val)
        s = [c.sign * x for x in f]
        out.append((tuple(f), frozenset(v for v in range(c.card) if s[v] == max(s))))
    return out


def census(cells, cls):
    """(cells, unique-argmax targets, partial ties, constant in the candidate)."""
    uniq = sum(len(a) == 1 for _, a in cls)
    const = sum(len(a) == c.card for c, (_, a) in zip(cells, cls))
    return len(cells), uniq, len(cells) - uniq - const, const


def check_decisive(cells, cls, values):
    """Every unique-argmax target holds its argmax, every partial-tie target a member of its argmax set."""
    values = np.asarray(values)
    bad = [(c, int(values[c.target]), sorted(a)) for c, (_, a) in zip(cells, cls) if int(values[c.target]) not in a]
    assert not bad, (len(bad), bad[:6])


# ------------------------------------------------------------------------------------------------------------- variants
Variant = namedtuple("Variant", "family kw env hbv")


def _v(family, env=(), hbv=True, **kw):
    return Variant(family, kw, tuple(env), hbv)


# name -> Variant: the graphs and switches (NSK_DIAG=1) that put every function on every family that supports it
VARIANTS = {
    "main": _v("truth"),
    "tables": _v("truth", lcard=2, reps=8),
    "no_ztab": _v("truth", lcard=2, reps=8, fns=FAST, env=("NSK_NO_ZTAB",)),
    "per_factor": _v("truth", per_factor=True),
    "lane": _v("truth", per_factor=True, env=("NSK_NO_SHAPE",)),
    "general": _v("truth", env=("NSK_NO_EP",)),
    "roles": _v("wide", env=("NSK_NO_EP",)),
    "one_lane": _v("truth", env=("NSK_NO_HEAVY",)),
    "generic": _v("truth", env=("NSK_NO_GENERAL", "NSK_NO_FAST")),
    "generic_lane": _v("truth", env=("NSK_NO_GENERAL", "NSK_NO_FAST", "NSK_NO_HEAVY")),
    "self": _v("self", env=("NSK_NO_EP",)),
    "literal": _v("literal", env=("NSK_NO_EP",), hbv=False),
}
FAMILIES = {"truth": truth_graph, "wide": wide_family, "self": self_family, "literal": literal_family}


def build_variant(name, **kw):
    v = VARIANTS[name]
    args = dict(v.kw)
    args.update(kw)
    return FAMILIES[v.family](**args)


def set_switches(monkeypatch, name):
    for k in VARIANTS[name].env:
        monkeypatch.setenv("NSK_DIAG", "1")
        monkeypatch.setenv(k, "1")
