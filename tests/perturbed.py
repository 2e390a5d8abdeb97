"""Perturbed Ising grids: a perfect 2-D or 3-D grid plus perturbations placed by cell, for the tests that take the
table-segment and wide-quad paths just past the grid pattern (tests/test_perturbed_grids*.py).

The 2-D grid is graphgen.ising_grid's graph (variable ids row-major; per cell, in id order, the factor to the cell
above, then the one to the left).  The 3-D grid of an A x B x C box is its analogue with six neighbours: per cell the
factors to the previous cell along axis 0, 1, 2 in that order.  Both are 2-colourable (parity of the coordinate sum).
A variable's member slots are its factors in factor-id order (compute_var_map), so an interior 2-D cell reads
[up, left, right, down] and an interior 3-D cell [-axis0, -axis1, -axis2, +axis2, +axis1, +axis0].

Perturbations:

- ``swap(y1, ax1, y2, ax2)``: degree-preserving double-edge swap.  x1 = y1 + stride(ax1) and x2 = y2 + stride(ax2) emit
  the factors f1 = (x1, y1) and f2 = (x2, y2); afterwards f1 = (x1, y2) and f2 = (x2, y1).  y1 and y2 must have one
  colour.  Every variable keeps its number of factors, and the swap is refused unless f2 takes f1's rank in y1's
  factor list and vice versa, and the weight ids agree, so every slot program, and therefore every class, stays as
  it was.  Exactly four member slots change: y1's and y2's slot of the swapped factor, and x1's and x2's slot of
  their own factor.  Those four are the exceptions.
- ``remove(cell, axis)``: drops the factor the cell emits along ``axis``.  Both ends lose a slot and move to another
  class.
- ``set_weight(cell, axis, wid)``: the factor the cell emits along ``axis`` reads weight ``wid``.
- ``evidence`` / ``is_evidence`` of ``graph()``: islands of evidence variables.

``exceptions()`` lists the member slots the perturbations changed, per variable and slot, for the tests to count.
"""

import numpy as np

import util  # noqa: F401  (puts the repository on sys.path)
from numbskull_amd.numbskulltypes import Weight, Variable, Factor, FactorToVar

FUNC_EQUAL = 3


class Grid:
    def __init__(self, dims, weight=0.25, two_weights=False, fixed=True, nweights=None):
        self.dims = tuple(int(d) for d in dims)
        assert len(self.dims) in (2, 3)
        nd = len(self.dims)
        self.nvar = int(np.prod(self.dims))
        self.strides = tuple(int(np.prod(self.dims[a + 1:])) for a in range(nd))
        coords = np.stack(np.unravel_index(np.arange(self.nvar), self.dims), axis=1)
        self.parity = coords.sum(axis=1) % 2
        exists = coords > 0                                   # [cell, axis]: a previous cell along the axis
        self.fid_of = np.full((self.nvar, nd), -1, np.int64)
        self.fid_of[exists] = np.arange(int(exists.sum()))
        emit = np.repeat(np.arange(self.nvar, dtype=np.int64), nd).reshape(self.nvar, nd)[exists]
        other = (np.arange(self.nvar, dtype=np.int64)[:, None] - np.array(self.strides, np.int64)[None, :])[exists]
        axis = np.tile(np.arange(nd), self.nvar).reshape(self.nvar, nd)[exists]
        self.f_emit, self.f_other = emit, other.copy()
        # two_weights: weight 1 on the last axis' factors, weight 0 on the others (graphgen.ising_grid's horizontal and vertical)
        self.f_wid = np.where(axis == nd - 1, 1, 0).astype(np.int64) if two_weights else np.zeros(len(emit), np.int64)
        self.f_alive = np.ones(len(emit), np.bool_)
        self.nweights = nweights or (2 if two_weights else 1)
        self.weight, self.fixed = weight, fixed
        self._orig = None

    def cell(self, *c):
        return int(np.ravel_multi_index(c, self.dims))

    def coords(self, v):
        return tuple(int(x) for x in np.unravel_index(v, self.dims))

    def factors_of(self, v):
        """Live factors that read v, in factor-id order: [(fid, the other member, weight id)]."""
        m = self.f_alive & ((self.f_emit == v) | (self.f_other == v))
        ids = np.nonzero(m)[0]
        return [(int(f), int(self.f_other[f] if self.f_emit[f] == v else self.f_emit[f]), int(self.f_wid[f])) for f in ids]

    def _snapshot(self, vs):
        if self._orig is None:
            self._orig = {}
        for v in vs:
            self._orig.setdefault(int(v), [(o, w) for _, o, w in self.factors_of(v)])

    def swap(self, y1, ax1, y2, ax2, keep_order=True):
        """``keep_order=False``: the swap may move the swapped factors to other ranks of y1's and y2's factor lists
        (their slots are permuted: more than four exceptions).  Where every factor of those variables reads one weight
        id the slot program, and the class, stay the same all the same; otherwise the two variables change class."""
        s1, s2 = self.strides[ax1], self.strides[ax2]
        x1, x2 = y1 + s1, y2 + s2
        assert self.parity[y1] == self.parity[y2] and y1 != y2, "y1 and y2 must have one colour"
        f1, f2 = int(self.fid_of[x1, ax1]), int(self.fid_of[x2, ax2])
        assert f1 >= 0 and f2 >= 0 and self.f_alive[f1] and self.f_alive[f2]
        assert self.f_other[f1] == y1 and self.f_other[f2] == y2, "the factor was moved by an earlier swap"
        assert self.f_wid[f1] == self.f_wid[f2], "a swap keeps every slot program: one weight id"
        assert y2 not in [o for _, o, _ in self.factors_of(x1)] and y1 not in [o for _, o, _ in self.factors_of(x2)]
        # checked before anything changes: a refused swap leaves the grid as it was
        for v, old, new in ((y1, f1, f2), (y2, f2, f1)):
            before = [f for f, _, _ in self.factors_of(v)]
            after = sorted(f for f in before if f != old) + [new]
            if keep_order:
                assert sorted(after).index(new) == before.index(old), ("the swap would reorder the slots of", v)
        self._snapshot((x1, x2, y1, y2))
        self.f_other[f1], self.f_other[f2] = y2, y1
        return self

    def remove(self, v, ax):
        f = int(self.fid_of[v, ax])
        assert f >= 0 and self.f_alive[f]
        self._snapshot((int(self.f_emit[f]), int(self.f_other[f])))
        self.f_alive[f] = False
        return self

    def set_weight(self, v, ax, wid):
        f = int(self.fid_of[v, ax])
        assert f >= 0 and 0 <= wid < self.nweights
        self.f_wid[f] = wid
        return self

    def exceptions(self):
        """{variable: [slot, ...]} of the member slots whose member the perturbations changed."""
        out = {}
        for v, old in (self._orig or {}).items():
            new = [(o, w) for _, o, w in self.factors_of(v)]
            if len(new) != len(old):
                out[v] = list(range(max(len(new), len(old))))
                continue
            d = [j for j, (a, b) in enumerate(zip(old, new)) if a != b]
            if d:
                out[v] = d
        return out

    def graph(self, evidence=None, is_evidence=None, initial=None):
        """(weight, variable, factor, fmap, domain_mask, edges) for NumbSkull.loadFactorGraph.  ``evidence``: values
        of the evidence variables (every variable when ``is_evidence`` is None, as graphgen.ising_grid does)."""
        n = self.nvar
        variable = np.zeros(n, Variable)
        variable["cardinality"] = 2
        if evidence is not None:
            variable["isEvidence"] = 1 if is_evidence is None else np.asarray(is_evidence, np.int8)
            variable["initialValue"] = np.asarray(evidence, np.int64).reshape(n)
        if initial is not None:
            q = variable["isEvidence"] == 0
            variable["initialValue"][q] = np.asarray(initial, np.int64).reshape(n)[q]
        wrec = np.zeros(self.nweights, Weight)
        wrec["isFixed"] = bool(self.fixed)
        wrec["initialValue"] = self.weight
        live = np.nonzero(self.f_alive)[0]
        nf = len(live)
        factor = np.zeros(nf, Factor)
        factor["factorFunction"] = FUNC_EQUAL
        factor["featureValue"] = 1.0
        factor["arity"] = 2
        factor["ftv_offset"] = 2 * np.arange(nf, dtype=np.int64)
        factor["weightId"] = self.f_wid[live]
        fmap = np.zeros(2 * nf, FactorToVar)
        fmap["vid"][0::2] = self.f_emit[live]
        fmap["vid"][1::2] = self.f_other[live]
        return wrec, variable, factor, fmap, np.zeros(n, np.bool_), 2 * nf


def run_cells(g, row, quad, offsets, parity=None):
    """Interior cells of one colour on a grid row, by their place in the row's run: ``row`` is the cell's coordinates
    but the last (2-D: the row index), ``parity`` the colour (default: the row's own, whose first interior cell is
    the second interior column).  The interior cells of one colour of a row, in id order, form one run that the
    compiler starts on a multiple of 256 positions, so offset o of quad q is the run's (256 q + o)-th cell."""
    row = (row,) if np.isscalar(row) else tuple(row)
    par = sum(row) % 2 if parity is None else parity
    c0 = 1 if (sum(row) + 1) % 2 == par else 2           # first interior column of that colour
    return [g.cell(*row, c0 + 2 * (256 * quad + o)) for o in offsets]


# ---------------------------------------------------------------------------------------------------------- the cases
# 2-D cases perturb quad 0 of row 6 of a 16 x 1000 grid: the run of row 6's interior cells of colour 0 (columns 2, 4,
# ..., 998), whose quad 0 has no exception of its own (no border neighbour).  swap(a, 1, c, 0) with c < a on one row:
# a's slot 2 (right) and c's slot 3 (down) change in that quad; a + 1 (slot 1, the row's other colour) and c + 1000
# (slot 0, row 7) are the swap's other two exceptions, in quads of the other colour.  The swaps of one quad are spaced
# so that the compiler's run detection takes them for exceptions, not for the start of a new run.
ROW = 6


def _spaced(g, n, quad=0, row=ROW, parity=None):
    for k in range(n):
        c, a = run_cells(g, row, quad, [10 + 30 * k, 22 + 30 * k], parity)
        g.swap(a, 1, c, 0)
    return g


def _split(g, oc, oa=100, row=ROW):
    """One exception in quad 0 (c, slot 3) and one in quad 1 (a, slot 2)."""
    g.swap(run_cells(g, row, 1, [oa])[0], 1, run_cells(g, row, 0, [oc])[0], 0)
    return g


def _pairs(g, pairs, row=ROW, quad=0):
    for oc, oa in pairs:
        c, a = run_cells(g, row, quad, [oc, oa])
        g.swap(a, 1, c, 0)
    return g


def _slots0to3(g):
    _pairs(g, [(60, 72)])                                       # slots 3 (offset 60) and 2 (offset 72)
    c, a = run_cells(g, ROW - 1, 0, [120, 131])                 # row 5, colour 1: c + 1000 = offset 120 of row 6, slot 0
    g.swap(a, 1, c, 0)
    c, a = run_cells(g, ROW, 0, [170, 180], parity=1)           # row 6, colour 1: a + 1 = offset 180 of the quad, slot 1
    g.swap(a, 1, c, 0)
    return g


def _rest_many(g):
    """Ten or more exceptions in both quads of both colours' runs of rows 2-40 of a 48 x 1000 grid: more than 64
    quads that are not wide per launch, beside the wide quads of rows 41-46."""
    for r in range(2, 41):
        for q in (0, 1):
            for par in (0, 1):
                _spaced(g, 5, quad=q, row=r, parity=par)
    return g


def _many_segments(g):
    """Vertical factors of row pair k read weight k mod 9: the interior classes are (weight above, weight below)
    pairs of two rows each (rows 2k and 2k + 18 alike), so each colour has more than 8 table segments.  (Reasoned
    from the layout: no figure of the plan counts segments; ztab_entries, 304 = 19 four-slot programs x 16, shows the
    classes.)"""
    for v in range(g.nvar):
        r, c = g.coords(v)
        if r > 0:
            g.set_weight(v, 0, (r // 2) % 9)
    return g


def _removed(g):
    """Two interior vertical edges and one horizontal edge dropped: four cells with 3 slots leave their classes."""
    g.remove(g.cell(8, 300), 0).remove(g.cell(9, 601), 0).remove(g.cell(11, 40), 1)
    return g


def _island(g, rng_seed=4):
    """An evidence island in the middle of row 7's and row 8's runs (sampled or not, as sample_evidence says)."""
    n = g.nvar
    ev = np.zeros(n, np.int8)
    for r in (7, 8):
        ev[g.cell(r, 400):g.cell(r, 530)] = 1
    vals = np.random.default_rng(rng_seed).integers(0, 2, n)
    return ev, vals


def _vertical(g, n, row=ROW):
    """swap(y1, 0, y2, 0) on one row: y1's and y2's slot 3 (down) in row 6's quad 0, the cells below them (slot 0) in
    row 7's run of their colour.  One weight class: the learning versions use it."""
    for k in range(n):
        y1, y2 = run_cells(g, row, 0, [10 + 30 * k, 22 + 30 * k])
        g.swap(y1, 0, y2, 0)
    return g


def _g(dims, **kw):
    return lambda: Grid(dims, **kw)


# name -> (grid builder, perturbation, with an evidence island)
CASES = {
    "grid16x1000": (_g((16, 1000)), lambda g: g, False),
    "exc1": (_g((16, 1000)), lambda g: _split(g, 50), False),
    "exc7": (_g((16, 1000)), lambda g: _split(_spaced(g, 3), 200), False),
    "exc8": (_g((16, 1000)), lambda g: _spaced(g, 4), False),
    "exc9": (_g((16, 1000)), lambda g: _split(_spaced(g, 4), 200), False),
    "exc10": (_g((16, 1000)), lambda g: _spaced(g, 5), False),
    "first": (_g((16, 1000)), lambda g: _pairs(g, [(0, 30)]), False),
    "last": (_g((16, 1000)), lambda g: _pairs(g, [(230, 255)]), False),
    "first_last_mid": (_g((16, 1000)), lambda g: _pairs(g, [(0, 127), (200, 255)]), False),
    # slot 3's first and last live positions both exceptions: only the middle candidate gives the base
    "middle_base": (_g((16, 1000)), lambda g: g.swap(*run_cells(g, ROW, 0, [0]), 0, *run_cells(g, ROW, 0, [255]), 0), False),
    "lane": (_g((16, 1000)), lambda g: _pairs(g, [(40, 42), (41, 43)]), False),
    "slots0to3": (_g((16, 1000)), _slots0to3, False),
    "grid3d": (_g((4, 8, 1000)), lambda g: g, False),
    "slots45_3d": (_g((4, 8, 1000)), lambda g: _swaps_3d(g), False),
    "rest_many": (_g((48, 1000)), _rest_many, False),
    "many_segments": (_g((28, 2000), nweights=9), _many_segments, False),
    "removed_island": (_g((16, 1000)), _removed, True),
    "vswap8": (_g((16, 1000)), lambda g: _vertical(g, 4), False),
}

# what the host-only plan makes of each case at NSK_DIAG=1 NSK_WIDE_MIN=0 (tests/test_perturbed_grids_cpu.py): the
# GPU tests rely on these paths being taken
_Q = ("tab_quads", "wide_quads", "ztab_entries", "nfast", "ncolors")
EXPECTED = {k: dict(zip(_Q, v)) for k, v in {
    "grid16x1000": (67, 62, 28, 16000, 2),
    "exc1": (67, 62, 28, 16000, 2),
    "exc7": (67, 62, 28, 16000, 2),
    "exc8": (67, 62, 28, 16000, 2),
    "exc9": (67, 61, 28, 16000, 2),         # the quad of 9 exceptions falls back, nothing else moves
    "exc10": (67, 61, 28, 16000, 2),
    "first": (67, 62, 28, 16000, 2),
    "last": (67, 62, 28, 16000, 2),
    "first_last_mid": (67, 62, 28, 16000, 2),
    "middle_base": (67, 62, 28, 16000, 2),
    "lane": (67, 62, 28, 16000, 2),
    "slots0to3": (67, 62, 28, 16000, 2),
    "grid3d": (130, 120, 120, 32000, 2),    # 5- and 6-slot classes: two-chunk tiles and quads
    "slots45_3d": (130, 120, 120, 32000, 2),
    # 164 quads that are not wide; by the layout about 82 in each colour's launch (no figure reports a launch's share)
    "rest_many": (196, 32, 28, 48000, 2),
    "many_segments": (224, 219, 304, 56000, 2),
    "removed_island": (69, 37, 28, 16000, 2),
    "vswap8": (67, 62, 28, 16000, 2),
}.items()}

# cases whose swaps keep to one weight class, so that they have a two-weight learning version
LEARN_CASES = ("vswap8", "grid3d", "slots45_3d", "many_segments", "removed_island")


def _swaps_3d(g):
    """3-D: swap(y1, 1, y2, 0) with y2 < y1 on one row: y1's slot 4 (+axis 1) and y2's slot 5 (+axis 0) change, in
    quad 0 of row (1, 3); y1 + 1000 (slot 1) and y2 + 8000 (slot 0) are the other two."""
    for k in range(3):
        y2, y1 = run_cells(g, (1, 3), 0, [20 + 40 * k, 35 + 40 * k])
        g.swap(y1, 1, y2, 0)
    return g


def build_case(name, two_weights=False, fixed=True, evidence_seed=None):
    """(Grid, graph tuple) of a case.  ``two_weights`` / ``fixed=False`` / ``evidence_seed``: the learning version
    (every variable evidence with seeded values; a case's evidence island stays as it is).  Learning versions need
    swaps within one weight class: cases whose swaps mix vertical and horizontal factors are refused there."""
    make, perturb, island = CASES[name]
    g = make()
    if two_weights:
        g = Grid(g.dims, weight=g.weight, two_weights=True, fixed=fixed, nweights=max(g.nweights, 2))
    g.fixed = fixed
    perturb(g)
    if evidence_seed is not None:
        vals = np.random.default_rng(evidence_seed).integers(0, 2, g.nvar)
        return g, g.graph(evidence=vals)
    if island:
        ev, vals = _island(g)
        return g, g.graph(evidence=vals, is_evidence=ev)
    return g, g.graph()


def shard_grid(rows, cols, variant, learn, rng):
    """Graph of the perturbed-grid shard tests (tests/test_wide_quads_gpu.py), cut into range shards of whole rows.
    ``"deep"`` (two shards of 96 rows): swaps join cells of rows 10-30 of shard 0 to cells of rows 60-81 of shard 1,
    so tiles far from the cut read ghosts.  ``"two_readers"`` (three shards): cell (48, 500) of shard 1 is read by
    (11, 100) of shard 0 and by (80, 301) of shard 2.  The swaps may permute slots (keep_order=False): with one
    weight the classes stay; the learning version's two weights move the swapped cells to classes of their own."""
    g = Grid((rows, cols), weight=0.0 if learn else 0.1, two_weights=learn, fixed=not learn)
    if variant == "deep":
        g.swap(g.cell(10, 100), 0, g.cell(70, 300), 0, keep_order=False)
        g.swap(g.cell(20, 501), 0, g.cell(80, 701), 0, keep_order=False)
        g.swap(g.cell(30, 2), 1, g.cell(60, 900), 1, keep_order=False)
    elif variant == "two_readers":
        z = g.cell(48, 500)
        g.swap(g.cell(10, 100), 0, z, 0, keep_order=False)       # (11, 100) reads z
        g.swap(z, 1, g.cell(80, 300), 1, keep_order=False)       # (80, 301) reads z
    else:
        raise ValueError(variant)
    return g.graph(evidence=rng.integers(0, 2, g.nvar)) if learn else g.graph()
