"""Shapes of the wide-quad trip-loop tests: one list for tests/test_wide_trips_gpu.py (the runs against the oracle) and
tests/test_wide_trips_cpu.py (what the host-only plan says about the same graphs), so that the two cannot drift apart.

A grid-capped wide launch of `c` workgroups (NSK_TABW_GRID_CAP / NSK_LEARN_TABW_GRID_CAP, a multiple of 8) has
wpx = c / 2 waves per XCD, and each XCD walks per = ceil(T / 8) of the launch's T virtual quads: a wave makes a second
trip only if per > wpx, that is T > 4 c, and a third only if T > 8 c (tests/test_wide_trips_gpu.py has the whole
arithmetic).  Every shape here is the smallest of its kind whose colour classes hold more than 4 c quads each under the
caps listed with it."""

import numpy as np

import util  # noqa: F401  (puts the repository on sys.path)
from numbskull_amd import graphgen
from perturbed import Grid, build_case, _spaced

# the switches both modules set: wide quads and wide learning launches on graphs the oracle walks in seconds
ENV = {"NSK_DIAG": "1", "NSK_WIDE_MIN": "0", "NSK_WIDE_LEARN_MIN": "0"}


def evidence_grid(rows=60, cols=1200):
    """Two weights; the cells of columns 900 .. 1199 are evidence with seeded values (the pattern of
    tests/test_wide_quads_gpu.py test_wide_quads_with_two_weights_and_evidence): the classes split by evidence flag, and
    the evidence cells' runs of 150 are too short to be padded into wide quads.  60 rows, not that test's 48: from 56
    rows on nine tenths of the table quads are wide (48 rows: 216 of 245)."""
    n = rows * cols
    rng = np.random.default_rng(3)
    ev = np.where(np.arange(n) % cols < 900, 0, 1) * rng.integers(0, 2, n)
    g = graphgen.ising_grid(rows, cols, weight=0.2, fixed=True, two_weights=True, evidence=ev)
    g[1]["isEvidence"] = (np.arange(n) % cols >= 900).astype(g[1]["isEvidence"].dtype)
    return g


def learning_grid(half, rows=28, cols=1000):
    """Two free weights, seeded values, every variable evidence (tests/test_wide_quads_gpu.py
    test_learning_on_a_padded_layout) -- or, `half`, only the lower half of the rows: whole rows, so that every run keeps
    its 500 cells per colour and stays wide while each colour gets segments of both evidence flags.  28 rows, not that
    test's 24: the smallest even count at which nine tenths of the table quads are wide in both versions (24 rows: 94 of
    105 and 95 of 106)."""
    n = rows * cols
    rng = np.random.default_rng(1)
    g = graphgen.ising_grid(rows, cols, weight=0.2, fixed=False, two_weights=True, evidence=rng.integers(0, 2, n))
    if half:
        g[1]["isEvidence"] = (np.arange(n) >= (rows // 2) * cols).astype(g[1]["isEvidence"].dtype)
    return g


def later_trip_exceptions():
    """(Grid, graph) of tests/perturbed.py's "exc8" moved to quad 0 of row 3 of a 16 x 1000 grid: eight exceptions in the
    fifth quad of the interior segment (two quads per row, rows 1 and 2 in front), in the row's own colour."""
    g = _spaced(Grid((16, 1000)), 4, quad=0, row=3)
    return g, g.graph()


# name -> (graph builder, the grid caps the GPU module runs it under)
SHAPES = {
    "grid40x1000": (lambda: graphgen.ising_grid(40, 1000, weight=0.3), (8, 16)),     # 80 quads per class: three trips under 8
    "grid33x1537": (lambda: graphgen.ising_grid(33, 1537, weight=0.3), (8,)),        # odd width: rows of 768 / 769 cells
    "grid9x4099": (lambda: graphgen.ising_grid(9, 4099, weight=0.3), (8,)),          # wide three-slot border rows
    "grid16x1000": (lambda: graphgen.ising_grid(16, 1000, weight=0.25), (8,)),
    "grid24x1000": (lambda: graphgen.ising_grid(24, 1000, weight=0.3), (8,)),
    "evidence60x1200": (evidence_grid, (8,)),
    "exc8": (lambda: build_case("exc8")[1], (8,)),
    "slots45_3d": (lambda: build_case("slots45_3d")[1], (8,)),
    "exc8_row3": (lambda: later_trip_exceptions()[1], (8,)),
    "learn28x1000": (lambda: learning_grid(False), (8,)),
    "learn28x1000_half": (lambda: learning_grid(True), (8,)),
}


def graph(name):
    return SHAPES[name][0]()


def min_quads(ncolors, cap):
    """What every class of a handle needs for a second trip under `cap`, summed: ncolors (4 cap + 1) table quads."""
    return ncolors * (4 * cap + 1)
