"""Host-only plans of the perturbed grids (tests/perturbed.py): the classification each GPU case of
tests/test_perturbed_grids_gpu.py relies on, and the graph compiler's independence of the thread count on layouts with
wide quads that carry exceptions."""

import json
import os
import subprocess
import sys

import pytest

from util import session, REPO
from perturbed import CASES, EXPECTED, ROW, build_case, run_cells


@pytest.fixture(autouse=True)
def _wide_quads_on_small_graphs(monkeypatch):
    monkeypatch.setenv("NSK_DIAG", "1")
    monkeypatch.setenv("NSK_WIDE_MIN", "0")
    monkeypatch.setenv("NSK_WIDE_LEARN_MIN", "0")


@pytest.mark.parametrize("name", sorted(CASES))
def test_perturbed_grid_plans_take_the_intended_path(name):
    g, graph = build_case(name)
    info = session(graph)[1].plan()[1]
    assert {k: info[k] for k in EXPECTED[name]} == EXPECTED[name], info


def test_exception_counts_around_the_bound():
    """Quad 0 of row 6 holds exactly 1, 7, 8, 9 and 10 exceptions (4 per swap, 2 of them in that quad); up to 8 it
    stays wide, from 9 on it falls back, one quad less, the same number of table quads."""
    def in_quad(name):
        g, _ = build_case(name)
        quad = set(run_cells(g, ROW, 0, range(256)))
        return sum(len(s) for v, s in g.exceptions().items() if v in quad)
    assert [in_quad(n) for n in ("exc1", "exc7", "exc8", "exc9", "exc10")] == [1, 7, 8, 9, 10]
    base = EXPECTED["grid16x1000"]
    for n in ("exc1", "exc7", "exc8"):
        assert EXPECTED[n]["wide_quads"] == base["wide_quads"]
    for n in ("exc9", "exc10"):
        assert EXPECTED[n]["wide_quads"] == base["wide_quads"] - 1 and EXPECTED[n]["tab_quads"] == base["tab_quads"]


_PLAN_SCRIPT = r"""
import hashlib, json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from util import session
from perturbed import build_case, Grid, _spaced, run_cells
out = {}
big = Grid((80, 5000))                          # 400 000 variables: wide quads at the default bound
for r in range(2, 78, 3):
    _spaced(big, 3, quad=r % 9, row=r)
cases = [(n, build_case(n)[1]) for n in ("rest_many", "slots45_3d", "exc9", "many_segments", "removed_island")]
for name, g in cases + [("big", big.graph())]:
    if name == "big":
        os.environ.pop("NSK_WIDE_MIN")                 # the default bound
    color, info = session(g)[1].plan()
    out[name] = [hashlib.sha256(np.ascontiguousarray(color).tobytes()).hexdigest(), info]
print(json.dumps(out, sort_keys=True))
"""


def test_graph_compiler_is_independent_of_the_thread_count_on_perturbed_grids():
    """As tests/test_cabi.py's thread-count test, on layouts whose wide quads carry exceptions in many quads (the
    per-thread exception lists are merged in quad order): colours, every figure of the plan and the layout hash.  The
    400 000-variable grid takes wide quads at the default bound; the others need NSK_WIDE_MIN=0."""
    outs = []
    for threads in ("1", "7"):
        env = dict(os.environ, NSK_COMPILE_THREADS=threads, NSK_LAYOUT_HASH="1", NSK_DIAG="1")
        env["NSK_WIDE_MIN"] = "0"
        r = subprocess.run([sys.executable, "-c", _PLAN_SCRIPT, REPO],
                           env=env, capture_output=True, text=True, timeout=600, cwd=REPO)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]
    assert outs[0]["big"][1]["wide_quads"] > 0 and outs[0]["big"][1]["wide_quads"] < outs[0]["big"][1]["tab_quads"]
    assert all(outs[0][k][1]["layout_hash"] != 0 for k in outs[0])
    assert all(outs[0][k][1]["wide_quads"] > 0 for k in outs[0])
