"""The graph compiler reads its diagnostic switches once per compile_graph call, never once per process: a switch set
or removed between two plans of one process takes effect at the next plan."""

from numbskull_amd import graphgen
from util import session

# the smallest Ising grid (fewest variables; rows <= cols) that plans to a wide quad under NSK_DIAG=1 NSK_WIDE_MIN=0
ROWS, COLS = 1, 387


def test_switches_are_read_at_every_plan(monkeypatch):
    for name in ("NSK_DIAG", "NSK_WIDE_MIN", "NSK_NO_WIDE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("NSK_LAYOUT_HASH", "1")
    fg = session(graphgen.ising_grid(ROWS, COLS, weight=0.3))[1]
    plain = fg.plan()[1]
    assert plain["layout_hash"] != 0 and plain["wide_quads"] == 0      # (far below the default bound)

    monkeypatch.setenv("NSK_DIAG", "1")
    monkeypatch.setenv("NSK_WIDE_MIN", "0")
    wide = fg.plan()[1]
    assert wide["wide_quads"] > 0
    assert wide["layout_hash"] != plain["layout_hash"]

    monkeypatch.setenv("NSK_NO_WIDE", "1")
    assert fg.plan()[1]["wide_quads"] == 0

    monkeypatch.delenv("NSK_DIAG")                 # the others stay set: without NSK_DIAG they count for nothing
    assert fg.plan()[1]["layout_hash"] == plain["layout_hash"]
