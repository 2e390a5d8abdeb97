"""Call sequences on a resident handle against the oracle: one upload, then raw C-ABI calls (tests/resident.py has the
driver, the comparison rules and the scripts; tests/test_resident_calls_cpu.py shows on the oracle alone that no script
can pass by standing still).

Every other parity test goes through the FactorGraph methods, whose upload before and download after each call reset what
a handle carries over: weights_dirty and the weight caches behind it, the uint8 position tally and its sweep counter,
cnt_dirty, chain_regular, and with them the keys of the segment plans and of the captured sweep graphs.  Here that state
survives from call to call, as it does for a caller of include/numbskull_amd.h and in bench.py.

A and B -- the tally residue.  A captured replay of n sweeps folds the uint8 position tally BEFORE it when
pos_tally_sweeps + n > 255; the eager loop used to fold AFTER a sweep, and only when the counter then equalled 255.  A
replay may leave the counter at 255 exactly: nsk_gibbs_sweeps(15) then (241) = 15 eager + 3 x 64 + 3 x 16 captured + 1
eager, and that eager sweep added to bytes that held 255 -- 256 counts lost per wrapped slot, in the wide-quad kernel's
dword add a carry into the neighbouring slot as well -- after which the counter never equalled 255 again.  The eager loop
now folds before a tallied sweep that would take a byte past 255, whatever left the residue.  Before that change, on an
MI355X: of A's sequences (15, 241), (15, 240, 1) and (15, burn-in 5, 241) failed at the final tally comparison, captured,
and (15, 241) with three chains; (15, 240, 16), (14, 241) and (1, 254, 1) passed, as did all six under NSK_NO_GRAPH; both
of B's failed.  All pass with it.

C -- weights across calls: learn / sweep / learn / sweep without an upload, then a weight upload alone.  The case tables
do hold a graph with at most 256 weights and an odd number of colours (tests/tiles.py "gen_m3_blocker": 30 weights, 5
colours), so the lagged pipeline is left on either weight set.  D -- the keys of the plans and captured graphs.  E -- a
seed with a non-zero high half and sweep indices that cross 2^32 inside a call.

Whether the scripts depend on the state they are about was checked once with seven builds that each drop one piece of
it: a weight upload that does not set weights_dirty (weights_grid, weights_mixed_routes and weights_per_factor fail), the
captured graphs' key without the burn-in bit, the plans' key without sample_evidence (keys_evidence_grid fails on
either), a lagged learning call that always copies the second weight set back (weights_odd_colours alone fails), learning
sweeps with the sweep index's high half left 0 (counter_learning fails), eager inference sweeps without it (all five
counter scripts fail) and captured sweeps keyed by the seed's low half alone (the four counter scripts on grids fail);
every other test of the module passed on each."""

import ctypes as C

import numpy as np
import pytest

from numbskull_amd import _lib

import resident
import tiles
from util import oracle_of

pytestmark = pytest.mark.gpu


def _run(monkeypatch, name, profile=False):
    """The script `name` on a fresh handle; returns (info, sweep-kernel launches when `profile`)."""
    sc, fg, hbv = resident.handle(monkeypatch, name)
    info = fg.info()
    resident.check_info(sc, info)
    if sc.tile == "mixed_routes":
        kinds = set(np.unique(_lib.route_fields(fg.routes().astype(np.int64))["kind"]).tolist())
        assert tiles.MIXED_KINDS <= kinds, kinds
    og = oracle_of(fg, hbv)
    m = resident.Mirror(og, fg.colors(), sc.seed, fg=fg, tally256=sc.tally256)
    ms, n = C.c_double(), C.c_int64()
    if profile:
        _lib.check(_lib.lib().nsk_profile_begin(fg._engine()))
    try:
        m.run(sc.calls)
        if profile:
            _lib.check(_lib.lib().nsk_profile_end(fg._engine(), C.byref(ms), C.byref(n)))
    finally:
        fg.close()
    return info, n.value


def _names(prefix):
    return sorted(n for n in resident.SCRIPTS if n.startswith(prefix))


def test_every_script_is_run_by_a_test_of_this_module():
    covered = _names("fold_") + _names("weights_") + _names("keys_") + _names("counter_")
    assert sorted(covered) == sorted(resident.SCRIPTS) and len(covered) == len(set(covered))


# ---- A: captured, and the eager loop alone (NSK_NO_GRAPH)
@pytest.mark.parametrize("name", [n for n in _names("fold_") if "wide" not in n and "chains" not in n])
def test_tally_residue_across_calls(monkeypatch, name):
    _run(monkeypatch, name)


def test_tally_residue_across_calls_of_three_chains(monkeypatch):
    """nsk_set_chains(3): every class launch serves all chains -- as many sweep launches as the one-chain handle makes --
    and each chain is held against its own oracle run."""
    _, three = _run(monkeypatch, "fold_chains_15_241", profile=True)
    _, one = _run(monkeypatch, "fold_15_241", profile=True)
    assert one == three > 0, (one, three)


# ---- B: the packed tally unpacked into cnt_pos; NSK_NO_PACK_TALLY: the wide kernel's dword adds into cnt_pos
@pytest.mark.parametrize("name", _names("fold_wide_"))
def test_tally_residue_on_wide_quads(monkeypatch, name):
    info, _ = _run(monkeypatch, name)
    assert info["wide_quads"] > 0


# ---- C
@pytest.mark.parametrize("name", _names("weights_"))
def test_weights_across_calls(monkeypatch, name):
    _run(monkeypatch, name)


# ---- D
@pytest.mark.parametrize("name", _names("keys_"))
def test_plan_and_capture_keys_across_calls(monkeypatch, name):
    _run(monkeypatch, name)


# ---- E
@pytest.mark.parametrize("name", _names("counter_"))
def test_counter_words_across_calls(monkeypatch, name):
    _run(monkeypatch, name)
