"""A diagnostic switch that the segment plans read takes effect at the next call on the same handle.

The sweep drivers plan a handle's segment launches once and keep the plans (numbskull_amd/csrc/nsk_seg_plan.h); the key of
that cache is every option the plans were made from, the diagnostic switches among them, and planning again drops the
captured sweep sequences.  So a resident handle (one upload, then raw C-ABI calls: tests/resident.py) whose switches
change between two calls must go on sampling what the oracle samples -- the grid, the kernel and the rest list are no part
of the semantics -- through captured replays and eager sweeps alike, and end where a fresh handle ends that was driven
through the same calls under the same switches.  The smallest wide grids of tests/wide_trips.py, under its switches:
16 x 1000 for inference (under NSK_TABW_GRID_CAP=8 its waves make second trips), 28 x 1000 for learning."""

import numpy as np
import pytest

from numbskull_amd import _lib

import resident
import wide_trips as wt
from util import session, oracle_of

pytestmark = pytest.mark.gpu

# (switch set before the call, the call): 20 sweeps = one captured sequence of 16 and four eager sweeps
INFERENCE = [(None, ("gibbs", 20, 1, 0)),
             (("NSK_TABW_GRID_CAP", "8"), ("gibbs", 20, 1, 0)),
             (("NSK_NO_WIDE_KERNEL", "1"), ("gibbs", 20, 1, 0)),
             (("NSK_NO_TABW_REST", "1"), ("gibbs", 20, 1, 0)),
             (None, ("gibbs", 3, 1, 0))]
LEARNING = [(None, ("learn", 2, 0.02, 2, 1, 0)),
            (("NSK_LEARN_TABW_GRID_CAP", "8"), ("learn", 2, 0.02, 1, 3, 0)),
            (("NSK_NO_WIDE_LEARN", "1"), ("learn", 2, 0.02, 2, 1, 0))]


def _drive(monkeypatch, name, seed, steps, mirror):
    """A fresh handle of shape `name` through `steps`.  With `mirror` (the oracle's side, already run or not): values --
    after a learning call the evidence chain and the weights too -- and tallies against the oracle after every call.
    Returns the final (values, evidence values, weights, tallies)."""
    for k, v in wt.ENV.items():
        monkeypatch.setenv(k, v)
    for switch, _ in steps:
        if switch:
            monkeypatch.delenv(switch[0], raising=False)
    _, fg = session(wt.graph(name), seed=seed)
    try:
        info = fg.info()
        assert 0 < info["wide_quads"] < info["tab_quads"] and info["nfast"] == info["nvar"], info        # wide launches with a rest list
        L, h = _lib.lib(), fg._engine()
        if mirror:
            m = resident.Mirror(oracle_of(fg), fg.colors(), seed, fg=fg)
        else:
            fg._push(0, 0)
        for switch, call in steps:
            if switch:
                monkeypatch.setenv(*switch)
            if mirror:
                m.run([call])           # (compares the values after the call, and values and tallies at its end)
            elif call[0] == "gibbs":
                _lib.check(L.nsk_gibbs_sweeps(h, call[1], call[2], call[3]))
            else:
                _lib.check(L.nsk_learn_sweeps(h, call[1], call[2], resident.DECAY, call[3], resident.REG_PARAM, call[4], call[5]))
        vv, ve, wv, cnt = (np.empty_like(a) for a in oracle_of(fg).initial_state())
        _lib.check(L.nsk_state_download(h, _lib.ptr(vv), _lib.ptr(ve), _lib.ptr(wv), _lib.ptr(cnt)))
        if mirror:
            assert all(moved for _, moved, _ in m.lively), m.lively
            assert np.array_equal(vv, m.vv[0]) and np.array_equal(cnt, m.cnt[0]) and np.array_equal(wv.view(np.uint64), m.wv.view(np.uint64))
        return vv, ve, wv, cnt
    finally:
        fg.close()


@pytest.mark.parametrize("name,seed,steps", [("grid16x1000", 9, INFERENCE), ("learn28x1000", 5, LEARNING)], ids=["inference", "learning"])
def test_switches_changed_between_calls_on_one_handle(monkeypatch, name, seed, steps):
    first = _drive(monkeypatch, name, seed, steps, mirror=True)
    again = _drive(monkeypatch, name, seed, steps, mirror=False)
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)
