"""What the oracle alone says about the scripts of tests/resident.py (host-only; tests/test_resident_calls_gpu.py runs the
same scripts on a handle): a script must not be able to pass by standing still, and the fold scripts must reach the state
the fold is about.

- Every call that samples changes the values, and every learning call the weights.
- The fold scripts' graphs, at the 256th tallied sweep: some tally slot equals 256 -- a byte of the uint8 position tally
  that wraps unless it was folded in time -- and some slot is below 256 -- the neighbour a carry out of that byte would
  land in (resident.Mirror.gibbs asserts it for every chain; here it is run for every such script).

The oracle here numbers its generators by variable id (``oracle_of(fg, layout=False)``), the device by its layout: the
figures differ from a GPU run's, the properties are those of the graphs and call lengths."""

import pytest

import resident
from util import oracle_of


def _mirror(monkeypatch, name):
    sc, fg, hbv = resident.handle(monkeypatch, name)
    color, info = fg.plan()
    og = oracle_of(fg, hbv, layout=False)
    og.set_grad_shift(info["grad_shift"])
    og.device_lag = bool(info["learn_lag"])
    return sc, info, resident.Mirror(og, color, sc.seed, tally256=sc.tally256)


@pytest.mark.parametrize("name", sorted(resident.SCRIPTS))
def test_every_call_of_a_script_is_lively(monkeypatch, name):
    sc, info, m = _mirror(monkeypatch, name)
    resident.check_info(sc, info)
    assert info["nvar"] <= 16000
    m.run(sc.calls)
    assert len(m.lively) == sum(c[0] in ("gibbs", "learn") for c in sc.calls) > 0
    for call, values, weights in m.lively:
        assert values, (name, call, "left the values as they were")
        assert weights is not False, (name, call, "left the weights as they were")


def test_the_fold_scripts_meet_their_precondition(monkeypatch):
    """(asserted inside every run above; this is the figure)  The 48 x 40 grid at weight 1.0: most slots still at 256."""
    sc, info, m = _mirror(monkeypatch, "fold_15_241")
    m.run(sc.calls)
    cnt = m.cnt[0]
    print("slots at 256: %d of %d, minimum %d" % ((cnt == 256).sum(), len(cnt), cnt.min()))
    assert m.tallied == 256 and (cnt == 256).sum() > len(cnt) // 2 and cnt.min() < 256
    names = [n for n, s in resident.SCRIPTS.items() if s.tally256]
    assert len(names) == 15 and all(n.startswith("fold_") for n in names)


def test_the_weight_scripts_cover_both_ends_of_the_lag(monkeypatch):
    """Learn calls of 1 and 2 sweeps on a lagged handle with an odd number of colours: an odd and an even number of classes."""
    sc, info, m = _mirror(monkeypatch, "weights_odd_colours")
    assert info["learn_lag"] == 1 and info["ncolors"] % 2 == 1 and len(m.wv) <= 256
    assert {c[1] for c in sc.calls if c[0] == "learn"} == {1, 2}
