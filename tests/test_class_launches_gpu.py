"""How many kernels a colour class gets is decided on the host (numbskull_amd/csrc/nsk_class_plan.h) and the bit-for-bit
parity tests cannot see all of it: a launch that moved to another stream or lost a block leaves the samples as they
were.  Per graph of the parity set (GRAPHS, and the CLASS_GRAPHS added for the two kinds of class GRAPHS lacked): the
kernel-launch count (the profile bracket's) of a 3-sweep eager inference call,
with and without sample_evidence, and of a 1-epoch learning call -- each taken on the SECOND call, so one-time set-up is
out of it -- equals the table below.

The table's numbers were MEASURED ON THE PARENT COMMIT of the change that introduced the class plans (the drivers that
decided the launches inside the sweep loop), not on the planned drivers: they pin the launch sets of the two to each
other.  A change that adds or removes a launch on purpose re-measures them and says so.

The graph set must contain every kind of class the plans tell apart (asserted from the route words)."""

import ctypes as C

import numpy as np
import pytest

from numbskull_amd import _lib
from util import session
from test_hip_parity import _small_graphs, GRAPHS, CLASS_GRAPHS

pytestmark = pytest.mark.gpu

# name: (inference with sample_evidence, inference without, learning) -- measured on the parent commit (see above)
LAUNCHES = {
    "grid4x5": (6, 6, 2),
    "grid32": (6, 6, 2),
    "mixed": (15, 15, 5),
    "lf": (6, 6, 2),
    "headquirk": (12, 12, 4),
    "headquirk_vid": (9, 9, 3),
    "pairs": (6, 0, 2),
    "grid57x33": (6, 6, 2),
    "lr3000": (21, 21, 7),
    "lr_bigcard": (24, 21, 8),
    "lr_manyw": (21, 21, 7),
    "pairs_manyw": (6, 6, 2),
    "boolw": (27, 27, 9),
    "hubs": (15, 12, 5),
    "gencat": (33, 33, 11),
    "gencat_vid": (42, 42, 14),
    "gencat_bigw": (42, 42, 14),
    "gencat_i32": (42, 42, 14),
    "lr_selfdup": (15, 15, 5),
    "gencat4": (21, 21, 7),
    "gencat4_vid": (54, 45, 17),
    "gencat4_i32": (54, 45, 17),
    "boolw_hub": (27, 27, 9),
    "generic_lanes": (3, 3, 1),
}


def _bracket(fg, call):
    L = _lib.lib()
    ms, n = C.c_double(), C.c_int64()
    call()                                                  # the first call carries the one-time set-up
    _lib.check(L.nsk_profile_begin(fg._engine()))
    call()
    _lib.check(L.nsk_profile_end(fg._engine(), C.byref(ms), C.byref(n)))
    return n.value


def _counts(g, hbv):
    ns, fg = session(g, seed=77, head_by_vid=hbv)
    got = (_bracket(fg, lambda: fg.inference(0, 3, True)),
           _bracket(fg, lambda: fg.inference(0, 3, False)),
           _bracket(fg, lambda: fg.learn(0, 1, 0.01, 0.9, 2, 0.05, 1)))
    return fg, got


def _class_kinds(fg, card):
    """the kinds of colour classes of a handle's layout, as the class plans tell them apart"""
    color, route = np.asarray(fg.colors()), np.asarray(fg.routes())
    kind = route & 15
    found = set()
    for k in np.unique(color[color >= 0]):
        mine = color == k
        kinds = set(kind[mine].tolist())
        general = mine & (kind == _lib.ROUTE_GENERAL)
        if _lib.ROUTE_GROUP in kinds:
            found.add("ep")
        elif general.any() and (card[general] > 2).any():
            found.add("categorical general")
        elif general.any() and _lib.ROUTE_HUB in kinds:
            found.add("binary general with hubs")
        elif _lib.ROUTE_HUB in kinds and not general.any():
            found.add("hubs only")
        if _lib.ROUTE_GENERIC in kinds:
            found.add("generic lanes")
        if kinds & {_lib.ROUTE_SHAPE, _lib.ROUTE_LANE}:      # (never inside a segment: rest tiles)
            found.add("rest tiles")
    return found


_kinds_seen = {}


@pytest.mark.parametrize("name", GRAPHS + CLASS_GRAPHS)
def test_launch_counts_equal_the_parent_commits(golden, name):
    g, hbv = _small_graphs(golden)[name]
    fg, got = _counts(g, hbv)
    _kinds_seen[name] = _class_kinds(fg, np.asarray(g[1]["cardinality"]))
    print("LAUNCHES", repr(name), got, sorted(_kinds_seen[name]))
    assert got == LAUNCHES[name], (name, got, LAUNCHES[name])


def test_the_graph_set_has_every_kind_of_class(golden):
    graphs = _small_graphs(golden)
    seen = set()
    for name in GRAPHS + CLASS_GRAPHS:
        if name not in _kinds_seen:
            g, hbv = graphs[name]
            ns, fg = session(g, seed=77, head_by_vid=hbv)
            _kinds_seen[name] = _class_kinds(fg, np.asarray(g[1]["cardinality"]))
        seen |= _kinds_seen[name]
    assert seen >= {"ep", "categorical general", "binary general with hubs", "hubs only", "generic lanes", "rest tiles"}, seen
