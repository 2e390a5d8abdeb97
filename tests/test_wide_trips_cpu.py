"""Host-only plans of the shapes of tests/test_wide_trips_gpu.py (tests/wide_trips.py): what that module's multi-trip
condition needs of them and a box without a GPU can check.  A launch of T virtual quads under a grid cap of c workgroups
sends its waves on a second trip only if T > 4 c, and a sweep of these graphs is one launch per colour, so the handle's
table quads must number at least ncolors (4 c + 1) -- necessary, not sufficient: the GPU module bounds every class from
the device layout.  A change of the layout that leaves one of these shapes with fewer quads, or with too few wide ones
for its launches to be the wide kernels', fails here first."""

import pytest

from util import session
import wide_trips as wt


@pytest.fixture(autouse=True)
def _wide_quads_on_small_graphs(monkeypatch):
    for k, v in wt.ENV.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("name", sorted(wt.SHAPES))
def test_shapes_are_wide_and_large_enough_for_a_second_trip(name):
    caps = wt.SHAPES[name][1]
    assert caps and all(c >= 8 and c % 8 == 0 for c in caps)
    color, info = session(wt.graph(name))[1].plan()
    assert info["wide_quads"] * 10 >= info["tab_quads"] * 9 > 0, info
    assert info["tab_quads"] - info["wide_quads"] <= 64 and info["nfast"] == info["nvar"], info
    assert info["ncolors"] == int(color.max()) + 1 >= 2
    for cap in caps:
        assert info["tab_quads"] >= wt.min_quads(info["ncolors"], cap), (info, cap)


def test_the_first_shape_is_large_enough_for_a_third_trip():
    """40 x 1000 under cap 8 is the GPU module's three-trip case: T > 8 c in every class."""
    color, info = session(wt.graph("grid40x1000"))[1].plan()
    assert info["tab_quads"] >= info["ncolors"] * (8 * 8 + 1), info
