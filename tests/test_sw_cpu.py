"""Swendsen-Wang without a GPU: the host plan of every case (nsk_sw_plan), its refusals, and the rule itself --
diagnostics.sw_tables and sw_step -- against the model: the full transition matrix of one cluster update leaves the
Boltzmann law of the theta tables invariant.  The weights of the two invariance graphs are multiples of 1 / 16, so the
fixed-point fields H are the fields exactly and 1e-12 is float64 round-off over 2^n states."""

import itertools

import numpy as np
import pytest

import bp
import sw
from numbskull_amd.diagnostics import sw_tables, sw_step
from oracle import binding as orc
from util import session


@pytest.mark.parametrize("name", sorted(sw.CASES))
@pytest.mark.parametrize("tile", [1024, 64])
def test_the_plan_places_everything_once(name, tile):
    build, hbv, sev, _ = sw.CASES[name]
    _, fg = session(build(), head_by_vid=hbv)
    p = fg.plan_sw(sev, tile)
    lay = bp.bp_layout(fg.factor, fg.fmap, fg.variable, fg.variable["initialValue"], bool(sev))
    nfree = [len(ax) for ax in lay["axes"]]
    with_factor = sorted({v for ax in lay["axes"] for v in ax})
    assert sorted(p["order"]) == with_factor and p["nvars"] == len(with_factor)
    assert list(p["bond_factor"]) == [f for f, k in enumerate(nfree) if k == 2] and p["nfields"] == nfree.count(1)
    assert [list(p["order"][e]) for e in p["bond_ends"]] == [lay["axes"][f] for f in p["bond_factor"]]
    # a bond is in exactly one tile, that of both its ends, or in the cross list; tiles are runs of at most `tile` ordinals
    assert (p["bond_tile"] == -1).sum() == p["ncross"] and p["bond_tile"].max(initial=-1) < p["ntiles"]
    tile_of = np.full(p["nvars"], -1)
    for b in np.flatnonzero(p["bond_tile"] >= 0):
        for o in p["bond_ends"][b]:
            assert tile_of[o] in (-1, p["bond_tile"][b])
            tile_of[o] = p["bond_tile"][b]
    known = tile_of[tile_of >= 0]
    assert (np.diff(known) >= 0).all() and np.bincount(known, minlength=1).max() <= tile
    if name == "grid40" and tile == 1024:
        assert p["ntiles"] == 2 and 0 < p["ncross"] < 0.1 * p["nbonds"]


def _transition(g, keep):
    """P of one update over the states of the free variables, from sw_step's clusters and decisions and sw_tables' probabilities; pi"""
    m = bp.Model(g)
    t = sw_tables(m.theta, m.layout, exp=orc.exp_det)
    order = np.asarray(sorted({v for ax in m.layout["axes"] for v in ax}), np.int64)
    assert len(order) == keep
    ends = np.searchsorted(order, t["bond_vars"])
    H, n, nb, top = t["H"][order], len(order), len(t["J"]), 1.0 - 2.0 ** -53
    states = list(itertools.product((0, 1), repeat=n))
    index = {s: i for i, s in enumerate(states)}
    P, logpi = np.zeros((len(states),) * 2), np.zeros(len(states))
    for i, s in enumerate(states):
        x = m.x.copy()
        x[order] = s
        for f, ax in enumerate(m.layout["axes"]):
            logpi[i] += m.theta[m.layout["table_off"][f] + (int(np.ravel_multi_index(x[ax], m.layout["shapes"][f])) if ax else 0)]
        for drawn in itertools.product((0, 1), repeat=nb):          # u(b, 4) >= q_b or not, independently
            pb = np.prod(np.where(drawn, 1.0 - t["q"], t["q"]))
            if pb == 0.0:
                continue
            ub = np.where(drawn, top, 0.0) if nb else np.zeros(0)
            step = lambda uc: sw_step(x, order, ends, t["J"], t["q"], H, ub, uc, exp=orc.exp_det)      # noqa: E731
            _, labels, _, _, moved = step(np.full(n, top))
            roots = np.flatnonzero(labels == np.arange(n))
            D = np.array([np.where(x[order][labels == r] == 0, H[labels == r], -H[labels == r]).sum() for r in roots]) * 2.0 ** -32
            sigma = 1.0 / (1.0 + np.exp(-D))
            # sw_step's own decision: nobody at the largest uniform, every cluster just below sigma, none just above it
            uc = np.full(n, top)
            uc[roots] = sigma * (1.0 - 1e-9)
            assert moved == 0 and step(uc)[4] == n and step(np.where(uc < top, uc * (1.0 + 2e-9), top))[4] == 0
            for flips in itertools.product((0, 1), repeat=len(roots)):
                y = x.copy()
                y[order] = np.where(np.asarray(flips)[np.searchsorted(roots, labels)] == 1, 1 - x[order], x[order])
                P[i, index[tuple(y[order])]] += pb * np.prod(np.where(flips, sigma, 1.0 - sigma))
    pi = np.exp(logpi - logpi.max())
    return P, pi / pi.sum()


@pytest.mark.parametrize("name", ["grid2x3", "mixed5"])
def test_the_update_leaves_the_boltzmann_law_invariant(name):
    if name == "grid2x3":
        g = sw.pairwise(6, [(sw.EQUAL, 0, 1, 0.4375), (sw.EQUAL, 1, 2, 0.875), (sw.EQUAL, 3, 4, -0.5), (sw.EQUAL, 4, 5, 0.4375),
                            (sw.EQUAL, 0, 3, 1.0), (sw.EQUAL, 1, 4, 0.4375), (sw.EQUAL, 2, 5, 0.25)], [(0, 0.5), (4, -0.75), (5, 0.125)])
    else:
        g = sw.pairwise(6, [(sw.EQUAL, 0, 1, -1.0), (sw.EQUAL, 1, 2, -1.0), (sw.EQUAL, 2, 0, -1.0), (sw.IMPLY, 0, 3, 0.75),
                            (sw.AND, 3, 4, -0.5), (sw.OR, 4, 1, 1.25), (sw.IMPLY, 5, 2, 0.875)], [(4, 0.25), (3, -0.5)], evid={5: 1})
    P, pi = _transition(g, 6 if name == "grid2x3" else 5)
    assert np.abs(P.sum(axis=1) - 1.0).max() < 1e-12
    assert np.abs(pi @ P - pi).max() < 1e-12 and (P > 0).sum() > len(pi)


@pytest.mark.parametrize("cards,factor,text", [
    ([2, 3, 2], (sw.EQUAL, [0, 1], [0, 0], 0.5), "factor 1 has a free member of cardinality 3"),
    ([2, 2, 2], (sw.AND, [0, 1, 2], [0, 0, 0], 0.5), "factor 1 has 3 distinct free members"),
])
def test_refusals_by_classification(cards, factor, text):
    _, fg = session(bp.spec_graph(cards, [0] * 3, [0] * 3, [(sw.ISTRUE, [0], [0], 0.3), factor, (sw.AND, [0, 1, 2], [0, 0, 0], 0.1)]))
    with pytest.raises(ValueError, match="nsk_sw_setup: " + text):
        fg.plan_sw()
