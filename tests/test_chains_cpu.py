"""Several chains, host side: split-R-hat against a direct computation, the --chains option, the C-ABI symbols."""

import argparse
import ctypes as C
import os
import re

import numpy as np

from numbskull_amd import _lib, numbskull
from numbskull_amd.factorgraph import split_rhat

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nsk_set_chains", "nsk_get_chains", "nsk_chains_upload", "nsk_chains_download")


def _rhat_direct(draws):
    """draws: (chains, 2 h) 0/1 of one tally slot -> split-R-hat from the textbook formula, chain by chain."""
    R, T = draws.shape
    h = T // 2
    halves = [draws[r, :h] for r in range(R)] + [draws[r, h:2 * h] for r in range(R)]
    M = len(halves)
    p = np.array([x.mean() for x in halves])
    B = h / (M - 1) * sum((pj - p.mean()) ** 2 for pj in p)
    W = np.mean([h / (h - 1) * pj * (1 - pj) for pj in p])
    if W == 0:
        return np.nan
    return np.sqrt(((h - 1) / h * W + B / h) / W)


def test_split_rhat_matches_a_direct_computation():
    rng = np.random.default_rng(3)
    R, h, nslot = 5, 40, 6
    draws = (rng.random((R, 2 * h, nslot)) < np.linspace(0.1, 0.9, nslot)).astype(np.int64)
    draws[1, :, 0] = 1 - draws[1, :, 0]                     # one chain stuck elsewhere: R-hat well above 1
    draws[:, :, 4] = 1                                      # every draw 1: W = 0 -> NaN
    draws[:, :, 5] = 0                                      # every draw 0 -> NaN
    halves = np.concatenate([draws[:, :h].sum(axis=1), draws[:, h:].sum(axis=1)])   # (2 R, nslot)
    got = split_rhat(halves, h)
    for s in range(nslot):
        want = _rhat_direct(draws[:, :, s])
        if np.isnan(want):
            assert np.isnan(got[s]), s
        else:
            assert abs(got[s] - want) < 1e-12, (s, got[s], want)
    assert np.isnan(got[4]) and np.isnan(got[5]) and got[0] > 1.1


def test_split_rhat_is_nan_for_short_halves():
    assert np.isnan(split_rhat(np.array([[1, 0], [0, 1]]), 1)).all()
    assert np.isnan(split_rhat(np.array([[1, 0], [0, 1]]), 0)).all()
    assert split_rhat(np.zeros((4, 0)), 5).shape == (0,)


def test_chains_option():
    opts = {names[0]: o for names, o in numbskull.engine_arguments}
    assert "--chains" in opts and opts["--chains"]["default"] == 1
    names = [n[0] for n, _ in numbskull.engine_arguments]
    assert abs(names.index("--chains") - names.index("--scan")) == 1
    assert "--chains" not in [n[0] for n, _ in numbskull.arguments + numbskull.flags]
    parser = argparse.ArgumentParser()
    for n, o in numbskull.arguments + numbskull.engine_arguments + numbskull.flags + numbskull.engine_flags:
        parser.add_argument(*n, **o)
    ns = numbskull.NumbSkull(**vars(parser.parse_args(["--chains", "8", "--seed", "5"])))
    assert ns.chains == 8 and ns.seed == 5
    assert numbskull.NumbSkull().chains == 1 and numbskull.NumbSkull(chains=4).chains == 4


def test_chains_graph_rows():
    """NumbSkull(chains=R) loads graphs with at least R rows of var_value, one chain_count row each."""
    from numbskull_amd import graphgen
    g = graphgen.ising_grid(5, 4, weight=0.3)
    ns = numbskull.NumbSkull(chains=6, quiet=True)
    ns.loadFactorGraph(*g[:5], int(g[5]))
    fg = ns.factorGraphs[0]
    assert fg.var_value.shape == (6, 20) and fg.chain_count.shape == (6, len(fg.count))
    assert (fg.var_value == fg.var_value[0]).all()
    fg.chain_count[:] = 3
    fg.count[:] = 2
    fg.clear()
    assert not fg.chain_count.any() and not fg.count.any()


def test_header_declares_and_library_exports_the_chain_entry_points():
    hdr = open(os.path.join(REPO, "include", "numbskull_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(nsk_graph \*g" % name, hdr), name
        assert name in _lib.SYMBOLS
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
