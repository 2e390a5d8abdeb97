"""Per-weight sufficient statistics on the device (nsk_weight_stats, the stats column of a sample trace).

Yardstick: the factor values of the oracle's eval_factor (test_log_potential_gpu._oracle_values), grouped by weightId
on the host and added with math.fsum -- never values of the library.  A weight whose terms are all integers must match
EXACTLY (integer sums below 2^53 are exact in any order); any other weight within
|S_w - fsum| <= (n_w + 1) * 2^-53 * sum |t|, which holds for any summation order of n_w terms (Higham, Accuracy and
Stability of Numerical Algorithms, 2nd edition, section 4.2; one more u for the rounding of fsum's result) -- derived,
not measured.  A weight without a factor must read exactly 0.0.  Everything the sums are supposed to be independent of
is checked bit for bit.

moment_gap end to end (the last test): the target is the EXACT expectation of the statistics, by enumeration of a
pair's four states, not the evidence chain's statistics.  The evidence of ising_pairs is itself one draw from the
planted distribution, so its statistics lie a standard deviation of ONE state from the expectation, while the standard
error of a mean over 4000 recorded states is some sixty times smaller: only the exact expectation can be held to
5 * mcse."""

import ctypes as C
import math

import numpy as np
import pytest

import numbskull_amd
from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import moment_gap
from test_hip_parity import GRAPHS
from test_log_potential_gpu import _graph, _oracle_values, _bits
from util import session, oracle_of

pytestmark = pytest.mark.gpu

SEED = 77


def _groups(wid):
    """weight id -> indices of its factors, for the weights that have any"""
    order = np.argsort(wid, kind="stable")
    ids, start = np.unique(wid[order], return_index=True)
    return {int(w): order[s:e] for w, s, e in zip(ids, start, list(start[1:]) + [len(order)])}


def _check_stats(S, t, wid, nweight, what):
    """S against the terms t (float64, one per factor) grouped by wid"""
    assert S.shape == (nweight,) and S.dtype == np.float64, what
    groups = _groups(wid)
    worst = 0.0
    for w, idx in groups.items():
        terms = t[idx]
        ref = math.fsum(terms.tolist())
        if np.array_equal(terms, np.rint(terms)):
            assert S[w] == ref, (what, "weight", w, S[w], ref)
        else:
            bound = (len(terms) + 1) * 2.0 ** -53 * math.fsum(np.abs(terms).tolist())
            worst = max(worst, abs(S[w] - ref) / bound if bound else 0.0)
            assert abs(S[w] - ref) <= bound, (what, "weight", w, S[w], ref, bound)
    empty = np.ones(nweight, np.bool_)
    empty[list(groups)] = False
    assert np.array_equal(_bits(S[empty]), np.zeros(int(empty.sum()), np.int64)), (what, "weights without a factor")
    print("%s: %d weights with factors, %d without, worst |diff| / bound %.3g" % (what, len(groups), int(empty.sum()), worst))


def _stats_of_chains(fg, which, first, n, scaled=0):
    out = np.zeros((n, len(fg.weight)), np.float64)
    _lib.check(_lib.lib().nsk_weight_stats(fg._engine(), which, first, n, scaled, _lib.ptr(out)))
    return out


# ---------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("name", GRAPHS)
def test_statistics_match_the_oracle_grouped_by_weight(golden, name):
    g, hbv = _graph(golden, name)
    wid = np.asarray(g[2]["weightId"], np.int64)
    nw = len(g[0])
    _, fg = session(g, seed=SEED, head_by_vid=hbv)
    og = oracle_of(fg, hbv)
    fg.inference(2, 3, True)
    _check_stats(fg.weight_statistics(), _oracle_values(og, fg.var_value[0]), wid, nw, name + " free")
    fg.learn(1, 3, 0.01, 0.95, 2, 0.01, 1)
    _check_stats(fg.weight_statistics(evidence_chain=True), _oracle_values(og, fg.var_value_evid[0]), wid, nw, name + " evidence")
    _check_stats(fg.weight_statistics(), _oracle_values(og, fg.var_value[0]), wid, nw, name + " free after learning")
    _, f3 = session(g, seed=SEED, head_by_vid=hbv, chains=3)
    f3.inference(2, 3, True, var_copy="all")
    S = f3.weight_statistics(var_copy="all")
    assert S.shape == (3, nw) and S.dtype == np.float64
    for r in range(3):
        _check_stats(S[r], _oracle_values(og, f3.var_value[r]), wid, nw, "%s chain %d" % (name, r))


# ---------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("two", [False, True])
def test_weights_of_several_pieces(two):
    """79 600 factors under one weight (39 pieces of 2048, the last of 1776), or 39 800 under each of two (20 pieces,
    the last of 888): the second launch adds the piece partials"""
    g = graphgen.ising_grid(200, 200, weight=0.3, two_weights=two)
    wid = np.asarray(g[2]["weightId"], np.int64)
    assert len(g[2]) == 79600 and len(g[0]) == (2 if two else 1)
    _, fg = session(g, seed=SEED, chains=2)
    og = oracle_of(fg)
    fg.inference(2, 3, True, var_copy="all")
    S = fg.weight_statistics(var_copy="all")
    for r in range(2):
        e = _oracle_values(og, fg.var_value[r])
        assert np.array_equal(e, np.rint(e))
        _check_stats(S[r], e, wid, len(g[0]), "grid200 chain %d" % r)
    assert not np.array_equal(S[0], S[1])


# ---------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("name", ["hubs", "mixed"])
def test_feature_scaled_terms(golden, name):
    g, hbv = _graph(golden, name)
    w, v, f, fm, dm, edges = [x.copy() if isinstance(x, np.ndarray) else x for x in g]
    feat = np.random.default_rng(SEED).uniform(0.3, 1.7, len(f))       # non-dyadic
    f["featureValue"] = feat
    wid = np.asarray(f["weightId"], np.int64)
    _, fg = session((w, v, f, fm, dm, edges), seed=SEED, head_by_vid=hbv)
    og = oracle_of(fg, hbv)
    # (featureValue enters no conditional, but the layout reserves its fast paths for featureValue == 1 and the draws
    # are keyed by layout position: the state is this handle's own, not the unscaled graph's)
    fg.inference(2, 3, True)
    e = _oracle_values(og, fg.var_value[0])
    S0 = fg.weight_statistics()
    _check_stats(S0, e, wid, len(w), name + " unscaled")
    before = fg.info()["device_bytes"]
    S1 = fg.weight_statistics(feature_scaled=True)
    assert fg.info()["device_bytes"] in (before, before + 8 * len(f))   # the feature values, unless the kernels read them already
    _check_stats(S1, feat * e, wid, len(w), name + " scaled")           # fl(feat * e), one rounding each
    assert not np.array_equal(S0, S1)
    assert np.array_equal(_bits(fg.weight_statistics()), _bits(S0))     # scaled = 0 on the same handle is unchanged
    assert np.array_equal(_bits(fg.weight_statistics(feature_scaled=True)), _bits(S1))


# ---------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("name", GRAPHS)
def test_identity_with_the_log_potential(golden, name):
    """sum_w w * S_w against log_potential(): both are sums of the same nfactor products up to one rounding per
    addition and per product w * S_w.  (factor_values only scales the bound; it equals the oracle, test_log_potential_gpu.)"""
    g, hbv = _graph(golden, name)
    wid = np.asarray(g[2]["weightId"], np.int64)
    _, fg = session(g, seed=SEED, head_by_vid=hbv)
    fg.learn(1, 2, 0.01, 0.95, 2, 0.01, 1)
    fg.inference(1, 2, True)
    wv = fg.weight_value[0]
    S = fg.weight_statistics()
    lhs = math.fsum((wv * S).tolist())
    lp = fg.log_potential()
    scale = math.fsum(np.abs(wv[wid] * fg.factor_values()).tolist())
    bound = (len(wid) + len(wv) + 2) * 2.0 ** -53 * scale
    print("%s: sum w S %.17g lp %.17g |diff| %.3g bound %.3g" % (name, lhs, lp, abs(lhs - lp), bound))
    assert abs(lhs - lp) <= bound, (name, lhs, lp, bound)


# ---------------------------------------------------------------------------------------------- e
@pytest.mark.parametrize("name", ["grid57x33", "lr3000", "hubs", "boolw", "gencat_i32"])
def test_the_sums_are_reproducible_bit_for_bit(golden, name):
    g, hbv = _graph(golden, name)
    nw = len(g[0])
    _, src = session(g, seed=SEED, head_by_vid=hbv)
    src.inference(1, 2, True)
    x = src.var_value[0].copy()
    _, one = session(g, seed=SEED + 1, head_by_vid=hbv)
    one.var_value[0][:] = x
    S1 = one.weight_statistics()
    assert np.array_equal(_bits(one.weight_statistics()), _bits(S1))                    # two consecutive calls
    _, three = session(g, seed=SEED + 2, head_by_vid=hbv, chains=3)
    three.inference(0, 2, True, var_copy="all")
    three.var_value[0][:] = x
    three.var_value[2][:] = x
    S3 = three.weight_statistics(var_copy="all")
    assert np.array_equal(_bits(S3[0]), _bits(S1)) and np.array_equal(_bits(S3[2]), _bits(S1))
    assert np.array_equal(_bits(_stats_of_chains(three, _lib.BUF_VALUE, 1, 2)), _bits(S3[1:]))    # a sub-range of the chains
    assert np.array_equal(_bits(_stats_of_chains(three, _lib.BUF_VALUE, 2, 1)[0]), _bits(S1))
    one.var_value_evid[0][:] = x
    assert np.array_equal(_bits(one.weight_statistics(evidence_chain=True)), _bits(S1))
    # all weights against a trace column of a selection with a repeat
    ids = [nw - 1, 0, nw - 1]
    _, a = session(g, seed=SEED, head_by_vid=hbv, chains=3)
    _, b = session(g, seed=SEED, head_by_vid=hbv, chains=3)
    rows_a, all_a = a.sample(4, thin=2, sample_evidence=True, var_copy="all", weight_statistics=True)
    rows_b, sel_b = b.sample(4, thin=2, sample_evidence=True, var_copy="all", weight_statistics=ids)
    assert np.array_equal(rows_a, rows_b)
    assert all_a.shape == (2, 3, nw) and sel_b.shape == (2, 3, 3)
    assert np.array_equal(_bits(sel_b), _bits(all_a[:, :, ids]))


# ---------------------------------------------------------------------------------------------- f
@pytest.mark.parametrize("name", ["grid57x33", "lr3000", "gencat_i32", "hubs"])
@pytest.mark.parametrize("nchains", [1, 3])
@pytest.mark.parametrize("thin", [1, 3])
@pytest.mark.parametrize("with_lp", [False, True])
def test_trace_rows_carry_the_statistics_of_their_state(golden, name, nchains, thin, with_lp):
    g, hbv = _graph(golden, name)
    nw = len(g[0])
    vc = "all" if nchains > 1 else 0
    _, a = session(g, seed=SEED, head_by_vid=hbv, chains=nchains)
    _, b = session(g, seed=SEED, head_by_vid=hbv, chains=nchains)
    _, tw = session(g, seed=SEED, head_by_vid=hbv)
    res_a = a.sample(10, thin=thin, burnin_epochs=2, sample_evidence=True, var_copy=vc, log_potential=with_lp, weight_statistics=True)
    res_b = b.sample(10, thin=thin, burnin_epochs=2, sample_evidence=True, var_copy=vc, log_potential=with_lp)
    assert isinstance(res_a, tuple) and len(res_a) == (3 if with_lp else 2)
    rows, stats = res_a[0], res_a[-1]
    if with_lp:
        assert np.array_equal(rows, res_b[0]) and np.array_equal(_bits(res_a[1]), _bits(res_b[1]))
    else:
        assert isinstance(res_b, np.ndarray) and np.array_equal(rows, res_b)
    assert stats.shape == (10 // thin, nchains, nw) and stats.dtype == np.float64
    for i in range(rows.shape[0]):
        for r in range(nchains):
            tw.var_value[0][:] = rows[i, r]
            assert np.array_equal(_bits(stats[i, r]), _bits(tw.weight_statistics())), ("row", i, "chain", r)
    # the flagged call leaves what the unflagged one leaves
    assert np.array_equal(a.var_value, b.var_value) and np.array_equal(a.count, b.count)
    assert np.array_equal(a.chain_count, b.chain_count)
    assert a.info()["sweeps_done"] == b.info()["sweeps_done"]
    # no columns at all: the rows are empty, the stats column is not
    _, d = session(g, seed=SEED, head_by_vid=hbv, chains=nchains)
    res_d = d.sample(10, var_ids=[], thin=thin, burnin_epochs=2, sample_evidence=True, var_copy=vc, log_potential=with_lp, weight_statistics=True)
    assert res_d[0].shape == (10 // thin, nchains, 0)
    assert np.array_equal(_bits(res_d[-1]), _bits(stats))


# ---------------------------------------------------------------------------------------------- g
def test_packed_tally_rows_of_the_million_grid():
    """a one-chain handle of wide quads keeps its tally in bits 1-7 of the value bytes between the runs of a traced
    call: the stats column must read bit 0 only"""
    g = graphgen.ising_grid(1000, 1000, weight=0.3, two_weights=True)
    _, fg = session(g, seed=SEED)
    _, tw = session(g, seed=SEED)
    assert fg.info()["wide_quads"] > 0
    rows, stats = fg.sample(12, thin=4, weight_statistics=True)
    assert rows.shape == (3, 1, 10 ** 6) and stats.shape == (3, 1, 2)
    vid = g[3]["vid"]
    wid = np.asarray(g[2]["weightId"], np.int64)
    for i in range(3):
        tw.var_value[0][:] = rows[i, 0]
        assert np.array_equal(_bits(stats[i, 0]), _bits(tw.weight_statistics())), ("row", i)
        x = rows[i, 0].astype(np.int64)
        e = np.where(x[vid[0::2]] == x[vid[1::2]], 1, -1)
        assert stats[i, 0, 0] == e[wid == 0].sum() and stats[i, 0, 1] == e[wid == 1].sum()      # integers: exact
    assert np.array_equal(rows[2, 0], fg.var_value[0])


# ---------------------------------------------------------------------------------------------- h
def test_refusals_and_lifecycle(golden):
    L = _lib.lib()
    g, hbv = _graph(golden, "hubs")
    nw = len(g[0])
    assert nw >= 3
    _, fg = session(g, seed=SEED, chains=2)
    _, parent = session(g, seed=SEED, chains=2)
    h = fg._engine()
    fg._chains()
    parent._chains()
    for x in (fg, parent):
        assert L.nsk_gibbs_sweeps(x._engine(), 2, 0, 0) == _lib.OK
    assert fg.info()["device_bytes"] == parent.info()["device_bytes"]          # a handle that never asks
    out = np.zeros(8 * nw)
    one = _lib.as_c(np.array([1, 0, 1]), np.int64)
    assert L.nsk_trace_weight_stats(h, None, 0, 0) == _lib.E_INVALID            # no trace
    assert L.nsk_trace_weight_stats(h, None, -1, 0) == _lib.E_INVALID
    assert L.nsk_trace_download_weight_stats(h, 0, 0, _lib.ptr(out)) == _lib.E_INVALID
    assert fg.info()["device_bytes"] == parent.info()["device_bytes"]          # refused calls allocate nothing
    for which in (-1, _lib.BUF_WEIGHT, 7):
        assert L.nsk_weight_stats(h, which, 0, 1, 0, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_weight_stats(h, _lib.BUF_VALUE, 2, 1, 0, _lib.ptr(out)) == _lib.E_INVALID      # chain >= chains
    assert L.nsk_weight_stats(h, _lib.BUF_VALUE, 1, 2, 0, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_weight_stats(h, _lib.BUF_VALUE, -1, 1, 0, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_weight_stats(h, _lib.BUF_VALUE, 0, 0, 0, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_weight_stats(h, _lib.BUF_VALUE_EVID, 1, 1, 0, _lib.ptr(out)) == _lib.E_INVALID # the evidence chain exists once
    assert L.nsk_weight_stats(h, _lib.BUF_VALUE_EVID, 0, 2, 0, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_weight_stats(h, _lib.BUF_VALUE, 0, 2, 0, None) == _lib.E_INVALID               # a null out
    assert fg.info()["device_bytes"] == parent.info()["device_bytes"]
    assert L.nsk_weight_stats(h, _lib.BUF_VALUE, 0, 2, 0, _lib.ptr(out)) == _lib.OK
    grown = fg.info()["device_bytes"] - parent.info()["device_bytes"]
    assert grown >= 4 * len(fg.factor) + 2 * nw * 8                             # the by-weight list, the result (+ records, plan)
    assert L.nsk_weight_stats(h, _lib.BUF_VALUE, 0, 2, 0, _lib.ptr(out)) == _lib.OK
    assert fg.info()["device_bytes"] - parent.info()["device_bytes"] == grown   # nothing more at the next call
    # a trace with the column (the log-potential's own buffers first: they stay once its column was on)
    assert L.nsk_log_potential(h, _lib.BUF_VALUE, 0, 2, _lib.ptr(out)) == _lib.OK
    assert L.nsk_trace_setup(h, None, 0, 2, 4) == _lib.OK
    bytes_trace = fg.info()["device_bytes"]
    bad = _lib.as_c(np.array([0, nw]), np.int64)
    assert L.nsk_trace_weight_stats(h, _lib.ptr(bad), 2, 0) == _lib.E_INDEX
    bad[1] = -1
    assert L.nsk_trace_weight_stats(h, _lib.ptr(bad), 2, 0) == _lib.E_INDEX
    assert L.nsk_trace_weight_stats(h, _lib.ptr(one), 0, 0) == _lib.E_INVALID   # a list needs at least one id
    assert L.nsk_trace_weight_stats(h, None, 2, 0) == _lib.E_INVALID
    assert fg.info()["device_bytes"] == bytes_trace
    assert L.nsk_trace_download_weight_stats(h, 0, 0, _lib.ptr(out)) == _lib.E_INVALID      # no column yet
    assert L.nsk_trace_weight_stats(h, _lib.ptr(one), 3, 0) == _lib.OK
    assert fg.info()["device_bytes"] >= bytes_trace + 4 * 2 * 3 * 8
    with_sel = fg.info()["device_bytes"]
    assert L.nsk_gibbs_sweeps(h, 4, 0, 0) == _lib.OK
    assert L.nsk_trace_download_weight_stats(h, 0, 2, _lib.ptr(out)) == _lib.OK
    now = _stats_of_chains(fg, _lib.BUF_VALUE, 0, 2)
    assert np.array_equal(_bits(out[6:12]), _bits(now[:, [1, 0, 1]].reshape(-1)))
    assert L.nsk_trace_download_weight_stats(h, 0, 3, _lib.ptr(out)) == _lib.E_INVALID      # beyond the rows recorded
    assert L.nsk_trace_download_weight_stats(h, 2, 1, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_trace_download_weight_stats(h, -1, 1, _lib.ptr(out)) == _lib.E_INVALID
    # nsk_trace_clear keeps the column
    assert L.nsk_trace_clear(h) == _lib.OK
    assert L.nsk_trace_download_weight_stats(h, 0, 1, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_gibbs_sweeps(h, 2, 0, 0) == _lib.OK
    assert L.nsk_trace_download_weight_stats(h, 0, 1, _lib.ptr(out)) == _lib.OK
    now = _stats_of_chains(fg, _lib.BUF_VALUE, 0, 2)
    assert np.array_equal(_bits(out[:6]), _bits(now[:, [1, 0, 1]].reshape(-1)))
    # calling it again replaces the column (all weights), independent of the lp column
    assert L.nsk_trace_log_potential(h, 1) == _lib.OK
    assert L.nsk_trace_weight_stats(h, None, 0, 0) == _lib.OK
    assert L.nsk_trace_clear(h) == _lib.OK
    assert L.nsk_gibbs_sweeps(h, 2, 0, 0) == _lib.OK
    assert L.nsk_trace_download_weight_stats(h, 0, 1, _lib.ptr(out)) == _lib.OK
    assert np.array_equal(_bits(out[:2 * nw]), _bits(_stats_of_chains(fg, _lib.BUF_VALUE, 0, 2).reshape(-1)))
    lp = np.zeros(2)
    assert L.nsk_trace_download_log_potential(h, 0, 1, _lib.ptr(lp)) == _lib.OK
    now_lp = np.zeros(2)
    assert L.nsk_log_potential(h, _lib.BUF_VALUE, 0, 2, _lib.ptr(now_lp)) == _lib.OK
    assert np.array_equal(_bits(lp), _bits(now_lp))
    assert L.nsk_trace_log_potential(h, 0) == _lib.OK
    # switched off: the column and its work list go, the trace stays
    assert L.nsk_trace_weight_stats(h, None, -1, 0) == _lib.OK
    assert L.nsk_trace_download_weight_stats(h, 0, 1, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_trace_weight_stats(h, _lib.ptr(one), 3, 0) == _lib.OK
    assert fg.info()["device_bytes"] == with_sel
    # replacing the trace resets the column to off ...
    assert L.nsk_trace_setup(h, None, 0, 1, 2) == _lib.OK
    assert L.nsk_gibbs_sweeps(h, 1, 0, 0) == _lib.OK
    assert L.nsk_trace_download_weight_stats(h, 0, 1, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_trace_weight_stats(h, _lib.ptr(one), 3, 1) == _lib.OK
    # ... and so does tearing it down
    assert L.nsk_trace_setup(h, None, 0, 1, 0) == _lib.OK
    assert L.nsk_trace_weight_stats(h, _lib.ptr(one), 3, 0) == _lib.E_INVALID
    assert L.nsk_trace_download_weight_stats(h, 0, 0, _lib.ptr(out)) == _lib.E_INVALID
    rows = C.c_int64(-1)
    assert L.nsk_trace_rows(h, C.byref(rows), None, None) == _lib.OK and rows.value == 0
    # an own_range handle
    from numbskull_amd.distributed import shard_range
    ns = numbskull_amd.NumbSkull(quiet=True, seed=SEED)
    w, v, f, fm, dm, edges = [x.copy() if isinstance(x, np.ndarray) else x for x in g]
    ns.loadFactorGraph(w, v, f, fm, dm, int(edges), own_range=shard_range(0, 2, len(v)))
    sh = ns.factorGraphs[0]
    assert L.nsk_weight_stats(sh._engine(), _lib.BUF_VALUE, 0, 1, 0, _lib.ptr(out)) == _lib.E_INVALID
    with pytest.raises(ValueError):
        sh.weight_statistics()


@pytest.mark.parametrize("name", ["grid57x33", "lr3000", "gencat_i32", "hubs"])
def test_the_calls_only_read(golden, name):
    L = _lib.lib()
    g, hbv = _graph(golden, name)
    _, a = session(g, seed=SEED, head_by_vid=hbv)
    _, b = session(g, seed=SEED, head_by_vid=hbv)
    for fg in (a, b):
        fg.learn(1, 2, 0.01, 0.95, 2, 0.01, 1)
        fg.inference(1, 4, True)

    def state(fg):
        n, nw = len(fg.variable), len(fg.weight)
        vv, ve, wv, cnt = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(nw), np.zeros(len(fg.count), np.int64)
        _lib.check(L.nsk_state_download(fg._engine(), _lib.ptr(vv), _lib.ptr(ve), _lib.ptr(wv), _lib.ptr(cnt)))
        return vv, ve, wv, cnt, fg.info()["sweeps_done"]

    before = state(a)
    for which in (_lib.BUF_VALUE, _lib.BUF_VALUE_EVID):
        for scaled in (0, 1):
            _stats_of_chains(a, which, 0, 1, scaled)
    for x, y in zip(before, state(a)):
        assert np.array_equal(x, y)
    a.weight_statistics()
    # continuing the chain gives the samples of a twin that never asked
    ra, _ = a.sample(6, thin=2, sample_evidence=True, weight_statistics=[0])
    rb = b.sample(6, thin=2, sample_evidence=True)
    assert np.array_equal(ra, rb)
    assert np.array_equal(a.var_value, b.var_value) and np.array_equal(a.count, b.count)
    a.learn(0, 2, 0.01, 0.95, 2, 0.01, 1)
    b.learn(0, 2, 0.01, 0.95, 2, 0.01, 1)
    assert np.array_equal(a.weight_value, b.weight_value) and np.array_equal(a.var_value_evid, b.var_value_evid)


# ---------------------------------------------------------------------------------------------- i
def test_moment_gap_of_planted_pairs():
    """2000 independent pairs under their planted weights: the mean statistics of 4 chains x 1000 recorded states
    against the exact expectation (enumeration of a pair's four states; module docstring) within 5 standard errors"""
    a_, b_, c_, n = 1.0, 1.0, 0.5, 2000
    g = graphgen.ising_pairs(n, a_, b_, c_, seed=3)
    g[0]["initialValue"] = [a_, b_, c_]
    g[0]["isFixed"] = True
    _, fg = session(g, seed=SEED, chains=4)
    rows, stats = fg.sample(2000, var_ids=[0], thin=2, sample_evidence=True, var_copy="all", weight_statistics=True)
    assert stats.shape == (1000, 4, 3)
    sx, sy = np.array([-1.0, -1.0, 1.0, 1.0]), np.array([-1.0, 1.0, -1.0, 1.0])
    se = np.where(sx == sy, 1.0, -1.0)
    p = np.exp(a_ * sx + b_ * sy + c_ * se)
    p /= p.sum()
    target = n * np.array([(p * sx).sum(), (p * sy).sum(), (p * se).sum()])
    gap, mcse = moment_gap(stats, target)
    print("target", target, "gap", gap, "mcse", mcse, "gap / mcse", gap / mcse)
    assert np.all(np.isfinite(mcse)) and np.all(mcse > 0)
    assert np.all(np.abs(gap) <= 5 * mcse), (gap, mcse)
    # the evidence chain's statistics are one draw of the same distribution: a standard deviation of one state away,
    # which is 'far' on the scale of mcse -- reported, not asserted (module docstring)
    ev = fg.weight_statistics(evidence_chain=True)
    sd = stats.reshape(-1, 3).std(axis=0, ddof=1)
    print("evidence statistics", ev, "(evidence - target) / sd of a state", (ev - target) / sd)
    assert np.all(np.abs(ev - target) <= 5 * sd)
