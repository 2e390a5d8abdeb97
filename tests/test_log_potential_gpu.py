"""Log-potential on the device (nsk_log_potential, nsk_factor_values, the lp column of a sample trace).

Yardsticks: factor values must EQUAL the oracle's eval_factor (oracle.binding.Graph.eval_factor, pinned to the
reference; called with var_samp = the factor's first member and value = that member's current value, which is the
state as it is).  The log-potential is compared with math.fsum of the float64 terms t_f = w_f * e_f under the bound
|lp - ref| <= (nfactor + 1) * 2^-53 * sum |t_f|, which holds for ANY summation order of fewer than 9e7 terms
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd edition, section 4.2: the error of recursive or tree
summation of n terms is at most (n - 1) u sum |t| + O(u^2), u = 2^-53; one more u for the rounding of fsum's result)
-- derived, not measured.  Everything the sum is supposed to be independent of is checked bit for bit."""

import ctypes as C
import math

import numpy as np
import pytest

import numbskull_amd
from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import best_sample
from test_hip_parity import _small_graphs, GRAPHS
from util import session, oracle_of

pytestmark = pytest.mark.gpu

SEED = 77
_CACHE = {}


def _graph(golden, name):
    if not _CACHE:
        _CACHE.update(_small_graphs(golden))
    return _CACHE[name]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _oracle_values(og, state):
    """eval_factor of every factor on `state` through the oracle"""
    state = np.ascontiguousarray(state, np.int64)
    f, vid = og.factor, og.fmap["vid"]
    out = np.zeros(len(f))
    for fid in range(len(f)):
        s, a = int(f[fid]["ftv_offset"]), int(f[fid]["arity"])
        vs = int(vid[s]) if a >= 1 and int(f[fid]["factorFunction"]) != -1 else -1
        rc, out[fid] = og.eval_factor(fid, vs, int(state[vs]) if vs >= 0 else 0, state)
        assert rc == 0, ("oracle refuses factor", fid)
    return out


def _check_lp(lp, e, weights, wid, what):
    t = weights[wid] * e                    # float64 products, rounded once each
    ref = math.fsum(t.tolist())
    bound = (len(t) + 1) * 2.0 ** -53 * math.fsum(np.abs(t).tolist())
    print("%s: lp %.17g ref %.17g |diff| %.3g bound %.3g" % (what, lp, ref, abs(lp - ref), bound))
    assert abs(lp - ref) <= bound, (what, lp, ref, bound)


def _factor_values_of_chain(fg, which, chain):
    out = np.zeros(len(fg.factor), np.float64)
    _lib.check(_lib.lib().nsk_factor_values(fg._engine(), which, chain, _lib.ptr(out)))
    return out


def _lp_of_chains(fg, which, first, n):
    out = np.zeros(n, np.float64)
    _lib.check(_lib.lib().nsk_log_potential(fg._engine(), which, first, n, _lib.ptr(out)))
    return out


# ---------------------------------------------------------------------------------------------- 1 and 2
@pytest.mark.parametrize("name", GRAPHS)
def test_factor_values_equal_the_oracle_and_the_sum_is_within_the_derived_bound(golden, name):
    g, hbv = _graph(golden, name)
    wid = np.asarray(g[2]["weightId"], np.int64)
    # free chain after a few sweeps
    _, fg = session(g, seed=SEED, head_by_vid=hbv)
    og = oracle_of(fg, hbv)
    fg.inference(2, 3, True)
    e = fg.factor_values()
    assert e.shape == (len(fg.factor),) and e.dtype == np.float64
    assert np.array_equal(e, _oracle_values(og, fg.var_value[0])), name
    _check_lp(fg.log_potential(), e, fg.weight_value[0], wid, name + " free")
    # evidence chain (and learned weights) after a few learning sweeps
    fg.learn(1, 3, 0.01, 0.95, 2, 0.01, 1)
    e = fg.factor_values(evidence_chain=True)
    assert np.array_equal(e, _oracle_values(og, fg.var_value_evid[0])), name
    _check_lp(fg.log_potential(evidence_chain=True), e, fg.weight_value[0], wid, name + " evidence")
    e = fg.factor_values()
    assert np.array_equal(e, _oracle_values(og, fg.var_value[0])), name
    _check_lp(fg.log_potential(), e, fg.weight_value[0], wid, name + " free after learning")
    # every chain of a 3-chain handle
    _, f3 = session(g, seed=SEED, head_by_vid=hbv, chains=3)
    f3.inference(2, 3, True, var_copy="all")
    lp = f3.log_potential(var_copy="all")
    assert lp.shape == (3,) and lp.dtype == np.float64
    for r in range(3):
        e = _factor_values_of_chain(f3, _lib.BUF_VALUE, r)
        assert np.array_equal(e, _oracle_values(og, f3.var_value[r])), (name, r)
        _check_lp(lp[r], e, f3.weight_value[0], wid, "%s chain %d" % (name, r))
        assert _bits(_lp_of_chains(f3, _lib.BUF_VALUE, r, 1))[0] == _bits(lp)[r]       # (a sub-range of the chains)


# ---------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", GRAPHS)
def test_the_sum_is_reproducible_bit_for_bit(golden, name):
    g, hbv = _graph(golden, name)
    _, src = session(g, seed=SEED, head_by_vid=hbv)
    src.inference(1, 2, True)
    x = src.var_value[0].copy()
    _, one = session(g, seed=SEED + 1, head_by_vid=hbv)
    one.var_value[0][:] = x
    lp1 = one.log_potential()
    assert isinstance(lp1, float)
    assert _bits(one.log_potential())[0] == _bits(lp1)[0]                               # two consecutive calls
    _, three = session(g, seed=SEED + 2, head_by_vid=hbv, chains=3)
    three.inference(0, 2, True, var_copy="all")
    three.var_value[0][:] = x
    three.var_value[2][:] = x
    lp3 = three.log_potential(var_copy="all")
    assert _bits(lp3)[0] == _bits(lp1)[0] and _bits(lp3)[2] == _bits(lp1)[0], (lp1, lp3)
    assert np.array_equal(_bits(three.log_potential(var_copy="all")), _bits(lp3))
    # the evidence chain, after nsk_state_upload of the same array
    one.var_value_evid[0][:] = x
    assert _bits(one.log_potential(evidence_chain=True))[0] == _bits(lp1)[0]
    # ... and through the C-ABI on the one-chain handle as it stands
    assert _bits(_lp_of_chains(one, _lib.BUF_VALUE_EVID, 0, 1))[0] == _bits(lp1)[0]
    assert _bits(_lp_of_chains(one, _lib.BUF_VALUE, 0, 1))[0] == _bits(lp1)[0]


# ---------------------------------------------------------------------------------------------- 4
def _twin_lp(tw, state):
    tw.var_value[0][:] = state
    return tw.log_potential()


@pytest.mark.parametrize("name", ["grid57x33", "lr3000", "gencat_i32", "hubs"])
@pytest.mark.parametrize("nchains", [1, 3])
@pytest.mark.parametrize("thin", [1, 3])
def test_trace_rows_carry_the_log_potential_of_their_state(golden, name, nchains, thin):
    g, hbv = _graph(golden, name)
    vc = "all" if nchains > 1 else 0
    _, a = session(g, seed=SEED, head_by_vid=hbv, chains=nchains)
    _, b = session(g, seed=SEED, head_by_vid=hbv, chains=nchains)
    _, c = session(g, seed=SEED, head_by_vid=hbv, chains=nchains)
    _, tw = session(g, seed=SEED, head_by_vid=hbv)
    rows, lp = a.sample(10, thin=thin, burnin_epochs=2, sample_evidence=True, var_copy=vc, log_potential=True)
    plain = b.sample(10, thin=thin, burnin_epochs=2, sample_evidence=True, var_copy=vc)
    assert isinstance(plain, np.ndarray)
    assert rows.dtype == plain.dtype and np.array_equal(rows, plain)
    assert lp.shape == (10 // thin, nchains) and lp.dtype == np.float64
    for i in range(rows.shape[0]):
        for r in range(nchains):
            assert _bits(lp[i, r])[0] == _bits(_twin_lp(tw, rows[i, r]))[0], ("row", i, "chain", r)
    # the flagged call leaves what the unflagged one leaves
    assert np.array_equal(a.var_value, b.var_value) and np.array_equal(a.count, b.count)
    assert np.array_equal(a.chain_count, b.chain_count)
    assert a.info()["sweeps_done"] == b.info()["sweeps_done"]
    # a column subset keeps the same lp column (it speaks of the whole state)
    ids = [len(a.variable) - 1, 3, 0, 3]
    sub, lp_sub = c.sample(10, var_ids=ids, thin=thin, burnin_epochs=2, sample_evidence=True, var_copy=vc,
                           log_potential=True)
    assert np.array_equal(sub, rows[:, :, ids])
    assert np.array_equal(_bits(lp_sub), _bits(lp))
    # no columns at all: the rows are empty, the lp column is not
    _, d = session(g, seed=SEED, head_by_vid=hbv, chains=nchains)
    none, lp_none = d.sample(10, var_ids=[], thin=thin, burnin_epochs=2, sample_evidence=True, var_copy=vc,
                             log_potential=True)
    assert none.shape == (10 // thin, nchains, 0)
    assert np.array_equal(_bits(lp_none), _bits(lp))
    assert best_sample(lp) == tuple(int(k) for k in np.unravel_index(np.argmax(lp), lp.shape))


# ---------------------------------------------------------------------------------------------- 5
def test_packed_tally_rows_of_the_million_grid():
    """a one-chain handle of wide quads keeps its tally in bits 1-7 of the value bytes between the runs of a traced
    call: the lp column must read bit 0 only"""
    g = graphgen.ising_grid(1000, 1000, weight=0.3)
    _, fg = session(g, seed=SEED)
    _, tw = session(g, seed=SEED)
    assert fg.info()["wide_quads"] > 0
    before = fg.info()["device_bytes"]
    rows, lp = fg.sample(12, thin=4, log_potential=True)
    assert fg.info()["device_bytes"] > before           # the factor records went up, and are reported
    assert rows.shape == (3, 1, 10 ** 6) and lp.shape == (3, 1)
    assert rows.min() == 0 and rows.max() == 1
    for i in range(3):
        assert _bits(lp[i, 0])[0] == _bits(_twin_lp(tw, rows[i, 0]))[0], ("row", i)
    assert np.array_equal(rows[2, 0], fg.var_value[0])
    # the final state against numpy on the grid's factors
    x = fg.var_value[0]
    vid = g[3]["vid"]
    e = np.where(x[vid[0::2]] == x[vid[1::2]], 1.0, -1.0)
    wid = np.asarray(g[2]["weightId"], np.int64)
    final = fg.log_potential()
    _check_lp(final, e, fg.weight_value[0], wid, "1M grid")
    assert _bits(final)[0] == _bits(lp[2, 0])[0]


# ---------------------------------------------------------------------------------------------- 6
def test_refusals_and_lifecycle(golden):
    L = _lib.lib()
    g, hbv = _graph(golden, "grid57x33")
    _, fg = session(g, seed=SEED, chains=2)
    h = fg._engine()
    fg._chains()
    out = np.zeros(8)
    assert L.nsk_trace_log_potential(h, 1) == _lib.E_INVALID            # no trace
    assert L.nsk_trace_log_potential(h, 0) == _lib.E_INVALID
    assert L.nsk_trace_download_log_potential(h, 0, 0, _lib.ptr(out)) == _lib.E_INVALID
    for which in (-1, _lib.BUF_WEIGHT, 7):
        assert L.nsk_log_potential(h, which, 0, 1, _lib.ptr(out)) == _lib.E_INVALID
        assert L.nsk_factor_values(h, which, 0, _lib.ptr(np.zeros(len(fg.factor)))) == _lib.E_INVALID
    assert L.nsk_log_potential(h, _lib.BUF_VALUE, 2, 1, _lib.ptr(out)) == _lib.E_INVALID       # chain >= chains
    assert L.nsk_log_potential(h, _lib.BUF_VALUE, 1, 2, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_log_potential(h, _lib.BUF_VALUE, -1, 1, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_log_potential(h, _lib.BUF_VALUE, 0, 0, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_log_potential(h, _lib.BUF_VALUE_EVID, 1, 1, _lib.ptr(out)) == _lib.E_INVALID  # the evidence chain exists once
    assert L.nsk_log_potential(h, _lib.BUF_VALUE_EVID, 0, 2, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_factor_values(h, _lib.BUF_VALUE, 2, _lib.ptr(np.zeros(len(fg.factor)))) == _lib.E_INVALID
    assert L.nsk_log_potential(h, _lib.BUF_VALUE, 0, 2, _lib.ptr(out)) == _lib.OK
    # a trace with the column: rows beyond those recorded
    assert L.nsk_trace_setup(h, None, 0, 2, 4) == _lib.OK
    bytes_trace = fg.info()["device_bytes"]
    assert L.nsk_trace_log_potential(h, 1) == _lib.OK
    assert fg.info()["device_bytes"] == bytes_trace + 4 * 2 * 8
    assert L.nsk_gibbs_sweeps(h, 4, 0, 0) == _lib.OK
    assert L.nsk_trace_download_log_potential(h, 0, 2, _lib.ptr(out)) == _lib.OK
    first = out[:4].copy()
    assert np.array_equal(_bits(first[2:]), _bits(_lp_of_chains(fg, _lib.BUF_VALUE, 0, 2)))
    assert L.nsk_trace_download_log_potential(h, 0, 3, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_trace_download_log_potential(h, 2, 1, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_trace_download_log_potential(h, -1, 1, _lib.ptr(out)) == _lib.E_INVALID
    # nsk_trace_clear keeps the column
    assert L.nsk_trace_clear(h) == _lib.OK
    assert L.nsk_trace_download_log_potential(h, 0, 1, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_gibbs_sweeps(h, 2, 0, 0) == _lib.OK
    assert L.nsk_trace_download_log_potential(h, 0, 1, _lib.ptr(out)) == _lib.OK
    assert np.array_equal(_bits(out[:2]), _bits(_lp_of_chains(fg, _lib.BUF_VALUE, 0, 2)))
    # switched off: the buffer goes, the trace stays
    assert L.nsk_trace_log_potential(h, 0) == _lib.OK
    assert fg.info()["device_bytes"] == bytes_trace
    assert L.nsk_trace_download_log_potential(h, 0, 1, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_trace_log_potential(h, 1) == _lib.OK
    # replacing the trace resets the column to off ...
    assert L.nsk_trace_setup(h, None, 0, 1, 2) == _lib.OK
    assert L.nsk_gibbs_sweeps(h, 1, 0, 0) == _lib.OK
    assert L.nsk_trace_download_log_potential(h, 0, 1, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_trace_log_potential(h, 1) == _lib.OK
    # ... and so does tearing it down: the buffer is gone, an untraced call works and records nothing
    with_lp = fg.info()["device_bytes"]
    assert L.nsk_trace_setup(h, None, 0, 1, 0) == _lib.OK
    assert fg.info()["device_bytes"] < with_lp
    assert L.nsk_gibbs_sweeps(h, 3, 0, 0) == _lib.OK
    rows = C.c_int64(-1)
    assert L.nsk_trace_rows(h, C.byref(rows), None, None) == _lib.OK and rows.value == 0
    assert L.nsk_trace_log_potential(h, 1) == _lib.E_INVALID
    assert L.nsk_trace_download_log_potential(h, 0, 0, _lib.ptr(out)) == _lib.E_INVALID
    # an own_range handle
    from numbskull_amd.distributed import shard_range
    ns = numbskull_amd.NumbSkull(quiet=True, seed=SEED)
    w, v, f, fm, dm, edges = [x.copy() if isinstance(x, np.ndarray) else x for x in g]
    ns.loadFactorGraph(w, v, f, fm, dm, int(edges), own_range=shard_range(0, 2, len(v)))
    sh = ns.factorGraphs[0]
    assert L.nsk_log_potential(sh._engine(), _lib.BUF_VALUE, 0, 1, _lib.ptr(out)) == _lib.E_INVALID
    assert L.nsk_factor_values(sh._engine(), _lib.BUF_VALUE, 0, _lib.ptr(np.zeros(len(f)))) == _lib.E_INVALID
    with pytest.raises(Exception):
        sh.log_potential()


# ---------------------------------------------------------------------------------------------- 7
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
    h = a._engine()
    out, ev = np.zeros(1), np.zeros(len(a.factor))
    for which in (_lib.BUF_VALUE, _lib.BUF_VALUE_EVID):
        assert L.nsk_log_potential(h, which, 0, 1, _lib.ptr(out)) == _lib.OK
        assert L.nsk_factor_values(h, which, 0, _lib.ptr(ev)) == _lib.OK
    after = state(a)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    a.log_potential()
    a.factor_values()
    # continuing the chain gives the samples of a twin that never asked
    ra = a.sample(6, thin=2, sample_evidence=True)
    rb = b.sample(6, thin=2, sample_evidence=True)
    assert np.array_equal(ra, rb)
    assert np.array_equal(a.var_value, b.var_value) and np.array_equal(a.count, b.count)
    assert np.array_equal(a.weight_value, b.weight_value)
    a.learn(0, 2, 0.01, 0.95, 2, 0.01, 1)
    b.learn(0, 2, 0.01, 0.95, 2, 0.01, 1)
    assert np.array_equal(a.weight_value, b.weight_value) and np.array_equal(a.var_value_evid, b.var_value_evid)


def test_a_handle_that_never_asks_holds_nothing_for_it(golden):
    g, hbv = _graph(golden, "grid57x33")
    _, a = session(g, seed=SEED)
    _, b = session(g, seed=SEED)
    a.inference(1, 3, True)
    b.inference(1, 3, True)
    assert a.info()["device_bytes"] == b.info()["device_bytes"]
    b.log_potential()
    grown = b.info()["device_bytes"] - a.info()["device_bytes"]
    nf, ne = len(b.factor), len(b.fmap)
    assert grown >= 16 * nf + 8 * ne            # f_rec, m_rec (+ v_card, the partials)
    b.log_potential()
    b.factor_values()
    assert b.info()["device_bytes"] - a.info()["device_bytes"] == grown     # nothing more at the next calls
