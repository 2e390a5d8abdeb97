"""PCD with latent variables on the device against the oracle (nsk_pcd_latent_steps, FactorGraph.learn_pcd(clamped=K) /
weight_moments(chains=...); tests/pcd_latent.py has the graphs and the mirror, tests/test_pcd_latent_cpu.py holds the numpy
rule to a hand-written loop, shows that every case here is lively in the mirror and that the learner raises the exact
likelihood of the evidence with the oracle as the sampler).

Every check is bit for bit: equality for the states and the int64 moments, uint64 views for gmax and the weights, and
sweeps_done == s0 + 2 k nsteps.  A population of several chains takes the batched chain launches where the graph lives in
table segments and sweeps chain after chain elsewhere (pcd_latent.BATCHED; asserted from launch counts below); a
population of one takes the one-chain launches."""

import ctypes as C

import numpy as np
import pytest

import numbskull_amd
from numbskull_amd import _lib, graphgen
import pcd
import pcd_latent as pl
import wide_trips
from util import session, oracle_of, phases_from_colors

pytestmark = pytest.mark.gpu

SEED = pl.SEED


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class Handle(object):
    """A resident handle with R chains, all at the initial values, and its oracle"""

    def __init__(self, name, R, seed=SEED, graph=None, hbv=False):
        if graph is None:
            build, hbv, _ = pcd.GRAPHS[name]
            graph = build()
        self.seed, self.R = seed, R
        _, self.fg = session(graph, seed=seed, head_by_vid=hbv)
        fg = self.fg
        self.og = oracle_of(fg, hbv)
        self.color = fg.colors()
        self.L, self.h = _lib.lib(), fg._engine()
        fg._push(0, 0)                      # the one full upload
        if R > 1:
            _lib.check(self.L.nsk_set_chains(self.h, R))
        vv, _, self.w0, _ = self.og.initial_state()
        self.x0 = [vv.copy() for _ in range(R)]
        self.nvar, self.nw = len(vv), len(self.w0)
        self.free = ~self.og.weight["isFixed"].astype(bool)
        self.ev = pl.evidence_mask(self.og)
        self.init = self.og.variable["initialValue"].astype(np.int64)

    def close(self):
        self.fg.close()

    def values(self):
        out = np.empty((self.R, self.nvar), np.int64)
        _lib.check(self.L.nsk_chains_download(self.h, _lib.ptr(out), None))
        return out

    def weights(self):
        w = np.empty(self.nw, np.float64)
        _lib.check(self.L.nsk_state_download(self.h, None, None, _lib.ptr(w), None))
        return w

    def tallies(self):
        out = np.empty((self.R, int(self.og.cstart[-1])), np.int64)
        _lib.check(self.L.nsk_chains_download(self.h, None, _lib.ptr(out)))
        return out

    def info(self, key):
        return self.fg.info()[key]

    def disturb(self):
        """two nsk_gibbs_sweeps(h, 2, 1, 1) calls and their mirror: (rows, sweep index)"""
        for n in pl.DISTURB:
            _lib.check(self.L.nsk_gibbs_sweeps(self.h, n, 1, 1))
        return pl.disturbed(self.og, self.color, self.seed, self.x0, self.w0)

    def latent(self, K, clamp, nsteps, sps, free_se, step, decay, reg, normalize, outputs=True):
        gmax = np.full(nsteps, np.nan) if outputs else None
        rows = np.full((nsteps, 2, self.nw), -1, np.int64) if outputs else None
        rc = self.L.nsk_pcd_latent_steps(self.h, K, clamp, nsteps, sps, free_se, step, decay, reg, normalize, _lib.ptr(gmax), _lib.ptr(rows))
        return rc, gmax, rows

    def launches(self, call):
        """the sweep-kernel launches of ``call()`` (nsk_profile_begin / end)"""
        ms, n = C.c_double(), C.c_int64()
        _lib.check(self.L.nsk_profile_begin(self.h))
        call()
        _lib.check(self.L.nsk_profile_end(self.h, C.byref(ms), C.byref(n)))
        return n.value

    def same_values(self, want, what):
        got = self.values()
        for r in range(self.R):
            bad = np.nonzero(got[r] != want[r])[0]
            assert len(bad) == 0, (what, "chain", r, "differing variables", len(bad), bad[:12])


def _one_call(H, x, w, sweep, K, nsteps, sps, normalize, reg, what, clamp=1, free_se=1, values=pcd.factor_values):
    """one nsk_pcd_latent_steps call against the mirror started at (x, w, sweep); returns the mirror"""
    step = pcd.stepsize(normalize)
    done0 = H.info("sweeps_done")
    rc, gmax, rows = H.latent(K, clamp, nsteps, sps, free_se, step, pl.DECAY, reg, normalize)
    _lib.check(rc)
    m = pl.Run(H.og, H.color, H.seed, x, w, K, nsteps, sps, free_se, step, pl.DECAY, reg, normalize, sweep0=sweep, clamp=bool(clamp), values=values)
    for t in range(nsteps):
        assert np.array_equal(rows[t], m.moments[t]), (what, "moments of step", t, rows[t], m.moments[t])
    assert np.array_equal(_bits(gmax), _bits(m.gmax)), (what, gmax, m.gmax)
    got = H.weights()
    assert np.array_equal(_bits(got), _bits(m.w)), (what, got, m.w)
    assert np.array_equal(_bits(got[~H.free]), _bits(H.w0[~H.free]))
    H.same_values(m.final, what)
    assert H.info("sweeps_done") == done0 + 2 * sps * nsteps
    assert m.sweep == sweep + 2 * sps * nsteps
    assert (m.w[H.free] != np.asarray(w)[H.free]).any() and (rows[:, 0] != rows[:, 1]).any(), "the case stands still"
    return m


def _one_sweep_launches(graph, hbv, n, se):
    """the sweep-kernel launches of ONE plain burn-in sweep of an n-chain handle: the existing entry point"""
    _, fg = session(graph, seed=SEED, head_by_vid=hbv)
    try:
        L, h = _lib.lib(), fg._engine()
        fg._push(0, 0)
        if n > 1:
            _lib.check(L.nsk_set_chains(h, n))
        ms, count = C.c_double(), C.c_int64()
        _lib.check(L.nsk_profile_begin(h))
        _lib.check(L.nsk_gibbs_sweeps(h, 1, se, 1))
        _lib.check(L.nsk_profile_end(h, C.byref(ms), C.byref(count)))
        return count.value
    finally:
        fg.close()


# ------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("RK", pl.PARITY_CHAINS, ids=lambda rk: "R%d_K%d" % rk)
@pytest.mark.parametrize("name", pl.PARITY_GRAPHS)
def test_parity_with_the_mirror(name, RK):
    R, K = RK
    H = Handle(name, R)
    try:
        if name == "grid_int32":
            assert H.info("value_bytes") == 4
        x, sweep = H.disturb()
        assert any((r[H.ev] != H.init[H.ev]).any() for r in x[:K]), "nothing for the clamp to restore"
        w = H.w0
        for k, (sps, normalize, reg) in enumerate(pl.parity_calls(name, RK)):
            m = _one_call(H, x, w, sweep, K, pl.STEPS, sps, normalize, reg, (name, RK, "call", k))
            x, w, sweep = m.final, m.w, m.sweep
            for r in range(K):
                assert np.array_equal(x[r][H.ev], H.init[H.ev])
    finally:
        H.close()


@pytest.mark.parametrize("name", pl.PARITY_GRAPHS)
def test_which_launches_the_parity_graphs_take(name):
    """pl.BATCHED from launch counts: a population of two takes the launches of one chain where one class launch serves
    every chain, twice as many where it sweeps chain after chain -- so both paths are among the parity cases"""
    build, hbv, _ = pcd.GRAPHS[name]
    for se in (0, 1):
        one, two = _one_sweep_launches(build(), hbv, 1, se), _one_sweep_launches(build(), hbv, 2, se)
        assert one > 0 and two == (one if pl.BATCHED[name] else 2 * one), (name, se, one, two)


def test_the_update_across_a_block_edge():
    """pl.edge_graph(): NSK_BLOCK + 1 = 257 weights, so k_pcd_update's second block holds slot 256 alone; slot 255, the first
    block's last lane, and two more are fixed.  2 clamped chains + 1 free one, 2 steps: weights, gmax and both rows of
    moments are the mirror's bit for bit, and weights on both sides of the edge move (tests/test_pcd_latent_cpu.py: the
    mirror alone says so)."""
    R, K = pl.EDGE_RK
    H = Handle(None, R, graph=pl.edge_graph(), hbv=True)
    try:
        fixed = list(pl.EDGE_FIXED)
        assert H.nw == pl.EDGE_WEIGHTS == 257 and not H.free[fixed].any() and H.free[256]
        assert np.array_equal(H.fg.weight_slots()[fixed], fixed)        # a fixed weight's slot is its id
        x, sweep = H.disturb()
        m = _one_call(H, x, H.w0, sweep, K, pl.EDGE_STEPS, 1, 1, 0.01, "block edge")
        assert (m.moments[0] != m.moments[1]).any(), "the case stands still"
        assert (m.w[:256] != H.w0[:256]).any() and m.w[256] != H.w0[256]
    finally:
        H.close()


# ------------------------------------------------------------------------------------------------------- 2. the launches
@pytest.mark.parametrize("RK", [(4, 2), (3, 1)], ids=lambda rk: "R%d_K%d" % rk)
def test_both_launch_paths_by_their_launch_counts(RK, monkeypatch):
    """28 x 1000, the lower half of the rows evidence, two free weights, wide quads switched on as in tests/wide_trips.py
    (tests/test_pcd_latent_cpu.py: every variable routes to a table).  The call's sweep-kernel launches are those of the
    two populations as handles of their own: nsteps k (L0(K) + L1(R - K)); a population of two takes one chain's
    launches, L(2) == L(1).  States, moments and weights are the mirror's."""
    for k, v in wide_trips.ENV.items():
        monkeypatch.setenv(k, v)
    R, K = RK
    nsteps, sps = 3, 2
    L = {(n, se): _one_sweep_launches(pl.launch_graph(), False, n, se) for n in (1, 2) for se in (0, 1)}
    assert L[2, 0] == L[1, 0] > 0 and L[2, 1] == L[1, 1] > 0, L
    H = Handle(None, R, graph=pl.launch_graph())
    try:
        assert H.nw == 2 and H.free.all() and H.info("value_bytes") == 1
        x, sweep = H.disturb()
        got = []
        count = H.launches(lambda: got.append(_one_call(H, x, H.w0, sweep, K, nsteps, sps, 1, 0.01, ("launch grid", RK), values=pl.equal_values)))
        assert count == nsteps * sps * (L[K, 0] + L[R - K, 1]), (count, L)
        # a plain call on the whole handle behind it: the plans and the tables are the whole handle's again
        m = got[0]
        _lib.check(H.L.nsk_gibbs_sweeps(H.h, 2, 1, 1))
        order, ps = phases_from_colors(H.color)
        cnt = np.zeros(int(H.og.cstart[-1]), np.int64)
        for r in range(R):
            for s in range(2):
                assert H.og.gibbs_dev(order, ps, m.final[r], m.w, cnt, H.seed ^ (r << 32), m.sweep + s, True, burnin=True) == 0
        H.same_values(m.final, "a plain sweep call behind the latent call")
    finally:
        H.close()


# ------------------------------------------------------------------------------------------------------- 3. around the call
def test_the_handle_afterwards():
    """grid16x1000 with two evidence rows, 3 chains, K = 1: 80 tallied sweeps with a trace (captured sequences of both
    sizes), a latent call, 80 tallied sweeps -- states and per-chain tallies are the oracle's for all 160 sweeps, the
    weights changing in between; the trace rows are untouched by the call; device_bytes is what it was, once warmed"""
    H = Handle(None, 3, graph=pl.handle_graph())
    try:
        L, h, R, se, K = H.L, H.h, H.R, 1, 1
        order, ps = phases_from_colors(H.color)
        cnt = [np.zeros(int(H.og.cstart[-1]), np.int64) for _ in range(R)]
        x, w = [s.copy() for s in H.x0], H.w0
        sweep = 0

        def tallied(n):
            nonlocal sweep
            _lib.check(L.nsk_gibbs_sweeps(h, n, se, 0))
            for r in range(R):
                for s in range(n):
                    assert H.og.gibbs_dev(order, ps, x[r], w, cnt[r], H.seed ^ (r << 32), sweep + s, True, burnin=False) == 0
            sweep += n

        def trace():
            rows, cap, packed = C.c_int64(), C.c_int64(), C.c_int64()
            _lib.check(L.nsk_trace_rows(h, C.byref(rows), C.byref(cap), C.byref(packed)))
            out, idx = np.zeros((rows.value, R, len(vids)), np.int8), np.zeros(rows.value, np.int64)
            _lib.check(L.nsk_trace_download(h, 0, rows.value, _lib.ptr(out), _lib.ptr(idx)))
            return out, idx

        vids = np.arange(0, H.nvar, 37, dtype=np.int64)
        _lib.check(L.nsk_trace_setup(h, _lib.ptr(vids), len(vids), 80, 4))      # a row every 80 sweeps: one run of 64 + 16
        tallied(80)
        rows0, idx0 = trace()
        assert len(rows0) == 1 and rows0.any()
        S = np.zeros((R, H.nw))
        _lib.check(L.nsk_weight_stats(h, _lib.BUF_VALUE, 0, R, 0, _lib.ptr(S)))         # warm: what a nsk_weight_stats call leaves
        H.values()                                                                     # ... and the staging of the state transfers
        H.weights()
        bytes0 = H.info("device_bytes")
        m = _one_call(H, x, w, sweep, K, 3, 2, 1, 0.01, "between the tallied sweeps", values=pl.equal_values)
        assert H.info("device_bytes") == bytes0
        assert H.info("sweeps_done") == 80 + 12
        rows1, idx1 = trace()
        assert np.array_equal(rows1, rows0) and np.array_equal(idx1, idx0)
        x, w, sweep = [s.copy() for s in m.final], m.w, m.sweep
        assert _bits(w[0]) != _bits(H.w0[0])
        tallied(80)                                             # ... under the learned weights, captured afresh or still valid
        rows2, idx2 = trace()
        assert len(rows2) == 2 and np.array_equal(rows2[:1], rows0) and idx2[0] == idx0[0] and idx2[1] == idx0[0] + 12 + 80
        for r in range(R):
            assert np.array_equal(rows2[1, r], x[r][vids])
        H.same_values(x, "after the second tallied call")
        got = H.tallies()
        assert np.array_equal(got, np.stack(cnt)) and got.max() > 0
        assert np.array_equal(_bits(H.weights()), _bits(w))
    finally:
        H.close()


# ------------------------------------------------------------------------------------------------------- 4. clamp
@pytest.mark.parametrize("clamp", [1, 0])
def test_clamp(clamp):
    """clamp = 1: the clamped rows' evidence variables read initialValue after every call and the free rows' do not;
    clamp = 0: the disturbed rows are kept and the mirror without the reset matches"""
    H = Handle("mixed_clamped", 5)
    try:
        K = 2
        x, sweep = H.disturb()
        held = [r[H.ev].copy() for r in x[:K]]
        assert any((e != H.init[H.ev]).any() for e in held)
        w = H.w0
        for k in range(2):
            m = _one_call(H, x, w, sweep, K, pl.STEPS, 1, 1, 0.01, ("clamp", clamp, "call", k), clamp=clamp)
            x, w, sweep = m.final, m.w, m.sweep
            got = H.values()
            for r in range(K):
                assert np.array_equal(got[r][H.ev], H.init[H.ev] if clamp else held[r]), (r, k)
            # (three evidence variables: a free row now and then meets their initial values, not all three rows at once)
            assert not all((r[H.ev] == H.init[H.ev]).all() for r in got[K:])
            assert m.restored == (bool(clamp) and k == 0)
    finally:
        H.close()


# ------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_handle_as_it_was():
    H = Handle("grid_w0.6_clamped", 3)
    try:
        L, h = H.L, H.h
        _lib.check(L.nsk_gibbs_sweeps(h, 2, 1, 1))
        v0, w0, done0 = H.values(), H.weights(), H.info("sweeps_done")

        def call(K=1, clamp=1, nsteps=3, sps=1, se=1, step=0.1, decay=0.9, reg=0.0, normalize=1, handle=h):
            return L.nsk_pcd_latent_steps(handle, K, clamp, nsteps, sps, se, step, decay, reg, normalize, None, None)

        assert call(handle=None) == _lib.E_INVALID
        for K in (0, 3, -1, 4):
            assert call(K=K) == _lib.E_INVALID, K
        assert "nclamped" in L.nsk_last_error().decode()
        for bad in (2, -1):
            assert call(clamp=bad) == _lib.E_INVALID and call(normalize=bad) == _lib.E_INVALID
        for n in (0, -1, 65537):
            assert call(nsteps=n) == _lib.E_INVALID
        assert call(sps=0) == _lib.E_INVALID and call(sps=-3) == _lib.E_INVALID
        assert call(sps=(2 ** 31 - 1) // 6 + 1) == _lib.E_INVALID              # 2 nsteps k > 2^31 - 1
        for bad in (float("nan"), float("inf")):
            assert call(step=bad) == _lib.E_INVALID and call(decay=bad) == _lib.E_INVALID and call(reg=bad) == _lib.E_INVALID
        assert call(reg=-1e-3) == _lib.E_INVALID
        assert np.array_equal(H.values(), v0) and np.array_equal(_bits(H.weights()), _bits(w0))
        assert H.info("sweeps_done") == done0
        # optional outputs may be NULL
        assert call() == _lib.OK
        assert H.info("sweeps_done") == done0 + 6 and _bits(H.weights()[0]) != _bits(w0[0])
    finally:
        H.close()
    # one chain: no free population
    H = Handle("grid_w0.6_clamped", 1)
    try:
        for K in (0, 1):
            assert H.latent(K, 1, 2, 1, 1, 0.1, 1.0, 0.0, 1)[0] == _lib.E_INVALID
        # the sequential scan
        _lib.check(H.L.nsk_set_scan(H.h, _lib.SCAN_SEQUENTIAL))
        assert H.latent(1, 1, 2, 1, 1, 0.1, 1.0, 0.0, 1)[0] == _lib.E_INVALID
        assert "sequential" in H.L.nsk_last_error().decode()
        assert H.info("sweeps_done") == 0 and np.array_equal(_bits(H.weights()), _bits(H.w0))
    finally:
        H.close()
    # a handle energy_whole_graph refuses: an own_range shard
    from numbskull_amd.distributed import shard_range
    ns = numbskull_amd.NumbSkull(quiet=True, seed=SEED)
    w, v, f, fm, dm, edges = [a.copy() if isinstance(a, np.ndarray) else a for a in graphgen.ising_grid(8, 8, weight=0.3)]
    ns.loadFactorGraph(w, v, f, fm, dm, int(edges), own_range=shard_range(0, 2, len(v)))
    sh = ns.factorGraphs[0]
    try:
        assert _lib.lib().nsk_pcd_latent_steps(sh._engine(), 1, 1, 1, 1, 1, 0.1, 1.0, 0.0, 1, None, None) == _lib.E_INVALID
    finally:
        sh.close()


# ------------------------------------------------------------------------------------------------------- 6. the range rule
def test_the_range_rule():
    """B_0 = 1e6 a UFO factor; (R, K) = (3, 1): the larger population has two chains, so 536 factors pass and 537 do not"""
    assert 536 * 2e6 < 2 ** 30 <= 537 * 2e6
    for n, want in ((536, _lib.OK), (537, _lib.E_RANGE)):
        H = Handle(None, 3, graph=pcd.ufo_graph(n))
        try:
            v0, w0 = H.values(), H.weights()
            rc = H.latent(1, 1, 1, 1, 1, 0.1, 1.0, 0.0, 1, outputs=False)[0]
            assert rc == want, (n, rc)
            if want != _lib.OK:
                assert "2^30" in H.L.nsk_last_error().decode()
                assert np.array_equal(H.values(), v0) and np.array_equal(_bits(H.weights()), _bits(w0)) and H.info("sweeps_done") == 0
        finally:
            H.close()


# ------------------------------------------------------------------------------------------------------- 7. the Python API
def test_learn_pcd_with_clamped_rows_is_the_mirror():
    build, hbv, _ = pcd.GRAPHS["mixed_clamped"]
    _, fg = session(build(), seed=5, head_by_vid=hbv, chains=8)
    try:
        og, color = oracle_of(fg, hbv), fg.colors()
        w0, count0 = og.initial_state()[2], fg.count.copy()
        # rows that differ from the initial values, so that the clamp has something to restore
        fg.var_value[:] = np.random.default_rng(8).integers(0, 2, fg.var_value.shape)
        x0 = fg.var_value.copy()
        res = fg.learn_pcd(5, 0.3, decay=0.9, reg_param=0.01, sweeps=2, sample_evidence=True, moments=True, clamped=3)
        m = pl.Run(og, color, 5, x0, w0, 3, 5, 2, True, 0.3, 0.9, 0.01, 1)
        assert m.restored
        assert sorted(res) == sorted(["grad_max", "target", "chains", "factors_per_weight", "moments", "clamped"])
        assert res["target"] is None and res["chains"] == 8 and res["clamped"] == 3
        assert np.array_equal(_bits(fg.weight_value[0]), _bits(m.w)) and np.array_equal(fg.var_value, np.stack(m.final))
        assert np.array_equal(_bits(res["grad_max"]), _bits(m.gmax))
        assert res["moments"].shape == (5, 2, len(w0)) and res["moments"].dtype == np.int64 and np.array_equal(res["moments"], m.moments)
        assert np.array_equal(fg.count, count0) and (m.w != w0).any()
        Mc, Kc = fg.weight_moments(chains=(0, 3), counts=True)
        Mf, Kf = fg.weight_moments(chains=(3, 5), counts=True)
        assert (Kc, Kf) == (3, 5) and np.array_equal(Mc, m.moments[-1, 0]) and np.array_equal(Mf, m.moments[-1, 1])
        assert np.array_equal(_bits(fg.weight_moments(chains=(3, 5))), _bits(Mf.astype(np.float64) * 2.0 ** -32 / 5.0))
        # clamp=False and the flags: the mirror without the reset, from where the first call ended
        x1, w1 = fg.var_value.copy(), fg.weight_value[0].copy()
        res = fg.learn_pcd(2, 0.03, normalize=False, sample_evidence=False, clamped=7, clamp=False)
        m2 = pl.Run(og, color, 5, x1, w1, 7, 2, 1, False, 0.03, 1.0, 0.0, 0, sweep0=m.sweep, clamp=False)
        assert "moments" not in res and res["clamped"] == 7
        assert np.array_equal(_bits(fg.weight_value[0]), _bits(m2.w)) and np.array_equal(fg.var_value, np.stack(m2.final))
        assert np.array_equal(_bits(res["grad_max"]), _bits(m2.gmax))
        # clamped=0 is today's call with today's keys
        res = fg.learn_pcd(1, 0.1, target=pcd.target_of(og), clamped=0)
        assert sorted(res) == sorted(["grad_max", "target", "chains", "factors_per_weight"])
    finally:
        fg.close()
