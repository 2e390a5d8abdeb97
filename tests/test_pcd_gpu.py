"""PCD learning on the device against the oracle (nsk_weight_moments, nsk_pcd_steps, FactorGraph.weight_moments / learn_pcd;
tests/pcd.py has the graphs and the mirror, tests/test_pcd_cpu.py holds the numpy restatement of the rules to hand-written
loops, shows that every case here is lively in the mirror and recovers planted weights with the oracle as the sampler).

Every check is bit for bit: equality for the int64 moments and the states, uint64 views for gmax and the weights.  Parity
runs on raw C-ABI calls on a resident handle, two calls one behind the other (tests/pcd.py CALLS), over 1, 2, 3, 64, 65 and
1024 chains -- a lone chain, the smallest populations, as many chains as a wave has lanes, one more, and the most a handle
holds, where every lane and wave of the moment launches loops over four chains.

The moment kernels cut the weights where the statistics do (16 factors a lane, 2048 a wave's piece) and loop when the grid
is capped; the diagnostic cap NSK_MOMENTS_GRID_CAP = 8 blocks gives the lanes and the waves of tests/pcd.py trips_graph a
third trip, asserted from the launch arithmetic (_lib.moments_trips)."""

import ctypes as C

import numpy as np
import pytest

import numbskull_amd
from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import moment_counts
import pcd
from util import session, oracle_of, phases_from_colors

pytestmark = pytest.mark.gpu

SEED = 9


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class Handle(object):
    """A resident handle with R chains, all at the initial values, and its oracle"""

    def __init__(self, name, R, seed=SEED, graph=None):
        build, hbv, self.se = pcd.GRAPHS[name] if graph is None else (lambda: graph, False, 1)
        self.seed, self.R = seed, R
        _, self.fg = session(build(), seed=seed, head_by_vid=hbv)
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

    def moments(self, which=_lib.BUF_VALUE, first=0, n=None):
        out = np.full(self.nw, -1, np.int64)
        rc = self.L.nsk_weight_moments(self.h, which, first, self.R if n is None else n, _lib.ptr(out))
        return rc, out

    def pcd(self, target, nsteps, sps, step, decay, reg, normalize, se=None, outputs=True):
        t = np.ascontiguousarray(target, np.float64)
        gmax = np.full(nsteps, np.nan) if outputs else None
        rows = np.full((nsteps, self.nw), -1, np.int64) if outputs else None
        rc = self.L.nsk_pcd_steps(self.h, _lib.ptr(t), nsteps, sps, int(self.se if se is None else se), step, decay, reg, normalize,
                                  _lib.ptr(gmax), _lib.ptr(rows))
        return rc, gmax, rows

    def same_values(self, want, what):
        got = self.values()
        for r in range(self.R):
            bad = np.nonzero(got[r] != want[r])[0]
            assert len(bad) == 0, (what, "chain", r, "differing variables", len(bad), bad[:12])


def _one_call(H, x, w, sweep, nsteps, sps, normalize, reg, what):
    """one nsk_pcd_steps call against the mirror started at (x, w, sweep); returns the mirror"""
    target, step = pcd.target_of(H.og), pcd.stepsize(normalize)
    done0 = H.info("sweeps_done")
    rc, gmax, rows = H.pcd(target, nsteps, sps, step, pcd.DECAY, reg, normalize)
    _lib.check(rc)
    m = pcd.Run(H.og, H.color, H.seed, x, w, target, nsteps, sps, H.se, step, pcd.DECAY, reg, normalize, sweep0=sweep)
    for t in range(nsteps):
        assert np.array_equal(rows[t], m.moments[t]), (what, "moments of step", t, rows[t], m.moments[t])
    assert np.array_equal(_bits(gmax), _bits(m.gmax)), (what, gmax, m.gmax)
    got = H.weights()
    assert np.array_equal(_bits(got), _bits(m.w)), (what, got, m.w)
    assert np.array_equal(_bits(got[~H.free]), _bits(H.w0[~H.free]))
    H.same_values(m.final, what)
    assert H.info("sweeps_done") == done0 + nsteps * sps == m.sweep
    assert (m.w[H.free] != np.asarray(w)[H.free]).any() and len({r.tobytes() for r in rows}) > 1, "the case stands still"
    return m


def _parity(H, calls, nsteps, what):
    x, w, sweep = H.x0, H.w0, 0
    for k, (sps, normalize, reg) in enumerate(calls):
        m = _one_call(H, x, w, sweep, nsteps, sps, normalize, reg, (what, "call", k))
        x, w, sweep = m.final, m.w, m.sweep
    return m


# ------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("R", pcd.PARITY_CHAINS)
@pytest.mark.parametrize("name", pcd.PARITY_GRAPHS)
def test_parity_with_the_mirror(name, R):
    H = Handle(name, R)
    try:
        if name == "grid_int32":
            assert H.info("value_bytes") == 4
        _parity(H, pcd.parity_calls(name, R), pcd.STEPS, (name, R))
    finally:
        H.close()


def test_1024_chains():
    H = Handle("grid_w1.0", 1024)
    try:
        _parity(H, [(1, 1, 0.01)], pcd.STEPS, "grid_w1.0 x 1024")
    finally:
        H.close()


def test_factor_values_that_are_not_integers():
    H = Handle("ratio", 5)
    try:
        m = _parity(H, [(1, 1, 0.01), (2, 0, 0.0)], pcd.STEPS, "ratio")
        e = np.stack([pcd.factor_values(H.og, x) for x in m.final])
        assert (e != np.rint(e)).any() and (m.moments % 2 ** 32 != 0).any()
        rc, M = H.moments()
        _lib.check(rc)
        assert np.array_equal(M, moment_counts(e, H.og.factor["weightId"], H.nw)) and np.array_equal(M, m.moments[-1])
    finally:
        H.close()


# ------------------------------------------------------------------------------------------------------- 2. the cuts
def test_weights_at_the_kernels_cuts():
    """weights of 0, 1, 16, 17, 2048, 2049 and 5000 factors, the one of 17 fixed; reg_param > 0: the weight without a
    factor and without a target shrinks"""
    H = Handle("cuts", 3)
    try:
        assert tuple(pcd.factors_per_weight(H.og)) == pcd.CUT_COUNTS and H.w0[0] != 0.0
        assert (_lib.MOMENTS_SHORT, _lib.MOMENTS_PIECE) == (16, 2048)
        rc, M = H.moments()
        _lib.check(rc)
        assert np.array_equal(M, pcd.moments_of(H.og, H.x0)) and M[0] == 0 and M[1:].any()
        m = _parity(H, [(1, 1, 0.01)], 4, "cuts")
        assert _bits(m.w[pcd.CUT_FIXED]) == _bits(H.w0[pcd.CUT_FIXED])
        assert (m.moments[:, 0] == 0).all() and 0 < abs(m.w[0]) < abs(H.w0[0])
        rc, M = H.moments()
        _lib.check(rc)
        assert np.array_equal(M, pcd.moments_of(H.og, m.final)) and np.array_equal(M, m.moments[-1])
    finally:
        H.close()


# ------------------------------------------------------------------------------------------------------- 3. later trips
@pytest.mark.parametrize("cap", [0, pcd.TRIP_CAP])
def test_later_trips_under_the_grid_cap(cap, monkeypatch):
    trips = (_lib.moments_trips(pcd.TRIP_SHORTS, _lib.MOMENTS_BLOCK, cap), _lib.moments_trips(pcd.TRIP_PIECES, _lib.MOMENTS_BLOCK // 64, cap))
    assert trips == ((3, 3) if cap else (1, 1))
    if cap:
        monkeypatch.setenv("NSK_DIAG", "1")
        monkeypatch.setenv("NSK_MOMENTS_GRID_CAP", str(cap))
    H = Handle("trips", 2)
    try:
        n = pcd.factors_per_weight(H.og)
        assert int((n == 1).sum()) == pcd.TRIP_SHORTS and int((n == 17).sum()) == pcd.TRIP_PIECES and len(n) == pcd.TRIP_SHORTS + pcd.TRIP_PIECES
        rc, M = H.moments()
        _lib.check(rc)
        assert np.array_equal(M, pcd.moments_of(H.og, H.x0)) and M.all()
        _parity(H, [(1, 1, 0.01)], 2, ("trips", cap))
    finally:
        H.close()


# ------------------------------------------------------------------------------------------------------- 4. nsk_weight_moments
def test_weight_moments_of_chain_ranges_and_of_the_evidence_chain():
    H = Handle("mixed_free", 5)
    try:
        L, h, R = H.L, H.h, H.R
        _lib.check(L.nsk_gibbs_sweeps(h, 3, 1, 1))
        x = H.values()
        assert len({r.tobytes() for r in x}) > 1
        wid = H.og.factor["weightId"]
        e = np.stack([pcd.factor_values(H.og, r) for r in x])
        for first, n in ((0, 5), (0, 1), (4, 1), (1, 3), (2, 3)):
            rc, M = H.moments(first=first, n=n)
            _lib.check(rc)
            assert np.array_equal(M, moment_counts(e[first:first + n], wid, H.nw)), (first, n)
        rc, M = H.moments(which=_lib.BUF_VALUE_EVID, n=1)
        _lib.check(rc)
        assert np.array_equal(M, moment_counts(pcd.factor_values(H.og, H.x0[0]), wid, H.nw))
        # the statistics of the same chains: integers on this graph, so the rounded sum of the doubles
        S = np.zeros((R, H.nw))
        _lib.check(L.nsk_weight_stats(h, _lib.BUF_VALUE, 0, R, 0, _lib.ptr(S)))
        assert np.array_equal(S, np.rint(S)) and S.any()
        rc, M = H.moments()
        assert np.array_equal(M, np.rint(S * 2.0 ** 32).astype(np.int64).sum(axis=0))
        for kw in (dict(which=_lib.BUF_WEIGHT), dict(which=-1), dict(first=5), dict(first=-1), dict(n=0), dict(first=3, n=3),
                   dict(which=_lib.BUF_VALUE_EVID, n=2), dict(which=_lib.BUF_VALUE_EVID, first=1, n=1)):
            assert H.moments(**kw)[0] == _lib.E_INVALID, kw
        assert L.nsk_weight_moments(h, _lib.BUF_VALUE, 0, 1, None) == _lib.E_INVALID
        assert L.nsk_weight_moments(None, _lib.BUF_VALUE, 0, 1, _lib.ptr(M)) == _lib.E_INVALID
        # the sequential scan is served: it is not a sweep
        _lib.check(L.nsk_set_chains(h, 1))
        _lib.check(L.nsk_set_scan(h, _lib.SCAN_SEQUENTIAL))
        one = np.zeros(H.nw, np.int64)
        _lib.check(L.nsk_weight_moments(h, _lib.BUF_VALUE, 0, 1, _lib.ptr(one)))
        assert np.array_equal(one, moment_counts(e[0], wid, H.nw))
    finally:
        H.close()


def test_weight_moments_of_many_waves_on_one_accumulator():
    """the 200 x 200 grid: 79 600 factors under one weight, 39 pieces a chain"""
    g = graphgen.ising_grid(200, 200, weight=0.3)
    assert len(g[2]) == 79600 and len(g[0]) == 1
    _, fg = session(g, seed=SEED, chains=3)
    try:
        fg.inference(2, 3, True, var_copy="all")
        S = fg.weight_statistics(var_copy="all")
        assert np.array_equal(S, np.rint(S)) and len(np.unique(S)) == 3
        M, R = fg.weight_moments(var_copy="all", counts=True)
        assert R == 3 and np.array_equal(M, np.rint(S * 2.0 ** 32).astype(np.int64).sum(axis=0))
        assert np.array_equal(_bits(fg.weight_moments(var_copy="all")), _bits(S.sum(axis=0) / 3.0))
        M1, R1 = fg.weight_moments(var_copy=1, counts=True)
        assert R1 == 1 and M1[0] == int(S[1, 0]) << 32
    finally:
        fg.close()


def test_weight_moments_changes_nothing():
    H = Handle("grid_w1.0", 3)
    try:
        L, h = H.L, H.h
        _lib.check(L.nsk_gibbs_sweeps(h, 5, 1, 0))
        _lib.check(H.moments()[0])                              # warm
        x, c, w, done, nbytes = H.values(), H.tallies(), H.weights(), H.info("sweeps_done"), H.info("device_bytes")
        assert c.any()
        rc, M = H.moments()
        _lib.check(rc)
        assert np.array_equal(M, pcd.moments_of(H.og, x))
        assert np.array_equal(H.values(), x) and np.array_equal(H.tallies(), c) and np.array_equal(_bits(H.weights()), _bits(w))
        assert H.info("sweeps_done") == done and H.info("device_bytes") == nbytes
    finally:
        H.close()


# ------------------------------------------------------------------------------------------------------- 5. around the call
def test_tallied_sweeps_around_a_call():
    """20 tallied sweeps with a trace, nsk_pcd_steps, 20 tallied sweeps: the later sweeps run under the learned weights, the
    tallies are those of the 40, the trace keeps its rows, and the call leaves no allocation behind"""
    H = Handle("grid_w1.0", 3)
    try:
        L, h, R, se = H.L, H.h, H.R, 1
        H.se = se
        order, ps = phases_from_colors(H.color)
        cnt = [np.zeros(int(H.og.cstart[-1]), np.int64) for _ in range(R)]
        x, w = [s.copy() for s in H.x0], H.w0
        sweep = 0

        def tallied(n):
            nonlocal sweep
            _lib.check(L.nsk_gibbs_sweeps(h, n, se, 0))
            for s in range(n):
                for r in range(R):
                    assert H.og.gibbs_dev(order, ps, x[r], w, cnt[r], H.seed ^ (r << 32), sweep + s, True, burnin=False) == 0
            sweep += n

        vids = np.arange(0, H.nvar, 5, dtype=np.int64)
        _lib.check(L.nsk_trace_setup(h, _lib.ptr(vids), len(vids), 5, 16))
        tallied(20)
        rows0, cap, packed = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(L.nsk_trace_rows(h, C.byref(rows0), C.byref(cap), C.byref(packed)))
        assert rows0.value == 4
        _lib.check(H.moments()[0])                              # warm: the records of the factor walk and the by-weight list stay
        H.values()                                              # ... and the staging of the state transfers
        H.weights()
        bytes0 = H.info("device_bytes")
        m = _one_call(H, x, w, sweep, 5, 3, 1, 0.01, "between the tallied sweeps")
        assert H.info("device_bytes") == bytes0
        assert H.info("sweeps_done") == 20 + 15
        rows1 = C.c_int64()
        _lib.check(L.nsk_trace_rows(h, C.byref(rows1), C.byref(cap), C.byref(packed)))
        assert rows1.value == rows0.value
        x, w, sweep = [s.copy() for s in m.final], m.w, m.sweep
        assert _bits(w[0]) != _bits(H.w0[0])
        tallied(20)                                             # ... under the learned weights: the refresh behind the last update
        _lib.check(L.nsk_trace_rows(h, C.byref(rows1), C.byref(cap), C.byref(packed)))
        assert rows1.value == 8
        H.same_values(x, "after the second tallied call")
        got = H.tallies()
        assert np.array_equal(got, np.stack(cnt)) and got.max() > 0
        # the sweeps under the old weights would have ended elsewhere
        assert np.array_equal(_bits(H.weights()), _bits(w))
    finally:
        H.close()


# ------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_handle_as_it_was():
    H = Handle("grid_w1.0", 3)
    try:
        L, h = H.L, H.h
        _lib.check(L.nsk_gibbs_sweeps(h, 2, 1, 1))
        v0, w0, done0 = H.values(), H.weights(), H.info("sweeps_done")
        good = np.array([4.0])

        def call(target=good, nsteps=3, sps=1, step=0.1, decay=0.9, reg=0.0, normalize=1, handle=h):
            t = None if target is None else np.ascontiguousarray(target, np.float64)
            return L.nsk_pcd_steps(handle, _lib.ptr(t), nsteps, sps, 1, step, decay, reg, normalize, None, None)

        assert call(handle=None) == _lib.E_INVALID
        assert call(target=None) == _lib.E_INVALID
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(target=[bad]) == _lib.E_INVALID
        for n in (0, -1, 65537):
            assert call(nsteps=n) == _lib.E_INVALID
        assert call(sps=0) == _lib.E_INVALID and call(sps=-3) == _lib.E_INVALID
        assert call(sps=(2 ** 31 - 1) // 3 + 1) == _lib.E_INVALID
        for bad in (float("nan"), float("inf")):
            assert call(step=bad) == _lib.E_INVALID and call(decay=bad) == _lib.E_INVALID and call(reg=bad) == _lib.E_INVALID
        assert call(reg=-1e-3) == _lib.E_INVALID
        for bad in (2, -1):
            assert call(normalize=bad) == _lib.E_INVALID
        assert np.array_equal(H.values(), v0) and np.array_equal(_bits(H.weights()), _bits(w0))
        assert H.info("sweeps_done") == done0
        # optional outputs may be NULL
        assert call() == _lib.OK
        assert H.info("sweeps_done") == done0 + 3 and _bits(H.weights()[0]) != _bits(w0[0])
    finally:
        H.close()
    # the sequential scan
    H = Handle("grid_w1.0", 1)
    try:
        _lib.check(H.L.nsk_set_scan(H.h, _lib.SCAN_SEQUENTIAL))
        assert H.pcd([4.0], 2, 1, 0.1, 1.0, 0.0, 1)[0] == _lib.E_INVALID
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
        one, t = np.zeros(1, np.int64), np.array([1.0])
        assert _lib.lib().nsk_pcd_steps(sh._engine(), _lib.ptr(t), 1, 1, 1, 0.1, 1.0, 0.0, 1, None, None) == _lib.E_INVALID
        assert _lib.lib().nsk_weight_moments(sh._engine(), _lib.BUF_VALUE, 0, 1, _lib.ptr(one)) == _lib.E_INVALID
    finally:
        sh.close()


def test_the_range_rule():
    """B_0 = 1e6 a UFO factor: 1073 of them stay below 2^30 at one chain, 1074 do not; two chains halve the count"""
    assert 1073 * 1e6 < 2 ** 30 <= 1074 * 1e6 and 536 * 2e6 < 2 ** 30 <= 537 * 2e6
    for n, R, want in ((1073, 1, _lib.OK), (1074, 1, _lib.E_RANGE), (536, 2, _lib.OK), (537, 2, _lib.E_RANGE)):
        H = Handle(None, R, graph=pcd.ufo_graph(n))
        try:
            v0, w0 = H.values(), H.weights()
            M = np.zeros(1, np.int64)
            assert H.L.nsk_weight_moments(H.h, _lib.BUF_VALUE, 0, R, _lib.ptr(M)) == want, (n, R)
            assert H.L.nsk_weight_moments(H.h, _lib.BUF_VALUE, 0, 1, _lib.ptr(M)) == (want if R == 1 else _lib.OK)
            rc = H.pcd([0.0], 1, 1, 0.1, 1.0, 0.0, 1, outputs=False)[0]
            assert rc == want, (n, R, rc)
            if want != _lib.OK:
                assert "2^30" in H.L.nsk_last_error().decode()
                assert np.array_equal(H.values(), v0) and np.array_equal(_bits(H.weights()), _bits(w0)) and H.info("sweeps_done") == 0
        finally:
            H.close()


# ------------------------------------------------------------------------------------------------------- 7. the Python API
def test_learn_pcd_is_the_mirror():
    build, hbv, se = pcd.GRAPHS["mixed_free"]
    _, fg = session(build(), seed=5, head_by_vid=hbv, chains=8)
    try:
        og, color = oracle_of(fg, hbv), fg.colors()
        w0, x0, count0 = og.initial_state()[2], fg.var_value.copy(), fg.count.copy()
        assert x0.shape[0] == 8
        target = pcd.target_of(og)
        res = fg.learn_pcd(5, 0.3, decay=0.9, reg_param=0.01, sweeps=2, sample_evidence=True, target=target, moments=True)
        m = pcd.Run(og, color, 5, x0, w0, target, 5, 2, True, 0.3, 0.9, 0.01, 1)
        assert sorted(res) == sorted(["grad_max", "target", "chains", "factors_per_weight", "moments"])
        assert np.array_equal(_bits(fg.weight_value[0]), _bits(m.w)) and np.array_equal(fg.var_value, np.stack(m.final))
        assert np.array_equal(_bits(res["grad_max"]), _bits(m.gmax)) and np.array_equal(res["moments"], m.moments)
        assert res["moments"].dtype == np.int64 and res["chains"] == 8
        assert np.array_equal(res["factors_per_weight"], pcd.factors_per_weight(og)) and np.array_equal(res["target"], target)
        assert np.array_equal(fg.count, count0) and (m.w != w0).any()
        # target=None: the evidence chain's statistics (integers on this graph); weight_copy and normalize=False
        ev = fg.weight_statistics(evidence_chain=True)
        w1 = fg.weight_value[0].copy()
        x1 = fg.var_value.copy()
        res = fg.learn_pcd(2, 0.03, normalize=False)
        assert np.array_equal(_bits(res["target"]), _bits(ev)) and "moments" not in res
        m2 = pcd.Run(og, color, 5, x1, w1, ev, 2, 1, True, 0.03, 1.0, 0.0, 0, sweep0=m.sweep)
        assert np.array_equal(_bits(fg.weight_value[0]), _bits(m2.w)) and np.array_equal(fg.var_value, np.stack(m2.final))
        assert np.array_equal(_bits(res["grad_max"]), _bits(m2.gmax))
        # weight_moments is the chains' mean of weight_statistics where the factor values are integers
        S = fg.weight_statistics(var_copy="all")
        assert np.array_equal(S, np.rint(S))
        assert np.array_equal(_bits(fg.weight_moments(var_copy="all")), _bits(S.sum(axis=0) / 8.0))
        assert np.array_equal(_bits(fg.weight_moments(var_copy=3)), _bits(S[3]))
        assert np.array_equal(_bits(fg.weight_moments(evidence_chain=True)), _bits(ev))
        for kw in (dict(epochs=0), dict(sweeps=0), dict(stepsize=float("nan")), dict(reg_param=-1.0), dict(target=np.zeros(2))):
            args = dict(epochs=2, stepsize=0.1)
            args.update(kw)
            with pytest.raises(ValueError):
                fg.learn_pcd(**args)
    finally:
        fg.close()
