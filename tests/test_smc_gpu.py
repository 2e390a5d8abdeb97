"""Population annealing on the device against the oracle (nsk_smc_sweeps, FactorGraph.smc_sweeps / log_partition(resample=...);
tests/smc.py has the fold and the mirror, tests/temper.py the graphs and the log-potential, tests/test_smc_cpu.py holds the
numpy restatement of the rule and the estimator to hand-written loops and to exact enumerations).

Parity runs on raw C-ABI calls on a resident handle: the rows kept in front of every decision against the fold of the
device's own log-potentials, the decisions and ancestors against ``smc_resample`` of those rows, the states against the
oracle's replay with the device's ancestors applied, over populations of 1, 2, 3, 64, 65 and 1024 chains -- a lone chain,
the smallest populations, one wave of the decide block, one lane more, and the most a handle holds.

The schedule opens with two steps of 0.01, whose log-weights are as good as equal -- no population resamples there -- and
goes on in steps of 0.3 and more, where the effective sample size falls under 0.9 R within a step or two."""

import ctypes as C

import numpy as np
import pytest

from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import smc_resample, ais_estimate, thermodynamic_integral
from oracle import binding as orc

import smc
import temper
from test_temper_gpu import _tolerance
from util import session, oracle_of, phases_from_colors

pytestmark = pytest.mark.gpu

BETAS = np.array([0.0, 0.01, 0.02, 0.4, 0.7, 1.0])
BETAS_1024 = np.array([0.0, 0.01, 0.5, 1.0])
SEED = 9


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _grid_3x7():
    return graphgen.ising_grid(3, 7, weight=0.8)


def _grid_int32():
    """the clamped grid with an evidence variable of 200 values: int32 values on the device"""
    g = list(temper.clamped_grid())
    var = g[1].copy()
    var["cardinality"][5] = 200
    g[1] = var
    return tuple(g)


# name -> (graph builder, head_by_vid, sample_evidence)
GRAPHS = {k: v[:3] for k, v in temper.SMALL.items()}
GRAPHS["grid_3x7"] = (_grid_3x7, False, 0)
GRAPHS["grid_int32"] = (_grid_int32, False, 0)

# (graph, chains) -> threshold, where 0.9 does not show both an event and a step without one (two chains of mixed_free
# never fall under 1.87 of 2)
THRESHOLD = {("mixed_free", 2): 0.95}


class Handle(object):
    """A resident handle with R chains, all at the initial values, and its oracle"""

    def __init__(self, name, R, seed=SEED):
        build, hbv, self.se = GRAPHS[name]
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
        self.nvar = len(vv)

    def value_bytes(self):
        """(the slots of a chain's value array, the bytes of a slot)"""
        iid, nid = np.zeros(self.nvar, np.int32), C.c_int64()
        _lib.check(self.L.nsk_graph_get_layout(self.h, _lib.ptr(iid), C.byref(nid)))
        assert np.array_equal(iid, self.fg.layout()) and iid.max() < nid.value
        return nid.value, self.fg.info()["value_bytes"]

    def values(self):
        out = np.empty((self.R, self.nvar), np.int64)
        _lib.check(self.L.nsk_chains_download(self.h, _lib.ptr(out), None))
        return out

    def weights(self):
        w = np.empty(len(self.w0), np.float64)
        _lib.check(self.L.nsk_state_download(self.h, None, None, _lib.ptr(w), None))
        return w

    def smc(self, betas, sps, threshold, offsets):
        b = np.ascontiguousarray(betas, np.float64)
        T, R = len(b), self.R
        off = np.ascontiguousarray(offsets, np.float64)
        logw, lp, pre = np.full(R, np.nan), np.full((T, R), np.nan), np.full((T - 1, R), np.nan)
        anc, flag = np.full((T - 1, R), -1, np.int32), np.full(T - 1, -1, np.int32)
        rc = self.L.nsk_smc_sweeps(self.h, _lib.ptr(b), T, sps, int(self.se), threshold, _lib.ptr(off), _lib.ptr(logw), _lib.ptr(lp),
                                   _lib.ptr(pre), _lib.ptr(anc), _lib.ptr(flag))
        return rc, logw, lp, pre, anc, flag

    def same_values(self, want, what):
        got = self.values()
        for r in range(self.R):
            bad = np.nonzero(got[r] != want[r])[0]
            assert len(bad) == 0, (what, "chain", r, "differing variables", len(bad), bad[:12])


def _parity(H, name, betas, sps=1):
    """the checks (a) - (d) of one call on a fresh handle; returns the mirror"""
    T, R = len(betas), H.R
    threshold = THRESHOLD.get((name, R), 0.9)
    offsets = np.random.default_rng(1000 + R).random(T - 1)
    w_before, done0 = H.weights(), H.fg.info()["sweeps_done"]
    rc, logw, lp, pre, anc, flag = H.smc(betas, sps, threshold, offsets)
    _lib.check(rc)
    assert set(flag.tolist()) <= {0, 1}
    # (a) the rows in front of the decisions are the fold of the device's own log-potentials, reset behind an event;
    # (d) so is what the call leaves
    want_pre, want_logw = smc.fold(betas, lp, flag)
    assert np.array_equal(_bits(pre), _bits(want_pre)), (pre, want_pre)
    assert np.array_equal(_bits(logw), _bits(want_logw)), (logw, want_logw)
    # (b) decisions and ancestors: the rule, on the device's rows, with the specified exp
    for t in range(T - 1):
        f, a, S, Q = smc_resample(pre[t], offsets[t], threshold, exp=orc.exp_det)
        print("%s R %d step %d: ESS %.3f of %d, threshold %.2f, resampled %d, copies %d" %
              (name, R, t, S * S / Q, R, threshold, flag[t], int((anc[t] != np.arange(R)).sum())))
        assert f == bool(flag[t]) and np.array_equal(a, anc[t]), (t, f, flag[t], a, anc[t])
    # (c) the oracle's replay with the device's ancestors ends in the device's states; every log-potential within the
    # header's bound of the exactly rounded sum
    m = smc.Schedule(H.og, H.color, H.seed, H.x0, H.w0, betas, sps, H.se, threshold, offsets, resampled=flag, ancestors=anc)
    assert all(m.moved), m.moved
    H.same_values(m.final, ("after the schedule", name, R))
    assert (np.abs(lp - m.lp) <= m.bound).all(), np.abs(lp - m.lp) / m.bound
    # the mirror's own decisions, from its own sums, are the device's
    assert np.array_equal(m.own_resampled, flag != 0) and np.array_equal(m.own_ancestors, anc)
    if R >= 2:
        assert m.own_resampled.any() and not m.own_resampled.all(), m.own_resampled
        assert len(np.unique(lp)) > 1
        copied = [t for t in range(T - 1) if (anc[t] != np.arange(R)).any()]
        assert all(flag[t] for t in copied)
        assert copied or R < 16            # (two or three chains may all survive an event)
    else:
        assert not flag.any() and not anc.any()
    assert H.fg.info()["sweeps_done"] == done0 + T * sps
    assert np.array_equal(_bits(H.weights()), _bits(w_before)) and w_before.any()
    return m


@pytest.mark.parametrize("R", [1, 2, 3, 64, 65])
@pytest.mark.parametrize("name", sorted(temper.SMALL))
def test_population_parity_with_the_oracle(name, R):
    H = Handle(name, R)
    try:
        _parity(H, name, BETAS)
    finally:
        H.fg.close()


def test_a_population_of_1024_chains():
    H = Handle("grid_w1.0", 1024)
    try:
        _parity(H, "grid_w1.0", BETAS_1024)
    finally:
        H.fg.close()


# What the copy kernel moves for a chain: whole 16-byte accesses and the tail behind them, of int8 and of int32 slots.  The
# compiled layout pads even a 12-variable graph to 64 k + 1 slots, so no handle has a chain of under 16 value bytes: the
# kernel's path without a whole access cannot be reached through the library.  The slot counts are asserted, so that a
# layout change fails here instead of hollowing the cases out.
@pytest.mark.parametrize("name,nid,vbytes,whole,tail", [("grid_w1.0", 449, 1, 28, 1), ("grid_3x7", 385, 1, 24, 1), ("grid_int32", 513, 4, 128, 4)])
def test_the_copy_at_its_byte_counts(name, nid, vbytes, whole, tail):
    H = Handle(name, 16)
    try:
        assert H.value_bytes() == (nid, vbytes)
        assert divmod(nid * vbytes, 16) == (whole, tail)
        _parity(H, name, BETAS, sps=2)
    finally:
        H.fg.close()


def test_outputs_are_optional_and_threshold_zero_is_the_tempered_call():
    H, H2 = Handle("grid_w1.0", 5), Handle("grid_w1.0", 5)
    try:
        b = np.ascontiguousarray(BETAS)
        T = len(b)
        _lib.check(H.L.nsk_smc_sweeps(H.h, _lib.ptr(b), T, 1, 0, 0.0, None, None, None, None, None, None))
        logw, lp = np.full(5, np.nan), np.full((T, 5), np.nan)
        _lib.check(H2.L.nsk_tempered_sweeps(H2.h, _lib.ptr(b), T, 1, 0, _lib.ptr(logw), _lib.ptr(lp), None, None))
        assert np.array_equal(H.values(), H2.values())
        # the same again with every output: nothing resampled, the tempered call's bits
        logw2, lp2, pre = np.full(5, np.nan), np.full((T, 5), np.nan), np.full((T - 1, 5), np.nan)
        anc, flag = np.full((T - 1, 5), -1, np.int32), np.full(T - 1, -1, np.int32)
        _lib.check(H.L.nsk_smc_sweeps(H.h, _lib.ptr(b), T, 1, 0, 0.0, None, _lib.ptr(logw2), _lib.ptr(lp2), _lib.ptr(pre), _lib.ptr(anc),
                                      _lib.ptr(flag)))
        _lib.check(H2.L.nsk_tempered_sweeps(H2.h, _lib.ptr(b), T, 1, 0, _lib.ptr(logw), _lib.ptr(lp), None, None))
        assert np.array_equal(_bits(lp2), _bits(lp)) and np.array_equal(_bits(logw2), _bits(logw)) and np.array_equal(_bits(pre[-1]), _bits(logw))
        assert not flag.any() and np.array_equal(anc, np.tile(np.arange(5, dtype=np.int32), (T - 1, 1)))
        assert np.array_equal(H.values(), H2.values())
        # one step: nothing is decided, nothing is written behind the empty arrays
        one = np.array([0.7])
        logw1 = np.full(5, np.nan)
        _lib.check(H.L.nsk_smc_sweeps(H.h, _lib.ptr(one), 1, 2, 0, 0.5, None, _lib.ptr(logw1), None, None, None, None))
        assert np.array_equal(logw1, np.zeros(5))
        assert H.fg.info()["sweeps_done"] == 2 * T + 2
    finally:
        H.fg.close()
        H2.fg.close()


def test_tallied_sweeps_around_a_resampled_call():
    """20 tallied sweeps, a resampled call, 20 tallied sweeps: the tallies are those of the 40, a trace keeps its rows, the
    sweep index runs on and the call leaves no allocation behind"""
    H = Handle("grid_w1.0", 3)
    try:
        L, h, R, se = H.L, H.h, H.R, 1
        H.se = se
        order, ps = phases_from_colors(H.color)
        cnt = [np.zeros(int(H.og.cstart[-1]), np.int64) for _ in range(R)]
        x = [s.copy() for s in H.x0]
        sweep = 0

        def tallied(n):
            nonlocal sweep
            _lib.check(L.nsk_gibbs_sweeps(h, n, se, 0))
            for s in range(n):
                for r in range(R):
                    assert H.og.gibbs_dev(order, ps, x[r], H.w0, cnt[r], H.seed ^ (r << 32), sweep + s, True, burnin=False) == 0
            sweep += n

        vids = np.arange(0, H.nvar, 5, dtype=np.int64)
        _lib.check(L.nsk_trace_setup(h, _lib.ptr(vids), len(vids), 5, 16))
        tallied(20)
        rows0, cap, packed = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(L.nsk_trace_rows(h, C.byref(rows0), C.byref(cap), C.byref(packed)))
        assert rows0.value == 4
        lp0 = np.zeros(R)
        _lib.check(L.nsk_log_potential(h, _lib.BUF_VALUE, 0, R, _lib.ptr(lp0)))      # warm: the records of the factor walk stay
        H.values()                                                                  # ... and the staging of the state transfers
        bytes0 = H.fg.info()["device_bytes"]
        offsets = np.random.default_rng(3).random(len(BETAS) - 1)
        rc, logw, lp, pre, anc, flag = H.smc(BETAS, 3, 0.9, offsets)
        _lib.check(rc)
        assert H.fg.info()["device_bytes"] == bytes0
        assert H.fg.info()["sweeps_done"] == 20 + 3 * len(BETAS)
        rows1 = C.c_int64()
        _lib.check(L.nsk_trace_rows(h, C.byref(rows1), C.byref(cap), C.byref(packed)))
        assert rows1.value == rows0.value
        m = smc.Schedule(H.og, H.color, H.seed, x, H.w0, BETAS, 3, se, 0.9, offsets, sweep0=sweep, resampled=flag, ancestors=anc)
        assert flag.any() and (anc != np.arange(R)).any()
        H.same_values(m.final, "behind the resampled call")
        x, sweep = [s.copy() for s in m.final], m.sweep
        assert sweep == 20 + 3 * len(BETAS)
        tallied(20)
        _lib.check(L.nsk_trace_rows(h, C.byref(rows1), C.byref(cap), C.byref(packed)))
        assert rows1.value == 8
        H.same_values(x, "after the second tallied call")
        got = np.empty((R, len(cnt[0])), np.int64)
        _lib.check(L.nsk_chains_download(h, None, _lib.ptr(got)))
        assert np.array_equal(got, np.stack(cnt)) and got.max() > 0
    finally:
        H.fg.close()


def test_refusals_leave_the_handle_as_it_was():
    H = Handle("grid_w1.0", 3)
    try:
        L, h = H.L, H.h
        _lib.check(L.nsk_gibbs_sweeps(h, 2, 1, 1))
        v0, w0, done0 = H.values(), H.weights(), H.fg.info()["sweeps_done"]
        good, off = np.array([0.0, 0.5, 1.0]), np.array([0.25, 0.75])

        def call(betas=good, nsteps=3, sps=1, threshold=0.5, offsets=off, handle=h):
            b = None if betas is None else np.ascontiguousarray(betas, np.float64)
            o = None if offsets is None else np.ascontiguousarray(offsets, np.float64)
            return L.nsk_smc_sweeps(handle, _lib.ptr(b), nsteps, sps, 1, threshold, _lib.ptr(o), None, None, None, None, None)

        assert call(handle=None) == _lib.E_INVALID
        assert call(betas=None) == _lib.E_INVALID
        for n in (0, -1):
            assert call(nsteps=n) == _lib.E_INVALID
        assert call(betas=np.zeros(65537), nsteps=65537, offsets=np.zeros(65536)) == _lib.E_INVALID
        assert call(sps=0) == _lib.E_INVALID
        assert call(sps=(2 ** 31 - 1) // 3 + 1) == _lib.E_INVALID
        for bad in (float("nan"), float("inf"), -0.25):
            assert call(betas=[0.0, bad, 1.0]) == _lib.E_INVALID
        for bad in (float("nan"), -0.01, 1.01, float("inf")):
            assert call(threshold=bad) == _lib.E_INVALID
            assert "threshold" in L.nsk_last_error().decode()
        for bad in (float("nan"), -0.01, 1.0, float("inf")):
            assert call(offsets=[0.5, bad]) == _lib.E_INVALID
            assert call(offsets=[bad, 0.5], threshold=0.0) == _lib.E_INVALID
        assert call(offsets=None) == _lib.E_INVALID
        assert np.array_equal(H.values(), v0) and np.array_equal(_bits(H.weights()), _bits(w0))
        assert H.fg.info()["sweeps_done"] == done0
        # no offsets are needed where nothing can resample
        assert call(offsets=None, threshold=0.0) == _lib.OK
        assert call(betas=[0.3], nsteps=1, offsets=None) == _lib.OK
        assert H.fg.info()["sweeps_done"] == done0 + 4
    finally:
        H.fg.close()


# ------------------------------------------------------------------------------------------------------- the Python API
def test_log_partition_with_resampling_is_the_estimate_of_the_mirror():
    build = temper.SMALL["grid_w1.0"][0]
    _, fg = session(build(), seed=5, chains=32)
    _, fg2 = session(build(), seed=5, chains=32)
    try:
        og, color = oracle_of(fg), fg.colors()
        w0 = og.initial_state()[2]
        count0, x0 = fg.count.copy(), fg.var_value.copy()
        betas = np.linspace(0, 1, 9)
        res = fg.log_partition(steps=8, resample=0.5)
        assert np.array_equal(_bits(res["betas"]), _bits(betas))
        offsets = np.random.default_rng(0).random(8)
        m = smc.Schedule(og, color, 5, x0, w0, betas, 1, 0, 0.5, offsets)
        lz0 = temper.log_z0(og, color, 0)
        want, ess, events = m.estimate(lz0)
        tol = _tolerance(m, want)
        print("log_z %.17g mirror %.17g |diff| %.3g tolerance %.3g ess %.2f events %d" % (res["log_z"], want, abs(res["log_z"] - want), tol, ess, events))
        assert res["log_z0"] == lz0 and abs(res["log_z"] - want) <= tol
        assert res["resamplings"] == events and 1 <= events < 8
        assert abs(res["ess"] - ess) <= 1e-6 and np.isnan(res["stderr"]) and np.isfinite(res["log_z_ti"])
        assert sorted(res) == sorted(["log_z", "stderr", "ess", "log_z0", "log_weights", "log_z_ti", "betas", "resamplings"])
        assert np.array_equal(fg.var_value, np.stack(m.final)) and np.array_equal(fg.count, count0)
        # resample=None on the same handle is the tempered path, bit for bit: the same calls by hand on a second session
        # brought to the same sweep index
        fg.var_value[:] = x0
        a = fg.log_partition(steps=8)
        fg2.tempered_sweeps(betas)
        fg2.var_value[:] = x0
        t = fg2.tempered_sweeps(betas, 1, False, 0)
        lz, se, es = ais_estimate(t["log_weights"], lz0)
        assert sorted(a) == sorted(["log_z", "stderr", "ess", "log_z0", "log_weights", "log_z_ti", "betas"])
        assert a["log_z"] == lz and a["stderr"] == se and a["ess"] == es and a["log_z0"] == lz0
        assert np.array_equal(_bits(a["log_weights"]), _bits(t["log_weights"]))
        assert a["log_z_ti"] == thermodynamic_integral(betas, t["log_potentials"], lz0)
        assert np.array_equal(fg.var_value, fg2.var_value)
        plain = temper.Schedule(og, color, 5, x0, w0, betas, 1, 0, sweep0=m.sweep)
        assert np.array_equal(fg.var_value, np.stack(plain.final))
        assert abs(a["log_z"] - plain.estimate(lz0)[0]) <= _tolerance(plain, a["log_z"])
    finally:
        fg.close()
        fg2.close()


def test_smc_sweeps_and_log_evidence():
    _, fg = session(temper.clamped_grid(), seed=5, chains=32)
    try:
        og, color = oracle_of(fg), fg.colors()
        w0, x0 = og.initial_state()[2], fg.var_value.copy()
        betas = np.array([0.0, 0.05, 0.5, 1.0])
        res = fg.smc_sweeps(betas, sweeps=2, threshold=0.9, seed=7)
        offsets = np.random.default_rng(7).random(3)
        assert np.array_equal(res["offsets"], offsets) and res["resampled"].dtype == bool and res["ancestors"].dtype == np.int32
        m = smc.Schedule(og, color, 5, x0, w0, betas, 2, 0, 0.9, offsets, resampled=res["resampled"], ancestors=res["ancestors"])
        assert np.array_equal(fg.var_value, np.stack(m.final))
        assert np.array_equal(m.own_resampled, res["resampled"]) and res["resampled"].any() and not res["resampled"].all()
        pre, lw = smc.fold(betas, res["log_potentials"], res["resampled"])
        assert np.array_equal(_bits(pre), _bits(res["logw_pre"])) and np.array_equal(_bits(lw), _bits(res["log_weights"]))
        # log_evidence: two resampled runs from the same rows, var_value restored
        fg.var_value[:] = x0
        ev = fg.log_evidence(steps=8, resample=0.5)
        assert np.array_equal(fg.var_value, x0)
        assert np.isnan(ev["stderr"]) and ev["log_evidence"] == ev["clamped"]["log_z"] - ev["free"]["log_z"]
        assert "resamplings" in ev["clamped"] and "resamplings" in ev["free"]
        b8, off8 = np.linspace(0, 1, 9), np.random.default_rng(0).random(8)
        mc = smc.Schedule(og, color, 5, x0, w0, b8, 1, 0, 0.5, off8, sweep0=m.sweep)
        mf = smc.Schedule(og, color, 5, x0, w0, b8, 1, 1, 0.5, off8, sweep0=mc.sweep)
        zc, zf = mc.estimate(temper.log_z0(og, color, 0))[0], mf.estimate(temper.log_z0(og, color, 1))[0]
        assert abs(ev["log_evidence"] - (zc - zf)) <= _tolerance(mc, zc) + _tolerance(mf, zf)
    finally:
        fg.close()
