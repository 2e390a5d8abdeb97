"""Tempered sweep schedules on the device against the oracle (nsk_tempered_sweeps, FactorGraph.tempered_sweeps /
log_partition / log_evidence / anneal; tests/temper.py has the graphs, the mirror and the comparison rules,
tests/test_temper_cpu.py holds the estimator built on that mirror to exact enumerations).

Parity runs on raw C-ABI calls on a resident handle (one upload, as tests/resident.py): the states after the call, the
log-potentials of every step, the folded log-weights, the best states, the weights restored bit for bit, and the tables
refreshed back to the base weights -- under schedules of one sweep a step and of 17, where a step of a table-only
handle is one captured 16-sweep sequence plus an eager sweep and the draw tables change between the replays."""

import ctypes as C

import numpy as np
import pytest

from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import ais_log_weights

import resident
import temper
import tiles
import wide_trips
from util import session, oracle_of, phases_from_colors

pytestmark = pytest.mark.gpu

BETAS = np.array([0.0, 0.25, 0.5, 1.0, 1.5])
M64 = (1 << 64) - 1


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _mixed_lr():
    g = list(graphgen.mixed_lr_graph(3000, seed=5, nweights=40))
    w = g[0].copy()
    w["initialValue"] = np.random.default_rng(8).normal(0, 0.5, 40)        # (the generator leaves them 0)
    g[0] = w
    return tuple(g)


# name -> (graph builder, seed, chains, sample_evidence, switches, tests/tiles.py case, what nsk_graph_info must say)
CASES = {
    "table_grid_3_chains": (resident.table_grid, 9, 3, 1, {}, None, {}),
    "table_grid_1_chain": (resident.table_grid, 9, 1, 1, {}, None, {}),
    "evidence_grid_clamped": (resident.evidence_grid, 21, 2, 0, {}, None, {}),
    "evidence_grid_free": (resident.evidence_grid, 21, 2, 1, {}, None, {}),
    "wide_fold_grid": (resident.wide_fold_grid, 3, 1, 1, wide_trips.ENV, None, {"wide_quads": ">0"}),
    "mixed_lr_3000": (_mixed_lr, 5, 2, 1, {}, "lr", {}),
    "mixed_routes": (lambda: tiles.build_case("mixed_routes", learn=True)[0], 47, 2, 1, {}, "mixed_routes", {"weight_slots": 1}),
}


class Handle(object):
    """A resident handle with R chains, all at the initial values, and its oracle"""

    def __init__(self, monkeypatch, name):
        build, self.seed, self.R, self.se, env, tile, expect = CASES[name]
        hbv = False
        if tile == "lr":
            hbv = True
        elif tile:
            tiles.set_switches(monkeypatch, tile)
            hbv = tiles.CASES[tile].hbv
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _, self.fg = session(build(), seed=self.seed, head_by_vid=hbv)
        fg = self.fg
        info = fg.info()
        for k, want in expect.items():
            assert (info[k] > 0) if want == ">0" else (info[k] == want), (k, want, info[k])
        self.og = oracle_of(fg, hbv)
        self.color = fg.colors()
        self.L, self.h = _lib.lib(), fg._engine()
        fg._push(0, 0)                      # the one full upload
        if self.R > 1:
            _lib.check(self.L.nsk_set_chains(self.h, self.R))
        vv, _, self.w0, _ = self.og.initial_state()
        self.x0 = [vv.copy() for _ in range(self.R)]
        self.nvar = len(vv)

    def values(self):
        out = np.empty((self.R, self.nvar), np.int64)
        _lib.check(self.L.nsk_chains_download(self.h, _lib.ptr(out), None))       # (count = NULL: nothing is folded)
        return out

    def upload(self, states):
        vv = np.ascontiguousarray(np.stack(states), np.int64)
        _lib.check(self.L.nsk_chains_upload(self.h, _lib.ptr(vv), None))

    def weights(self):
        w = np.empty(len(self.w0), np.float64)
        _lib.check(self.L.nsk_state_download(self.h, None, None, _lib.ptr(w), None))
        return w

    def lp(self):
        out = np.zeros(self.R, np.float64)
        _lib.check(self.L.nsk_log_potential(self.h, _lib.BUF_VALUE, 0, self.R, _lib.ptr(out)))
        return out

    def tempered(self, betas, sps, se, best=True):
        b = np.ascontiguousarray(betas, np.float64)
        T = len(b)
        logw, lp = np.full(self.R, np.nan), np.full((T, self.R), np.nan)
        bv = np.full((self.R, self.nvar), -1, np.int64) if best else None
        bu = np.full(self.R, np.nan) if best else None
        rc = self.L.nsk_tempered_sweeps(self.h, _lib.ptr(b), T, sps, int(se), _lib.ptr(logw), _lib.ptr(lp), _lib.ptr(bv), _lib.ptr(bu))
        return rc, logw, lp, bv, bu

    def same_values(self, want, what):
        got = self.values()
        for r in range(self.R):
            bad = np.nonzero(got[r] != want[r])[0]
            assert len(bad) == 0, (what, "chain", r, "differing variables", len(bad), bad[:12])


@pytest.mark.parametrize("sps", [1, 17])
@pytest.mark.parametrize("name", sorted(CASES))
def test_schedule_parity_with_the_oracle(monkeypatch, name, sps):
    H = Handle(monkeypatch, name)
    try:
        T, R = len(BETAS), H.R
        w_before = H.weights()
        assert np.array_equal(_bits(w_before), _bits(H.w0)) and w_before.any()
        done0 = H.fg.info()["sweeps_done"]
        rc, logw, lp, bv, bu = H.tempered(BETAS, sps, H.se)
        _lib.check(rc)
        m = temper.Schedule(H.og, H.color, H.seed, H.x0, H.w0, BETAS, sps, H.se)
        assert all(m.moved), m.moved
        # (g) the sweeps are counted
        assert H.fg.info()["sweeps_done"] == done0 + T * sps
        # (a) every chain's values, bit for bit
        H.same_values(m.final, ("after the schedule", name, sps))
        # (b) every step's log-potential within the header's bound of the exactly rounded sum on the mirror's state
        for t in range(T):
            for r in range(R):
                print("step %d chain %d lp %.17g reference %.17g |diff| %.3g bound %.3g" %
                      (t, r, lp[t, r], m.lp[t, r], abs(lp[t, r] - m.lp[t, r]), m.bound[t, r]))
        assert (np.abs(lp - m.lp) <= m.bound).all(), np.abs(lp - m.lp) / m.bound
        assert len(np.unique(lp)) > 1
        # (d) the fold, on the device's own log-potentials
        assert np.array_equal(_bits(logw), _bits(ais_log_weights(BETAS, lp))), (logw, ais_log_weights(BETAS, lp))
        # (e) the weights are the base weights again
        assert np.array_equal(_bits(H.weights()), _bits(w_before))
        # (h) the best state is the first maximum's
        steps, states = m.best()
        dev_steps = np.argmax(lp, axis=0)
        assert np.array_equal(_bits(bu), _bits(lp[dev_steps, np.arange(R)]))
        for r in range(R):
            # (the mirror's first maximum is the device's unless two steps tie within the rounding of the sums)
            assert np.array_equal(bv[r], m.states[int(dev_steps[r])][r]), ("best state", r, dev_steps[r], steps[r])
        # (c) the very bits of nsk_log_potential: the last row right after, two earlier rows on the mirror's states
        assert np.array_equal(_bits(H.lp()), _bits(lp[T - 1]))
        for t in (1, 3):
            H.upload(m.states[t])
            assert np.array_equal(_bits(H.lp()), _bits(lp[t])), t
        H.upload(m.final)
        # (f) sweeps that follow sample under the base weights: the tables were refreshed back
        order, ps = phases_from_colors(H.color)
        cnt = [np.zeros(int(H.og.cstart[-1]), np.int64) for _ in range(R)]
        x = [s.copy() for s in m.final]
        _lib.check(H.L.nsk_gibbs_sweeps(H.h, 3, H.se, 0))
        for s in range(3):
            for r in range(R):
                assert H.og.gibbs_dev(order, ps, x[r], H.w0, cnt[r], H.seed ^ (r << 32), (m.sweep + s) & M64, bool(H.se), burnin=False) == 0
        H.same_values(x, ("three sweeps under the base weights", name, sps))
        got = np.empty((R, len(cnt[0])), np.int64)
        _lib.check(H.L.nsk_chains_download(H.h, None, _lib.ptr(got)))
        assert np.array_equal(got, np.stack(cnt))
    finally:
        H.fg.close()


def test_outputs_are_optional_and_one_step_folds_nothing(monkeypatch):
    H = Handle(monkeypatch, "table_grid_3_chains")
    try:
        b = np.array([0.7])
        logw = np.full(H.R, np.nan)
        _lib.check(H.L.nsk_tempered_sweeps(H.h, _lib.ptr(b), 1, 2, 1, _lib.ptr(logw), None, None, None))
        assert np.array_equal(logw, np.zeros(H.R))
        m = temper.Schedule(H.og, H.color, H.seed, H.x0, H.w0, b, 2, 1)
        H.same_values(m.final, "one step")
        # best_lp alone; nothing at all
        bu = np.full(H.R, np.nan)
        _lib.check(H.L.nsk_tempered_sweeps(H.h, _lib.ptr(b), 1, 1, 1, None, None, None, _lib.ptr(bu)))
        assert np.array_equal(_bits(bu), _bits(H.lp()))
        _lib.check(H.L.nsk_tempered_sweeps(H.h, _lib.ptr(b), 1, 1, 1, None, None, None, None))
        assert H.fg.info()["sweeps_done"] == 4
        assert np.array_equal(_bits(H.weights()), _bits(H.w0))
    finally:
        H.fg.close()


def test_tallied_sweeps_around_a_tempered_call(monkeypatch):
    """20 tallied sweeps, a tempered call, 20 tallied sweeps: the tallies are those of the 40, a trace keeps its rows, and
    the call leaves no allocation behind"""
    H = Handle(monkeypatch, "table_grid_3_chains")
    try:
        L, h, R, se = H.L, H.h, H.R, 1
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

        vids = np.arange(0, H.nvar, 7, dtype=np.int64)
        _lib.check(L.nsk_trace_setup(h, _lib.ptr(vids), len(vids), 5, 16))
        tallied(20)
        rows0, cap, packed = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(L.nsk_trace_rows(h, C.byref(rows0), C.byref(cap), C.byref(packed)))
        assert rows0.value == 4
        H.lp()                                                  # warm: the records of the factor walk stay
        H.values()                                              # ... and the staging of the state transfers
        bytes0 = H.fg.info()["device_bytes"]
        rc, logw, lp, bv, bu = H.tempered(BETAS, 3, se)
        _lib.check(rc)
        assert H.fg.info()["device_bytes"] == bytes0
        rows1 = C.c_int64()
        _lib.check(L.nsk_trace_rows(h, C.byref(rows1), C.byref(cap), C.byref(packed)))
        assert rows1.value == rows0.value
        m = temper.Schedule(H.og, H.color, H.seed, x, H.w0, BETAS, 3, se, sweep0=sweep)
        x, sweep = [s.copy() for s in m.final], m.sweep
        assert np.array_equal(_bits(logw), _bits(ais_log_weights(BETAS, lp)))
        tallied(20)
        _lib.check(L.nsk_trace_rows(h, C.byref(rows1), C.byref(cap), C.byref(packed)))
        assert rows1.value == 8
        H.same_values(x, "after the second tallied call")
        got = np.empty((R, len(cnt[0])), np.int64)
        _lib.check(L.nsk_chains_download(h, None, _lib.ptr(got)))
        assert np.array_equal(got, np.stack(cnt)) and got.max() > 0
    finally:
        H.fg.close()


def test_refusals_leave_the_handle_as_it_was(monkeypatch):
    H = Handle(monkeypatch, "table_grid_3_chains")
    try:
        L, h = H.L, H.h
        _lib.check(L.nsk_gibbs_sweeps(h, 2, 1, 1))
        v0, w0, done0 = H.values(), H.weights(), H.fg.info()["sweeps_done"]
        good = np.array([0.0, 0.5, 1.0])

        def call(betas, nsteps, sps, handle=h):
            b = None if betas is None else np.ascontiguousarray(betas, np.float64)
            return L.nsk_tempered_sweeps(handle, _lib.ptr(b), nsteps, sps, 1, None, None, None, None)

        assert call(good, 3, 1, handle=None) == _lib.E_INVALID
        assert call(None, 3, 1) == _lib.E_INVALID
        assert call(good, 0, 1) == _lib.E_INVALID
        assert call(good, -1, 1) == _lib.E_INVALID
        assert call(np.zeros(65537), 65537, 1) == _lib.E_INVALID
        assert call(good, 3, 0) == _lib.E_INVALID
        assert call(good, 3, (2 ** 31 - 1) // 3 + 1) == _lib.E_INVALID
        for bad in (float("nan"), float("inf"), -0.25):
            assert call([0.0, bad, 1.0], 3, 1) == _lib.E_INVALID
            assert call([0.0, 0.5, bad], 3, 1) == _lib.E_INVALID
        assert np.array_equal(H.values(), v0) and np.array_equal(_bits(H.weights()), _bits(w0))
        assert H.fg.info()["sweeps_done"] == done0
        # the generator too: the next sweeps are those of sweep indices 2, 3
        order, ps = phases_from_colors(H.color)
        cnt = np.zeros(int(H.og.cstart[-1]), np.int64)
        x = [s.copy() for s in H.x0]
        _lib.check(L.nsk_gibbs_sweeps(h, 2, 1, 1))
        for s in range(4):
            for r in range(H.R):
                assert H.og.gibbs_dev(order, ps, x[r], H.w0, cnt, H.seed ^ (r << 32), s, True, burnin=True) == 0
        H.same_values(x, "sweeps after the refusals")
    finally:
        H.fg.close()


def test_the_sequential_scan_and_partition_handles_are_refused():
    good = np.array([0.0, 0.5, 1.0])
    _, fg = session(resident.table_grid(), seed=1, scan="sequential")
    try:
        h = fg._engine()
        fg._push(0, 0)
        assert _lib.lib().nsk_tempered_sweeps(h, _lib.ptr(good), 3, 1, 1, None, None, None, None) == _lib.E_INVALID
        assert fg.info()["sweeps_done"] == 0
    finally:
        fg.close()
    import numbskull_amd
    from numbskull_amd.distributed import shard_range
    ns = numbskull_amd.NumbSkull(quiet=True, seed=1)
    w, v, f, fm, dm, edges = [x.copy() if isinstance(x, np.ndarray) else x for x in resident.table_grid()]
    ns.loadFactorGraph(w, v, f, fm, dm, int(edges), own_range=shard_range(0, 2, len(v)))      # NSK_FLAG_PARTITION
    fg = ns.factorGraphs[0]
    try:
        h = fg._engine()
        fg._push(0, 0)
        v0, w0 = fg.var_value[0].copy(), fg.weight_value[0].copy()
        assert _lib.lib().nsk_tempered_sweeps(h, _lib.ptr(good), 3, 1, 1, None, None, None, None) == _lib.E_INVALID
        assert "NSK_FLAG_PARTITION" in _lib.lib().nsk_last_error().decode()
        fg._pull(0, 0)
        assert np.array_equal(fg.var_value[0], v0) and np.array_equal(_bits(fg.weight_value[0]), _bits(w0))
        assert fg.info()["sweeps_done"] == 0
    finally:
        fg.close()


# ------------------------------------------------------------------------------------------------------- the Python API
def _python_handle(build, hbv=False, chains=64):
    _, fg = session(build(), seed=5, head_by_vid=hbv, chains=chains)
    og = oracle_of(fg, hbv)
    return fg, og, fg.colors()


def _tolerance(m, log_z):
    """max over chains of sum_t |betas[t + 1] - betas[t]| bound[t] (log-mean-exp is 1-Lipschitz in the sup norm) plus the
    estimator's own roundings"""
    return float((np.abs(np.diff(m.betas))[:, None] * m.bound[:-1]).sum(axis=0).max()) + 8 * 2.0 ** -53 * abs(log_z)


def test_log_partition_is_the_estimate_of_the_mirrors_log_weights():
    fg, og, color = _python_handle(lambda: graphgen.ising_grid(3, 4, weight=0.3))
    try:
        count0 = fg.count.copy()
        x0 = fg.var_value.copy()
        res = fg.log_partition(steps=20)
        assert np.array_equal(_bits(res["betas"]), _bits(np.linspace(0, 1, 21)))
        m = temper.Schedule(og, color, 5, x0, og.initial_state()[2], res["betas"], 1, 0)
        lz0 = temper.log_z0(og, color, 0)
        assert res["log_z0"] == lz0 and abs(lz0 - 12 * np.log(2.0)) <= 1e-12
        want, stderr, ess, ti = m.estimate(lz0)
        tol = _tolerance(m, want)
        print("log_z %.17g mirror %.17g |diff| %.3g tolerance %.3g stderr %.4f ess %.1f ti %.6f" %
              (res["log_z"], want, abs(res["log_z"] - want), tol, res["stderr"], res["ess"], res["log_z_ti"]))
        assert abs(res["log_z"] - want) <= tol
        assert abs(res["log_z"] - 9.119036) <= 3 * res["stderr"]            # (the enumeration of tests/temper.py)
        assert abs(res["stderr"] - stderr) <= 1e-9 and abs(res["ess"] - ess) <= 1e-6 and abs(res["log_z_ti"] - ti) <= 1e-9
        assert np.array_equal(fg.var_value, np.stack(m.final))              # var_value holds the final states
        assert np.array_equal(fg.count, count0)
        # a schedule of the caller's, two sweeps a step, the free partition function: the sweep index runs on
        b = np.array([0.0, 0.1, 0.3, 0.6, 1.0])
        res2 = fg.log_partition(betas=b, sweeps=2, sample_evidence=True)
        m2 = temper.Schedule(og, color, 5, m.final, og.initial_state()[2], b, 2, 1, sweep0=m.sweep)
        want2 = m2.estimate(lz0)[0]
        assert abs(res2["log_z"] - want2) <= _tolerance(m2, want2)
    finally:
        fg.close()


def test_log_evidence_is_the_difference_of_two_runs():
    fg, og, color = _python_handle(temper.clamped_grid)
    try:
        x0 = fg.var_value.copy()
        w0 = og.initial_state()[2]
        res = fg.log_evidence(steps=20)
        assert np.array_equal(fg.var_value, x0)
        betas = np.linspace(0, 1, 21)
        mc = temper.Schedule(og, color, 5, x0, w0, betas, 1, 0)
        mf = temper.Schedule(og, color, 5, x0, w0, betas, 1, 1, sweep0=mc.sweep)
        zc, sc = mc.estimate(temper.log_z0(og, color, 0))[:2]
        zf, sf = mf.estimate(temper.log_z0(og, color, 1))[:2]
        assert abs(res["clamped"]["log_z0"] - 9 * np.log(2.0)) <= 1e-12 and abs(res["free"]["log_z0"] - 12 * np.log(2.0)) <= 1e-12
        tol = _tolerance(mc, zc) + _tolerance(mf, zf)
        print("log_evidence %.17g mirror %.17g tolerance %.3g stderr %.4f" % (res["log_evidence"], zc - zf, tol, res["stderr"]))
        assert abs(res["log_evidence"] - (zc - zf)) <= tol
        assert abs(res["stderr"] - np.sqrt(sc * sc + sf * sf)) <= 1e-9
        # against the enumeration: log P(x0 = 1, x5 = 0, x11 = 1) under the free model
        vv = og.initial_state()[0]
        exact = temper.exact_log_z(og, w0, vv, temper.sampled_mask(og, color, 0)) - temper.exact_log_z(og, w0, vv, temper.sampled_mask(og, color, 1))
        assert abs(res["log_evidence"] - exact) <= 3 * res["stderr"], (res["log_evidence"], exact, res["stderr"])
    finally:
        fg.close()


def test_anneal_keeps_the_best_state_and_polishes_it():
    fg, og, color = _python_handle(lambda: graphgen.ising_grid(3, 4, weight=0.3), chains=8)
    try:
        count0 = fg.count.copy()
        x0 = fg.var_value.copy()
        betas = np.linspace(0.2, 3, 15)
        res = fg.anneal(betas)
        w0 = og.initial_state()[2]
        m = temper.Schedule(og, color, 5, x0, w0, betas, 1, 0)
        assert (np.abs(res["sampled_log_potentials"] - m.lp.max(axis=0)) <= m.bound.max(axis=0)).all()
        assert (res["log_potentials"] >= res["sampled_log_potentials"]).all()       # ICM cannot lower U on EQUAL factors
        chain = res["chain"]
        assert res["log_potential"] == res["log_potentials"][chain] == res["log_potentials"].max()
        assert res["log_potential"] >= res["sampled_log_potential"] == res["sampled_log_potentials"][chain]
        assert np.array_equal(res["values"], fg.var_value[chain])
        fg.var_value[:] = res["values"]                                             # every row: the returned state
        assert np.array_equal(_bits(fg.log_potential(var_copy="all")), _bits(np.full(8, res["log_potential"])))
        ref, bound = temper.log_potential(og, res["values"], w0)
        assert abs(res["log_potential"] - ref) <= bound
        assert np.array_equal(fg.count, count0)
        assert res["converged"] and res["sweeps"] >= 1
    finally:
        fg.close()
