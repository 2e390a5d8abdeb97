"""Parallel tempering on the device against the oracle (nsk_pt_sweeps, FactorGraph.parallel_tempering; tests/pt.py has the
graphs, the cases and the mirror, tests/test_pt_cpu.py shows every case here lively and away from ties, without a GPU).

Parity runs on raw C-ABI calls on a resident handle whose chains carry tallies and a pending uint8 position tally from
three tallied sweeps: the decisions against ``pt_swap_rule`` on the device's own log-potentials, integer for integer; the
log-potentials within the header's bound of the mirror's; every chain's state, the tallied chain's counts, the other
chains' untouched counts and sweeps_done against the mirror; and a following tallied nsk_gibbs_sweeps call against the
mirror's continuation, which shows the sweep index, the restored weights and the rebuilt tables."""

import ctypes as C

import numpy as np
import pytest

from numbskull_amd import _lib
from numbskull_amd.diagnostics import pt_swap_rule, pt_paths
from oracle import binding as orc

import pt
from util import session, oracle_of, phases_from_colors

pytestmark = pytest.mark.gpu

PRE = pt.PRE     # tallied sweeps in front of the call: every chain has counts, and the uint8 tally is pending at entry


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class Handle(object):
    """A resident handle with R chains, all at the initial values, its oracle and the oracle's copy of the chains"""

    def __init__(self, name, R, seed=pt.SEED):
        build, hbv, self.se = pt.GRAPHS[name]
        self.name, self.seed, self.R = name, seed, R
        _, self.fg = session(build(), seed=seed, head_by_vid=hbv)
        fg = self.fg
        self.og = oracle_of(fg, hbv)
        # the generators the tests without a GPU ran their mirrors with are this handle's
        assert np.array_equal(np.load(pt.GOLDEN)[name], pt.device_generators(fg))
        self.color = fg.colors()
        self.L, self.h = _lib.lib(), fg._engine()
        fg._push(0, 0)                      # the one full upload
        if R > 1:
            _lib.check(self.L.nsk_set_chains(self.h, R))
        vv, _, self.w0, cnt = self.og.initial_state()
        self.nvar, self.sweep = len(vv), 0
        self.x = [vv.copy() for _ in range(R)]
        self.cnt = [cnt.copy() for _ in range(R)]

    def close(self):
        self.fg.close()

    def value_bytes(self):
        iid, nid = np.zeros(self.nvar, np.int32), C.c_int64()
        _lib.check(self.L.nsk_graph_get_layout(self.h, _lib.ptr(iid), C.byref(nid)))
        return nid.value, self.fg.info()["value_bytes"]

    def values(self):
        out = np.empty((self.R, self.nvar), np.int64)
        _lib.check(self.L.nsk_chains_download(self.h, _lib.ptr(out), None))
        return out

    def counts(self):
        out = np.empty((self.R, len(self.cnt[0])), np.int64)
        _lib.check(self.L.nsk_chains_download(self.h, None, _lib.ptr(out)))
        return out

    def weights(self):
        w = np.empty(len(self.w0), np.float64)
        _lib.check(self.L.nsk_state_download(self.h, None, None, _lib.ptr(w), None))
        return w

    def tallied(self, n):
        """n tallied sweeps of every chain, on the device and in the oracle"""
        order, ps = phases_from_colors(self.color)
        _lib.check(self.L.nsk_gibbs_sweeps(self.h, n, int(self.se), 0))
        for s in range(n):
            for r in range(self.R):
                assert self.og.gibbs_dev(order, ps, self.x[r], self.w0, self.cnt[r], self.seed ^ (r << 32), self.sweep + s,
                                         bool(self.se), burnin=False) == 0
        self.sweep += n

    def call(self, betas, T, sps, uniforms, tally=-1, want_lp=True, want_acc=True):
        b = np.ascontiguousarray(betas, np.float64)
        u = None if uniforms is None else np.ascontiguousarray(uniforms, np.float64)
        lp = np.full((T, self.R), np.nan) if want_lp else None
        acc = np.full((T, self.R - 1), -7, np.int32) if want_acc else None
        rc = self.L.nsk_pt_sweeps(self.h, _lib.ptr(b), T, sps, int(self.se), _lib.ptr(u), tally, _lib.ptr(lp), _lib.ptr(acc))
        return rc, lp, acc

    def mirror(self, betas, T, sps, uniforms, tally=-1, lp=None):
        """the oracle's run from the oracle's copy of the chains, which it then becomes"""
        m = pt.Run(self.og, self.color, self.seed, self.x, self.w0, betas, T, sps, self.se, uniforms, tally, sweep0=self.sweep,
                   lp=lp, cnt0=self.cnt)
        self.x, self.cnt, self.sweep = [s.copy() for s in m.final], [c.copy() for c in m.cnt], m.sweep
        return m

    def same_state(self, what):
        got, cnt = self.values(), self.counts()
        for r in range(self.R):
            bad = np.nonzero(got[r] != self.x[r])[0]
            assert len(bad) == 0, (what, "chain", r, "differing variables", len(bad), bad[:12])
            assert np.array_equal(cnt[r], self.cnt[r]), (what, "the tally of chain", r)


def _uniforms(name, R):
    return pt.case_uniforms(name, R) if R > 1 else None


def _parity(H, betas, T, sps, uniforms, tally):
    """one call on a handle that has tallied; the mirror is driven by the device's log-potentials"""
    R = H.R
    H.tallied(PRE)
    w_before, done0 = H.weights(), H.fg.info()["sweeps_done"]
    cnt_before = np.stack(H.cnt)
    rc, lp, acc = H.call(betas, T, sps, uniforms, tally)
    _lib.check(rc)
    u = np.zeros((T, 0)) if uniforms is None else uniforms
    # the decisions: the rule, on the device's rows, with the specified exp
    for t in range(T):
        want = pt_swap_rule(betas, lp[t], u[t], t, exp=orc.exp_det)
        assert np.array_equal(want, acc[t]), (t, want, acc[t])
    m = H.mirror(betas, T, sps, u, tally, lp=lp)
    print("%s R %d: accepted %d refused %d of %d proposed, swaps of differing states %d, bound %.3g" %
          (H.name, R, (acc == 1).sum(), (acc == 0).sum(), (acc >= 0).sum(), sum(m.differing), m.bound.max()))
    assert (np.abs(lp - m.lp) <= m.bound).all(), np.abs(lp - m.lp) / m.bound
    # the mirror's own decisions, from its own sums, are the device's: no decision lies near a tie
    assert m.safe.all() and np.array_equal(m.own, acc)
    H.same_state(("behind the call", H.name, R))
    assert H.fg.info()["sweeps_done"] == done0 + T * sps and H.sweep == PRE + T * sps
    # only the tallied chain's counts have grown, by one a sweep and variable at the most
    for r in range(R):
        grown = m.cnt[r] - cnt_before[r]
        assert (grown.any() and grown.max() <= T * sps) if r == tally else not grown.any()
    assert np.array_equal(_bits(H.weights()), _bits(w_before)) and w_before.any()
    # the next plain call goes on where the mirror goes on: the sweep index, the base weights, the tables
    H.tallied(2)
    H.same_state(("behind the following sweeps", H.name, R))
    return m, lp, acc


@pytest.mark.parametrize("R", pt.CHAINS)
@pytest.mark.parametrize("name", pt.PARITY_GRAPHS)
def test_parity_with_the_oracle(name, R):
    H = Handle(name, R)
    try:
        if name in pt.SLOTS:
            assert H.value_bytes() == pt.SLOTS[name]
        T = pt.case_steps(R)
        m, lp, acc = _parity(H, pt.case_betas(name, R), T, pt.SPS, _uniforms(name, R), pt.case_tally(name, R))
        assert acc.shape == (T, R - 1)
        if R > 1:
            assert (acc == 1).any() and (acc == 0).any() and sum(m.differing) > 0
            assert ((acc[0::2, 0::2] >= 0).all() and (acc[0::2, 1::2] == -1).all() and (acc[1::2, 0::2] == -1).all() and
                    (acc[1::2, 1::2] >= 0).all())
    finally:
        H.close()


@pytest.mark.parametrize("cap", [None, "1"])
def test_equal_betas_accept_every_proposal_and_the_swap_loops(cap, monkeypatch):
    """d = 0 for every pair: every proposal is accepted whatever the uniform, and the states are the permutation the even-odd
    scheme gives.  9473 value bytes a chain: with the swap's grid capped at one block, its 256 lanes make three trips of
    whole accesses (592 of them) and lane 0 of block 0 takes the byte behind; uncapped, three blocks make one trip."""
    if cap:
        monkeypatch.setenv("NSK_DIAG", "1")
        monkeypatch.setenv("NSK_PT_SWAP_GRID_CAP", cap)
    R, T = 5, 4
    H = Handle("grid_96", R)
    try:
        assert H.value_bytes() == pt.SLOTS["grid_96"] and 9473 // 16 > 2 * 256
        betas, u = np.full(R, 0.7), np.random.RandomState(1).random_sample((T, R - 1))
        x0 = [s.copy() for s in H.x]
        rc, lp, acc = H.call(betas, T, 1, u)
        _lib.check(rc)
        assert ((acc == 1) == (acc >= 0)).all() and (acc == 1).sum() == 2 * T
        m = H.mirror(betas, T, 1, u, lp=lp)
        assert np.array_equal(m.own, acc) and m.safe.all() and sum(m.differing) == 2 * T
        assert (np.abs(lp - m.lp) <= m.bound).all()
        H.same_state("behind the call")
        # the states are the permutation: the same chains swept without swaps, dealt to the slots of pt_paths -- except
        # that a moved state goes on under its new slot's stream, so the check is on the first step only
        still = pt.Run(H.og, H.color, H.seed, x0, H.w0, betas, 1, 1, H.se, u[:1], swaps=False)
        where = pt_paths(acc[:1])[0][0]
        assert where.tolist() == [1, 0, 3, 2, 4] == pt.permutation(acc[:1], R)
        for s in range(R):
            assert np.array_equal(m.states[0][s], still.final[where[s]]) and (s == 4 or not np.array_equal(m.states[0][s], still.final[s]))
    finally:
        H.close()


def test_a_call_leaves_tallies_memory_and_the_log_potential_alone():
    H = Handle("grid_w1.0", 3)
    try:
        L, h, R = H.L, H.h, H.R
        H.tallied(5)
        lp0 = np.zeros(R)
        _lib.check(L.nsk_log_potential(h, _lib.BUF_VALUE, 0, R, _lib.ptr(lp0)))      # warm: the records of the factor walk stay
        H.values()                                                                  # ... and the staging of the state transfers
        cnt0, bytes0 = H.counts(), H.fg.info()["device_bytes"]
        betas, u = pt.case_betas("grid_w1.0", R), pt.case_uniforms("grid_w1.0", R)
        T = len(u)
        rc, lp, acc = H.call(betas, T, pt.SPS, u, -1)
        _lib.check(rc)
        assert H.fg.info()["device_bytes"] == bytes0
        assert np.array_equal(H.counts(), cnt0) and cnt0.max() > 0
        H.mirror(betas, T, pt.SPS, u, -1, lp=lp)
        H.same_state("behind an untallied call")
        # the log-potential of the states the call left is what the call's own walk would give: same kernels, same bits
        lp1 = np.zeros(R)
        _lib.check(L.nsk_log_potential(h, _lib.BUF_VALUE, 0, R, _lib.ptr(lp1)))
        one = np.full((1, R), np.nan)
        zero, u0 = np.zeros(R), np.zeros((1, R - 1))
        # (betas of 0 weights: the sweep draws uniformly, the score is under the base weights all the same)
        rc = L.nsk_pt_sweeps(h, _lib.ptr(zero), 1, 1, int(H.se), _lib.ptr(u0), -1, _lib.ptr(one), None)
        _lib.check(rc)
        lp2 = np.zeros(R)
        _lib.check(L.nsk_log_potential(h, _lib.BUF_VALUE, 0, R, _lib.ptr(lp2)))
        acc1 = pt_swap_rule(zero, one[0], np.zeros(R - 1), 0, exp=orc.exp_det)
        assert acc1.tolist() == [1, -1]                                             # equal betas: accepted
        assert np.array_equal(_bits(lp2[[1, 0, 2]]), _bits(one[0])) and len(np.unique(lp1)) > 1
        # with outputs left out the same call is served, and with a tallied chain only that chain's counts move
        cnt1 = H.counts()
        rc, _, _ = H.call(betas, T, pt.SPS, u, 1, want_lp=False, want_acc=False)
        _lib.check(rc)
        cnt2 = H.counts()
        assert np.array_equal(cnt2[[0, 2]], cnt1[[0, 2]]) and (cnt2[1] - cnt1[1]).max() > 0
        assert H.fg.info()["device_bytes"] == bytes0
    finally:
        H.close()


def test_the_launches_are_those_of_the_chains_sweeps():
    R, T = 3, 4
    H, one = Handle("grid_w1.0", R), Handle("grid_w1.0", 1)
    try:
        L = H.L
        ms, n1, nR = C.c_double(), C.c_int64(), C.c_int64()
        betas, u = pt.case_betas("grid_w1.0", R), np.random.RandomState(2).random_sample((T, R - 1))
        _lib.check(L.nsk_gibbs_sweeps(one.h, 1, 0, 1))                 # (the first call carries the one-time set-up)
        _lib.check(L.nsk_profile_begin(one.h))
        for t in range(T):
            _lib.check(L.nsk_gibbs_sweeps(one.h, pt.SPS, 0, 1))
        _lib.check(L.nsk_profile_end(one.h, C.byref(ms), C.byref(n1)))
        _lib.check(H.call(betas, 1, 1, u[:1])[0])
        _lib.check(L.nsk_profile_begin(H.h))
        _lib.check(H.call(betas, T, pt.SPS, u)[0])
        _lib.check(L.nsk_profile_end(H.h, C.byref(ms), C.byref(nR)))
        assert n1.value > 0 and nR.value == R * n1.value, (n1.value, nR.value)
    finally:
        H.close()
        one.close()


def test_refusals_leave_the_handle_as_it_was():
    H = Handle("grid_w1.0", 3)
    try:
        L, h = H.L, H.h
        H.tallied(2)
        v0, w0, c0, done0 = H.values(), H.weights(), H.counts(), H.fg.info()["sweeps_done"]
        good, uni = np.array([0.2, 0.5, 1.0]), np.full((3, 2), 0.5)

        def call(betas=good, nsteps=3, sps=1, uniforms=uni, tally=-1, handle=h):
            b = None if betas is None else np.ascontiguousarray(betas, np.float64)
            u = None if uniforms is None else np.ascontiguousarray(uniforms, np.float64)
            return L.nsk_pt_sweeps(handle, _lib.ptr(b), nsteps, sps, 0, _lib.ptr(u), tally, None, None)

        assert call(handle=None) == _lib.E_INVALID
        assert call(betas=None) == _lib.E_INVALID
        for n in (0, -1, 65537):
            assert call(nsteps=n, uniforms=np.full((max(n, 1), 2), 0.5)) == _lib.E_INVALID
        assert call(sps=0) == _lib.E_INVALID
        assert call(sps=(2 ** 31 - 1) // 3 + 1) == _lib.E_INVALID
        for bad in (float("nan"), float("inf"), -0.25):
            for k in range(3):
                b = good.copy()
                b[k] = bad
                assert call(betas=b) == _lib.E_INVALID
        assert call(uniforms=None) == _lib.E_INVALID
        for bad in (float("nan"), -0.01, 1.0, float("inf")):
            for k in (0, 5):                    # the first and the last: all are checked
                u = uni.copy()
                u.ravel()[k] = bad
                assert call(uniforms=u) == _lib.E_INVALID
                assert "uniform" in L.nsk_last_error().decode()
        for bad in (-2, 3, 1024):
            assert call(tally=bad) == _lib.E_INVALID
        # a handle that records a sample trace
        _lib.check(L.nsk_trace_setup(h, None, 0, 1, 4))
        assert call() == _lib.E_INVALID and "trace" in L.nsk_last_error().decode()
        _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
        assert np.array_equal(H.values(), v0) and np.array_equal(_bits(H.weights()), _bits(w0)) and np.array_equal(H.counts(), c0)
        assert H.fg.info()["sweeps_done"] == done0
        # the generator too: the next sweeps are the mirror's next
        H.tallied(1)
        H.same_state("behind the refusals")
        assert call() == _lib.OK and call(tally=2) == _lib.OK
        assert H.fg.info()["sweeps_done"] == done0 + 1 + 6
    finally:
        H.close()
    # the sequential scan
    build, hbv, _ = pt.GRAPHS["grid_w1.0"]
    _, fg = session(build(), seed=3, scan="sequential")
    try:
        fg._push(0, 0)
        one = np.ones(1)
        assert _lib.lib().nsk_pt_sweeps(fg._engine(), _lib.ptr(one), 1, 1, 0, None, -1, None, None) == _lib.E_INVALID
    finally:
        fg.close()


# ------------------------------------------------------------------------------------------------------- the Python API
def test_parallel_tempering_is_the_mirror():
    build, hbv, se = pt.GRAPHS["grid_w1.0"]
    R, T, sps = 4, 10, 2
    _, fg = session(build(), seed=5, chains=R)
    try:
        og, color = oracle_of(fg, hbv), fg.colors()
        w0, x0, count0 = og.initial_state()[2], fg.var_value.copy(), fg.count.copy()
        betas = pt.pt_ladder(R, 0.2)
        with pytest.raises(ValueError):
            fg.parallel_tempering(betas[:3], T)
        with pytest.raises(ValueError):
            fg.parallel_tempering(betas, T, target=R)
        res = fg.parallel_tempering(betas, T, sweeps=sps, seed=11)
        u = np.random.RandomState(11).random_sample((T, R - 1))
        assert np.array_equal(res["uniforms"], u)
        m = pt.Run(og, color, 5, x0, w0, betas, T, sps, se, u, lp=res["lp"])
        assert np.array_equal(m.own, res["accepted"]) and m.safe.all() and (np.abs(res["lp"] - m.lp) <= m.bound).all()
        assert np.array_equal(fg.var_value, np.stack(m.final)) and np.array_equal(fg.count, count0)
        acc = res["accepted"]
        assert (acc == 1).any() and (acc == 0).any()
        rate = (acc == 1).sum(axis=0) / (acc >= 0).sum(axis=0)
        assert np.array_equal(res["swap_rate"], rate)
        paths, trips = pt_paths(acc)
        assert np.array_equal(res["paths"], paths) and np.array_equal(res["round_trips"], trips)
        assert sorted(res) == sorted(["lp", "accepted", "swap_rate", "paths", "round_trips", "uniforms"])
        # with a target the cold chain's tally reaches count, as a chain's reaches it from inference(var_copy="all")
        x1 = fg.var_value.copy()
        res = fg.parallel_tempering(betas, T, sweeps=sps, seed=12, target=R - 1)
        u = np.random.RandomState(12).random_sample((T, R - 1))
        m2 = pt.Run(og, color, 5, x1, w0, betas, T, sps, se, u, tally_chain=R - 1, sweep0=m.sweep, lp=res["lp"])
        assert np.array_equal(m2.own, res["accepted"]) and m2.safe.all()
        assert np.array_equal(fg.var_value, np.stack(m2.final))
        assert np.array_equal(fg.count, count0 + m2.tally[R - 1]) and m2.tally[R - 1].max() > 0
        assert np.array_equal(fg.chain_count, m2.tally) and not m2.tally[:R - 1].any()
    finally:
        fg.close()
