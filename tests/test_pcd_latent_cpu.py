"""Host side of PCD with latent variables (FactorGraph.learn_pcd(clamped=K), nsk_pcd_latent_steps): the numpy rule against
a hand-written loop, the liveliness of every case the GPU tests hold the device to (tests/pcd_latent.py: the mirror), the
exact likelihood of what the learner learns with the oracle as the sampler, the argument errors raised before a device is
touched and the declarations (no GPU)."""

import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import pcd_latent_step, pcd_step
import pcd
import pcd_latent as pl
import temper
from util import REPO, session, oracle_of

# the likelihood run (deterministic: the oracle's runs are functions of the seed)
LIK_CHAINS, LIK_CLAMPED, LIK_STEPS, LIK_SWEEPS, LIK_STEP, LIK_DECAY, LIK_SEED = 64, 32, 40, 2, 0.5, 0.97, 5


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------- (a) the rule
def _step_by_hand(w, fixed, Mc, K, Mf, Rf, n_w, step, reg, normalize):
    """every operation exact in fractions and rounded once by float()"""
    F = Fraction
    out, gmax = [], 0.0
    for i in range(len(w)):
        if fixed[i]:
            out.append(float(w[i]))
            continue
        mc = float(F(float(F(int(Mc[i])))) * F(1, 2 ** 32))            # the conversion, then the exact scaling
        mc = float(F(mc) / F(K))
        mf = float(F(float(F(int(Mf[i])))) * F(1, 2 ** 32))
        mf = float(F(mf) / F(Rf))
        g = float(F(mc) - F(mf))
        if normalize:
            g = float(F(g) / F(max(int(n_w[i]), 1)))
        a = float(F(float(reg)) * F(float(w[i])))
        b = float(F(g) - F(a))
        c = float(F(float(step)) * F(b))
        out.append(float(F(float(w[i])) + F(c)))
        gmax = max(gmax, abs(g))
    return out, gmax


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("reg", [0.0, 0.01])
def test_pcd_latent_step_is_the_rule(normalize, reg):
    rng = np.random.default_rng(2)
    nw, K, Rf = 9, 3, 7
    w = rng.normal(0, 1, nw)
    fixed = np.zeros(nw, bool)
    fixed[[2, 6]] = True
    n_w = np.array([3, 1, 5, 0, 17, 2048, 2, 2049, 1])                # weight 3 has no factor
    Mc = (rng.normal(0, 1, nw) * n_w * K * 2.0 ** 32).astype(np.int64)
    Mf = (rng.normal(0, 1, nw) * n_w * Rf * 2.0 ** 32).astype(np.int64)
    step = np.float64(0.3)
    for t in range(3):                                                  # decay: the products formed in t order
        got, gmax = pcd_latent_step(w, fixed, Mc, K, Mf, Rf, n_w, step, reg, normalize)
        want, wmax = _step_by_hand(w, fixed, Mc, K, Mf, Rf, n_w, step, reg, normalize)
        assert np.array_equal(_bits(got), _bits(want)) and _bits(gmax) == _bits(wmax)
        assert np.array_equal(_bits(got[fixed]), _bits(w[fixed]))
        moving = ~fixed & ((Mc != 0) | (Mf != 0) | (reg > 0))
        assert (got[moving] != w[moving]).all() and moving.sum() >= 6
        # pcd_step with the clamped mean as its target and the free chains as its chains
        mc = (Mc.astype(np.float64) * 2.0 ** -32) / np.float64(K)
        alt, amax = pcd_step(w, fixed, Mf, Rf, mc, n_w, step, reg, normalize)
        assert np.array_equal(_bits(got), _bits(alt)) and _bits(gmax) == _bits(amax)
        w, step = got, step * np.float64(0.9)
        Mc, Mf = Mc // 2 - 12345, Mf // 3 + 777
    assert pcd_latent_step(w, np.ones(nw, bool), Mc, K, Mf, Rf, n_w, step, reg, normalize)[1] == 0.0
    with pytest.raises(ValueError):
        pcd_latent_step(w, fixed, Mc.astype(np.float64), K, Mf, Rf, n_w, step, reg, normalize)
    with pytest.raises(ValueError):
        pcd_latent_step(w, fixed, Mc, 0, Mf, Rf, n_w, step, reg, normalize)


# ------------------------------------------------------------------------------------------------------- (b) liveliness
def _host_case(graph, hbv, seed=pl.SEED):
    _, fg = session(graph, seed=seed, head_by_vid=hbv)
    og = oracle_of(fg, hbv, layout=False)
    color, _ = fg.plan()
    assert og.check_coloring(color) == (-1, -1)
    return fg, og, color


def _mirror_case(name, R, K, calls, steps=pl.STEPS, clamp=True, free_se=1):
    build, hbv, _ = pcd.GRAPHS[name]
    fg, og, color = _host_case(build(), hbv)
    vv, _, w0, _ = og.initial_state()
    x, sweep = pl.disturbed(og, color, pl.SEED, [vv] * R, w0)
    w, runs = w0, []
    for sps, normalize, reg in calls:
        m = pl.Run(og, color, pl.SEED, x, w, K, steps, sps, free_se, pcd.stepsize(normalize), pl.DECAY, reg, normalize, sweep0=sweep, clamp=clamp)
        x, w, sweep = m.final, m.w, m.sweep
        runs.append(m)
    return fg, og, color, runs


@pytest.mark.parametrize("RK", pl.PARITY_CHAINS, ids=lambda rk: "R%d_K%d" % rk)
@pytest.mark.parametrize("name", pl.PARITY_GRAPHS)
def test_the_parity_cases_are_lively(name, RK):
    R, K = RK
    fg, og, color, runs = _mirror_case(name, R, K, pl.parity_calls(name, RK))
    free = ~og.weight["isFixed"].astype(bool)
    assert free.any() and pl.evidence_mask(og).any() and not pl.evidence_mask(og).all()
    assert runs[0].restored, "the disturbance left the clamped rows' evidence at the initial values"
    for m in runs:
        # populations of one or two chains of a dozen variables now and then sit still through a step's sweeps
        assert m.lively(free, 1, most=min(K, R - K) <= 2), (m.moved_latent, m.moved_free, m.moved_free_evidence, m.weights, m.moments)
        assert np.array_equal(_bits(m.w[~free]), _bits(m.w0[~free]))
    # every free weight changes in the course of the case (in each call from three chains on)
    assert (runs[0].changed_weights(free) | runs[1].changed_weights(free)).all()
    assert R < 3 or all(m.changed_weights(free).all() for m in runs)
    # which of the two paths a population of several chains takes (pl.BATCHED): both are among the parity cases
    assert pl.all_tables(fg.plan_routes(), color) == pl.BATCHED[name]


def test_the_grids_of_the_batched_launches():
    """the sampled variables of the launch-count graph and of the handle graph route to tables, evidence or not: under
    both sample_evidence flags; and the restated factor values of a grid are eval_factor's"""
    for g in (pl.launch_graph(), pl.handle_graph()):
        fg, og, color = _host_case(g, False)
        assert pl.all_tables(fg.plan_routes(), color) and (np.asarray(color) >= 0).all()
        ev = pl.evidence_mask(og)
        assert ev.any() and not ev.all() and not og.weight["isFixed"].any()
    fg, og, color = _host_case(graphgen.ising_grid(3, 5, weight=0.3, two_weights=True), False)
    for x in np.random.default_rng(6).integers(0, 2, (3, 15)):
        assert np.array_equal(_bits(pl.equal_values(og, x)), _bits(pcd.factor_values(og, x)))


def test_the_block_edge_case_is_lively():
    """tests/test_pcd_latent_gpu.py test_the_update_across_a_block_edge: the mirror alone moves a free weight, its two
    rows of moments differ, the moments differ between the steps, and weights on both sides of the edge move"""
    fg, og, color = _host_case(pl.edge_graph(), True)
    R, K = pl.EDGE_RK
    vv, _, w0, _ = og.initial_state()
    free = ~og.weight["isFixed"].astype(bool)
    assert len(w0) == pl.EDGE_WEIGHTS == 257 and not free[list(pl.EDGE_FIXED)].any() and free.sum() == 257 - len(pl.EDGE_FIXED)
    x, sweep = pl.disturbed(og, color, pl.SEED, [vv] * R, w0)
    m = pl.Run(og, color, pl.SEED, x, w0, K, pl.EDGE_STEPS, 1, 1, pcd.stepsize(1), pl.DECAY, 0.01, 1, sweep0=sweep)
    assert (m.w[free] != w0[free]).any() and (m.moments[:, 0] != m.moments[:, 1]).any() and (m.moments[0] != m.moments[1]).any()
    assert (m.w[:256] != w0[:256]).any() and m.w[256] != w0[256]
    assert np.array_equal(_bits(m.w[~free]), _bits(w0[~free]))


def test_the_clamp_cases_are_lively():
    """tests/test_pcd_latent_gpu.py test_clamp: 5 chains, 2 clamped, with and without the reset"""
    for clamp in (True, False):
        fg, og, color, runs = _mirror_case("mixed_clamped", 5, 2, [(1, 1, 0.01)], clamp=clamp)
        m = runs[0]
        ev, init = pl.evidence_mask(og), og.variable["initialValue"].astype(np.int64)
        assert m.restored == clamp
        kept = [bool((x[ev] == init[ev]).all()) for x in m.final]
        # (three evidence variables: a free row now and then meets their initial values, not all three rows at once)
        assert kept[:2] == [clamp, clamp] and not all(kept[2:])
        assert m.lively(~og.weight["isFixed"].astype(bool), 1, most=True)


# ------------------------------------------------------------------------------------------------------- (c) likelihood
def _exact_gradient(og, w, ev, init):
    """E[S | evidence] - E[S] per weight by enumeration of the 2^nvar states (binary variables, EQUAL factors)"""
    n = len(og.variable)
    states = (np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1
    vid = og.fmap["vid"].astype(np.int64)
    e = np.where(states[:, vid[0::2]] == states[:, vid[1::2]], 1.0, -1.0)
    S = np.zeros((len(states), len(w)))
    np.add.at(S.T, og.factor["weightId"].astype(np.int64), e.T)
    U = S @ w

    def mean(mask):
        p = np.exp(U[mask] - U[mask].max())
        return (p[:, None] * S[mask]).sum(axis=0) / p.sum()

    return mean((states[:, ev] == init[ev]).all(axis=1)) - mean(np.ones(len(states), bool))


def _log_likelihood(og, w, ev, init):
    return temper.exact_log_z(og, w, init, ~ev) - temper.exact_log_z(og, w, init, np.ones(len(ev), bool))


def test_the_learner_raises_the_exact_likelihood_of_the_evidence():
    """The mirror's run on pl.likelihood_graph() (a 3 x 4 grid, 6 of 12 variables observed, one free weight from 0.6):
    LIK_CHAINS chains, LIK_CLAMPED of them clamped, LIK_STEPS steps of LIK_SWEEPS sweeps a phase, stepsize LIK_STEP
    decaying by LIK_DECAY, normalize on, the free phase sampling the evidence variables.  It gave
        exact log P(evidence | w):   w_0 = 0.6 -> -5.237789, learned w = 0.141853 -> -4.084566
        largest |exact gradient|:    w_0 -> 5.869501, learned -> 0.046937
    (the oracle is deterministic: this is not a statistical test)."""
    fg, og, color = _host_case(pl.likelihood_graph(), False, seed=LIK_SEED)
    vv, _, w0, _ = og.initial_state()
    ev, init = pl.evidence_mask(og), og.variable["initialValue"].astype(np.int64)
    assert int(ev.sum()) == 6 and len(w0) == 1 and not og.weight["isFixed"].any()
    x = np.random.default_rng(1).integers(0, 2, len(vv))
    assert np.array_equal(_bits(pl.equal_values(og, x)), _bits(pcd.factor_values(og, x)))
    m = pl.Run(og, color, LIK_SEED, [vv] * LIK_CHAINS, w0, LIK_CLAMPED, LIK_STEPS, LIK_SWEEPS, 1, LIK_STEP, LIK_DECAY, 0.0, 1,
               values=pl.equal_values)
    ll0, ll1 = _log_likelihood(og, w0, ev, init), _log_likelihood(og, m.w, ev, init)
    g0, g1 = np.abs(_exact_gradient(og, w0, ev, init)).max(), np.abs(_exact_gradient(og, m.w, ev, init)).max()
    print("weights %s -> %s; log-likelihood %.6f -> %.6f; largest |gradient| %.6f -> %.6f" % (w0, m.w, ll0, ll1, g0, g1))
    # the enumeration's gradient is the derivative of the enumeration's log-likelihood
    h = 1e-5
    num = (_log_likelihood(og, w0 + h, ev, init) - _log_likelihood(og, w0 - h, ev, init)) / (2 * h)
    assert abs(num - _exact_gradient(og, w0, ev, init)[0]) < 1e-6
    assert ll1 > ll0
    assert g1 < g0


# ------------------------------------------------------------------------------------------------------- the Python API
def test_argument_errors_come_before_the_device():
    _, fg = session(pcd.learnable(temper.clamped_grid()), chains=3)
    for kw in (dict(clamped=3), dict(clamped=-1), dict(clamped=4), dict(clamped=1, target=[0.5]), dict(clamped=1, epochs=0),
               dict(clamped=1, sweeps=0), dict(clamped=2, epochs=65536, sweeps=16384), dict(clamped=1, stepsize=float("nan")),
               dict(clamped=1, reg_param=-0.1), dict(clamped=1, decay=float("inf"))):
        args = dict(epochs=3, stepsize=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            fg.learn_pcd(**args)
    for chains in ((0, 4), (-1, 1), (3, 1), (1, 0), (2, 2)):
        with pytest.raises(ValueError):
            fg.weight_moments(chains=chains)
    with pytest.raises(ValueError):
        fg.weight_moments(chains=(0, 1), evidence_chain=True)
    assert fg._handle is None
    _, one = session(pcd.learnable(temper.clamped_grid()))
    with pytest.raises(ValueError):
        one.learn_pcd(3, 0.1, clamped=1)                # one row: no free population
    assert one._handle is None


def test_header_declares_and_library_exports_the_entry_point():
    hdr = open(os.path.join(REPO, "include", "numbskull_amd.h")).read()
    assert re.search(r"\bint nsk_pcd_latent_steps\(nsk_graph \*g, int64_t nclamped, int clamp,\s*int64_t nsteps, int64_t sweeps_per_step, "
                     r"int free_sample_evidence,\s*double step, double decay, double reg_param, int normalize,\s*double \*gmax /\*[^*]*\*/,\s*"
                     r"int64_t \*moments /\*[^*]*\*/\);", hdr)
    lib = C.CDLL(_lib.LIB_PATH)
    assert "nsk_pcd_latent_steps" in _lib.SYMBOLS and hasattr(lib, "nsk_pcd_latent_steps")
    assert _lib.lib().nsk_pcd_latent_steps.argtypes == [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_double,
                                                        C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
