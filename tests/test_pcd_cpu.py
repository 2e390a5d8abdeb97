"""Host side of PCD learning (FactorGraph.weight_moments / learn_pcd, nsk_weight_moments, nsk_pcd_steps): the numpy
restatement of the moments and of the update against hand-written loops in Python ints and fractions, the liveliness of
every case the GPU tests hold the device to (tests/pcd.py: the mirror), the recovery of planted weights with the oracle as
the sampler, the argument errors raised before a device is touched and the declarations (no GPU).

Recovery (deterministic: the oracle's runs are functions of the seeds).  RECOVERY_PAIRS independent pairs
(graphgen.ising_pairs) at the planted weights (1.0, 1.0, 0.5); the target is the pair count times the exact moments of a
pair (enumeration of its four states); RECOVERY_CHAINS chains from the weights 0, RECOVERY_STEPS steps of one sweep,
stepsize RECOVERY_STEP decaying by RECOVERY_DECAY a step, normalize on.  Measured final max |w - planted| over the chain
seeds 1000, 1017, ..., 1119:
    0.007095, 0.006180, 0.004328, 0.007194, 0.003267, 0.003168, 0.010067, 0.002665
The bound asserted on every run is twice the largest of them, RECOVERY_BOUND = 0.020134, which lies below 0.1 -- a fifth of the
smallest planted weight; a learner that does not move ends at 0.5 to 1.0."""

import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import moment_counts, pcd_step
import pcd
import temper
from util import REPO, session, oracle_of

RECOVERY_PAIRS, RECOVERY_CHAINS, RECOVERY_STEPS, RECOVERY_STEP, RECOVERY_DECAY = 500, 8, 300, 0.5, 0.99
RECOVERY_SEEDS = tuple(1000 + 17 * k for k in range(8))
RECOVERY_MEASURED = (0.007095, 0.006180, 0.004328, 0.007194, 0.003267, 0.003168, 0.010067, 0.002665)
RECOVERY_BOUND = 2 * max(RECOVERY_MEASURED)
PLANTED = (1.0, 1.0, 0.5)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------- (a) the rules
def _counts_by_hand(values, wid, nweight):
    M = [0] * nweight
    for row in values:
        for e, w in zip(row, wid):
            M[int(w)] += round(Fraction(float(e)) * 2 ** 32)           # (round() of a Fraction: to nearest, ties to even)
    return M


def _step_by_hand(w, fixed, M, R, target, n_w, step, reg, normalize):
    """every operation exact in fractions and rounded once by float()"""
    F = Fraction
    out, gmax = [], 0.0
    for i in range(len(w)):
        if fixed[i]:
            out.append(float(w[i]))
            continue
        m = float(F(float(F(int(M[i])))) * F(1, 2 ** 32))              # the conversion, then the exact scaling
        m = float(F(m) / F(R))
        g = float(F(float(target[i])) - F(m))
        if normalize:
            g = float(F(g) / F(max(int(n_w[i]), 1)))
        a = float(F(float(reg)) * F(float(w[i])))
        b = float(F(g) - F(a))
        c = float(F(float(step)) * F(b))
        out.append(float(F(float(w[i])) + F(c)))
        gmax = max(gmax, abs(g))
    return out, gmax


def test_moment_counts_is_the_rule():
    rng = np.random.default_rng(0)
    wid = np.array([0, 2, 2, 5, 5, 5, 0, 2])
    # integers, non-integers, negatives, exact ties of the rounding (k + 1/2) * 2^-32 both ways
    e = np.stack([rng.integers(-3, 4, 8).astype(np.float64), rng.normal(0, 2, 8), -np.log(np.arange(2, 10.0)), np.array([50.5, 0, 0, 0, 0, 0, 50.25, 0]),
                  np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3.5, -2.5, 4.5]) * 2.0 ** -32])
    got = moment_counts(e, wid, 7)
    assert got.dtype == np.int64 and got.tolist() == _counts_by_hand(e, wid, 7)
    assert got[1] == got[3] == got[4] == got[6] == 0                    # weights without a factor read 0
    assert (got < 0).any() and (got > 0).any()
    assert moment_counts(e[4], wid, 7).tolist() == _counts_by_hand(e[4:5], wid, 7)      # one chain, one dimension
    assert moment_counts(e[4], wid, 7).tolist() == [0 - 2, 0, 2 + 2 + 4, 0, 0, 0 - 2 + 4, 0]       # ties go to even
    # the sum over chains is the sum of the chains' counts, in any order
    assert np.array_equal(got, sum(moment_counts(e[[r]], wid, 7) for r in (2, 0, 4, 3, 1)))
    with pytest.raises(IndexError):
        moment_counts(e, wid, 5)
    with pytest.raises(ValueError):
        moment_counts(e, wid[:-1], 7)
    with pytest.raises(OverflowError):
        moment_counts(np.array([[np.inf] * 8]), wid, 7)


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("reg", [0.0, 0.01])
def test_pcd_step_is_the_rule(normalize, reg):
    rng = np.random.default_rng(1)
    nw, R = 9, 7
    w = rng.normal(0, 1, nw)
    fixed = np.zeros(nw, bool)
    fixed[[2, 6]] = True
    n_w = np.array([3, 1, 5, 0, 17, 2048, 2, 2049, 1])                # weight 3 has no factor
    M = (rng.normal(0, 1, nw) * n_w * R * 2.0 ** 32).astype(np.int64)   # negative moments among them
    M[3] = 0
    target = rng.normal(0, 1, nw) * n_w
    target[3] = 0.7
    step = np.float64(0.3)
    for t in range(3):                                                  # decay: the products formed in t order
        got, gmax = pcd_step(w, fixed, M, R, target, n_w, step, reg, normalize)
        want, wmax = _step_by_hand(w, fixed, M, R, target, n_w, step, reg, normalize)
        assert np.array_equal(_bits(got), _bits(want)) and _bits(gmax) == _bits(wmax)
        assert np.array_equal(_bits(got[fixed]), _bits(w[fixed])) and (got[~fixed] != w[~fixed]).all()
        # the weight without a factor: its moment is 0, so it moves by step * (target - reg * w); with no target it shrinks
        t0 = target.copy()
        t0[3] = 0.0
        shrunk = pcd_step(w, fixed, M, R, t0, n_w, step, reg, normalize)[0][3]
        assert (abs(shrunk) < abs(w[3])) if reg > 0 else (shrunk == w[3])
        w, step = got, step * np.float64(0.9)
        M = M // 2 - 12345
        M[3] = 0
    assert pcd_step(w, np.ones(nw, bool), M, R, target, n_w, step, reg, normalize)[1] == 0.0
    with pytest.raises(ValueError):
        pcd_step(w, fixed, M.astype(np.float64), R, target, n_w, step, reg, normalize)


# ------------------------------------------------------------------------------------------------------- (b) liveliness
def _mirror_case(name, R, calls, steps=pcd.STEPS, seed=9):
    build, hbv, se = pcd.GRAPHS[name]
    _, fg = session(build(), seed=seed, head_by_vid=hbv)
    og = oracle_of(fg, hbv, layout=False)
    color, _ = fg.plan()
    assert og.check_coloring(color) == (-1, -1)
    vv, _, w0, _ = og.initial_state()
    x, w, sweep, runs = [vv.copy() for _ in range(R)], w0, 0, []
    for sps, normalize, reg in calls:
        m = pcd.Run(og, color, seed, x, w, pcd.target_of(og), steps, sps, se, pcd.stepsize(normalize), pcd.DECAY, reg, normalize, sweep0=sweep)
        x, w, sweep = m.final, m.w, m.sweep
        runs.append(m)
    return og, runs


@pytest.mark.parametrize("R", pcd.PARITY_CHAINS)
@pytest.mark.parametrize("name", pcd.PARITY_GRAPHS)
def test_the_parity_cases_are_lively(name, R):
    og, runs = _mirror_case(name, R, pcd.parity_calls(name, R))
    free = ~og.weight["isFixed"].astype(bool)
    assert free.any()
    for m in runs:
        assert m.lively(free, most=R <= 3), (m.moved, m.weights, m.moments)
        assert np.array_equal(_bits(m.w[~free]), _bits(m.w0[~free]))


@pytest.mark.parametrize("name,R,steps", [("grid_w1.0", 1024, pcd.STEPS), ("ratio", 5, pcd.STEPS), ("cuts", 3, 4), ("trips", 2, 2)])
def test_the_other_cases_are_lively(name, R, steps):
    og, runs = _mirror_case(name, R, [(1, 1, 0.01)], steps=steps)
    free = ~og.weight["isFixed"].astype(bool)
    m = runs[0]
    assert m.lively(free), (m.moved, m.weights, m.moments)
    if name == "ratio":             # the factor values are really not integers: neither are the moments, in units of 2^32
        e = np.stack([pcd.factor_values(og, x) for x in m.final])
        assert (e != np.rint(e)).any() and (m.moments % 2 ** 32 != 0).any()
    if name == "cuts":
        n = pcd.factors_per_weight(og)
        assert tuple(n) == pcd.CUT_COUNTS and (np.flatnonzero(~free) == [pcd.CUT_FIXED]).all()
        assert (m.moments[:, 0] == 0).all() and abs(m.w[0]) < abs(m.w0[0])      # the weight without a factor shrinks
    if name == "trips":
        assert _lib.moments_trips(pcd.TRIP_SHORTS, _lib.MOMENTS_BLOCK, pcd.TRIP_CAP) == 3
        assert _lib.moments_trips(pcd.TRIP_PIECES, _lib.MOMENTS_BLOCK // 64, pcd.TRIP_CAP) == 3
        assert _lib.moments_trips(pcd.TRIP_SHORTS - 1, _lib.MOMENTS_BLOCK, pcd.TRIP_CAP) == 2
        assert _lib.moments_trips(pcd.TRIP_PIECES - 1, _lib.MOMENTS_BLOCK // 64, pcd.TRIP_CAP) == 2
        assert _lib.moments_trips(pcd.TRIP_SHORTS, _lib.MOMENTS_BLOCK) == 1 == _lib.moments_trips(pcd.TRIP_PIECES, _lib.MOMENTS_BLOCK // 64)


# ------------------------------------------------------------------------------------------------------- (c) recovery
def _pair_values(og, x):
    """the factor values of graphgen.ising_pairs, restated: ISTRUE(x), ISTRUE(y), EQUAL(x, y) a pair, each +1 / -1"""
    a, b = x[0::2], x[1::2]
    e = np.empty(3 * len(a))
    e[0::3], e[1::3], e[2::3] = 2.0 * a - 1.0, 2.0 * b - 1.0, np.where(a == b, 1.0, -1.0)
    return e


def _exact_pair_moments():
    a_, b_, c_ = PLANTED
    sx, sy = np.array([-1.0, -1.0, 1.0, 1.0]), np.array([-1.0, 1.0, -1.0, 1.0])
    se = np.where(sx == sy, 1.0, -1.0)
    p = np.exp(a_ * sx + b_ * sy + c_ * se)
    p /= p.sum()
    return np.array([(p * sx).sum(), (p * sy).sum(), (p * se).sum()])


def test_planted_weights_are_recovered_with_the_oracle_as_the_sampler():
    n = RECOVERY_PAIRS
    _, fg = session(graphgen.ising_pairs(n, *PLANTED, seed=3), seed=5)
    og = oracle_of(fg, layout=False)
    color, _ = fg.plan()
    assert og.check_coloring(color) == (-1, -1)
    vv, _, w0, _ = og.initial_state()
    assert not w0.any() and not og.weight["isFixed"].any()
    # the restatement, pinned once against eval_factor on the data and on a random state
    for x in (vv, np.random.default_rng(2).integers(0, 2, len(vv))):
        assert np.array_equal(_bits(_pair_values(og, x)), _bits(pcd.factor_values(og, x)))
    target = n * _exact_pair_moments()
    errs = []
    for seed in RECOVERY_SEEDS:
        m = pcd.Run(og, color, seed, [vv] * RECOVERY_CHAINS, w0, target, RECOVERY_STEPS, 1, True, RECOVERY_STEP, RECOVERY_DECAY, 0.0, 1,
                    values=_pair_values)
        errs.append(float(np.abs(m.w - PLANTED).max()))
        print("seed %d: weights %s max error %.6f first grad_max %.4f last %.4f" % (seed, m.w, errs[-1], m.gmax[0], m.gmax[-1]))
    print("max errors", ", ".join("%.6f" % e for e in errs), "bound", RECOVERY_BOUND)
    assert RECOVERY_BOUND < 0.1
    assert all(e <= RECOVERY_BOUND for e in errs), (errs, RECOVERY_BOUND)


# ------------------------------------------------------------------------------------------------------- the Python API
def test_argument_errors_come_before_the_device():
    _, fg = session(pcd.learnable(temper.clamped_grid()), chains=2)
    for kw in (dict(epochs=0), dict(epochs=65537), dict(sweeps=0), dict(epochs=65536, sweeps=32768), dict(stepsize=float("nan")),
               dict(decay=float("inf")), dict(reg_param=-0.1), dict(reg_param=float("nan")), dict(target=[0.0, 1.0]),
               dict(target=[float("nan")]), dict(target=[[0.5]])):
        args = dict(epochs=3, stepsize=0.1, target=[0.5])
        args.update(kw)
        with pytest.raises(ValueError):
            fg.learn_pcd(**args)
    with pytest.raises(ValueError):
        fg.weight_moments(var_copy="all", evidence_chain=True)
    assert fg._handle is None


def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(REPO, "include", "numbskull_amd.h")).read()
    assert re.search(r"\bint nsk_weight_moments\(nsk_graph \*g, int which, int64_t first_chain, int64_t nchains,\s*int64_t \*moments /\*[^*]*\*/\);", hdr)
    assert re.search(r"\bint nsk_pcd_steps\(nsk_graph \*g, const double \*target /\*[^*]*\*/,\s*int64_t nsteps, int64_t sweeps_per_step, "
                     r"int sample_evidence,\s*double step, double decay, double reg_param, int normalize,\s*double \*gmax /\*[^*]*\*/,\s*"
                     r"int64_t \*moments /\*[^*]*\*/\);", hdr)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("nsk_weight_moments", "nsk_pcd_steps"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert _lib.lib().nsk_pcd_steps.argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double,
                                                 C.c_int, C.c_void_p, C.c_void_p]
    # the launch arithmetic of csrc/nsk_kernels_pcd.h, restated in _lib
    src = open(os.path.join(REPO, "numbskull_amd", "csrc", "nsk_kernels_pcd.h")).read()
    assert "#define NSK_MOMENTS_MAX_BLOCKS %d" % _lib.MOMENTS_MAX_BLOCKS in src
    internal = open(os.path.join(REPO, "numbskull_amd", "csrc", "nsk_internal.h")).read()
    assert "#define NSK_WSTATS_SHORT %d " % _lib.MOMENTS_SHORT in internal and "#define NSK_WSTATS_PIECE %d " % _lib.MOMENTS_PIECE in internal
    assert [_lib.moments_blocks(n, 256) for n in (1, 2048, 2049, 10 ** 7)] == [8, 8, 16, 2048]
    assert [_lib.moments_blocks(10 ** 7, 256, cap) for cap in (1, 8, 15, 16, 4096)] == [8, 8, 8, 16, 2048]
