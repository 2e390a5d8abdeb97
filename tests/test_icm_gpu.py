"""Greedy MAP search on the device (nsk_icm, FactorGraph.icm / map_estimate).

Yardstick: the host ICM of tests/icm.py -- the oracle's potential() (pinned to the reference) per (variable, value), the
handle's own colouring and weights, and numbskull_amd.diagnostics.icm_choice.  The algorithm draws no random numbers, so
values, sweep counts and per-sweep change counts must EQUAL the host's.  tests/test_icm_cpu.py ties the host ICM to
brute-force enumeration."""

import ctypes as C

import numpy as np
import pytest

import numbskull_amd
from numbskull_amd import _lib, graphgen
from numbskull_amd.diagnostics import icm_choice
from icm import host_icm, joint_exponent
from test_conditionals_cpu import evidence_grid
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


def _same(res, sweeps, changed, what):
    """a FactorGraph.icm result of one copy against the host ICM's (sweeps in nsk_icm's signed convention)"""
    assert res["sweeps"] == abs(sweeps) and res["converged"] == (sweeps > 0), (what, res["sweeps"], sweeps)
    assert np.array_equal(res["changed"], changed), (what, res["changed"], changed)


# ---------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("name", GRAPHS)
def test_icm_equals_the_host_icm_bit_for_bit(golden, name):
    g, hbv = _graph(golden, name)
    _, fg = session(g, seed=SEED, head_by_vid=hbv)
    og = oracle_of(fg, hbv)
    color = fg.colors()
    fg.inference(2, 3, True)
    for ev in (False, True):
        want, sweeps, changed = host_icm(og, color, fg.var_value[0], fg.weight_value[0], 6, ev)
        evid, count = fg.var_value_evid[0].copy(), fg.count.copy()
        res = fg.icm(max_sweeps=6, sample_evidence=ev)
        print("%s free, sample_evidence=%s: sweeps %d, changed %s" % (name, ev, sweeps, changed.tolist()))
        assert np.array_equal(fg.var_value[0], want), (name, ev)
        _same(res, sweeps, changed, (name, ev))
        assert np.array_equal(fg.var_value_evid[0], evid) and np.array_equal(fg.count, count)
    fg.learn(1, 3, 0.01, 0.95, 2, 0.01, 1)
    for ev in (False, True):
        want, sweeps, changed = host_icm(og, color, fg.var_value_evid[0], fg.weight_value[0], 6, ev)
        free = fg.var_value[0].copy()
        res = fg.icm(max_sweeps=6, evidence_chain=True, sample_evidence=ev)
        assert np.array_equal(fg.var_value_evid[0], want), (name, ev, "evidence chain")
        _same(res, sweeps, changed, (name, ev, "evidence chain"))
        assert np.array_equal(fg.var_value[0], free)
    # the free chain once more, under the learned weights (the generated graphs start with all weights 0, where every
    # value ties and nothing moves)
    want, sweeps, changed = host_icm(og, color, fg.var_value[0], fg.weight_value[0], 6, True)
    res = fg.icm(max_sweeps=6, sample_evidence=True)
    assert np.array_equal(fg.var_value[0], want), (name, "free after learning")
    _same(res, sweeps, changed, (name, "free after learning"))


def test_values_outside_their_domain_start_from_zero(golden):
    g, _ = _graph(golden, "grid4x5")
    _, fg = session(g, seed=SEED)
    og = oracle_of(fg)
    x = np.random.default_rng(4).integers(0, 2, len(fg.variable))
    x[[3, 8, 16]] = [5, -3, 127]
    fg.var_value[0][:] = x
    want, sweeps, changed = host_icm(og, fg.colors(), x, fg.weight_value[0], 10, True)
    res = fg.icm(max_sweeps=10, sample_evidence=True)
    assert changed[0] >= 3 and want.min() >= 0 and want.max() <= 1
    assert np.array_equal(fg.var_value[0], want)
    _same(res, sweeps, changed, "grid4x5 with values outside their domain")


# ---------------------------------------------------------------------------------------------- B
def test_chains_converge_apart(golden):
    g, _ = _graph(golden, "grid57x33")
    _, fg = session(g, seed=SEED, chains=3)
    og = oracle_of(fg)
    color = fg.colors()
    nvar = len(fg.variable)
    rng = np.random.default_rng(12)
    fg.var_value[0][:] = 0                      # a fixed point of a ferromagnet
    fg.var_value[1][:] = rng.integers(0, 2, nvar)
    fg.var_value[2][:] = rng.integers(0, 2, nvar)
    start = fg.var_value.copy()
    res = fg.icm(var_copy="all", max_sweeps=40)
    assert res["changed"].shape == (3, 40) and res["sweeps"].shape == res["converged"].shape == (3,)
    assert res["sweeps"][0] == 1 and res["converged"][0] and not res["changed"][0].any()
    assert np.array_equal(fg.var_value[0], start[0])
    for r in (1, 2):
        want, sweeps, changed = host_icm(og, color, start[r], fg.weight_value[0], 40)
        assert sweeps > 1, "the random state must need more than one sweep"
        assert np.array_equal(fg.var_value[r], want), r
        assert res["sweeps"][r] == sweeps and res["converged"][r]
        assert np.array_equal(res["changed"][r], changed), r
        assert not res["changed"][r, sweeps - 1:].any() and (res["changed"][r, :sweeps - 1] > 0).all()
    assert res["sweeps"][1] != res["sweeps"][2] or not np.array_equal(res["changed"][1], res["changed"][2])
    # a sub-range of the chains through the C-ABI: chain 2 alone, from its start
    L, h = _lib.lib(), fg._engine()
    fg.var_value[:] = start
    fg._push_chains(0, count=False)
    sw, ch = np.zeros(1, np.int64), np.zeros(40, np.int64)
    _lib.check(L.nsk_icm(h, _lib.BUF_VALUE, 2, 1, 40, 0, _lib.ptr(sw), _lib.ptr(ch)))
    fg._pull_chains(count=False)
    assert sw[0] == res["sweeps"][2] and np.array_equal(ch, res["changed"][2])
    assert np.array_equal(fg.var_value[:2], start[:2]) and np.array_equal(fg.var_value[2], want)


# ---------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("name", ["lr3000", "gencat", "hubs"])
def test_a_converged_state_is_a_fixed_point_of_the_devices_conditionals(golden, name):
    g, hbv = _graph(golden, name)
    _, fg = session(g, seed=SEED, head_by_vid=hbv)
    fg.learn(1, 3, 0.01, 0.95, 2, 0.01, 1)         # (lr3000 starts with all weights 0)
    fg.inference(2, 3, True)
    res = fg.icm(max_sweeps=200)
    assert res["converged"] and res["changed"][0] > 0, (name, res["sweeps"])
    free = np.nonzero(fg.variable["isEvidence"] == 0)[0]
    off, pot = fg.conditionals(free, potentials=True)
    x = fg.var_value[0][free]
    own = pot[off[:-1] + x]
    assert np.isfinite(pot).all()
    assert (own >= np.maximum.reduceat(pot, off[:-1])).all()
    assert np.array_equal(icm_choice(off, pot, x), x)
    before = fg.var_value[0].copy()
    again = fg.icm(max_sweeps=200)
    assert again["sweeps"] == 1 and again["converged"] and not again["changed"].any()
    assert np.array_equal(fg.var_value[0], before)


@pytest.mark.parametrize("name", ["grid57x33", "pairs"])
def test_icm_does_not_lower_the_log_potential_of_a_proper_energy(golden, name):
    g, hbv = _graph(golden, name)
    _, fg = session(g, seed=SEED, head_by_vid=hbv)
    fg.learn(1, 3, 0.01, 0.95, 2, 0.01, 1)         # (the pairs start with all weights 0; the grid's weight is fixed)
    fg.inference(2, 3, True)
    for ev in (False, True):
        before = fg.log_potential()
        res = fg.icm(max_sweeps=100, sample_evidence=ev)
        after = fg.log_potential()
        print("%s sample_evidence=%s: log-potential %.17g -> %.17g in %d sweeps" % (name, ev, before, after, res["sweeps"]))
        assert res["converged"] and after >= before


# ---------------------------------------------------------------------------------------------- D
def _grid_icm(x, color, n, w, max_sweeps):
    """ICM on the n x n Ising grid from the closed-form neighbour sums: (state, sweeps, changed) as host_icm"""
    x = np.asarray(x, np.int64).reshape(n, n).copy()
    col = np.asarray(color).reshape(n, n)
    changed, sweeps = np.zeros(max_sweeps, np.int64), -max_sweeps
    for s in range(max_sweeps):
        for c in range(int(col.max()) + 1):
            i, j = np.nonzero(col == c)
            p = np.zeros((len(i), 2))
            for di, dj in ((-1, 0), (0, -1), (1, 0), (0, 1)):
                ii, jj = i + di, j + dj
                ok = (ii >= 0) & (ii < n) & (jj >= 0) & (jj < n)
                nb = x[np.clip(ii, 0, n - 1), np.clip(jj, 0, n - 1)]
                for k in (0, 1):
                    p[:, k] += np.where(ok, np.where(nb == k, w, -w), 0.0)
            new = icm_choice(2 * np.arange(len(i) + 1), p.reshape(-1), x[i, j])
            changed[s] += int((new != x[i, j]).sum())
            x[i, j] = new
        if changed[s] == 0:
            sweeps = s + 1
            break
    return x.reshape(-1), sweeps, changed


def test_icm_on_the_million_grid_keeps_the_tally():
    """a one-chain handle of wide quads may keep its tally in bits 1-7 of the value bytes: the call sees plain values and
    the tally comes out as if it had not been made.  (Every potential is a sum of at most four terms +-0.3 whose partial
    sums are exact multiples wherever two values tie, so the closed form decides as the list walk does.)"""
    n, sweeps_max = 1000, 4
    g = graphgen.ising_grid(n, n, weight=0.3)
    _, fg = session(g, seed=SEED)
    _, tw = session(g, seed=SEED)
    assert fg.info()["wide_quads"] > 0
    L, h = _lib.lib(), fg._engine()
    fg.inference(0, 12)
    tw.inference(0, 12)
    assert np.array_equal(fg.var_value[0], tw.var_value[0])
    sw, ch = np.zeros(1, np.int64), np.zeros(sweeps_max, np.int64)
    _lib.check(L.nsk_icm(h, _lib.BUF_VALUE, 0, 1, sweeps_max, 0, _lib.ptr(sw), _lib.ptr(ch)))
    vv, cnt = np.zeros(n * n, np.int64), np.zeros(len(fg.count), np.int64)
    _lib.check(L.nsk_state_download(h, _lib.ptr(vv), None, None, _lib.ptr(cnt)))
    assert np.array_equal(cnt, tw.count) and fg.info()["sweeps_done"] == tw.info()["sweeps_done"] == 12
    want, sweeps, changed = _grid_icm(tw.var_value[0], fg.colors(), n, 0.3, sweeps_max)
    print("1M grid: sweeps %d, changed %s" % (sweeps, changed.tolist()))
    assert changed[0] > 0
    assert np.array_equal(vv, want) and sw[0] == sweeps and np.array_equal(ch, changed)
    # both handles go on from equal states
    for f in (fg, tw):
        f.var_value[0][:] = want
        f.count[:] = cnt
        f.inference(0, 3)
    assert np.array_equal(fg.var_value[0], tw.var_value[0]) and np.array_equal(fg.count, tw.count)


def test_icm_straight_behind_the_sweeps_of_the_million_grid():
    """the same without a download between the sweeps and the call: the position tally is still unfolded"""
    n = 1000
    g = graphgen.ising_grid(n, n, weight=0.3)
    _, fg = session(g, seed=SEED)
    _, tw = session(g, seed=SEED)
    L, h = _lib.lib(), fg._engine()
    fg._push(0, 0)
    fg._sweep(12, False, False)
    sw = np.zeros(1, np.int64)
    _lib.check(L.nsk_icm(h, _lib.BUF_VALUE, 0, 1, 2, 0, _lib.ptr(sw), None))
    fg._pull(0, 0, weights=False)
    tw.inference(0, 12)
    assert np.array_equal(fg.count, tw.count)
    want, sweeps, _ = _grid_icm(tw.var_value[0], fg.colors(), n, 0.3, 2)
    assert np.array_equal(fg.var_value[0], want) and sw[0] == sweeps


# ---------------------------------------------------------------------------------------------- E
def test_only_the_values_change(golden):
    g, hbv = _graph(golden, "gencat_i32")
    a, b, c = (session(g, seed=SEED, head_by_vid=hbv)[1] for _ in range(3))
    for fg in (a, b, c):
        fg.learn(1, 2, 0.01, 0.95, 2, 0.01, 1)
        fg.inference(1, 4, True)
    assert a.info()["value_bytes"] == 4
    before = a.var_value[0].copy()
    done = a.info()["sweeps_done"]
    res = a.icm(max_sweeps=6, sample_evidence=True)
    assert res["changed"][0] > 0 and not np.array_equal(a.var_value[0], before)
    assert a.info()["sweeps_done"] == done == b.info()["sweeps_done"]
    c.conditionals()
    assert a.info()["device_bytes"] == c.info()["device_bytes"]         # the counters are gone
    assert np.array_equal(a.var_value_evid, b.var_value_evid) and np.array_equal(a.count, b.count)
    assert np.array_equal(_bits(a.weight_value), _bits(b.weight_value))
    a.var_value[0][:] = before                                          # re-uploaded by the next call
    for fg in (a, b):
        fg.inference(0, 3, True)
        fg.learn(0, 1, 0.01, 0.95, 2, 0.01, 1)
    assert np.array_equal(a.var_value, b.var_value) and np.array_equal(a.var_value_evid, b.var_value_evid)
    assert np.array_equal(a.count, b.count) and np.array_equal(_bits(a.weight_value), _bits(b.weight_value))


# ---------------------------------------------------------------------------------------------- F
def test_refusals_and_lifecycle(golden):
    L = _lib.lib()
    g, hbv = _graph(golden, "gencat_i32")
    _, fg = session(g, seed=SEED, head_by_vid=hbv, chains=2)
    h = fg._engine()
    fg._chains()
    sw, ch = np.full(2, 99, np.int64), np.full((2, 5), 99, np.int64)

    def icm(which=_lib.BUF_VALUE, first=0, n=1, max_sweeps=5, s=sw, c=ch):
        return L.nsk_icm(h, which, first, n, max_sweeps, 1, _lib.ptr(s), _lib.ptr(c))

    for which in (-1, _lib.BUF_WEIGHT, 7):
        assert icm(which=which) == _lib.E_INVALID
    assert icm(first=2) == _lib.E_INVALID                                   # chain >= chains
    assert icm(first=1, n=2) == _lib.E_INVALID
    assert icm(first=-1) == _lib.E_INVALID
    assert icm(n=0) == _lib.E_INVALID
    assert icm(which=_lib.BUF_VALUE_EVID, first=1) == _lib.E_INVALID        # the evidence chain exists once
    assert icm(which=_lib.BUF_VALUE_EVID, n=2) == _lib.E_INVALID
    for bad in (0, -1, 4097):
        assert icm(max_sweeps=bad) == _lib.E_INVALID
    assert icm(s=None) == _lib.E_INVALID
    assert (sw == 99).all() and (ch == 99).all()                            # a refused call writes nothing
    assert icm(n=2) == _lib.OK and (sw != 99).all() and (ch != 99).all()
    sw[:] = 99
    assert icm(n=2, c=None) == _lib.OK and (sw != 99).all()                 # changed == NULL is fine
    assert icm(which=_lib.BUF_VALUE_EVID) == _lib.OK
    assert icm(n=2, max_sweeps=4096, c=None) == _lib.OK and (np.abs(sw) <= 4096).all()
    if (sw > 0).all():                                                      # from a fixed point the first sweep changes nothing
        assert icm(n=2, c=None) == _lib.OK and (sw == 1).all()
    # a handle with a trace is served, and its rows stay
    nvar = len(fg.variable)
    assert L.nsk_trace_setup(h, None, 0, 1, 4) == _lib.OK
    assert L.nsk_gibbs_sweeps(h, 3, 1, 0) == _lib.OK
    rows = np.zeros((3, 2, nvar), np.int32)
    idx = np.zeros(3, np.int64)
    assert L.nsk_trace_download(h, 0, 3, _lib.ptr(rows), _lib.ptr(idx)) == _lib.OK
    bytes_before = fg.info()["device_bytes"]
    assert icm(n=2) == _lib.OK and (ch[:, 0] > 0).all()
    assert fg.info()["device_bytes"] == bytes_before
    rows2, idx2 = np.zeros_like(rows), np.zeros_like(idx)
    nrows = C.c_int64(-1)
    assert L.nsk_trace_rows(h, C.byref(nrows), None, None) == _lib.OK and nrows.value == 3
    assert L.nsk_trace_download(h, 0, 3, _lib.ptr(rows2), _lib.ptr(idx2)) == _lib.OK
    assert np.array_equal(rows, rows2) and np.array_equal(idx, idx2)
    assert L.nsk_gibbs_sweeps(h, 1, 1, 0) == _lib.OK                        # ... and it goes on recording
    assert L.nsk_trace_rows(h, C.byref(nrows), None, None) == _lib.OK and nrows.value == 4
    assert L.nsk_trace_setup(h, None, 0, 1, 0) == _lib.OK
    # an own_range handle
    from numbskull_amd.distributed import shard_range
    ns = numbskull_amd.NumbSkull(quiet=True, seed=SEED)
    w, v, f, fm, dm, edges = [x.copy() if isinstance(x, np.ndarray) else x for x in _graph(golden, "grid57x33")[0]]
    ns.loadFactorGraph(w, v, f, fm, dm, int(edges), own_range=shard_range(0, 2, len(v)))
    sh = ns.factorGraphs[0]
    assert L.nsk_icm(sh._engine(), _lib.BUF_VALUE, 0, 1, 5, 0, _lib.ptr(sw), None) == _lib.E_INVALID
    with pytest.raises(ValueError):
        sh.icm()


# ---------------------------------------------------------------------------------------------- G
def test_map_estimate_finds_the_enumerated_map():
    """3 x 4 Ising grid, weight 0.5, variables 0, 5, 11 evidence at 1, 0, 1; 8 chains x 200 recorded sweeps.  The nine free
    variables have 512 states; three of them share the largest log-potential, 4.5, each with probability 0.0456 -- hence
    "the enumerated MAP, or its log-potential to the bit".  A chain's 200 rows miss all three with probability below
    1e-4 and the 1600 rows of eight chains never in practice; a chain that records one keeps it, ICM leaves a global
    maximum alone.  On the CPU oracle (chain r keyed seed ^ (r << 32), identity generator ids) best-of-chains plus the
    host ICM reached 4.5 for each of the seeds 60 .. 99, 77 among them."""
    g = evidence_grid()
    _, fg = session(g, seed=SEED, chains=8)
    og = oracle_of(fg)
    w = fg.weight_value[0].copy()
    base = og.variable["initialValue"].astype(np.int64)
    free = np.nonzero(og.variable["isEvidence"] == 0)[0]
    lps = np.zeros(1 << len(free))
    for s in range(len(lps)):
        x = base.copy()
        x[free] = (s >> np.arange(len(free))) & 1
        lps[s] = joint_exponent(og, x, w)
    best = base.copy()
    best[free] = (int(np.argmax(lps)) >> np.arange(len(free))) & 1
    res = fg.map_estimate(200)
    print("map_estimate: chain %d, log-potential %.17g (sampled %.17g), enumerated %.17g"
          % (res["chain"], res["log_potential"], res["sampled_log_potential"], lps.max()))
    assert np.array_equal(res["values"], best) or _bits(res["log_potential"])[0] == _bits(lps.max())[0]
    assert res["log_potential"] >= res["sampled_log_potential"] and res["converged"]
    assert np.array_equal(res["values"], fg.var_value[res["chain"]])
    assert res["log_potential"] == fg.log_potential(var_copy=res["chain"])


def test_map_estimate_polishes_every_chain(golden):
    g, hbv = _graph(golden, "lr3000")
    _, fg = session(g, seed=SEED, head_by_vid=hbv, chains=4)
    res = fg.map_estimate(20, thin=2, burnin_epochs=2)
    assert res["log_potentials"].shape == res["sampled_log_potentials"].shape == (4,)
    print("lr3000: sampled %s -> polished %s" % (res["sampled_log_potentials"].tolist(), res["log_potentials"].tolist()))
    assert (res["log_potentials"] >= res["sampled_log_potentials"]).all()
    assert res["chain"] == int(np.argmax(res["log_potentials"]))
    assert res["log_potential"] == res["log_potentials"][res["chain"]]
    assert np.array_equal(res["values"], fg.var_value[res["chain"]])
    assert np.array_equal(_bits(fg.log_potential(var_copy="all")), _bits(res["log_potentials"]))
    # under learned weights (the graph starts with all weights 0) the polish has work to do.  With categorical OR / IMPLY
    # factors potential() is not the gradient of one energy, so the gain is printed, not asserted; what map_estimate
    # composes is: the polished rows are fixed points, and the chain reported is the best of them
    fg.learn(1, 3, 0.01, 0.95, 2, 0.01, 1)
    res = fg.map_estimate(20, thin=2, burnin_epochs=2, max_sweeps=200)
    print("lr3000 learned: sampled %s -> polished %s" % (res["sampled_log_potentials"].tolist(), res["log_potentials"].tolist()))
    assert res["chain"] == int(np.argmax(res["log_potentials"])) and res["converged"]
    assert np.array_equal(res["values"], fg.var_value[res["chain"]])
    assert np.array_equal(_bits(fg.log_potential(var_copy="all")), _bits(res["log_potentials"]))
    states = fg.var_value.copy()
    again = fg.icm(max_sweeps=5, var_copy="all")
    assert (again["sweeps"] == 1).all() and np.array_equal(fg.var_value, states)
