"""Belief propagation through wide logical factors on the device (nsk_bp_setup_wide, k_bp_wide, k_bp_wide_terms): against
enumeration beyond the caps of the table route, against the table route on one graph (NSK_BP_WIDE_MIN), at the edges of the
64-position chunks against the rule in numpy at long double, and at its limits."""

import ctypes as C

import numpy as np
import pytest

import bp_wide
from numbskull_amd import _lib
from numbskull_amd.diagnostics import bp_wide_factor
from util import session

pytestmark = pytest.mark.gpu


def _p1(out):
    return out["beliefs"][out["offsets"][:-1] + 1]


@pytest.mark.parametrize("fn", bp_wide.FUNCTIONS)
@pytest.mark.parametrize("n,clamp", [(17, False), (20, False), (20, True)])
def test_against_enumeration_beyond_the_caps(fn, n, clamp):
    clamped = sorted(set(range(2, n, 3)) | {n - 1}) if clamp else []         # every third member and the head
    g, members = bp_wide.graph(fn, n, clamped=clamped, twice=(4, 2) if clamp else None, unary=bp_wide.unary_weights(n, 0.2, 0.6))
    _, fg = session(g, head_by_vid=True)
    with pytest.raises(ValueError, match="factor 0"):
        fg.belief_propagation(max_iters=4, tol=0)
    out = fg.belief_propagation(max_iters=4, tol=0, wide_factors=True)
    log_z, p1 = bp_wide.enumerate_exact(g, members)
    assert list(out["wide_factors"]) == [0]
    assert np.abs(_p1(out) - p1).max() <= 1e-12
    assert abs(out["log_z"] - log_z) <= 1e-10


@pytest.mark.parametrize("fn", bp_wide.FUNCTIONS)
@pytest.mark.parametrize("n", [2, 3, 7, 12])
@pytest.mark.parametrize("damping", [0.0, 0.5])
def test_both_routes_on_one_graph(fn, n, damping, monkeypatch):
    g, members = bp_wide.graph(fn, n, clamped=[1] if n > 2 else [], unary=bp_wide.unary_weights(n, 0.2, 0.6))
    _, fg = session(g, head_by_vid=True)
    log_z, p1 = bp_wide.enumerate_exact(g, members)
    got = {}
    for route in ("table", "wide"):
        monkeypatch.setenv("NSK_DIAG", "1")
        monkeypatch.setenv("NSK_BP_WIDE_MIN", "2" if route == "wide" else "4096")
        _, winfo, msgs, _ = bp_wide.device(fg, (1, 3), damping)         # after 1 and after 4 iterations
        assert winfo.nwide == (1 if route == "wide" else 0)
        out = fg.belief_propagation(max_iters=60, damping=damping, tol=0, wide_factors=True)
        got[route] = [msgs[0][0], msgs[1][0], _p1(out), out["log_z"]]
        assert np.abs(_p1(out) - p1).max() <= 1e-12 and abs(out["log_z"] - log_z) <= 1e-10
    for a, b in zip(got["table"][:3], got["wide"][:3]):
        assert np.abs(a - b).max() <= 1e-12
    assert abs(got["table"][3] - got["wide"][3]) <= 1e-10


@pytest.mark.parametrize("fn", [2, 1, 3, 7, 9, -7])
@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 2048])
def test_chunk_edges_against_the_rule_at_long_double(fn, n, monkeypatch):
    biased, fn = fn < 0, abs(fn)        # -7: LINEAR with a body of one mind and the head clamped against it
    # unary weights that keep the function's pattern product (AND: prod nu(1), OR: prod nu(0), ..) at 1e-3 or more
    u = 0.5 * np.log(1.0 / (1e3 ** (1.0 / n) - 1.0)) + 0.25          # sigmoid(2 u) ** n >= 1e-3
    sign = {2: 1.0, 1: -1.0, 3: 1.0, 7: 1.0, 9: -1.0}[fn]
    unary = np.full(n, sign * u)
    if fn == 9:
        unary[n - 1] = u                                             # the body differs from the head
    if fn == 7:         # no pattern: mixed messages and |w| = 1, so that both product streams leave the range of a double
        unary = np.full(n, 0.4) if biased else 0.3 * (-1.0) ** np.arange(n)
    clamped = sorted({0, min(63, n - 2), n - 1})                      # the first, the 64th and the last position
    values = np.where(unary > 0, 1, 0)
    if biased:
        values[n - 1] = 0
    nfac = 9
    g, members = bp_wide.graph(fn, n, w=-0.7 if fn in (1, 9) else 0.7, clamped=clamped, values=values, unary=unary, nfac=nfac)
    if fn == 7:
        g[0]["initialValue"][:nfac] = 1.0
    _, fg = session(g, head_by_vid=True)
    results = []
    for cap in (None, "1"):
        monkeypatch.delenv("NSK_BP_GRID_CAP", raising=False)
        if cap:
            monkeypatch.setenv("NSK_DIAG", "1")
            monkeypatch.setenv("NSK_BP_GRID_CAP", cap)
        _, winfo, msgs, terms = bp_wide.device(fg, (1, 1), terms=nfac)
        assert winfo.nwide == nfac and winfo.max_positions == n
        results.append((msgs[0][1], msgs[1][0], terms))     # v2f and the terms behind one iteration, f2v behind the next
    for a, b in zip(*results):
        assert np.array_equal(a, b)                                  # the capped grid's later trips: the same bits
    v2f, f2v, terms = results[0]
    cl = np.full(n, -1)
    cl[clamped] = values[clamped]
    nfree = n - len(clamped)
    worst = 0.0
    for k in (0, nfac - 1):         # factor k's edges are the free positions in order, two doubles each
        nu = np.zeros((n, 2))
        nu[cl < 0] = v2f[2 * nfree * k:2 * nfree * (k + 1)].reshape(nfree, 2)
        w = g[0]["initialValue"][k]
        ref, rterm = bp_wide_factor(fn, w, nu, cl, dtype=np.longdouble)
        own, oterm = bp_wide_factor(fn, w, nu, cl)
        pattern = {2: nu[cl < 0, 1], 1: nu[cl < 0, 0], 3: nu[cl < 0, 1], 7: nu[cl < 0, 1], 9: nu[cl < 0, 0]}[fn]
        assert (np.prod(pattern) if fn != 7 else ref[cl < 0].min()) >= 1e-3
        dev = f2v[2 * nfree * k:2 * nfree * (k + 1)].reshape(nfree, 2)
        tol = 16 * float(np.abs(own - ref).max()) + 16 * 2.0 ** -52
        err = float(np.abs(dev - ref[cl < 0]).max())
        tol_t = 16 * float(abs(oterm - rterm)) + 16 * 2.0 ** -52
        err_t = float(abs(terms[k] - rterm))
        worst = max(worst, err / tol, err_t / tol_t)
        assert err <= tol and err_t <= tol_t, (k, err, tol, err_t, tol_t)
    print("bp_wide fn %d n %d: worst error / tolerance %.3f" % (fn, n, worst))


def test_a_wide_factor_last_beside_a_categorical_table_factor():
    """the table route's edges of a mixed set-up (k_bp_factor_narrow) against k_bp_factor on the graph without the wide
    factor, bit for bit after one iteration, where the wide factor's messages have not reached them; the wide factor is
    the last factor, behind every table"""
    n = 18
    f = [(4, [v], [0], 0.1 * (v + 1)) for v in range(n)] + [(12, [0, n], [1, 2], 0.9), (15, [n], [1], -0.4)]
    cards = [2] * n + [3]
    f2v = []
    for wide in (False, True):
        g = bp_wide.bp.spec_graph(cards, [0] * (n + 1), [0] * (n + 1), f + ([(2, list(range(n)), [0] * n, 0.7)] if wide else []))
        _, fg = session(g)
        _, winfo, msgs, _ = bp_wide.device(fg, (1,))
        assert winfo.nwide == int(wide)
        f2v.append(msgs[0][0])
        if wide:
            out = fg.belief_propagation(max_iters=8, tol=0, wide_factors=True)
            assert np.isfinite(out["beliefs"]).all() and np.isfinite(out["log_z"]) and list(out["wide_factors"]) == [n + 2]
    assert len(f2v[0]) == n * 2 + 2 + 3 + 3 and np.array_equal(f2v[0], f2v[1][:len(f2v[0])])


def test_log_evidence_and_the_host_plan():
    n, clamped = 17, [2, 16]
    g, members = bp_wide.graph(2, n, clamped=clamped, unary=bp_wide.unary_weights(n, 0.2, 0.6))
    _, fg = session(g)
    got = fg.bp_log_evidence(max_iters=4, tol=0, wide_factors=True)
    free = tuple(g[:1]) + (g[1].copy(),) + tuple(g[2:])
    free[1]["isEvidence"][:] = 0
    want = bp_wide.enumerate_exact(g, members)[0] - bp_wide.enumerate_exact(free, members)[0]
    assert abs(got["log_evidence"] - want) <= 2e-10
    desc, keep = fg._descriptor()
    info, winfo, route = _lib.BpInfo(), _lib.BpWideInfo(), np.zeros(len(fg.factor), np.int32)
    _lib.check(_lib.lib().nsk_bp_wide_plan(C.byref(desc), 0, C.byref(info), C.byref(winfo), _lib.ptr(route)))
    assert route.tolist() == [1] + [0] * n and (winfo.nwide, winfo.wide_positions, winfo.max_positions) == (1, n, n)
    assert winfo.lds_bytes == 4 * 3 * 64 * 8 and winfo.device_bytes == 0 and info.nedges == 2 * n - 2 * len(clamped)


def _refused(g, text):
    _, fg = session(g, head_by_vid=True)
    fg._push(0, 0)                  # (the state's own arrays are there before the call)
    before = fg.info()["device_bytes"]
    with pytest.raises(ValueError, match=text):
        fg.belief_propagation(max_iters=2, wide_factors=True)
    assert fg.info()["device_bytes"] == before


def test_limits_are_refused_naming_the_factor():
    _refused(bp_wide.graph(2, 2049)[0], "factor 0 has more than NSK_BP_WIDE_MAX_MEMBERS = 2048")
    _refused(bp_wide.graph(2, 20, twice=(4, 2))[0], "factor 0 names a free member twice on the wide route")
    _refused(bp_wide.graph(8, 20)[0], "factor 0 ")
    g, _ = bp_wide.graph(2, 20)
    g[1]["cardinality"][3] = 3
    _refused(g, "factor 0 has more than NSK_BP_MAX_MEMBERS")


def test_other_calls_refuse_a_wide_set_up_and_clear_returns_the_bytes():
    g, _ = bp_wide.graph(2, 20)
    _, fg = session(g)
    L, h = _lib.lib(), fg._engine()
    fg._push(0, 0)
    before = fg.info()["device_bytes"]
    info, winfo = _lib.BpInfo(), _lib.BpWideInfo()
    _lib.check(L.nsk_bp_setup_wide(h, _lib.BUF_VALUE, 0, 0, C.byref(info), C.byref(winfo)))
    assert fg.info()["device_bytes"] - before == info.device_bytes > winfo.device_bytes > 0
    nw, it = len(g[0]), C.c_int64(0)
    z, zi = np.zeros(4 * nw + 64), np.zeros(4 * nw + 64, np.int64)
    rho = np.ones(len(g[2]))
    calls = [L.nsk_bp_residual_run(h, 2, 0.5, 0.0, 0.0, 0, C.byref(it), None, None, None),
             L.nsk_bp_map_run(h, 2, 0.0, 0.0, 0, C.byref(it), None),
             L.nsk_bp_trw_run(h, _lib.ptr(rho), 2, 0.0, 0.0, 0, C.byref(it), None),
             L.nsk_bp_moments(h, _lib.ptr(zi), None),
             L.nsk_bp_learn_steps(h, _lib.ptr(z), 1, 1, 0.0, 0.0, 1, 0.1, 1.0, 0.0, 0, None, None, None, None, None),
             L.nsk_bp_latent_steps(h, 1, 1, 0.0, 0.0, 1, 0.1, 1.0, 0.0, 0, None, None, None, None, None)]
    assert all(rc == _lib.E_INVALID for rc in calls), calls
    assert b"wide factors" in L.nsk_last_error()
    L.nsk_bp_clear(h)
    assert fg.info()["device_bytes"] == before


def test_a_set_up_without_wide_factors_is_nsk_bp_setup_s():
    g, _ = bp_wide.graph(2, 12, clamped=[3])
    _, fg = session(g)
    msgs = []
    for wide in (False, True):
        info, winfo, m, _ = bp_wide.device(fg, (3,), wide=wide)
        assert winfo.nwide == 0 and winfo.device_bytes == 0
        msgs.append((m[0], [getattr(info, k) for k, _ in _lib.BpInfo._fields_]))
    assert msgs[0][1] == msgs[1][1]
    assert all(np.array_equal(a, b) for a, b in zip(msgs[0][0], msgs[1][0]))
