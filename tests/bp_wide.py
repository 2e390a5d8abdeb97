"""The graphs of the wide-factor belief-propagation tests (nsk_bp_setup_wide): nfac copies of one wide logical factor over n
binary variables plus a unary ISTRUE factor with a weight of its own on every member -- a forest for nfac = 1, so belief
propagation is exact on it -- and the enumeration of its states in numpy."""

import ctypes as C
import functools

import numpy as np

import bp
from numbskull_amd import _lib

FUNCTIONS = (0, 1, 2, 3, 4, 7, 9, 13)       # IMPLY_NATURAL OR AND EQUAL ISTRUE LINEAR LOGICAL IMPLY_MLN


def unary_weights(n, lo=1.5, hi=2.5):
    return np.linspace(lo, hi, n) * np.where(np.arange(n) % 5 == 4, -0.2, 1.0)


def graph(fn, n, w=0.7, clamped=(), values=None, twice=None, unary=None, nfac=1):
    """clamped: the evidence members; values: every member's initial value; twice = (position, variable): the member at
    that position of the wide factor is that variable once more"""
    members = list(range(n))
    if twice is not None:
        members[twice[0]] = twice[1]
    unary = unary_weights(n) if unary is None else unary
    f = [(fn, members, [0] * n, w)] * nfac + [(4, [v], [0], float(unary[v])) for v in range(n)]
    evid = np.zeros(n, np.int64)
    evid[list(clamped)] = 1
    init = (np.arange(n) % 2 == 0).astype(np.int64) if values is None else np.asarray(values)
    return bp.spec_graph([2] * n, evid, init, f), members


def feature(fn, x):
    """the factor's value on the member values x (states, positions)"""
    body, head = x[:, :-1], x[:, -1:]
    if fn in (0, 2, 4):
        return np.where(x.all(1), 1.0, 0.0 if fn == 0 else -1.0)
    if fn == 1:
        return np.where(x.any(1), 1.0, -1.0)
    if fn == 3:
        return np.where((x == x[:, :1]).all(1), 1.0, -1.0)
    if fn == 7:
        return (body == head).sum(1).astype(np.float64)
    if fn == 9:
        return (body == head).any(1).astype(np.float64)
    return np.where(body.all(1), head[:, 0].astype(np.float64), 1.0)


@functools.lru_cache(maxsize=2)
def _states(evid, init, unary):
    """every state of the free variables (states, n) and the unary factors' part of its log-potential"""
    free = np.nonzero(np.asarray(evid) == 0)[0]
    x = np.tile(np.asarray(init, np.int8), (1 << len(free), 1))
    x[:, free] = (np.arange(1 << len(free))[:, None] >> np.arange(len(free))) & 1
    return x, (2.0 * x - 1.0) @ np.asarray(unary)


def enumerate_exact(g, members, nfac=1):
    """(log Z, P(x_v = 1) per variable) of a graph() over the states of its free variables"""
    weight, variable, factor = g[0], g[1], g[2]
    n = len(variable)
    fn, w = int(factor["factorFunction"][0]), weight["initialValue"]
    x, unary = _states(tuple(variable["isEvidence"]), tuple(variable["initialValue"]), tuple(w[nfac:nfac + n]))
    logp = nfac * w[0] * feature(fn, x[:, members]) + unary
    mx = logp.max()
    p = np.exp(logp - mx)
    return mx + np.log(p.sum()), (p @ x) / p.sum()


def device(fg, runs, damping=0.0, wide=True, terms=0):
    """set up (the wide route on or off), then nsk_bp_run per entry of runs: (info, winfo, [(f2v, v2f) behind each run],
    the wide terms behind the first run where terms > 0); the set-up is cleared"""
    L, h = _lib.lib(), fg._engine()
    fg._push(0, 0)
    info, winfo, ran, out, tv = _lib.BpInfo(), _lib.BpWideInfo(), C.c_int64(0), [], np.zeros(terms)
    if wide:
        _lib.check(L.nsk_bp_setup_wide(h, _lib.BUF_VALUE, 0, 0, C.byref(info), C.byref(winfo)))
    else:
        _lib.check(L.nsk_bp_setup(h, _lib.BUF_VALUE, 0, 0, C.byref(info)))
    for iters in runs:
        _lib.check(L.nsk_bp_run(h, iters, damping, 0.0, C.byref(ran), None))
        out.append((np.zeros(info.nmsg), np.zeros(info.nmsg)))
        _lib.check(L.nsk_bp_download(h, _lib.BP_F2V, _lib.ptr(out[-1][0])))
        _lib.check(L.nsk_bp_download(h, _lib.BP_V2F, _lib.ptr(out[-1][1])))
        if terms and len(out) == 1:
            _lib.check(L.nsk_bp_wide_terms(h, None, _lib.ptr(tv)))
    L.nsk_bp_clear(h)
    return info, winfo, out, tv
