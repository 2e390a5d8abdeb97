"""What the residual schedule costs and saves (nsk_bp_residual_run against nsk_bp_run) on tools/bp_cost.py's graph: the
1000 x 1000 Ising grid, every 97th variable evidence at alternating values.

    python tools/bp_residual_cost.py [--weights 0.3 1.0] [--iters 20] [--repeats 5] [--max 4096]

Per coupling weight one JSON line.  `round_us`: the time of a flooding iteration and of a residual round at frac = 0 --
every edge in every queue, the same bits: the price of the queues -- over `iters` of them with tol = 0.  `converge`: from
cold messages to tol = 1e-9 with at most `max` iterations or rounds enqueued, flooding and the residual schedule at
frac 0.5 and 0.1: milliseconds, iterations or rounds run, messages recomputed and committed.  Medians of `repeats` and the
spread (max - min), the calls taking turns; HIP events on the handle's stream (nsk_profile_*) after a warm-up."""

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def cost(weight, iters, repeats, most, rows=1000, cols=1000):
    import numbskull_amd
    from numbskull_amd import _lib, graphgen
    g = list(graphgen.ising_grid(rows, cols, weight=weight))
    ev = np.arange(0, rows * cols, 97)
    var = g[1].copy()
    var["isEvidence"][ev] = 1
    var["initialValue"][ev] = np.arange(len(ev)) % 2
    g[1] = var
    ns = numbskull_amd.NumbSkull(quiet=True, seed=1)
    ns.loadFactorGraph(*[x.copy() if isinstance(x, np.ndarray) else x for x in g[:5]], int(g[5]))
    fg = ns.factorGraphs[0]
    L, h = _lib.lib(), fg._engine()
    fg._push(0, 0)
    info = _lib.BpInfo()
    _lib.check(L.nsk_bp_setup(h, _lib.BUF_VALUE, 0, 0, C.byref(info)))
    ms, nl, n = C.c_double(), C.c_int64(), C.c_int64()
    upd, rec = np.zeros(most, np.int64), np.zeros(most, np.int64)

    def timed(call):
        _lib.check(L.nsk_synchronize(h))
        _lib.check(L.nsk_profile_begin(h))
        _lib.check(call())
        _lib.check(L.nsk_profile_mark(h))
        _lib.check(L.nsk_profile_read(h, C.byref(ms), C.byref(nl)))
        return ms.value

    def turns(calls):
        for c in calls.values():
            timed(c)
        out = {k: [] for k in calls}
        for _ in range(repeats):
            for k, c in calls.items():
                out[k].append(timed(c))
        return out

    def stats(v, scale=1.0):
        return {"median": round(float(np.median(v)) * scale, 2), "spread": round((max(v) - min(v)) * scale, 2)}

    per = turns({"flooding": lambda: L.nsk_bp_run(h, iters, 0.0, 0.0, C.byref(n), None),
                 "residual_frac0": lambda: L.nsk_bp_residual_run(h, iters, 0.0, 0.0, 0.0, 1, C.byref(n), None, None, None)})
    line = {"graph": "ising %d x %d, weight %g, every 97th variable evidence" % (rows, cols, weight), "edges": int(info.nedges),
            "repeats": repeats, "round_us": {k: stats(v, 1e3 / iters) for k, v in per.items()}, "converge": {}}

    def flooding():                                 # (the set-up's reset, outside the bracket, is what a cold start costs little of)
        return L.nsk_bp_run(h, most, 0.0, 1e-9, C.byref(n), None)

    def residual(frac):
        return lambda: L.nsk_bp_residual_run(h, most, frac, 0.0, 1e-9, 0, C.byref(n), None, _lib.ptr(upd), _lib.ptr(rec))

    counts = {}
    for k, c in (("flooding", flooding), ("residual_0.5", residual(0.5)), ("residual_0.1", residual(0.1))):
        t = []
        for _ in range(repeats + 1):                # (the first is the warm-up)
            if k == "flooding":
                _lib.check(L.nsk_bp_setup(h, _lib.BUF_VALUE, 0, 0, None))
            t.append(timed(c))
        ran = int(n.value)
        counts = {"recomputed": abs(ran) * int(info.nedges), "committed": abs(ran) * int(info.nedges)} if k == "flooding" else \
                 {"recomputed": int(rec.sum()), "committed": int(upd.sum())}
        line["converge"][k] = dict(ms=stats(t[1:]), ran=ran, **counts)
    print(json.dumps(line), flush=True)
    _lib.check(L.nsk_bp_clear(h))
    fg.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", nargs="+", type=float, default=[0.3, 1.0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max", type=int, default=4096)
    a = ap.parse_args()
    for w in a.weights:
        cost(w, a.iters, a.repeats, a.max)
