"""What a sweep of the dual MAP bound costs (nsk_bp_dual_run) on the clamped 1M Ising grid, beside one iteration of
max-product (nsk_bp_map_run) on the same set-up.

    python tools/dual_cost.py [--sweeps 20] [--repeats 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/dual_cost.py --repeats 2

The graph is tools/bp_cost.py's 1000 x 1000 grid (weight 0.3, every 97th variable evidence at alternating values).  `sweeps`
sweeps of nsk_bp_dual_run and `sweeps` iterations of nsk_bp_map_run, both with tol = 0 (no early exit) and warm (no
reset inside the window), are timed with HIP events on the handle's stream (nsk_profile_begin / nsk_profile_mark /
nsk_profile_read) after a warm-up of each, taking turns.  Prints one JSON line: the medians and the spread in microseconds
a sweep and an iteration, the launches a sweep takes, and the bytes a sweep must move -- D read and written, M written and
read, theta read once per free member -- with the bandwidth that floor stands for at the measured time."""

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def cost(sweeps, repeats, rows=1000, cols=1000):
    import numbskull_amd
    from numbskull_amd import _lib, graphgen
    g = list(graphgen.ising_grid(rows, cols, weight=0.3))
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
    res = np.zeros(sweeps)
    routes, cls = np.zeros(2, np.int64), np.zeros(rows * cols, np.int32)
    _lib.check(L.nsk_bp_dual_routes(h, _lib.ptr(routes)))
    _lib.check(L.nsk_bp_dual_classes(h, _lib.ptr(cls)))

    def timed(call):
        _lib.check(L.nsk_synchronize(h))
        _lib.check(L.nsk_profile_begin(h))
        _lib.check(call())
        _lib.check(L.nsk_profile_mark(h))
        _lib.check(L.nsk_profile_read(h, C.byref(ms), C.byref(nl)))
        return ms.value * 1e3 / sweeps

    calls = {"dual_sweep": lambda: L.nsk_bp_dual_run(h, sweeps, 0.0, 1, C.byref(n), _lib.ptr(res)),
             "map_iteration": lambda: L.nsk_bp_map_run(h, sweeps, 0.0, 0.0, 1, C.byref(n), None)}
    for c in calls.values():        # (the first call of each allocates and starts cold)
        timed(c)
        timed(c)
    out = {k: [] for k in calls}
    for _ in range(repeats):
        for k, c in calls.items():
            out[k].append(timed(c))
    med = {k: float(np.median(v)) for k, v in out.items()}
    layout = [np.zeros(len(fg.factor) + 1, np.int64), np.zeros(len(fg.factor) + 1, np.int64)]
    _lib.check(L.nsk_bp_layout(h, _lib.ptr(layout[0]), _lib.ptr(layout[1]), None, None))
    theta_reads = int(np.sum(np.diff(layout[0]) * np.diff(layout[1])))      # a table once per free member
    floor = 8 * (4 * info.nmsg + theta_reads)
    print(json.dumps({"graph": "ising %d x %d, weight 0.3, every 97th variable evidence" % (rows, cols), "sweeps": sweeps,
                      "repeats": repeats, "edges": int(info.nedges), "routes": routes.tolist(), "classes": int(cls.max()) + 1,
                      "median_us": {k: round(v, 1) for k, v in med.items()},
                      "spread_us": {k: round(max(v) - min(v), 1) for k, v in out.items()},
                      "dual_over_map": round(med["dual_sweep"] / med["map_iteration"], 2),
                      "floor_bytes_per_sweep": int(floor),
                      "floor_gb_per_s_at_median": round(floor / med["dual_sweep"] / 1e3, 1),
                      "last_residual": float(res[-1])}))
    _lib.check(L.nsk_bp_clear(h))
    fg.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    cost(a.sweeps, a.repeats)
