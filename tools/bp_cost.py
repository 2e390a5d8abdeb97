"""What belief propagation costs (nsk_bp_setup / nsk_bp_run) on the 1M and 10M Ising grids with a sprinkling of evidence.

    python tools/bp_cost.py [--grids 1m 10m] [--iters 20] [--repeats 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bp_cost.py --grids 1m --repeats 2

Per grid (1000 x 1000 and 2500 x 4000, weight 0.3, every 97th variable evidence at alternating values): the set-up --
structure on the host, uploads and tables, wall clock of nsk_bp_setup --, `iters` iterations of nsk_bp_run with tol = 0
(no early exit) and `iters` sweeps of nsk_gibbs_sweeps on the same handle, both timed with HIP events on the handle's
stream (nsk_profile_begin / nsk_profile_mark / nsk_profile_read) after a warm-up, taking turns.  Prints one JSON line per
grid: the medians and the spread in microseconds an iteration and a sweep, the bytes an iteration must move -- both
message arrays read and written once, psi read once -- and the bandwidth that floor stands for at the measured time.  The
kernel trace splits an iteration into its factor phase (k_bp_factor) and its variable phase (k_bp_var)."""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

GRIDS = {"1m": (1000, 1000), "10m": (2500, 4000)}


def cost(name, iters, repeats):
    import numbskull_amd
    from numbskull_amd import _lib, graphgen
    rows, cols = GRIDS[name]
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
    setup = []
    for _ in range(2):
        _lib.check(L.nsk_synchronize(h))
        t0 = time.perf_counter()
        _lib.check(L.nsk_bp_setup(h, _lib.BUF_VALUE, 0, 0, C.byref(info)))
        setup.append(time.perf_counter() - t0)
    ms, nl, n = C.c_double(), C.c_int64(), C.c_int64()
    res = np.zeros(iters)

    def timed(call):
        _lib.check(L.nsk_synchronize(h))
        _lib.check(L.nsk_profile_begin(h))
        _lib.check(call())
        _lib.check(L.nsk_profile_mark(h))
        _lib.check(L.nsk_profile_read(h, C.byref(ms), C.byref(nl)))
        return ms.value * 1e3 / iters

    calls = {"bp_iteration": lambda: L.nsk_bp_run(h, iters, 0.0, 0.0, C.byref(n), _lib.ptr(res)),
             "gibbs_sweep": lambda: L.nsk_gibbs_sweeps(h, iters, 0, 1)}
    for c in calls.values():
        timed(c)
    out = {k: [] for k in calls}
    for _ in range(repeats):
        for k, c in calls.items():
            out[k].append(timed(c))
    med = {k: float(np.median(v)) for k, v in out.items()}
    floor = 8 * (4 * info.nmsg + info.ntable)
    print(json.dumps({"graph": "ising %d x %d, weight 0.3, every 97th variable evidence" % (rows, cols), "iters": iters,
                      "repeats": repeats, "setup_seconds": [round(s, 3) for s in setup],
                      "setup_device_bytes": int(info.device_bytes), "edges": int(info.nedges), "table_entries": int(info.ntable),
                      "median_us": {k: round(v, 1) for k, v in med.items()},
                      "spread_us": {k: round(max(v) - min(v), 1) for k, v in out.items()},
                      "bp_over_sweep": round(med["bp_iteration"] / med["gibbs_sweep"], 2),
                      "floor_bytes_per_iteration": int(floor),
                      "floor_gb_per_s_at_median": round(floor / med["bp_iteration"] / 1e3, 1),
                      "last_residual": float(res[-1]), "iters_returned": int(n.value)}))
    _lib.check(L.nsk_bp_clear(h))
    fg.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", nargs="+", default=["1m", "10m"], choices=sorted(GRIDS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    for name in a.grids:
        cost(name, a.iters, a.repeats)
