#!/usr/bin/env python3
"""The cost of one Swendsen-Wang cluster update beside one Gibbs sweep (DESIGN.md "Swendsen-Wang cluster updates"):
``python tools/sw_cost.py [rows cols]`` on a machine with an MI355X -- the benchmark's 2500 x 4000 grid by default -- at
the weights 0.2, 0.44 and 1.0.  Host clock around calls that end in a synchronise; one JSON line a weight."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from util import session            # noqa: E402
from numbskull_amd import _lib, graphgen      # noqa: E402

rows, cols = (int(a) for a in sys.argv[1:3]) if len(sys.argv) > 2 else (2500, 4000)
t0 = time.time()
_, fg = session(graphgen.ising_grid(rows, cols, weight=0.2), seed=3)
L, h = _lib.lib(), fg._engine()
print("graph + compile", time.time() - t0, flush=True)
for w in (0.2, 0.44, 1.0):
    fg.weight_value[0][:] = w
    fg._push(0, 0)
    _lib.check(L.nsk_gibbs_sweeps(h, 64, 0, 1))
    _lib.check(L.nsk_synchronize(h))
    t0 = time.time()
    _lib.check(L.nsk_gibbs_sweeps(h, 256, 0, 1))
    _lib.check(L.nsk_synchronize(h))
    gibbs_ms = (time.time() - t0) / 256 * 1e3
    info = _lib.SwInfo()
    t0 = time.time()
    _lib.check(L.nsk_sw_setup(h, _lib.BUF_VALUE, 0, 0, C.byref(info)))
    setup_s = time.time() - t0
    cnt = np.zeros((3, 20, 1), np.int64)
    _lib.check(L.nsk_sw_sweeps(h, 3, 0, 1, None, None, None))
    reps = []
    for _ in range(3):
        t0 = time.time()
        _lib.check(L.nsk_sw_sweeps(h, 20, 0, 1, _lib.ptr(cnt[0]), _lib.ptr(cnt[1]), _lib.ptr(cnt[2])))
        reps.append((time.time() - t0) / 20 * 1e3)
    rec = {"grid": [rows, cols], "w": w, "gibbs_sweep_ms": gibbs_ms, "sw_update_ms": reps, "setup_s": setup_s,
           "nbonds": info.nbonds, "ncross": info.ncross, "ntiles": info.ntiles, "in_tiles": 1.0 - info.ncross / max(info.nbonds, 1),
           "clusters_mean": float(cnt[0].mean()), "largest_mean": float(cnt[1].mean()), "flipped_mean": float(cnt[2].mean()),
           "device_bytes": info.device_bytes}
    print(json.dumps(rec), flush=True)
