"""What population annealing costs (nsk_smc_sweeps) on the million-variable Ising grid with 16 chains.

    python tools/smc_cost.py steps [--repeats 7]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/smc_cost.py copy [--repeats 7]

steps: a 50-step schedule through nsk_tempered_sweeps and through nsk_smc_sweeps(threshold = 0), the same outputs asked
for (lp and log_weight), timed with HIP events on the handle's stream (nsk_profile_begin / nsk_profile_mark /
nsk_profile_read) after a warm-up, the two calls taking turns; and, the same way, a launch of a one-element kernel
(torch's in-place add on its own stream).  Prints one JSON line: the medians, the spread (largest minus smallest repeat)
and the difference per step -- the decide kernel's launch is all that the resampling call adds there.

copy: the calls whose copy kernels a kernel trace is to time -- nsk_smc_sweeps over (0, 0.5) with threshold 0.5, where one
chain outweighs the rest and its state fills the 15 other slots (k_smc_copy: 15 chains' value bytes read and written), and
nsk_tempered_sweeps of one step with best_values (k_temper_keep: 16 chains').  Prints the bytes each launch moves; the
kernel times are in the trace's statistics."""

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CHAINS, STEPS = 16, 50


def handle():
    import numbskull_amd
    from numbskull_amd import _lib, graphgen
    g = graphgen.ising_grid(1000, 1000, weight=0.3)
    ns = numbskull_amd.NumbSkull(quiet=True, seed=1)
    ns.loadFactorGraph(*[x.copy() if isinstance(x, np.ndarray) else x for x in g[:5]], int(g[5]))
    fg = ns.factorGraphs[0]
    h = fg._engine()
    fg._push(0, 0)
    _lib.check(_lib.lib().nsk_set_chains(h, CHAINS))
    return fg, h, _lib


def steps(repeats):
    import torch
    fg, h, _lib = handle()
    L = _lib.lib()
    betas = np.linspace(0.0, 1.0, STEPS)
    lp, logw = np.zeros((STEPS, CHAINS)), np.zeros(CHAINS)
    ms, nl = C.c_double(), C.c_int64()

    def timed(call):
        _lib.check(L.nsk_synchronize(h))
        _lib.check(L.nsk_profile_begin(h))
        _lib.check(call())
        _lib.check(L.nsk_profile_mark(h))
        _lib.check(L.nsk_profile_read(h, C.byref(ms), C.byref(nl)))
        return ms.value * 1e3

    def tempered():
        return L.nsk_tempered_sweeps(h, _lib.ptr(betas), STEPS, 1, 0, _lib.ptr(logw), _lib.ptr(lp), None, None)

    def smc():
        return L.nsk_smc_sweeps(h, _lib.ptr(betas), STEPS, 1, 0, 0.0, None, _lib.ptr(logw), _lib.ptr(lp), None, None, None)

    for _ in range(2):
        timed(tempered)
        timed(smc)
    res = {"tempered": [], "smc": []}
    for _ in range(repeats):
        res["tempered"].append(timed(tempered))
        res["smc"].append(timed(smc))
    x = torch.zeros(1, device="cuda")
    n = 2000
    launch = []
    for _ in range(repeats + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            x.add_(1.0)
        b.record()
        torch.cuda.synchronize()
        launch.append(a.elapsed_time(b) * 1e3 / n)
    launch = launch[2:]
    med = {k: float(np.median(v)) for k, v in res.items()}
    out = {"graph": "ising 1000 x 1000, weight 0.3", "chains": CHAINS, "steps": STEPS, "repeats": repeats,
           "us_per_call": {k: [round(x, 1) for x in v] for k, v in res.items()},
           "median_us_per_step": {k: round(v / STEPS, 3) for k, v in med.items()},
           "spread_us_per_step": {k: round((max(v) - min(v)) / STEPS, 3) for k, v in res.items()},
           "difference_us_per_step": round((med["smc"] - med["tempered"]) / STEPS, 3),
           "small_kernel_launch_us": round(float(np.median(launch)), 3),
           "small_kernel_launch_spread_us": round(max(launch) - min(launch), 3)}
    print(json.dumps(out))
    fg.close()


def copy(repeats):
    fg, h, _lib = handle()
    L = _lib.lib()
    info = fg.info()
    iid, nid = np.zeros(len(fg.variable), np.int32), C.c_int64()
    _lib.check(L.nsk_graph_get_layout(h, _lib.ptr(iid), C.byref(nid)))
    nbytes = nid.value * info["value_bytes"]
    betas, off = np.array([0.0, 0.5]), np.array([0.5])
    anc, flag = np.zeros((1, CHAINS), np.int32), np.zeros(1, np.int32)
    best = np.zeros((CHAINS, len(fg.variable)), np.int64)
    one = np.array([0.5])
    copies = []
    for _ in range(repeats + 2):
        _lib.check(L.nsk_smc_sweeps(h, _lib.ptr(betas), 2, 1, 0, 0.5, _lib.ptr(off), None, None, None, _lib.ptr(anc), _lib.ptr(flag)))
        copies.append(int((anc[0] != np.arange(CHAINS)).sum()))
        _lib.check(L.nsk_tempered_sweeps(h, _lib.ptr(one), 1, 1, 0, None, None, _lib.ptr(best), None))
    print(json.dumps({"value_bytes_per_chain": nbytes, "k_smc_copy_chains_per_launch": copies,
                      "k_smc_copy_bytes_read_and_written": [2 * c * nbytes for c in copies],
                      "k_temper_keep_chains_per_launch": CHAINS, "k_temper_keep_bytes_read_and_written": 2 * CHAINS * nbytes,
                      "launches_each": repeats + 2}))
    fg.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["steps", "copy"])
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    (steps if a.mode == "steps" else copy)(a.repeats)
