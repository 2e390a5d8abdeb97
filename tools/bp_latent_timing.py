"""What a step of latent-variable learning by belief propagation costs: nsk_bp_latent_steps, which runs the clamped and the
free set-up in the same launches, against nsk_bp_learn_steps on the clamped set-up plus nsk_bp_learn_steps on the free
set-up -- the two phases back to back.

    python tools/bp_latent_timing.py [--grids 32 512] [--iters 10] [--repeats 7] [--singles-only]
    NSK_LIB=/path/to/an/older/libnumbskull_amd.so python tools/bp_latent_timing.py --singles-only

Per grid (n x n Ising, weights 0.3 / -0.2 learnable, every third variable evidence at alternating values): one handle
with both set-ups resident; a call is `steps` steps of `iters` iterations at tol = 0 (no early exit), warm, and ends in
the call's own synchronise, so the host clock around it measures the work.  The three calls -- paired, single clamped,
single free -- take turns, after a warm-up of each, `repeats` times; the weights are pushed again before every call, so
every call does the same work.  Prints one JSON line per grid: median and spread (max - min) in microseconds a step, the
sum of the two single medians, the kernel launches a step, and paired over that sum.  --singles-only times the two
single calls alone: an older library (NSK_LIB) without the paired entry point gives the baseline that way."""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STEPS = {32: 200, 512: 40}          # steps a call: some tens of milliseconds of work either way


def cost(n, iters, repeats, singles_only):
    import numbskull_amd
    from numbskull_amd import _lib, graphgen
    g = list(graphgen.ising_grid(n, n, weight=0.3, fixed=False, two_weights=True))
    w = g[0].copy()
    w["initialValue"] = (0.3, -0.2)
    g[0] = w
    ev = np.arange(0, n * n, 3)
    var = g[1].copy()
    var["isEvidence"][ev] = 1
    var["initialValue"][ev] = np.arange(len(ev)) % 2
    g[1] = var
    ns = numbskull_amd.NumbSkull(quiet=True, seed=1)
    ns.loadFactorGraph(*[x.copy() if isinstance(x, np.ndarray) else x for x in g[:5]], int(g[5]))
    fg = ns.factorGraphs[0]
    L, h = _lib.lib(), fg._engine()
    fg._push(0, 0)
    steps = STEPS.get(n, max(1, min(4096, 65536 // iters, (1 << 23) // (n * n))))
    info = [_lib.BpInfo(), _lib.BpInfo()]
    if singles_only:                # (an older library has one set-up: it is rebuilt before every call, outside the clock)
        def prepare(slot):
            _lib.check(L.nsk_bp_setup(h, _lib.BUF_VALUE, 0, slot, C.byref(info[slot])))
    else:
        for slot in (0, 1):
            _lib.check(L.nsk_bp_select(h, slot))
            _lib.check(L.nsk_bp_setup(h, _lib.BUF_VALUE, 0, slot, C.byref(info[slot])))

        def prepare(slot):
            _lib.check(L.nsk_bp_select(h, slot))
    target = np.full(len(fg.weight), 0.5)
    args = (steps, iters, 0.0, 0.0, 1, 1e-4, 1.0, 0.0, 1, None, None, None, None, None)

    def timed(which):
        fg._push(0, 0)
        if which != "paired":
            prepare(0 if which == "single_clamped" else 1)
        _lib.check(L.nsk_synchronize(h))
        t0 = time.perf_counter()
        if which == "paired":
            _lib.check(L.nsk_bp_latent_steps(h, *args))
        else:
            _lib.check(L.nsk_bp_learn_steps(h, _lib.ptr(target), *args))
        return (time.perf_counter() - t0) * 1e6 / steps

    calls = ["single_clamped", "single_free"] + ([] if singles_only else ["paired"])
    for c in calls:
        timed(c)
        timed(c)
    out = {c: [] for c in calls}
    for _ in range(repeats):
        for c in calls:
            out[c].append(timed(c))
    med = {c: float(np.median(v)) for c, v in out.items()}

    def launches(i):                # refresh, psi, fnorm, moments, the update; a factor and a variable launch an iteration
        return 5 + (2 * iters if i.nedges > 0 else 0)       # (every variable is binary: one variable launch)

    both = med["single_clamped"] + med["single_free"]
    line = {"graph": "ising %d x %d, every third variable evidence" % (n, n), "library": os.environ.get("NSK_LIB", "in-tree"),
            "steps_per_call": steps, "iters_per_step": iters, "repeats": repeats,
            "edges": [int(i.nedges) for i in info], "table_entries": [int(i.ntable) for i in info],
            "median_us_per_step": {c: round(v, 1) for c, v in med.items()},
            "spread_us_per_step": {c: round(max(v) - min(v), 1) for c, v in out.items()},
            "sum_of_singles_us_per_step": round(both, 1),
            "kernel_launches_per_step": {"single_clamped": launches(info[0]), "single_free": launches(info[1]),
                                         "paired": max(launches(info[0]), launches(info[1]))}}
    if not singles_only:
        line["paired_over_sum_of_singles"] = round(med["paired"] / both, 3)
    print(json.dumps(line), flush=True)
    fg.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", nargs="+", type=int, default=[32, 512])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--singles-only", action="store_true")
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("at least 5 repeats: the spread is part of the result")
    for n in a.grids:
        cost(n, a.iters, a.repeats, a.singles_only)
