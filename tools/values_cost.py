"""What the effective sample size of every value of every variable costs on the device (nsk_trace_value_ess), and the
host path it replaces.

    python tools/values_cost.py [--rows 300] [--chains 3] [--lag 63] [--blocks 5] [--calls 8]

One handle: the `gencat` graph of the parity tests (6000 variables of cardinality 2 .. 8 and 30, int8 values), a
full-state trace at thin = 1, every (variable, value) an indicator.  Blocks of `--calls` calls are timed with HIP events
on the handle's stream (nsk_profile_begin / nsk_profile_mark / nsk_profile_read) after a warm-up call; the figures are
medians of `--blocks` blocks, with the spread (max - min).  Prints one JSON line:

  us_per_call   nsk_trace_value_ess with all four arrays: the indicator list sorted and uploaded, both kernels, the
                results back and scattered to the caller's order -- what a caller waits;
  us_device     the same call with no array asked for;
  host_s        the path it replaces, timed with the host clock: nsk_trace_download, then diagnostics.indicators,
                autocov_counts and ess_from_counts of the rows."""

import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=300)
    ap.add_argument("--chains", type=int, default=3)
    ap.add_argument("--lag", type=int, default=63)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=8)
    a = ap.parse_args()
    import numpy as np
    import numbskull_amd
    from numbskull_amd import _lib
    from numbskull_amd.diagnostics import autocov_counts, ess_from_counts, indicators
    from test_hip_parity import _general_tile_graph
    L = _lib.lib()
    g = _general_tile_graph()
    ns = numbskull_amd.NumbSkull(quiet=True, seed=1, chains=a.chains)
    ns.loadFactorGraph(*[x.copy() if isinstance(x, np.ndarray) else x for x in g[:5]], int(g[5]))
    fg = ns.factorGraphs[0]
    h = fg._engine()
    fg._push_chains(0)
    card = fg.variable["cardinality"].astype(np.int64)
    nvar, s = len(card), a.rows
    sel = np.stack([np.repeat(np.arange(nvar), card), np.concatenate([np.arange(k) for k in card])], axis=1)
    csel = _lib.as_c(sel, np.int64)
    nsel = len(csel)
    _lib.check(L.nsk_trace_setup(h, None, 0, 1, s))
    _lib.check(L.nsk_gibbs_sweeps(h, s, 1, 0))
    mean, tau, rhat2 = (np.zeros(nsel) for _ in range(3))
    trunc = np.zeros(nsel, np.uint8)
    ms, nl = C.c_double(), C.c_int64()

    def block(full):
        args = [_lib.ptr(x) if full else None for x in (mean, tau, rhat2, trunc)]
        _lib.check(L.nsk_profile_begin(h))
        for _ in range(a.calls):
            _lib.check(L.nsk_trace_value_ess(h, 0, s, a.lag, _lib.ptr(csel), nsel, *args))
        _lib.check(L.nsk_profile_mark(h))
        _lib.check(L.nsk_profile_read(h, C.byref(ms), C.byref(nl)))
        return ms.value * 1e3 / a.calls

    times = {True: [], False: []}
    for full in (True, False):
        block(full)                                          # warm-up (code object, first touch of the buffers)
    for _ in range(a.blocks):
        for full in (True, False):
            times[full].append(block(full))
    full, dev = sorted(times[True]), sorted(times[False])
    rows = np.zeros((s, a.chains, nvar), np.int8)
    t0 = time.perf_counter()
    _lib.check(L.nsk_trace_download(h, 0, s, _lib.ptr(rows), None))
    t1 = time.perf_counter()
    n, H, A, S1, S2 = autocov_counts(indicators(rows, sel), a.lag)
    want = ess_from_counts(n, H, A, S1, S2)
    t2 = time.perf_counter()
    same = all(np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip((mean, tau, rhat2, trunc), want))
    _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
    print(json.dumps({"graph": "gencat", "variables": nvar, "indicators": nsel, "rows": s, "chains": a.chains, "max_lag": a.lag,
                      "calls_per_block": a.calls, "blocks": a.blocks,
                      "us_per_call": round(full[len(full) // 2], 1), "spread_us": round(full[-1] - full[0], 1),
                      "us_device": round(dev[len(dev) // 2], 1), "spread_device_us": round(dev[-1] - dev[0], 1),
                      "host_download_s": round(t1 - t0, 4), "host_estimator_s": round(t2 - t1, 4), "host_s": round(t2 - t0, 4),
                      "device_equals_host": bool(same), "finite_tau_fraction": round(float(np.isfinite(tau).mean()), 4)}))


if __name__ == "__main__":
    main()
