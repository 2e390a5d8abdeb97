"""What the effective sample size from the trace costs on the device (nsk_trace_ess), and the host path it replaces.

    python tools/ess_cost.py [--side 1000] [--chains 8] [--rows 256,1024] [--lags 15,31,63] [--blocks 5] [--calls 8]
                             [--host-columns 8192]

One handle: a side x side Ising grid, `--chains` chains, a full-state trace (every variable, bit-packed) at thin = 1.
For each row count s the trace is recorded once; then, per max_lag, blocks of `--calls` calls are timed with HIP events on
the handle's stream (nsk_profile_begin / nsk_profile_mark / nsk_profile_read) after a warm-up call, the configurations
taking their blocks in turn; the figures are medians of `--blocks` blocks, with the spread (max - min).  Prints one
JSON line:

  us_per_call       nsk_trace_ess with all four arrays: the kernel, 25 bytes a device column back over PCIe and the
                    permutation to the caller's columns on the host threads -- what a caller waits;
  us_device         the same call with no array asked for: the kernel, its launch and the synchronisation alone;
  bytes_read        s x chains x words x 8: every packed row of the window once;
  gb_s, ratio_to_stream   bytes_read over us_device, against nsk_selftest_stream(width = 16) of the same run;
  host              the path it replaces -- nsk_trace_download + diagnostics.effective_sample_size -- timed with the
                    host clock on a trace of `--host-columns` listed columns and EXTRAPOLATED linearly to every
                    column of the grid (marked "extrapolated": the full download is 8 bytes per packed byte and was
                    not run)."""

import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--rows", default="256,1024")
    ap.add_argument("--lags", default="15,31,63")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--host-columns", type=int, default=8192)
    a = ap.parse_args()
    import numpy as np
    import numbskull_amd
    from numbskull_amd import _lib, graphgen
    from numbskull_amd.diagnostics import effective_sample_size
    L = _lib.lib()
    g = graphgen.ising_grid(a.side, a.side, weight=0.1)
    ns = numbskull_amd.NumbSkull(quiet=True, seed=1, chains=a.chains)
    ns.loadFactorGraph(*[x.copy() if isinstance(x, np.ndarray) else x for x in g[:5]], int(g[5]))
    fg = ns.factorGraphs[0]
    h = fg._engine()
    fg._push_chains(0)
    nvar = len(fg.variable)
    gbs = C.c_double()
    _lib.check(L.nsk_selftest_stream(0, 1 << 30, 16, 5, C.byref(gbs)))
    out = {"graph": "%dx%d grid" % (a.side, a.side), "chains": a.chains, "calls_per_block": a.calls, "blocks": a.blocks,
           "stream_gb_s": round(gbs.value, 1), "rows": {}}
    mean, tau, rhat2 = (np.zeros(nvar) for _ in range(3))
    trunc = np.zeros(nvar, np.uint8)
    ms, nl = C.c_double(), C.c_int64()

    def block(s, lag, full):
        args = [_lib.ptr(x) if full else None for x in (mean, tau, rhat2, trunc)]
        _lib.check(L.nsk_profile_begin(h))
        for _ in range(a.calls):
            _lib.check(L.nsk_trace_ess(h, 0, s, lag, *args))
        _lib.check(L.nsk_profile_mark(h))
        _lib.check(L.nsk_profile_read(h, C.byref(ms), C.byref(nl)))
        return ms.value * 1e3 / a.calls

    for s in [int(x) for x in a.rows.split(",")]:
        before = fg.info()["device_bytes"]
        _lib.check(L.nsk_trace_setup(h, None, 0, 1, s))
        nbytes = fg.info()["device_bytes"] - before        # the trace buffer: s x chains x words x 8 (a full-state trace has no column list)
        assert nbytes > 0 and nbytes % (s * a.chains * 8) == 0 and nbytes >= s * a.chains * nvar // 8
        _lib.check(L.nsk_gibbs_sweeps(h, s, 0, 0))
        res = {}
        cfgs = [(int(lag), full) for lag in a.lags.split(",") for full in (True, False)]
        for lag, full in cfgs:
            block(s, lag, full)                              # warm-up (code object, first touch of the buffers)
        times = {c: [] for c in cfgs}
        for _ in range(a.blocks):
            for c in cfgs:
                times[c].append(block(s, c[0], c[1]))
        for lag in [int(x) for x in a.lags.split(",")]:
            full, dev = sorted(times[(lag, True)]), sorted(times[(lag, False)])
            mf, md = full[len(full) // 2], dev[len(dev) // 2]
            res["max_lag_%d" % lag] = {"us_per_call": round(mf, 1), "spread_us": round(full[-1] - full[0], 1),
                                       "us_device": round(md, 1), "spread_device_us": round(dev[-1] - dev[0], 1),
                                       "gb_s": round(nbytes / md / 1e3, 1), "ratio_to_stream": round(nbytes / md / 1e3 / gbs.value, 3)}
        finite = float(np.isfinite(tau).mean())
        res["bytes_read"] = nbytes
        res["finite_tau_fraction"] = round(finite, 4)
        res["truncated_fraction_last_lag"] = round(float(trunc.mean()), 4)
        # the host path on a listed trace of some columns, extrapolated
        nc = min(a.host_columns, nvar)
        cols = _lib.as_c(np.linspace(0, nvar - 1, nc).astype(np.int64), np.int64)
        _lib.check(L.nsk_trace_setup(h, _lib.ptr(cols), nc, 1, s))
        _lib.check(L.nsk_gibbs_sweeps(h, s, 0, 0))
        _lib.check(L.nsk_synchronize(h))
        rows = np.zeros((s, a.chains, nc), np.int8)
        t0 = time.perf_counter()
        _lib.check(L.nsk_trace_download(h, 0, s, _lib.ptr(rows), None))
        t1 = time.perf_counter()
        ess = effective_sample_size(rows)
        t2 = time.perf_counter()
        res["host"] = {"columns": nc, "download_s": round(t1 - t0, 4), "estimator_s": round(t2 - t1, 4),
                       "extrapolated_s_all_columns": round((t2 - t0) * nvar / nc, 2), "extrapolated": True,
                       "finite_fraction": round(float(np.isfinite(ess).mean()), 4)}
        _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
        out["rows"][str(s)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
