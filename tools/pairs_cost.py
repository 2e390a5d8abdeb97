"""What the pairwise counts from the trace cost on the device (nsk_trace_pair_counts).

    python tools/pairs_cost.py [--side 1000] [--chains 4] [--rows 1024] [--blocks 5] [--calls 4]

One handle: a side x side Ising grid, `--chains` chains, a full-state trace (every variable, bit-packed) at thin = 1,
recorded once.  Two pair lists are timed, each in blocks of `--calls` calls with HIP events on the handle's stream
(nsk_profile_begin / nsk_profile_mark / nsk_profile_read) after a warm-up call, taking their blocks in turn; the figures
are medians of `--blocks` blocks, with the spread (max - min).  Prints one JSON line:

  factors     the two ends of every edge of the grid (diagnostics.factor_pairs): every word of the row is transposed
              and 2 side (side - 1) waves count;
  per_word    side^2 / 64 pairs (v, v + 1), v a multiple of 64: about as many words transposed, 1 / (2 x 64) of the
              pairs -- the call is the transposition and little else;
  us_per_call the whole call: both kernels, the pair list up, 24 bytes per pair and chain back over PCIe;
  trace_bytes rows x chains x words x 8: what k_trace_transpose reads, and writes again as T, when every word is
              touched;  pair_bytes  pairs x 2 x chains x ceil(rows / 64) x 8: what k_trace_pair_counts reads of T;
  result_bytes  pairs x chains x 24;
  stream_gb_s nsk_selftest_stream(width = 16) of the same run.

The events bracket the call, copies included.  The time of each kernel alone is the kernel trace of one run of this
script (rocprofv3 --kernel-trace --stats -- python tools/pairs_cost.py --blocks 1 --calls 1): k_trace_transpose and
k_trace_pair_counts are its two rows."""

import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    a = ap.parse_args()
    import numpy as np
    import numbskull_amd
    from numbskull_amd import _lib, graphgen
    from numbskull_amd.diagnostics import factor_pairs
    L = _lib.lib()
    g = graphgen.ising_grid(a.side, a.side, weight=0.1)
    ns = numbskull_amd.NumbSkull(quiet=True, seed=1, chains=a.chains)
    ns.loadFactorGraph(*[x.copy() if isinstance(x, np.ndarray) else x for x in g[:5]], int(g[5]))
    fg = ns.factorGraphs[0]
    h = fg._engine()
    fg._push_chains(0)
    nvar, s = len(fg.variable), a.rows
    gbs = C.c_double()
    _lib.check(L.nsk_selftest_stream(0, 1 << 30, 16, 5, C.byref(gbs)))
    before = fg.info()["device_bytes"]
    _lib.check(L.nsk_trace_setup(h, None, 0, 1, s))
    trace_bytes = fg.info()["device_bytes"] - before       # s x chains x words x 8 (a full-state trace has no column list)
    assert trace_bytes > 0 and trace_bytes % (s * a.chains * 8) == 0
    _lib.check(L.nsk_gibbs_sweeps(h, s, 0, 0))
    first = np.arange(0, nvar - 1, 64, dtype=np.int64)
    lists = {"factors": _lib.as_c(factor_pairs(fg.factor, fg.fmap), np.int64),
             "per_word": _lib.as_c(np.stack([first, first + 1], axis=1), np.int64)}
    outs = {k: np.zeros((len(p), a.chains, 3), np.int64) for k, p in lists.items()}
    ms, nl = C.c_double(), C.c_int64()

    def block(k):
        _lib.check(L.nsk_profile_begin(h))
        for _ in range(a.calls):
            _lib.check(L.nsk_trace_pair_counts(h, 0, s, _lib.ptr(lists[k]), len(lists[k]), _lib.ptr(outs[k])))
        _lib.check(L.nsk_profile_mark(h))
        _lib.check(L.nsk_profile_read(h, C.byref(ms), C.byref(nl)))
        return ms.value * 1e3 / a.calls

    for k in lists:
        block(k)                                            # warm-up (code object, first touch of the buffers)
    times = {k: [] for k in lists}
    for _ in range(a.blocks):
        for k in lists:
            times[k].append(block(k))
    nb = (s + 63) // 64
    out = {"graph": "%dx%d grid" % (a.side, a.side), "chains": a.chains, "rows": s, "calls_per_block": a.calls, "blocks": a.blocks,
           "stream_gb_s": round(gbs.value, 1), "trace_bytes": trace_bytes}
    for k, p in lists.items():
        t = sorted(times[k])
        n1 = outs[k][:, :, 1]
        assert (n1 > 0).any() and (outs[k][:, :, 0] <= n1).all() and (n1 <= s).all()
        out[k] = {"pairs": len(p), "us_per_call": round(t[len(t) // 2], 1), "spread_us": round(t[-1] - t[0], 1),
                  "pair_bytes": len(p) * 2 * a.chains * nb * 8, "result_bytes": len(p) * a.chains * 24}
    _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
