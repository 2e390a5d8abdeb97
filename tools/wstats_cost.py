"""What the per-weight statistics cost (nsk_weight_stats, the stats column of a sample trace), this library against the
parent commit's, block by block -- the method of tools/energy_cost.py.

    python tools/wstats_cost.py --graph 10m|boolw4m --lib-a PARENT.so [--lib-b THIS.so] [--sweeps 1024] [--blocks 5]

One process per library: the parent process runs this script as a worker per library and sends one command per line,
so the libraries take their blocks in turn, A B A B ..., in one command on one machine.  A block is timed with HIP
events on the handle's stream (nsk_profile_begin / nsk_profile_mark / nsk_profile_read) after a warm-up; the figures are
medians of `--blocks` blocks, with the spread (max - min) beside them.  Prints one JSON line:

  (a) column off, both libraries: us per untraced sweep, and per tallied sweep of a full-state trace at thin = 8 with
      the lp column -- this library must lie inside the parent's own block-to-block spread;
  (b) column on, this library: us per evaluation on the device alone, for the stats column and for the lp column in the
      same run: a full-state trace at thin = 1 with the column minus the same trace without it (nothing returns to the
      host between sweeps); and us per nsk_weight_stats / nsk_log_potential call as a caller waits for it;
  the bytes one evaluation of the statistics must move -- what the log-potential's walk moves without the weights
  (f_rec 16 a factor, m_rec 8 an edge, the members' values) + the by-weight list (4 a factor) + the work list (8 a
  short weight, 16 a piece) + the sums written (8 a weight with factors) -- over the device-only time, against what
  nsk_selftest_stream(width = 16) reports in the same run.

10m: the 2500 x 4000 grid with two weights (10^7 factors each); boolw4m: boolean_weighted_graph(4 000 000), one weight
per factor."""

import argparse
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

QUERIES = 32
# name -> (thin or None, lp column, stats column, runs on the parent's library too)
CONFIGS = [("untraced", (None, False, False, True)), ("all_thin8_lp", (8, True, False, True)),
           ("all_thin1", (1, False, False, False)), ("all_thin1_lp", (1, True, False, False)),
           ("all_thin1_ws", (1, False, True, False)), ("query_lp", (None, False, False, False)),
           ("query_ws", (None, False, False, False))]
SHORT, PIECE = 16, 2048         # nsk_internal.h NSK_WSTATS_SHORT, NSK_WSTATS_PIECE


def worker(graph, sweeps):
    import numpy as np
    import numbskull_amd
    from numbskull_amd import _lib, graphgen
    L = _lib.lib()
    g = graphgen.ising_grid(2500, 4000, weight=0.1, two_weights=True) if graph == "10m" else graphgen.boolean_weighted_graph(4000000)
    ns = numbskull_amd.NumbSkull(quiet=True, seed=1)
    ns.loadFactorGraph(*[x.copy() if isinstance(x, np.ndarray) else x for x in g[:5]], int(g[5]))
    fg = ns.factorGraphs[0]
    h = fg._engine()
    fg._push(0, 0)
    cfg = dict(CONFIGS)
    current = None
    gbs = C.c_double()
    _lib.check(L.nsk_selftest_stream(0, 1 << 30, 16, 5, C.byref(gbs)))
    info = fg.info()
    nf, ne, nw = len(fg.factor), len(fg.fmap), len(fg.weight)
    lens = np.bincount(np.asarray(fg.factor["weightId"], np.int64), minlength=nw)
    nshort = int(((lens >= 1) & (lens <= SHORT)).sum())
    npiece = int(((lens[lens > SHORT] + PIECE - 1) // PIECE).sum())
    walk = 16 * nf + (8 + info["value_bytes"]) * ne
    print(json.dumps({"ready": True, "stream_gb_s": gbs.value, "bytes_lp": walk + 8 * nw,
                      "bytes_ws": walk + 4 * nf + 8 * nshort + 16 * npiece + 8 * int((lens > 0).sum()),
                      "nfactor": nf, "nedge": ne, "nweight": nw, "short_weights": nshort, "pieces": npiece}), flush=True)
    out = np.zeros(max(nw, 1))
    ms, nl = C.c_double(), C.c_int64()
    for line in sys.stdin:
        name = line.strip()
        if name == "quit":
            break
        thin, lp, ws, _ = cfg[name]
        if name.startswith("query"):
            def call():
                if name == "query_lp":
                    _lib.check(L.nsk_log_potential(h, _lib.BUF_VALUE, 0, 1, _lib.ptr(out)))
                else:
                    _lib.check(L.nsk_weight_stats(h, _lib.BUF_VALUE, 0, 1, 0, _lib.ptr(out)))
            for _ in range(4):
                call()
            _lib.check(L.nsk_profile_begin(h))
            for _ in range(QUERIES):
                call()
            _lib.check(L.nsk_profile_mark(h))
            _lib.check(L.nsk_profile_read(h, C.byref(ms), C.byref(nl)))
            print(json.dumps({"us": ms.value * 1e3 / QUERIES, "bytes": fg.info()["device_bytes"]}), flush=True)
            continue
        if name != current:                     # set the configuration up (untimed)
            if current is not None and cfg[current][0] is not None:
                _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
            if thin is not None:
                _lib.check(L.nsk_trace_setup(h, None, 0, thin, sweeps // thin + 12))
                if lp:
                    _lib.check(L.nsk_trace_log_potential(h, 1))
                if ws:
                    _lib.check(L.nsk_trace_weight_stats(h, None, 0, 0))
            current = name
        elif thin is not None:
            _lib.check(L.nsk_trace_clear(h))
        _lib.check(L.nsk_gibbs_sweeps(h, 10, 0, 0))
        if thin is not None:
            _lib.check(L.nsk_trace_clear(h))
        _lib.check(L.nsk_synchronize(h))
        _lib.check(L.nsk_profile_begin(h))
        _lib.check(L.nsk_gibbs_sweeps(h, sweeps, 0, 0))
        _lib.check(L.nsk_profile_mark(h))
        _lib.check(L.nsk_profile_read(h, C.byref(ms), C.byref(nl)))
        print(json.dumps({"us": ms.value * 1e3 / sweeps, "launches": nl.value}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=["10m", "boolw4m"], default="10m")
    ap.add_argument("--lib-a", help="the parent commit's libnumbskull_amd.so")
    ap.add_argument("--lib-b", default=os.path.join(REPO, "numbskull_amd", "libnumbskull_amd.so"))
    ap.add_argument("--sweeps", type=int, default=1024)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.graph, a.sweeps)
    if not a.lib_a:
        ap.error("--lib-a: the parent commit's library is needed")
    procs, hello = {}, {}
    for tag, lib in (("parent", a.lib_a), ("this", a.lib_b)):
        env = dict(os.environ, NSK_LIB=os.path.abspath(lib))
        procs[tag] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--graph", a.graph,
                                       "--sweeps", str(a.sweeps)], env=env, stdin=subprocess.PIPE,
                                      stdout=subprocess.PIPE, text=True)
    for tag, p in procs.items():
        line = p.stdout.readline()
        if not line.startswith("{"):
            raise SystemExit("worker %s did not start" % tag)
        hello[tag] = json.loads(line)

    def block(tag, name):
        p = procs[tag]
        p.stdin.write(name + "\n")
        p.stdin.flush()
        line = p.stdout.readline()
        if not line:
            raise SystemExit("worker %s ended in %s" % (tag, name))
        return json.loads(line)["us"]

    out = {"graph": a.graph, "sweeps_per_block": a.sweeps, "queries_per_block": QUERIES, "shape": hello["this"], "blocks": {}}
    for name, (_, _, _, both) in CONFIGS:
        tags = ["parent", "this"] if both else ["this"]
        res = {t: [] for t in tags}
        for _ in range(a.blocks):
            for t in tags:                       # alternated block by block
                res[t].append(block(t, name))
        for t in tags:
            out["blocks"]["%s/%s" % (t, name)] = [round(x, 3) for x in res[t]]
    for p in procs.values():
        p.stdin.write("quit\n")
        p.stdin.flush()
        p.wait(timeout=120)
    med = {k: sorted(v)[len(v) // 2] for k, v in out["blocks"].items()}
    out["median_us"] = {k: round(v, 3) for k, v in med.items()}
    out["spread_us"] = {k: round(max(v) - min(v), 3) for k, v in out["blocks"].items()}
    stream = hello["this"]["stream_gb_s"]
    out["evaluation"] = {}
    for col, nbytes in (("lp", hello["this"]["bytes_lp"]), ("ws", hello["this"]["bytes_ws"])):
        device_us = med["this/all_thin1_" + col] - med["this/all_thin1"]
        out["evaluation"][col] = {"us_per_call": round(med["this/query_" + col], 3), "us_on_device": round(device_us, 3),
                                  "bytes": nbytes, "gb_s": round(nbytes / device_us / 1e3, 1) if device_us > 0 else None,
                                  "ratio_to_stream": round(nbytes / device_us / 1e3 / stream, 3) if device_us > 0 else None}
    out["stream_gb_s"] = round(stream, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
