"""What a sample trace costs (nsk_trace_setup): us per tallied sweep with and without a trace, this library against the
parent commit's, block by block.

    python tools/trace_cost.py --graph 10m|1m8 --lib-a PARENT.so [--lib-b THIS.so] [--sweeps 2048] [--blocks 5]

One process per library (a process loads one libnumbskull_amd.so); the parent process runs this script as a worker
per library and reads one command per line: the libraries therefore take their blocks in turn, A B A B ..., in one
command on one machine.  A block = `--sweeps` tallied sweeps timed with HIP events on the handle's stream
(nsk_profile_begin / nsk_profile_mark / nsk_profile_read) after 10 warm-up sweeps; nsk_trace_clear between blocks
keeps the buffer at one block.  Prints one JSON line: per configuration the blocks' us per sweep, their median and
spread, and the cost per record launch derived from the medians ((traced - untraced) x thin).

Configurations: 10m = the 10M-variable grid of bench.py, one chain: untraced; every variable at thin 1, 8 and 64;
10 000 columns at thin 1.  1m8 = the 1000 x 1000 grid, 8 chains: untraced; every variable at thin 8.  The parent's
library has no traces: it runs the untraced configuration only."""

import argparse
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _configs(graph):
    if graph == "10m":
        return [("untraced", None), ("all_thin1", (None, 1)), ("all_thin8", (None, 8)), ("all_thin64", (None, 64)),
                ("cols10000_thin1", (10000, 1))]
    return [("untraced", None), ("all_thin8", (None, 8))]


def worker(graph, sweeps):
    import numpy as np
    import numbskull_amd
    from numbskull_amd import _lib, graphgen
    L = _lib.lib()
    chains = 8 if graph == "1m8" else 1
    g = graphgen.ising_grid(2500, 4000, weight=0.1) if graph == "10m" else graphgen.ising_grid(1000, 1000, weight=0.3)
    ns = numbskull_amd.NumbSkull(quiet=True, seed=1, chains=chains)
    ns.loadFactorGraph(*[x.copy() if isinstance(x, np.ndarray) else x for x in g[:5]], int(g[5]))
    fg = ns.factorGraphs[0]
    h = fg._engine()
    if chains > 1:
        fg._push_chains(0)
    else:
        fg._push(0, 0)
    nvar = len(fg.variable)
    cfg = dict(_configs(graph))
    current = None
    print("ready", flush=True)
    for line in sys.stdin:
        name = line.strip()
        if name == "quit":
            break
        if name != current:                     # set the configuration up (untimed), warm up
            if hasattr(L, "nsk_trace_setup") and current is not None and cfg[current] is not None:
                _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
            if cfg[name] is not None:
                ncols, thin = cfg[name]
                ids = None if ncols is None else np.ascontiguousarray(np.arange(ncols, dtype=np.int64) * (nvar // ncols))
                _lib.check(L.nsk_trace_setup(h, _lib.ptr(ids), 0 if ids is None else len(ids), thin, sweeps // thin + 2))
            current = name
        elif cfg[name] is not None:
            _lib.check(L.nsk_trace_clear(h))
        _lib.check(L.nsk_gibbs_sweeps(h, 10, 0, 0))
        if cfg[name] is not None:
            _lib.check(L.nsk_trace_clear(h))
        _lib.check(L.nsk_synchronize(h))
        ms, nl = C.c_double(), C.c_int64()
        _lib.check(L.nsk_profile_begin(h))
        _lib.check(L.nsk_gibbs_sweeps(h, sweeps, 0, 0))
        _lib.check(L.nsk_profile_mark(h))
        _lib.check(L.nsk_profile_read(h, C.byref(ms), C.byref(nl)))
        print(json.dumps({"us_per_sweep": ms.value * 1e3 / sweeps, "launches": nl.value}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=["10m", "1m8"], default="10m")
    ap.add_argument("--lib-a", help="the parent commit's libnumbskull_amd.so")
    ap.add_argument("--lib-b", default=os.path.join(REPO, "numbskull_amd", "libnumbskull_amd.so"))
    ap.add_argument("--sweeps", type=int, default=2048)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.graph, a.sweeps)
    if not a.lib_a:
        ap.error("--lib-a: the parent commit's library is needed")
    procs = {}
    for tag, lib in (("parent", a.lib_a), ("this", a.lib_b)):
        env = dict(os.environ, NSK_LIB=os.path.abspath(lib))
        procs[tag] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--graph", a.graph,
                                       "--sweeps", str(a.sweeps)], env=env, stdin=subprocess.PIPE,
                                      stdout=subprocess.PIPE, text=True)
    for p in procs.values():
        if p.stdout.readline().strip() != "ready":
            raise SystemExit("a worker did not start")

    def block(tag, name):
        p = procs[tag]
        p.stdin.write(name + "\n")
        p.stdin.flush()
        line = p.stdout.readline()
        if not line:
            raise SystemExit("worker %s ended in %s" % (tag, name))
        return json.loads(line)["us_per_sweep"]

    out = {"graph": a.graph, "sweeps_per_block": a.sweeps, "blocks": {}}
    for name, spec in _configs(a.graph):
        tags = ["parent", "this"] if spec is None else ["this"]
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
    out["median_us_per_sweep"] = {k: round(v, 3) for k, v in med.items()}
    out["spread_us_per_sweep"] = {k: round(max(v) - min(v), 3) for k, v in out["blocks"].items()}
    base = med["this/untraced"]
    out["us_per_record_launch"] = {k.split("/")[1]: round((v - base) * dict(_configs(a.graph))[k.split("/")[1]][1], 3)
                                   for k, v in med.items() if not k.endswith("untraced")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
