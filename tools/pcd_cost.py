"""What a step of persistent contrastive divergence costs (nsk_pcd_steps), split into sweeps, moment pass and update, beside
the parent commit's time for the same burn-in sweeps alone and for nsk_weight_stats of the same chains -- the method of
tools/wstats_cost.py.

    python tools/pcd_cost.py --graph 10m|lr5m --chains R --lib-a PARENT.so [--lib-b THIS.so] [--steps 64] [--blocks 5]

One process per library: the parent process runs this script as a worker per library and sends one command per line, so the
libraries take their blocks in turn, A B A B ..., in one command on one machine.  A block is timed with HIP events on the
handle's stream (nsk_profile_begin / nsk_profile_mark / nsk_profile_read) after a warm-up; the figures are medians of
`--blocks` blocks, with the spread (max - min) beside them.  Prints one JSON line:

  sweep          us per burn-in sweep of all R chains, `steps` sweeps in one nsk_gibbs_sweeps call (both libraries)
  ws_device      us per evaluation of the statistics of all R chains on the device alone: a one-column trace at thin = 1
                 with the stats column minus the same trace without it (both libraries)
  pcd1, pcd2     us per step of one nsk_pcd_steps call of `steps` steps with sweeps_per_step = 1 and 2 (this library)
  split          sweep_in_step = pcd2 - pcd1 (one more sweep a step); the rest = pcd1 - sweep_in_step: the refresh of what
                 derives from the weights, zeroing M, the moment launches and the update; the rest over the parent's
                 ws_device; and the sweeps_per_step at which sweeps and rest are equal.  The events bracket the whole
                 call, so the rest also holds the call's host-side set-up (the range bound over all factors, the work
                 list) divided by `steps`: the kernel trace below is the figure for the launches alone

--trace: one call of `steps` steps and nothing else, to run under a kernel trace (rocprofv3 --kernel-trace --stats), which
splits the rest by kernel: k_moments_short / k_moments_piece, k_pcd_update, the refresh kernels.

10m: the 2500 x 4000 grid under ONE free weight (2 x 10^7 factors on one accumulator); lr5m: mixed_lr_graph(5 000 000) with
10^6 weights, head_by_vid."""

import argparse
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CONFIGS = [("sweep", True), ("trace", True), ("trace_ws", True), ("pcd1", False), ("pcd2", False)]


def build(graph, chains):
    import numpy as np
    import numbskull_amd
    from numbskull_amd import _lib, graphgen
    if graph == "10m":
        g, hbv = graphgen.ising_grid(2500, 4000, weight=0.1, fixed=False), False
    else:
        g, hbv = graphgen.mixed_lr_graph(5000000, nweights=1000000), True
        w = g[0].copy()
        w["isFixed"] = False
        g = (w,) + tuple(g[1:])
    ns = numbskull_amd.NumbSkull(quiet=True, seed=1, head_by_vid=hbv)
    ns.loadFactorGraph(*[x.copy() if isinstance(x, np.ndarray) else x for x in g[:5]], int(g[5]))
    fg = ns.factorGraphs[0]
    h = fg._engine()
    fg._push(0, 0)
    if chains > 1:
        _lib.check(_lib.lib().nsk_set_chains(h, chains))
    return fg, h


def worker(graph, chains, steps, trace_only):
    import numpy as np
    from numbskull_amd import _lib
    L = _lib.lib()
    fg, h = build(graph, chains)
    nw = len(fg.weight)
    target = np.zeros(nw)
    if trace_only:
        _lib.check(L.nsk_pcd_steps(h, _lib.ptr(target), 4, 1, 1, 1e-3, 1.0, 0.0, 1, None, None))
        _lib.check(L.nsk_pcd_steps(h, _lib.ptr(target), steps, 1, 1, 1e-3, 1.0, 0.0, 1, None, None))
        return
    lens = np.bincount(np.asarray(fg.factor["weightId"], np.int64), minlength=nw)
    print(json.dumps({"ready": True, "nvar": len(fg.variable), "nfactor": len(fg.factor), "nweight": nw, "chains": chains,
                      "short_weights": int(((lens >= 1) & (lens <= _lib.MOMENTS_SHORT)).sum()) if hasattr(_lib, "MOMENTS_SHORT") else None,
                      "pieces": int(((lens[lens > 16] + 2047) // 2048).sum())}), flush=True)
    ms, nl = C.c_double(), C.c_int64()
    one = np.zeros(1, np.int64)
    current = None
    for line in sys.stdin:
        name = line.strip()
        if name == "quit":
            break
        if name.startswith("trace") and name != current:        # set the configuration up (untimed)
            _lib.check(L.nsk_trace_setup(h, _lib.ptr(one), 1, 1, steps + 12))
            if name == "trace_ws":
                _lib.check(L.nsk_trace_weight_stats(h, None, 0, 0))
        elif current is not None and current.startswith("trace") and not name.startswith("trace"):
            _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
        current = name
        if name.startswith("pcd"):
            sps = int(name[3:])
            run = lambda n: L.nsk_pcd_steps(h, _lib.ptr(target), n, sps, 1, 1e-3, 1.0, 0.0, 1, None, None)     # noqa: E731
        elif name == "sweep":
            run = lambda n: L.nsk_gibbs_sweeps(h, n, 1, 1)      # noqa: E731
        else:
            run = lambda n: L.nsk_gibbs_sweeps(h, n, 1, 0)      # noqa: E731
        _lib.check(run(4))
        if name.startswith("trace"):
            _lib.check(L.nsk_trace_clear(h))
        _lib.check(L.nsk_synchronize(h))
        _lib.check(L.nsk_profile_begin(h))
        _lib.check(run(steps))
        _lib.check(L.nsk_profile_mark(h))
        _lib.check(L.nsk_profile_read(h, C.byref(ms), C.byref(nl)))
        print(json.dumps({"us": ms.value * 1e3 / steps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=["10m", "lr5m"], default="10m")
    ap.add_argument("--chains", type=int, default=1)
    ap.add_argument("--lib-a", help="the parent commit's libnumbskull_amd.so")
    ap.add_argument("--lib-b", default=os.path.join(REPO, "numbskull_amd", "libnumbskull_amd.so"))
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--trace", action="store_true", help="one call of --steps steps and nothing else (for a kernel trace)")
    a = ap.parse_args()
    if a.worker or a.trace:
        return worker(a.graph, a.chains, a.steps, a.trace)
    if not a.lib_a:
        ap.error("--lib-a: the parent commit's library is needed")
    procs, hello = {}, {}
    for tag, lib in (("parent", a.lib_a), ("this", a.lib_b)):
        env = dict(os.environ, NSK_LIB=os.path.abspath(lib))
        procs[tag] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--graph", a.graph, "--chains", str(a.chains),
                                       "--steps", str(a.steps)], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
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

    out = {"graph": a.graph, "chains": a.chains, "steps_per_block": a.steps, "shape": hello["this"], "blocks": {}}
    for name, both in CONFIGS:
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
    sweep_in_step = med["this/pcd2"] - med["this/pcd1"]
    rest = med["this/pcd1"] - sweep_in_step
    ws = {t: med[t + "/trace_ws"] - med[t + "/trace"] for t in ("parent", "this")}
    out["split_us"] = {"step": round(med["this/pcd1"], 3), "sweep_in_step": round(sweep_in_step, 3), "refresh_moments_update": round(rest, 3),
                       "parent_sweep": round(med["parent/sweep"], 3), "this_sweep": round(med["this/sweep"], 3),
                       "parent_ws_device": round(ws["parent"], 3), "this_ws_device": round(ws["this"], 3),
                       "rest_over_parent_ws": round(rest / ws["parent"], 3) if ws["parent"] > 0 else None,
                       "sweeps_per_step_that_equal_the_rest": round(rest / sweep_in_step, 1) if sweep_in_step > 0 else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
