"""Throughput of several chains in one handle against one-chain handles run one after another (nsk_set_chains).

    python tools/chains_bench.py [--rows 1000] [--cols 1000] [--chains 8] [--sweeps 400]

Prints one JSON line: updates/s of R chains of the grid in ONE handle (one nsk_gibbs_sweeps call of --sweeps sweeps:
every class launch serves all chains) and of R one-chain handles seeded seed ^ (r << 32), one call each, one after
another.  Each figure is timed after an untimed call of the same length (a handle captures its sweep sequences on its
first call of a length); tallied sweeps, device time between synchronisations."""

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np                                      # noqa: E402
import numbskull_amd                                    # noqa: E402
from numbskull_amd import _lib, graphgen               # noqa: E402


def _graph(ns, g):
    w, v, f, fm, dm, edges = [x.copy() if isinstance(x, np.ndarray) else x for x in g]
    ns.loadFactorGraph(w, v, f, fm, dm, int(edges))
    return ns.factorGraphs[-1]


def _timed(fgs, sweeps, all_rows):
    L = _lib.lib()
    for fg in fgs:                                      # state on the device, untimed
        if all_rows:
            fg._push_chains(0)
        else:
            fg._push(0, 0)
        _lib.check(L.nsk_synchronize(fg._engine()))
    t0 = time.perf_counter()
    for fg in fgs:
        fg._sweep(sweeps, False, False)
    for fg in fgs:
        _lib.check(L.nsk_synchronize(fg._engine()))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--cols", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=8)
    ap.add_argument("--sweeps", type=int, default=400)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    g = graphgen.ising_grid(a.rows, a.cols, weight=0.3)
    R, n = a.chains, a.rows * a.cols

    ns = numbskull_amd.NumbSkull(quiet=True, seed=a.seed, chains=R)
    fg = _graph(ns, g)
    fg.inference(3, 0, False, var_copy="all")
    fg._chains()
    _timed([fg], a.sweeps, True)                         # capture + warm
    t_batched = _timed([fg], a.sweeps, True)

    singles = []
    for r in range(R):
        nsr = numbskull_amd.NumbSkull(quiet=True, seed=a.seed ^ (r << 32))
        singles.append(_graph(nsr, g))
        singles[-1].inference(3, 0, False)
    _timed(singles, a.sweeps, False)
    t_seq = _timed(singles, a.sweeps, False)

    upd = float(n) * R * a.sweeps
    print(json.dumps({"graph": "ising_%dx%d" % (a.rows, a.cols), "chains": R, "sweeps": a.sweeps,
                      "batched_updates_per_s": upd / t_batched, "sequential_updates_per_s": upd / t_seq,
                      "batched_s": t_batched, "sequential_s": t_seq, "speedup": t_seq / t_batched}))


if __name__ == "__main__":
    main()
