"""What parallel tempering costs (nsk_pt_sweeps) on the million-variable Ising grid with 8 chains.

    python tools/pt_cost.py steps [--repeats 7]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/pt_cost.py swap [--repeats 7]

steps: 20 steps through nsk_tempered_sweeps (one table rebuild and one batched sweep of all chains a step) and through
nsk_pt_sweeps with 1 and with 4 sweeps a step (a table rebuild and the one-chain launches for every replica, then the score,
the decision and the swaps), lp asked for, timed with HIP events on the handle's stream (nsk_profile_begin /
nsk_profile_mark / nsk_profile_read) after a warm-up, the three calls taking turns.  Prints one JSON line: the medians and
the spread (largest minus smallest repeat) in microseconds a step, and what the two sweep counts say about a replica's
share: (pt4 - pt1) / (3 chains) is one chain's sweep, the rest of pt1 / chains is what comes in front of it -- the
scale and the rebuild -- with the step's score, decision and swaps spread over the chains.

swap: the calls whose copy kernels a kernel trace is to time -- nsk_pt_sweeps of two steps under equal betas, where every
proposal is accepted (k_pt_swap: 4 pairs at the even step, 3 at the odd one, both chains' value bytes read and written),
and nsk_smc_sweeps over (0, 0.5) with threshold 0.5, where one chain outweighs the rest (k_smc_copy: the copied chains'
value bytes read and written).  Prints the bytes each launch moves; the kernel times are in the trace's statistics."""

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CHAINS, STEPS = 8, 20


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
    from numbskull_amd.diagnostics import pt_ladder
    fg, h, _lib = handle()
    L = _lib.lib()
    schedule, ladder = np.linspace(0.0, 1.0, STEPS), pt_ladder(CHAINS, 0.1)
    uniforms = np.random.RandomState(0).random_sample((STEPS, CHAINS - 1))
    lp = np.zeros((STEPS, CHAINS))
    acc = np.zeros((STEPS, CHAINS - 1), np.int32)
    ms, nl = C.c_double(), C.c_int64()

    def timed(call):
        _lib.check(L.nsk_synchronize(h))
        _lib.check(L.nsk_profile_begin(h))
        _lib.check(call())
        _lib.check(L.nsk_profile_mark(h))
        _lib.check(L.nsk_profile_read(h, C.byref(ms), C.byref(nl)))
        return ms.value * 1e3

    def tempered():
        return L.nsk_tempered_sweeps(h, _lib.ptr(schedule), STEPS, 1, 0, None, _lib.ptr(lp), None, None)

    def pt(sps):
        return lambda: L.nsk_pt_sweeps(h, _lib.ptr(ladder), STEPS, sps, 0, _lib.ptr(uniforms), -1, _lib.ptr(lp), _lib.ptr(acc))

    calls = {"tempered": tempered, "pt1": pt(1), "pt4": pt(4)}
    for _ in range(2):
        for c in calls.values():
            timed(c)
    res = {k: [] for k in calls}
    for _ in range(repeats):
        for k, c in calls.items():
            res[k].append(timed(c))
    med = {k: float(np.median(v)) / STEPS for k, v in res.items()}
    sweep = (med["pt4"] - med["pt1"]) / (3 * CHAINS)
    out = {"graph": "ising 1000 x 1000, weight 0.3", "chains": CHAINS, "steps": STEPS, "repeats": repeats,
           "us_per_call": {k: [round(x, 1) for x in v] for k, v in res.items()},
           "median_us_per_step": {k: round(v, 2) for k, v in med.items()},
           "spread_us_per_step": {k: round((max(v) - min(v)) / STEPS, 2) for k, v in res.items()},
           "pt1_over_tempered": round(med["pt1"] / med["tempered"], 2),
           "one_chain_sweep_us": round(sweep, 2),
           "rest_per_replica_us": round(med["pt1"] / CHAINS - sweep, 2),
           "accepted_of_proposed": [int((acc == 1).sum()), int((acc >= 0).sum())]}
    print(json.dumps(out))
    fg.close()


def swap(repeats):
    fg, h, _lib = handle()
    L = _lib.lib()
    info = fg.info()
    iid, nid = np.zeros(len(fg.variable), np.int32), C.c_int64()
    _lib.check(L.nsk_graph_get_layout(h, _lib.ptr(iid), C.byref(nid)))
    nbytes = nid.value * info["value_bytes"]
    equal, uniforms = np.full(CHAINS, 0.5), np.full((2, CHAINS - 1), 0.5)
    acc = np.zeros((2, CHAINS - 1), np.int32)
    betas, off = np.array([0.0, 0.5]), np.array([0.5])
    anc, flag = np.zeros((1, CHAINS), np.int32), np.zeros(1, np.int32)
    pairs, copies = [], []
    for _ in range(repeats + 2):
        _lib.check(L.nsk_pt_sweeps(h, _lib.ptr(equal), 2, 1, 0, _lib.ptr(uniforms), -1, None, _lib.ptr(acc)))
        pairs.append([int((row == 1).sum()) for row in acc])
        _lib.check(L.nsk_smc_sweeps(h, _lib.ptr(betas), 2, 1, 0, 0.5, _lib.ptr(off), None, None, None, _lib.ptr(anc), _lib.ptr(flag)))
        copies.append(int((anc[0] != np.arange(CHAINS)).sum()))
    print(json.dumps({"value_bytes_per_chain": nbytes, "k_pt_swap_pairs_per_launch": pairs,
                      "k_pt_swap_bytes_read_and_written": [[4 * p * nbytes for p in row] for row in pairs],
                      "k_smc_copy_chains_per_launch": copies,
                      "k_smc_copy_bytes_read_and_written": [2 * c * nbytes for c in copies],
                      "launches": {"k_pt_swap": 2 * (repeats + 2), "k_smc_copy": repeats + 2}}))
    fg.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["steps", "swap"])
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    (steps if a.mode == "steps" else swap)(a.repeats)
