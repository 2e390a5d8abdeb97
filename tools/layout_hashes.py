#!/usr/bin/env python3
"""Hashes of the compiled layouts of a fixed corpus of graphs (host-only: nsk_graph_plan with NSK_LAYOUT_HASH=1, which
hashes every member of the compiled layout).  Run before and after a change to the graph compiler that must not move
anything: the two outputs are equal.

The corpus: eight mid-sized graphs; each of them again under NSK_DIAG=1 with every layout-changing switch set alone
(the grids with NSK_WIDE_MIN=0, so that the wide-quad builder runs at their size); the perturbed grids of
tests/perturbed.py as their CPU test plans them; the small graphs of tests/test_hip_parity.py.  Per plan: every field
of nsk_graph_info, a digest of the colours and a digest of the ghost list (nsk_graph_plan_needs).  Everything twice,
with NSK_COMPILE_THREADS=1 and =8 (the thread count is read once per process: two worker processes)."""
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one value per layout-changing switch of the compiler (CompileKnobs, nsk_compile_ctx.h)
SWITCHES = [("NSK_NO_DIRECT", "1"), ("NSK_NO_WORDER", "1"), ("NSK_NO_PACKED", "1"), ("NSK_NO_RECOLOUR", "1"),
            ("NSK_RECOLOUR_PASSES", "2"), ("NSK_NO_BALANCE", "1"), ("NSK_NO_KSTAT", "1"), ("NSK_NO_EP_WIN", "1"),
            ("NSK_NO_AFFINE", "1"), ("NSK_WIDE_MIN", "0"), ("NSK_NO_WIDE", "1"), ("NSK_NO_RUN_PAD", "1"),
            ("NSK_NO_HUB_EP", "1"), ("NSK_NO_LEARN_SEG", "1"), ("NSK_GEN_BLOCK", "4096"), ("NSK_EP_BLOCK", "256"),
            ("NSK_NO_PAD_SHAPE", "1"), ("NSK_NO_SHAPE", "1"), ("NSK_SHAPE_PARTS", "4"), ("NSK_NO_HEAVY", "1"),
            ("NSK_NO_EP", "1"), ("NSK_NO_ZTAB", "1"), ("NSK_NO_FAST", "1"), ("NSK_NO_GENERAL", "1"),
            ("NSK_GEN_MAX_ENTRIES", "8"), ("NSK_NO_WORD_CACHE", "1"), ("NSK_SHAPE_MAX_WORDS", "24")]


def worker():
    os.environ["NSK_LAYOUT_HASH"] = "1"
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import numpy as np
    import numbskull_amd
    from numbskull_amd import graphgen

    def load(g, own=None, **kw):
        ns = numbskull_amd.NumbSkull(quiet=True, **kw)
        extra = {} if own is None else {"own_range": own}
        ns.loadFactorGraph(*[x.copy() if isinstance(x, np.ndarray) else x for x in g[:5]], int(g[5]), **extra)
        return ns.factorGraphs[0]

    def plan(fg, env=None):
        saved = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            color, info = fg.plan()
            needs = fg.ghost_needs(host_only=True)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k)
                else:
                    os.environ[k] = v
        out = {k: (float(v) if isinstance(v, float) else int(v)) for k, v in info.items()}
        out["colors_sha"] = hashlib.sha256(np.ascontiguousarray(color).tobytes()).hexdigest()[:16]
        out["needs"] = [len(needs), hashlib.sha256(np.ascontiguousarray(needs).tobytes()).hexdigest()[:16]]
        return out

    out = {}
    graphs = {}
    bw = graphgen.boolean_weighted_graph(120000, seed=9)
    graphs["boolw_fixed"] = load(bw)
    bw[0]["isFixed"] = False
    rng = np.random.Generator(np.random.PCG64(1))
    bw[1]["isEvidence"] = rng.random(len(bw[1])) < 0.5
    graphs["boolw_learn"] = load(bw)
    lr = graphgen.mixed_lr_graph(150000, seed=4, nweights=3000)
    graphs["lr"] = load(lr, head_by_vid=True)
    graphs["lr_shard"] = load(lr, own=(30000, 90000), head_by_vid=True)
    graphs["lr_bigw"] = load(graphgen.mixed_lr_graph(100000, seed=5, nweights=600000), head_by_vid=True)
    graphs["grid"] = load(graphgen.ising_grid(300, 400, weight=0.1))
    ev = rng.integers(0, 2, 120000)
    graphs["grid_learn"] = load(graphgen.ising_grid(300, 400, weight=0.0, fixed=False, two_weights=True, evidence=ev))
    graphs["grid_shard"] = load(graphgen.ising_grid(300, 400, weight=0.1), own=(0, 60000))
    for name, fg in graphs.items():
        out[name] = plan(fg)
        for var, value in SWITCHES:
            env = {"NSK_DIAG": "1", var: value}
            if name.startswith("grid"):
                env.setdefault("NSK_WIDE_MIN", "0")
            out["%s|%s=%s" % (name, var, value)] = plan(fg, env)
    graphs.clear()

    # the perturbed grids, as tests/test_perturbed_grids_cpu.py plans them
    from perturbed import CASES, build_case
    wide = {"NSK_DIAG": "1", "NSK_WIDE_MIN": "0", "NSK_WIDE_LEARN_MIN": "0"}
    for name in sorted(CASES):
        out["perturbed|" + name] = plan(load(build_case(name)[1]), wide)

    # the small graphs of the oracle parity tests (planning needs no device)
    import test_hip_parity
    from conftest import GOLDEN
    small = test_hip_parity._small_graphs(lambda f: np.load(os.path.join(GOLDEN, f), allow_pickle=False))
    for name in sorted(small):
        g, hbv = small[name]
        out["parity|" + name] = plan(load(g, head_by_vid=hbv))
    print(json.dumps(out, sort_keys=True))


def main():
    out = {}
    for threads in ("1", "8"):
        env = dict(os.environ, NSK_COMPILE_THREADS=threads)
        for k in [k for k in env if k.startswith("NSK_") and k not in ("NSK_COMPILE_THREADS", "NSK_LIB")]:
            env.pop(k)                                  # the corpus sets its own switches
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=env, stdout=subprocess.PIPE, text=True, check=True)
        out["threads=" + threads] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out, sort_keys=True, indent=1))


if __name__ == "__main__":
    worker() if "--worker" in sys.argv else main()
