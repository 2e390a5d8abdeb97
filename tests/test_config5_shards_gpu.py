"""BASELINE configs[4] ("config #5") as BASELINE states it -- the mixed-arity LR graph range-partitioned
into EIGHT shards, learning included -- on one device: every shard is generated alone
(graphgen.mixed_lr_shard: own variables, the ghosts they read, the factors that touch them; what the
reference's minions load, salt/src/numbskull_minion.py:185), compiled into a handle of its own, and the
eight handles exchange boundaries through the REAL peer-to-peer path -- pairwise send lists, k_p2p_push
into the peers' buffers, flags, wait/unpack, in learning both chains and the epoch's weight deltas
(nsk_gibbs_sweeps_p2p / nsk_learn_sweeps_p2p; the peers' buffers are handed over as plain pointers,
nsk_p2p_import_local, since the ranks live in one process).  Owned values, ghosts, tallies, both chains and
the merged weights must equal the oracle's emulation of the partitioned run bit for bit
(numbskull_master.py:165-224 semantics: ghost values are one sweep old; w = w_start + sum of deltas,
:223-224).  The same harness runs the 10M grid of config #4 through the peer-to-peer path.

Per-shard phase timings (HIP events) go to gpurun_out/config5_shards_*.json (profiles/r4_*)."""
import ctypes as C
import json
import os

import numpy as np
import psutil
import pytest

from numbskull_amd import _lib, graphgen
from util import oracle_of, phases_from_colors
import numbskull_amd

pytestmark = pytest.mark.gpu
WORLD = 8
LR_SEED = 20240603


def make_parts(kind, nvar, learn, seed, weight=0.1):
    """One handle + PartitionedSampler per shard, every one on a stream of its own.  ``weight``: the inference grid's
    one weight."""
    import torch
    from numbskull_amd.distributed import PartitionedSampler, shard_range
    parts, streams = [], []
    grid = None
    if kind == "perturbed_grid":
        # tests/perturbed.py shard_grid: a grid whose swaps make tiles far from the cuts read ghosts, or give one
        # boundary value readers in two shards; nvar = (rows, cols, variant)
        from perturbed import shard_grid
        rows, cols, variant = nvar
        nvar = rows * cols
        grid = shard_grid(rows, cols, variant, learn, np.random.Generator(np.random.PCG64(20240602)))
        kind = "grid"
    elif kind in ("grid", "shuffled_grid"):
        rng = np.random.Generator(np.random.PCG64(20240602))
        rows, cols = nvar
        nvar = rows * cols
        grid = (graphgen.ising_grid(rows, cols, weight=0.0, fixed=False, two_weights=True,
                                    evidence=rng.integers(0, 2, nvar)) if learn
                else graphgen.ising_grid(rows, cols, weight=weight))
        if kind == "shuffled_grid":
            # the grid under randomly permuted variable ids (a loader that numbers variables in arrival order), then
            # repartitioned: numbskull_amd.partition puts a graph-aware variable order in front of the range partition
            # (the reference's find_connected_components / find_metis_parts, salt/src/messages.py:542-670)
            from numbskull_amd import partition
            grid = partition.relabel(grid, rng.permutation(nvar))
            lost = partition.comm_volume(nvar, grid[2], grid[3], WORLD)
            _, order = partition.find_parts(nvar, grid[2], grid[3], WORLD)
            found = partition.comm_volume(nvar, grid[2], grid[3], WORLD, order)
            assert found < lost / 20, (lost, found)
            grid = partition.relabel(grid, order)
            kind = "grid"
    if kind == "shuffled_lr":
        # config #5's generator at a size the emulation walks in seconds, its ids shuffled, then handed to the multilevel
        # partitioner (find_metis_parts, messages.py:593-670: objective communication volume)
        from numbskull_amd import partition
        whole = graphgen.mixed_lr_graph(nvar, seed=LR_SEED)
        native = partition.comm_volume(nvar, whole[2], whole[3], WORLD)
        grid = partition.relabel(whole, np.random.default_rng(LR_SEED).permutation(nvar))
        lost = partition.comm_volume(nvar, grid[2], grid[3], WORLD)
        _, order = partition.find_parts(nvar, grid[2], grid[3], WORLD, method="multilevel")
        found = partition.comm_volume(nvar, grid[2], grid[3], WORLD, order)
        assert found <= 1.1 * native and found < lost / 8, (native, lost, found)
        grid = partition.relabel(grid, order)
    shards = None
    if grid is None:      # all eight in one pass over the generator's blocks (a rank of a real run calls
        shards = graphgen.mixed_lr_shards(nvar, [shard_range(r, WORLD, nvar) for r in range(WORLD)],      # mixed_lr_shard)
                                          seed=LR_SEED)
    for r in range(WORLD):
        lo, hi = shard_range(r, WORLD, nvar)
        if grid is not None:
            sg, gids, own = graphgen.extract_shard(grid, lo, hi)
        else:
            sg, gids, own = shards[r]
            shards[r] = None
        ns = numbskull_amd.NumbSkull(quiet=True, seed=seed, head_by_vid=kind in ("lr", "shuffled_lr"))
        ns.loadFactorGraph(*sg[:5], int(sg[5]), own_range=own, global_ids=gids)
        fg = ns.factorGraphs[0]
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            ps = PartitionedSampler(fg, None, torch, r, 1, nvar_global=nvar)
        ps.world = WORLD
        assert fg.info()["nowned"] == hi - lo
        parts.append(ps)
        streams.append(st)
    return parts, streams, nvar


def wire_p2p(parts):
    """What PartitionedSampler._init_p2p does across processes, for handles that share one."""
    L = _lib.lib()
    needs = [p.global_needs() for p in parts]
    bases = (C.c_void_p * WORLD)()
    for p in parts:
        p.all_needs = needs
        _lib.check(p.p2p_setup())
        b = C.c_void_p()
        _lib.check(L.nsk_p2p_export(p.h, None, C.byref(b)))
        bases[p.rank] = b.value
    for p in parts:
        _lib.check(L.nsk_p2p_import_local(p.h, bases))
        p.p2p = True
    # the set-up self-test of PartitionedSampler._init_p2p (pattern payload, compared on the receiving side),
    # breadth-first like the exchanges below, one round per buffer parity
    for _ in range(2):
        for part in (1, 2, 3):
            for p in parts:
                _lib.check(L.nsk_p2p_selftest(p.h, 1, part))
    for p in parts:
        p.check()
    # ... and the fused exchange's own protocol (system-coherent loads / stores, no fences) where the shards qualify
    if all(p.fg.info()["p2p_fused"] for p in parts):
        for _ in range(2):
            for part in (1, 2):
                for p in parts:
                    _lib.check(L.nsk_p2p_selftest(p.h, 2, part))
        for p in parts:
            p.check()
    return needs


def run_case(kind, size, learn, tag, nsweeps=3, hyper=(1e-3, 0.95, 2, 0.01, 1), fused=False, probe=None, weight=0.1):
    """``probe(parts, needs)``: called once the shards are wired (what a test asserts about their exchange plans)."""
    import torch
    from numbskull_amd.distributed import shard_range, plan_pairs
    seed = 20240601
    parts, streams, nvar = make_parts(kind, size, learn, seed, weight)
    hbv = kind not in ("grid", "shuffled_grid", "perturbed_grid")
    oracles = []
    for p in parts:
        og = oracle_of(p.fg, head_by_vid=hbv)           # checks the layout and the colouring of every shard
        oracles.append((og, phases_from_colors(p.fg.colors()), og.initial_state()))
    needs = wire_p2p(parts)
    if probe is not None:
        probe(parts, needs)
    pairs = plan_pairs(needs, WORLD, nvar)
    L = _lib.lib()
    # what nsk_gibbs_sweeps_p2p / nsk_learn_sweeps_p2p enqueue per sweep -- the sweep's kernels, the pushes
    # (nsk_p2p_exchange part 1), then flags-wait + unpack (+ weight merge; part 2) -- issued breadth-first
    # over the eight handles: they share one process, hence a few hardware queues, and a rank's spinning
    # wait kernel must not sit in front of a peer's push in the same queue (ranks of a real run are
    # processes with queues of their own: tests/test_multirank_gpu.py runs those loops as they are)
    step, decay = hyper[0], hyper[1]
    st = step
    if fused:
        # the shard's own loop, nsk_gibbs_sweeps_p2p: a shard that lives in table segments exchanges its boundary
        # INSIDE its class launches (border tiles read the receive block and write into the readers'; no exchange
        # kernels).  One sweep per call, breadth-first: a call right behind a fused call continues it
        assert not learn and all(p.fg.info()["p2p_fused"] == 1 for p in parts), "the shards do not qualify for the fused exchange"
        for s in range(nsweeps):
            for p in parts:
                _lib.check(L.nsk_gibbs_sweeps_p2p(p.h, 1, 1, 0))
    for s in range(0 if fused else nsweeps):
        for p in parts:
            if learn:
                _lib.check(L.nsk_learn_sweeps(p.h, 1, st, 1.0, hyper[2], hyper[3], hyper[4], 0))
            else:
                _lib.check(L.nsk_gibbs_sweeps(p.h, 1, 1, 0))
            _lib.check(L.nsk_p2p_exchange(p.h, int(learn), 1))
        for part in (2, 3):                     # (3: the closing half of the weight merge; nothing in inference)
            for p in parts:
                _lib.check(L.nsk_p2p_exchange(p.h, int(learn), part))
        st *= decay
    for p in parts:
        p.check()
    torch.cuda.synchronize()

    def loc(r, ids):
        at = np.searchsorted(parts[r].gids, ids)
        assert np.array_equal(parts[r].gids[at], ids)
        return at

    for s in range(nsweeps):
        starts = [st[2].copy() for _, _, st in oracles]
        for og, (order, ps_), (vv, ve, wv, cnt) in oracles:
            if learn:
                assert og.learn_call(order, ps_, vv, ve, wv, 1, step, 1.0, hyper[2], hyper[3], hyper[4], False, seed, s) == 0
            else:
                assert og.gibbs_dev(order, ps_, vv, wv, cnt, seed, s, True) == 0
        step *= decay
        for r in range(WORLD):                   # owners publish what each peer reads of them
            for q in range(WORLD):
                if q != r and len(pairs[r][q]):
                    b = pairs[r][q]
                    oracles[q][2][0][loc(q, b)] = oracles[r][2][0][loc(r, b)]
                    oracles[q][2][1][loc(q, b)] = oracles[r][2][1][loc(r, b)]
        if learn:                                # w = w_start + (d_0 + d_1 + ...), numbskull_master.py:223-224
            total = sum(st[2] - s0 for (_, _, st), s0 in zip(oracles, starts))
            for (_, _, st), s0 in zip(oracles, starts):
                st[2][:] = s0 + total
    nghost = 0
    for r, p in enumerate(parts):
        vv, ve, wv, cnt = oracles[r][2]
        lo, hi = p.fg.own_range
        got = p.val.cpu().numpy().astype(np.int64)
        assert np.array_equal(got[lo:hi], vv[lo:hi]), ("owned values differ", r)
        gh = loc(r, np.asarray(needs[r], np.int64))
        nghost += len(gh)
        assert np.array_equal(got[gh], vv[gh]), ("ghost values differ", r)
        if learn:
            gote = p.val_evid.cpu().numpy().astype(np.int64)
            assert np.array_equal(gote[lo:hi], ve[lo:hi]), ("evidence-chain values differ", r)
            assert np.array_equal(gote[gh], ve[gh]), ("evidence-chain ghosts differ", r)
            assert np.array_equal(p.w.cpu().numpy(), wv), ("merged weights differ", r)
        else:
            p.fg._pull(0, 0)
            cs = p.fg.cstart
            assert np.array_equal(p.fg.count[cs[lo]:cs[hi]], cnt[cs[lo]:cs[hi]]), ("tallies differ", r)
    if learn:
        w0 = parts[0].w.cpu().numpy()
        assert all(np.array_equal(p.w.cpu().numpy(), w0) for p in parts), "ranks disagree on the merged weights"
        assert np.isfinite(w0).all() and np.abs(w0).max() > 0

    # phase timings per shard: the sweep kernels alone, then all pushes, then all flag/wait/unpack
    # (+ weight merge) kernels -- each rank's bracket on its own stream, marked first, read afterwards
    # (inference has no closing weight gather: its part 3 enqueues nothing, and the bracket around nothing is what every
    # other figure carries on top of its kernels -- recorded as such, not counted into the exchange)
    last = "gather_w_us" if learn else "empty_bracket_us"
    timing = {"sweep_us": [], "push_us": [], "wait_unpack_us": [], last: []}
    if fused:
        # a fused sweep is its class launches and nothing else: timed per shard over consecutive one-sweep calls
        ms, nl = C.c_double(), C.c_int64()
        for rep in range(6):
            row = []
            for p in parts:
                _lib.check(L.nsk_profile_begin(p.h))
                _lib.check(L.nsk_gibbs_sweeps_p2p(p.h, 1, 1, 1))
                _lib.check(L.nsk_profile_mark(p.h))
            for p in parts:
                _lib.check(L.nsk_profile_read(p.h, C.byref(ms), C.byref(nl)))
                row.append(ms.value * 1e3)
            timing["sweep_us"].append(row)
        for p in parts:
            p.check()
        out = {"config": "%s in 8 range shards, all on one MI355X, inference, boundary exchange fused into the class launches" % tag,
               "per_shard_us": {"sweep_incl_exchange_us": {"mean": float(np.mean(timing["sweep_us"][1:])), "max": float(np.max(timing["sweep_us"][1:]))}},
               "launches_per_sweep": int(nl.value),
               "note": "one shard's class launches (HIP events on the shard's stream, one launch latency included); border tiles "
                       "push into the readers' receive blocks and raise the flags themselves, the next sweep's border tiles wait"}
        os.makedirs("gpurun_out", exist_ok=True)
        with open("gpurun_out/config5_shards_%s_inference_fused.json" % tag.split()[0], "w") as f:
            json.dump(out, f, indent=1)
        for p in parts:
            p.fg.close()
        return out
    ms, nl = C.c_double(), C.c_int64()
    for _ in range(3):
        row = []
        for p in parts:
            _lib.check(L.nsk_profile_begin(p.h))
            if learn:
                _lib.check(L.nsk_learn_sweeps(p.h, 1, 1e-4, 1.0, hyper[2], hyper[3], hyper[4], 0))
            else:
                _lib.check(L.nsk_gibbs_sweeps(p.h, 1, 1, 1))
            _lib.check(L.nsk_profile_end(p.h, C.byref(ms), C.byref(nl)))
            row.append(ms.value * 1e3)
        timing["sweep_us"].append(row)
        for part, key in ((1, "push_us"), (2, "wait_unpack_us"), (3, last)):
            for p in parts:
                _lib.check(L.nsk_profile_begin(p.h))
                _lib.check(L.nsk_p2p_exchange(p.h, int(learn), part))
                _lib.check(L.nsk_profile_mark(p.h))
            row = []
            for p in parts:
                _lib.check(L.nsk_profile_read(p.h, C.byref(ms), C.byref(nl)))
                row.append(ms.value * 1e3)
            timing[key].append(row)
    for p in parts:
        p.check()
    sends = [int(sum(len(pairs[r][q]) for q in range(WORLD))) for r in range(WORLD)]
    owned = [p.fg.own_range[1] - p.fg.own_range[0] for p in parts]
    out = {"config": "%s in 8 range shards, all on one MI355X, %s, peer-to-peer exchange" % (tag, "learning" if learn else "inference"),
           "owned_per_rank": owned, "values_sent_per_rank": sends, "ghosts_per_rank": [len(n) for n in needs],
           "exchange_fraction": float(np.mean([np.mean(a) + np.mean(b) + (np.mean(c) if learn else 0.0) for a, b, c in
                                               zip(timing["push_us"][1:], timing["wait_unpack_us"][1:], timing[last][1:])])
                                      / np.mean([np.mean(a) for a in timing["sweep_us"][1:]])),
           "per_shard_us": {k: {"mean": float(np.mean(v[1:])), "max": float(np.max(v[1:]))} for k, v in timing.items()},
           "note": "one shard's kernels alone on the device (HIP events on the shard's stream); the push / wait brackets of "
                   "the eight shards overlap on the device; first repetition excluded"}
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/config5_shards_%s_%s.json" % (tag.split()[0], "learn" if learn else "inference"), "w") as f:
        json.dump(out, f, indent=1)
    for p in parts:
        p.fg.close()
    return out


@pytest.mark.parametrize("learn", [False, True])
def test_lr5m_eight_shards_p2p_match_emulation(learn):
    out = run_case("lr", 5_000_000, learn, "lr5m (5M-variable LR graph)")
    assert sum(out["ghosts_per_rank"]) > 0


@pytest.mark.parametrize("learn", [False, True])
def test_grid10m_eight_shards_p2p_match_emulation(learn):
    run_case("grid", (2500, 4000), learn, "ising10m (2500x4000 grid)", hyper=(1e-7, 0.95, 2, 0.01, 1))


def test_grid10m_eight_shards_fused_exchange_matches_emulation():
    """Config #4 through the shards' own loop: the boundary exchange rides in the table launches."""
    out = run_case("grid", (2500, 4000), False, "ising10m (2500x4000 grid)", nsweeps=5, fused=True)
    # one launch per colour class and nothing else (the grid's last shard holds the bottom row and the corners: more
    # segment entries than one launch carries, so one of its classes takes two)
    assert 2 <= out["launches_per_sweep"] <= 3, out


def test_shuffled_grid_repartitioned_eight_shards_match_emulation():
    """f4: a 1000x1000 grid whose variable ids arrive shuffled (the range partition then reads 88 % of all variables
    across the cuts) is given a graph-aware variable order (numbskull_amd.partition, "auto": here the breadth-first
    walk), cut by the reference's shard formula and sampled in 8 shards through the peer-to-peer exchange: bit-exact
    against the partitioned oracle emulation like any other graph."""
    out = run_case("shuffled_grid", (1000, 1000), False, "shuffled1m (1000x1000 grid, shuffled ids, repartitioned)", nsweeps=4)
    assert sum(out["ghosts_per_rank"]) < 40000, out["ghosts_per_rank"]          # (880 000 under the shuffled ids)


@pytest.mark.parametrize("learn", [False, True])
def test_shuffled_lr_graph_partitioned_eight_shards_match_emulation(learn):
    """f4 on the graph it is for: a 400 000-variable config-#5 graph whose ids arrive shuffled goes through the
    multilevel partitioner (communication volume within 10 % of the ids the generator was built on), is cut by the
    reference's shard formula and sampled / learned in 8 shards through the peer-to-peer exchange: bit-exact against
    the partitioned oracle emulation."""
    out = run_case("shuffled_lr", 400_000, learn, "shuffledlr400k (400k-variable LR graph, shuffled ids, multilevel partition)", nsweeps=3)
    assert sum(out["ghosts_per_rank"]) > 0


def test_lr50m_eight_shards_learning_p2p():
    """Config #5 at its stated size, 8-way: one learning epoch after one inference sweep per shard."""
    if psutil.virtual_memory().available < 110 * 2 ** 30:
        pytest.fail("config #5 at its stated size needs ~110 GB of free host memory: this box cannot exercise it")
    run_case("lr", 50_000_000, True, "lr50m (50M-variable LR graph)", nsweeps=2)
