"""nsk_graph_info.device_bytes is what the handle holds NOW: every array the library frees before the handle is
destroyed leaves the count by exactly what it entered it with (numbskull_amd/csrc/nsk_alloc.h), so a round trip through
another chain count, a repeated nsk_pf_setup, nsk_p2p_setup or nsk_exchange_setup, or every optional diagnostic
switched on and off again ends at the reading it started from -- and none of it changes a result bit."""

import ctypes as C

import numpy as np
import pytest

from numbskull_amd import _lib, graphgen
from test_log_potential_gpu import _bits
from util import session

pytestmark = pytest.mark.gpu

SEED = 77
CAP, CHAINS = 4, 2
WIDS = np.array([1, 0], np.int64)
_CACHE = {}


def _grid():
    return graphgen.ising_grid(8, 8, weight=0.2, two_weights=True)


def _bytes(fg):
    return fg.info()["device_bytes"]


def _nid(fg):
    nid = C.c_int64()
    _lib.check(_lib.lib().nsk_graph_get_layout(fg._engine(), None, C.byref(nid)))
    return nid.value


def _set_chains(fg, n):
    _lib.check(_lib.lib().nsk_set_chains(fg._engine(), n))
    return _bytes(fg)


def test_chains_round_trip():
    _, fg = session(_grid(), seed=SEED)
    a = _set_chains(fg, 2)
    three = _set_chains(fg, 3)
    back = _set_chains(fg, 2)
    print("2 chains %d, 3 chains %d, 2 chains again %d" % (a, three, back))
    assert back == a
    assert three >= a + _nid(fg) * fg.info()["value_bytes"]         # at least one more chain's values
    _, one = session(_grid(), seed=SEED)
    _set_chains(one, 2)
    b = _set_chains(one, 1)
    _set_chains(one, 2)
    again = _set_chains(one, 1)
    print("1 -> 2 -> 1: %d, -> 2 -> 1: %d" % (b, again))
    assert again == b


def test_partial_factors_twice():
    """the description of the first shard of test_partial_factors_gpu's voter graph that computes aggregates for its
    readers, handed to nsk_pf_setup as PartitionedSampler.p2p_setup hands it over"""
    from test_partial_factors_gpu import build
    L = _lib.lib()
    g = graphgen.voter_graph(2000, width=12, seed=3)
    parts, _ = build(g, len(g[1]), True, 5, False)
    try:
        p = next(q for q in parts if q.pf_out)
        ops = np.asarray([op for op, _ in p.pf_out], np.uint8)
        moff = np.zeros(len(p.pf_out) + 1, np.int64)
        np.cumsum([len(m) for _, m in p.pf_out], out=moff[1:])
        mem = np.ascontiguousarray(p._local(np.concatenate([m for _, m in p.pf_out])), np.int32)
        args = (p.h, len(ops), _lib.ptr(ops), _lib.ptr(moff), _lib.ptr(mem))
        _lib.check(L.nsk_pf_setup(*args))
        first = _bytes(p.fg)
        _lib.check(L.nsk_pf_setup(*args))
        second = _bytes(p.fg)
        print("%d aggregates over %d members: %d, again %d" % (len(ops), len(mem), first, second))
        assert second == first
    finally:
        for q in parts:
            q.fg.close()


def _two_shards():
    """ising_grid(16, 16) in two range shards on one device, as test_hip_parity's peer-to-peer timeout test builds them"""
    import torch
    import numbskull_amd
    from numbskull_amd.distributed import PartitionedSampler, shard_range
    g = graphgen.ising_grid(16, 16, weight=0.2)
    parts = []
    for r in range(2):
        ns = numbskull_amd.NumbSkull(quiet=True, seed=3)
        ns.loadFactorGraph(*[x.copy() if isinstance(x, np.ndarray) else x for x in g[:5]], int(g[5]),
                           own_range=shard_range(r, 2, 256))
        with torch.cuda.stream(torch.cuda.Stream()):
            ps = PartitionedSampler(ns.factorGraphs[0], None, torch, r, 1, nvar_global=256)
        ps.world = 2
        parts.append(ps)
    needs = [p.global_needs() for p in parts]
    for p in parts:
        p.all_needs = needs
    return parts


def _wire(parts):
    """nsk_p2p_setup / nsk_p2p_export on every shard, then nsk_p2p_import_local: the readings afterwards"""
    L = _lib.lib()
    bases = (C.c_void_p * 2)()
    for p in parts:
        _lib.check(p.p2p_setup())
        b = C.c_void_p()
        _lib.check(L.nsk_p2p_export(p.h, None, C.byref(b)))
        bases[p.rank] = b.value
    for p in parts:
        _lib.check(L.nsk_p2p_import_local(p.h, bases))
        p.p2p = True
    return [_bytes(p.fg) for p in parts]


def _swept(parts):
    """4 nsk_gibbs_sweeps_p2p sweeps, one per call and breadth-first over the shards (test_config5_shards_gpu.run_case: no
    rank waits for a peer whose sweep is not issued); values by variable id and tallies of every shard"""
    L = _lib.lib()
    for _ in range(4):
        for p in parts:
            _lib.check(L.nsk_gibbs_sweeps_p2p(p.h, 1, 1, 0))
    for p in parts:
        p.check()
    out = []
    for p in parts:
        p.fg._pull(0, 0)
        out.append((p.val.cpu().numpy().copy(), p.fg.count.copy()))
    return out


def test_p2p_setup_twice(monkeypatch):
    """A repeated nsk_p2p_setup frees the lists it replaces, keeps the fused plan and changes no result bit.  (Before
    set-ups freed what they replace the first one's lists stayed until the handle was destroyed: 28291 bytes per shard
    after the first set-up, 28419 after the second -- two lists of 16 internal ids.)"""
    monkeypatch.setenv("NSK_P2P_TIMEOUT_S", "5")            # (a peer that never arrives fails the test in 5 s, not 30)
    twice, once = _two_shards(), _two_shards()
    try:
        first = _wire(twice)
        second = _wire(twice)
        print("device_bytes per shard: first set-up %s, second %s" % (first, second))
        assert second == first
        _wire(once)
        fused = [p.fg.info()["p2p_fused"] for p in twice]
        print("p2p_fused", fused)
        assert fused == [p.fg.info()["p2p_fused"] for p in once]
        for (va, ca), (vb, cb) in zip(_swept(twice), _swept(once)):
            assert va.dtype == vb.dtype and np.array_equal(va, vb)
            assert np.array_equal(ca, cb) and ca.sum() > 0
        assert [_bytes(p.fg) for p in twice] == [_bytes(p.fg) for p in once]
    finally:
        for p in twice + once:
            p.fg.close()


def test_exchange_setup_twice():
    """... and so does a repeated nsk_exchange_setup: seven arrays replaced, the staging buffers re-wrapped by
    install_boundaries.  (Before: 26259 bytes after the first set-up, 26675 after the second.)"""
    from numbskull_amd.distributed import plan_boundaries
    L = _lib.lib()
    parts = _two_shards()
    try:
        p = parts[0]
        lists, slot = plan_boundaries(p.all_needs, 2, 256)
        p.install_boundaries(lists, slot)
        first = _bytes(p.fg)
        p.install_boundaries(lists, slot)
        second = _bytes(p.fg)
        print("slot %d: first set-up %d, second %d" % (slot, first, second))
        assert slot > 0 and second == first
        ptr, nb = C.c_void_p(), C.c_int64()
        _lib.check(L.nsk_device_buffer(p.h, _lib.BUF_RECV, C.byref(ptr), C.byref(nb)))
        assert ptr.value and nb.value == slot * 2 * p.fg.info()["value_bytes"]
        _lib.check(L.nsk_exchange_pack(p.h, _lib.BUF_VALUE))
        _lib.check(L.nsk_exchange_unpack(p.h, _lib.BUF_VALUE))
        _lib.check(L.nsk_synchronize(p.h))
    finally:
        for q in parts:
            q.fg.close()


def _everything_on_then_off():
    """two rounds of: every optional diagnostic on, 4 sweeps, the trace torn down -- the readings and what was downloaded"""
    if _CACHE:
        return _CACHE
    L = _lib.lib()
    _, fg = session(_grid(), seed=SEED, chains=CHAINS)
    h = fg._engine()
    fg._chains()
    nw = len(fg.weight)
    rounds = []
    for _ in range(2):
        r = {"base": _bytes(fg)}
        out = np.zeros(CHAINS * nw)
        assert L.nsk_log_potential(h, _lib.BUF_VALUE, 0, CHAINS, _lib.ptr(out)) == _lib.OK
        assert L.nsk_weight_stats(h, _lib.BUF_VALUE, 0, CHAINS, 1, _lib.ptr(out)) == _lib.OK
        assert L.nsk_trace_setup(h, None, 0, 1, CAP) == _lib.OK
        assert L.nsk_trace_log_potential(h, 1) == _lib.OK
        r["before_ws"] = _bytes(fg)
        assert L.nsk_trace_weight_stats(h, _lib.ptr(WIDS), len(WIDS), 0) == _lib.OK
        assert L.nsk_gibbs_sweeps(h, CAP, 0, 0) == _lib.OK
        r["with_all"] = _bytes(fg)
        packed = C.c_int64(-1)
        assert L.nsk_trace_rows(h, None, None, C.byref(packed)) == _lib.OK
        r["packed"] = packed.value
        r["lp"], r["ws"] = np.zeros((CAP, CHAINS)), np.zeros((CAP, CHAINS, len(WIDS)))
        assert L.nsk_trace_download_log_potential(h, 0, CAP, _lib.ptr(r["lp"])) == _lib.OK
        assert L.nsk_trace_download_weight_stats(h, 0, CAP, _lib.ptr(r["ws"])) == _lib.OK
        assert L.nsk_trace_setup(h, None, 0, 1, 0) == _lib.OK
        r["end"] = _bytes(fg)
        rounds.append(r)
    _CACHE.update(rounds=rounds, nid=_nid(fg), vbytes=fg.info()["value_bytes"], nw=nw)
    return _CACHE


def test_everything_optional_on_then_off():
    c = _everything_on_then_off()
    first, second = c["rounds"]
    for r in c["rounds"]:
        print({k: v for k, v in r.items() if k not in ("lp", "ws")})
    # an 8 x 8 grid of binary variables: bit-packed rows, ceil(nid / 64) words a chain
    assert first["packed"] == 1
    row_bytes = (c["nid"] + 63) // 64 * 8
    column = CAP * CHAINS * len(WIDS) * 8
    plan = first["with_all"] - first["before_ws"] - column
    assert plan >= 0
    share = CAP * CHAINS * row_bytes + CAP * CHAINS * 8 + column + plan
    assert first["end"] == first["with_all"] - share
    assert first["end"] > first["base"]                 # the records and lists the queries uploaded stay
    assert second["base"] == first["end"] and second["end"] == first["end"]
    assert second["with_all"] == first["with_all"]


def test_results_unaffected():
    """the last recorded row of each round above against a fresh handle that ran the same sweeps and asked once: the
    first round's on arrays allocated once, the second round's on a trace and columns rebuilt after the teardown"""
    L = _lib.lib()
    c = _everything_on_then_off()
    _, fg = session(_grid(), seed=SEED, chains=CHAINS)
    h = fg._engine()
    fg._chains()
    for r in c["rounds"]:
        assert L.nsk_gibbs_sweeps(h, CAP, 0, 0) == _lib.OK
        lp, ws = np.zeros(CHAINS), np.zeros((CHAINS, c["nw"]))
        assert L.nsk_log_potential(h, _lib.BUF_VALUE, 0, CHAINS, _lib.ptr(lp)) == _lib.OK
        assert L.nsk_weight_stats(h, _lib.BUF_VALUE, 0, CHAINS, 0, _lib.ptr(ws)) == _lib.OK
        assert np.array_equal(_bits(r["lp"][CAP - 1]), _bits(lp))
        assert np.array_equal(_bits(r["ws"][CAP - 1]), _bits(ws[:, WIDS]))
