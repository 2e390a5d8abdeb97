// nsk_exchange.hip -- the multi-GPU boundary exchange behind include/numbskull_amd.h: the collective path (NskGather:
// nsk_exchange_*, nsk_comm_*, nsk_*_sweeps_exchange), partial factors (nsk_pf_setup) and the peer-to-peer path (NskP2P:
// nsk_p2p_*, the fused-exchange plan).  The kernels are nsk_kernels_misc.h's; the fused launches nsk_gibbs.hip's.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>      // types only: the library is bound at run time with dlopen

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nsk_internal.h"
#include "nsk_kernels_misc.h"

using namespace nsk;

// RCCL entry points, bound at run time (nsk_comm_init)
struct RcclApi {
    void *lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
static RcclApi g_rccl;

// w_start / w_delta serve the weight merge of both paths: allocated by whichever set-up comes first
static int ensure_w_start(nsk_graph *g) {
    int rc;
    if (!g->w_start && (rc = dev_alloc(g, &g->w_start, (size_t)g->c.nweight))) return rc;
    return g->w_delta ? NSK_OK : dev_alloc(g, &g->w_delta, (size_t)g->c.nweight);
}

static void p2p_close_peers(nsk_graph *g) {
    for (int q = 0; q < 16; q++) {
        if (g->p2p.peer_ipc[q] && g->p2p.peer_base[q]) (void)hipIpcCloseMemHandle(g->p2p.peer_base[q]);
        g->p2p.peer_base[q] = nullptr;
        g->p2p.peer_ipc[q] = false;
    }
}

// How the entry points of the two paths open, in the order a caller meets the refusals: the handle, the path's set-up,
// one chain, no sample trace, the entry point's own argument check (bad_arg: its refusal, or null), then the device and
// the pending close of a fused sweep sequence.  The collective path's native RCCL loops (loop) need the communicator
// too and leave device and flush to the calls they make ...
static int gather_enter(nsk_graph *g, bool loop, const char *bad_arg = nullptr) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (loop && (!g->gather.comm || g->gather.world == 0)) return fail(NSK_E_INVALID, "nsk_exchange_setup / nsk_comm_init first");
    if (g->gather.world == 0) return fail(NSK_E_INVALID, "nsk_exchange_setup has not been called");
    NSK_ONE_CHAIN(g, "the exchange entry points");
    NSK_NO_TRACE(g, "the exchange entry points");
    if (bad_arg) return fail(NSK_E_INVALID, bad_arg);
    if (loop) return NSK_OK;
    HIPCHECK(hipSetDevice(g->device));
    return nsk_p2p_flush(g);
}
// ... and the peer-to-peer entry points say which of the trace check and device + flush apply to them
enum { P2P_NO_TRACE = 1, P2P_FLUSH = 2 };
static const char *bad_part(int part) { return part < 0 || part > 3 ? "bad part" : nullptr; }
static const char *bad_sweeps(int64_t n) { return n < 0 || n > INT32_MAX ? "bad sweep count" : nullptr; }
static int p2p_enter(nsk_graph *g, int checks, const char *bad_arg = nullptr) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!g->p2p.ready) return fail(NSK_E_INVALID, "nsk_p2p_setup / nsk_p2p_export / nsk_p2p_import first");
    NSK_ONE_CHAIN(g, "the peer-to-peer entry points");
    if (checks & P2P_NO_TRACE) NSK_NO_TRACE(g, "the peer-to-peer entry points");
    if (bad_arg) return fail(NSK_E_INVALID, bad_arg);
    if (!(checks & P2P_FLUSH)) return NSK_OK;
    HIPCHECK(hipSetDevice(g->device));
    return nsk_p2p_flush(g);
}

void nsk_exchange_release(nsk_graph *g) {
    p2p_close_peers(g);
    if (g->gather.comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy((ncclComm_t)g->gather.comm);
    g->gather.comm = nullptr;
}

extern "C" {

int nsk_ghost_needs(nsk_graph *g, int64_t *count, int32_t *vids) {
    if (!g || !count) return fail(NSK_E_INVALID, "null argument");
    *count = (int64_t)g->c.ghost_needs.size();
    if (vids && *count) memcpy(vids, g->c.ghost_needs.data(), (size_t)*count * sizeof(int32_t));
    return NSK_OK;
}

int nsk_exchange_setup(nsk_graph *g, int world, int rank, const int32_t *send_vids, int64_t nsend,
                       const int32_t *recv_vids, const int64_t *recv_off, int64_t slot) {
    if (!g || world < 1 || rank < 0 || rank >= world || nsend < 0 || slot < nsend || !recv_off)
        return fail(NSK_E_INVALID, "bad exchange description");
    NSK_ONE_CHAIN(g, "nsk_exchange_setup");
    HIPCHECK(hipSetDevice(g->device));
    const int64_t nrecv = recv_off[world];
    for (int64_t i = 0; i < nsend; i++)
        if (send_vids[i] < g->c.own_begin || send_vids[i] >= g->c.own_end)
            return fail(NSK_E_INDEX, "send list names a variable this handle does not own");
    std::vector<int32_t> rslot((size_t)nrecv);
    for (int src = 0; src < world; src++) {
        if (recv_off[src + 1] - recv_off[src] > slot) return fail(NSK_E_INVALID, "slot smaller than a rank's list");
        for (int64_t j = recv_off[src]; j < recv_off[src + 1]; j++) {
            if (recv_vids[j] < -1 || recv_vids[j] >= g->c.nvar) return fail(NSK_E_INDEX, "receive list out of range");
            rslot[j] = (src == rank || recv_vids[j] < 0) ? -1 : (int32_t)(src * slot + (j - recv_off[src]));
        }
    }
    std::vector<int32_t> sv(send_vids, send_vids + nsend), rv(recv_vids, recv_vids + nrecv);
    for (auto &x : sv) x = g->c.iid[x];                        // the kernels address values by internal id
    for (auto &x : rv) x = x < 0 ? 0 : g->c.iid[x];          // (skipped entries: slot -1, never written)
    // the arrays of a previous set-up go first; from here to commit() the handle is "not set up"
    HIPCHECK(hipStreamSynchronize(g->stream));
    NskGather &x = g->gather;
    for (void *old : {(void *)x.send_vids, (void *)x.recv_vids, (void *)x.recv_slot, x.send, x.recv, x.send_evid, x.recv_evid}) dev_free(g, old);
    x.reset();
    int rc;
    if ((rc = ensure_w_start(g))) return rc;
    NskGather n = x;
    NskRollback rb(g->mem, nsk_free_raw);
    if ((rc = dev_upload(g, &n.send_vids, sv))) return rc;
    if ((rc = dev_upload(g, &n.recv_vids, rv))) return rc;
    if ((rc = dev_upload(g, &n.recv_slot, rslot))) return rc;
    const size_t vb = (size_t)g->c.vbytes;
    uint8_t *t = nullptr;
    if ((rc = dev_alloc(g, &t, (size_t)slot * vb))) return rc; n.send = t;
    if ((rc = dev_alloc(g, &t, (size_t)slot * vb * world))) return rc; n.recv = t;
    if ((rc = dev_alloc(g, &t, (size_t)slot * vb))) return rc; n.send_evid = t;
    if ((rc = dev_alloc(g, &t, (size_t)slot * vb * world))) return rc; n.recv_evid = t;
    HIPCHECK(hipMemsetAsync(n.send, 0, (size_t)(slot ? slot : 1) * vb, g->stream));
    HIPCHECK(hipMemsetAsync(n.send_evid, 0, (size_t)(slot ? slot : 1) * vb, g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    rb.commit();
    n.world = world; n.slot = slot; n.nsend = nsend; n.nrecv = nrecv;
    x = n;
    return NSK_OK;
}

}  // extern "C"

template <typename VT>
static int exchange_kernels(nsk_graph *g, int which, bool pack) {
    VT *val = (VT *)(which == NSK_BUF_VALUE ? g->val : g->val_evid);
    VT *sb = (VT *)(which == NSK_BUF_VALUE ? g->gather.send : g->gather.send_evid);
    VT *rb = (VT *)(which == NSK_BUF_VALUE ? g->gather.recv : g->gather.recv_evid);
    if (pack) {
        const int n = (int)g->gather.nsend;
        if (n > 0)
            k_exchange_pack<VT><<<dim3((n + NSK_BLOCK - 1) / NSK_BLOCK), dim3(NSK_BLOCK), 0, g->stream>>>(
                val, g->gather.send_vids, sb, n);
    } else {
        const int n = (int)g->gather.nrecv;
        if (n > 0)
            k_exchange_unpack<VT><<<dim3((n + NSK_BLOCK - 1) / NSK_BLOCK), dim3(NSK_BLOCK), 0, g->stream>>>(
                val, g->gather.recv_vids, g->gather.recv_slot, rb, n);
    }
    HIPCHECK(hipGetLastError());
    return NSK_OK;
}

static int exchange_step(nsk_graph *g, int which, bool pack) {
    int rc = gather_enter(g, false, which != NSK_BUF_VALUE && which != NSK_BUF_VALUE_EVID ? "bad buffer id" : nullptr);
    return rc ? rc : NSK_BY_VT(g, exchange_kernels, g, which, pack);
}

extern "C" {

int nsk_exchange_pack(nsk_graph *g, int which) { return exchange_step(g, which, true); }
int nsk_exchange_unpack(nsk_graph *g, int which) { return exchange_step(g, which, false); }

// ---- peer-to-peer exchange ------------------------------------------------------------------------
// Partial factors (messages.py:1333-1355): `npf` aggregates over variables this handle holds; op 0 = "some member is
// 1" (OR), 1 = "no member is 0" (AND / ISTRUE); members of aggregate j = member_vids[member_off[j] .. member_off[j+1]).
// The value arrays grow by npf slots behind the internal ids; a peer-to-peer send list names aggregate j as variable
// id nvar + j, and every exchange recomputes the aggregates (both chains in learning) before it pushes.
int nsk_pf_setup(nsk_graph *g, int64_t npf, const uint8_t *op, const int64_t *member_off, const int32_t *member_vids) {
    if (!g || npf < 0 || (npf && (!op || !member_off || !member_vids))) return fail(NSK_E_INVALID, "bad partial-factor description");
    NSK_ONE_CHAIN(g, "nsk_pf_setup");
    HIPCHECK(hipSetDevice(g->device));
    { int frc = nsk_p2p_flush(g); if (frc) return frc; }
    std::vector<int32_t> off((size_t)npf + 1, 0), mem;
    std::vector<uint8_t> ops((size_t)npf);
    for (int64_t j = 0; j < npf; j++) {
        if (op[j] > 1 || member_off[j + 1] < member_off[j] || member_off[0] != 0) return fail(NSK_E_INVALID, "bad partial-factor description");
        ops[(size_t)j] = op[j];
        for (int64_t k = member_off[j]; k < member_off[j + 1]; k++) {
            if (member_vids[k] < 0 || member_vids[k] >= g->c.nvar) return fail(NSK_E_INDEX, "partial factor over a variable this handle does not hold");
            mem.push_back(g->c.iid[member_vids[k]]);
        }
        off[(size_t)j + 1] = (int32_t)mem.size();
    }
    HIPCHECK(hipStreamSynchronize(g->stream));
    nsk_drop_sweep_graph(g);
    // value arrays with npf more slots (contents kept)
    const size_t vb = (size_t)g->c.vbytes, nid = (size_t)g->c.nid;
    for (int chain = 0; chain < 2; chain++) {
        void *&arr = chain ? g->val_evid : g->val;
        uint8_t *bigger = nullptr;
        int rc = dev_alloc(g, &bigger, (nid + (size_t)npf) * vb + 16);
        if (rc) return rc;
        HIPCHECK(hipMemsetAsync(bigger, 0, (nid + (size_t)npf) * vb + 16, g->stream));
        HIPCHECK(hipMemcpyAsync(bigger, arr, nid * vb, hipMemcpyDeviceToDevice, g->stream));
        HIPCHECK(hipStreamSynchronize(g->stream));
        dev_free(g, arr);
        arr = bigger;
    }
    // (a second set-up replaces the first one's descriptions)
    dev_free(g, g->p2p.pf_op); g->p2p.pf_op = nullptr;
    dev_free(g, g->p2p.pf_off); g->p2p.pf_off = nullptr;
    dev_free(g, g->p2p.pf_mem); g->p2p.pf_mem = nullptr;
    int rc;
    if ((rc = dev_upload(g, &g->p2p.pf_op, ops))) return rc;
    if ((rc = dev_upload(g, &g->p2p.pf_off, off))) return rc;
    if ((rc = dev_upload(g, &g->p2p.pf_mem, mem))) return rc;
    HIPCHECK(hipStreamSynchronize(g->stream));
    g->p2p.npf = npf;
    return NSK_OK;
}

int nsk_p2p_setup(nsk_graph *g, int world, int rank, const int32_t *send_vids, const int64_t *send_off,
                  const int32_t *recv_vids, const int64_t *recv_off, const int64_t *peer_base,
                  const int64_t *peer_total) {
    if (!g || world < 1 || world > 16 || rank < 0 || rank >= world || !send_off || !recv_off || !peer_base || !peer_total)
        return fail(NSK_E_INVALID, "bad peer-to-peer description (at most 16 ranks: one node)");
    NSK_ONE_CHAIN(g, "nsk_p2p_setup");
    HIPCHECK(hipSetDevice(g->device));
    const int64_t nsend = send_off[world], nrecv = recv_off[world];
    if (send_off[0] != 0 || recv_off[0] != 0 || nsend < 0 || nrecv < 0) return fail(NSK_E_INVALID, "bad list offsets");
    for (int q = 0; q < world; q++) {
        if (send_off[q + 1] < send_off[q] || recv_off[q + 1] < recv_off[q]) return fail(NSK_E_INVALID, "bad list offsets");
        const int64_t seg = send_off[q + 1] - send_off[q];
        if (peer_base[q] < 0 || peer_base[q] + seg > peer_total[q]) return fail(NSK_E_INVALID, "a send segment does not fit its reader's buffer");
    }
    if (send_off[rank + 1] != send_off[rank] || recv_off[rank + 1] != recv_off[rank])
        return fail(NSK_E_INVALID, "a rank does not exchange with itself");
    if (peer_total[rank] != nrecv) return fail(NSK_E_INVALID, "peer_total[rank] must be this rank's receive total");
    std::vector<int32_t> sv((size_t)nsend), rv((size_t)nrecv);
    for (int64_t i = 0; i < nsend; i++) {
        if (send_vids[i] >= g->c.nvar && send_vids[i] < g->c.nvar + g->p2p.npf) {       // partial-factor aggregate (nsk_pf_setup)
            sv[(size_t)i] = (int32_t)(g->c.nid + (send_vids[i] - g->c.nvar));
            continue;
        }
        if (send_vids[i] < g->c.own_begin || send_vids[i] >= g->c.own_end)
            return fail(NSK_E_INDEX, "send list names a variable this handle does not own");
        sv[(size_t)i] = g->c.iid[send_vids[i]];               // the kernels address values by internal id
    }
    for (int64_t j = 0; j < nrecv; j++) {
        if (recv_vids[j] < 0 || recv_vids[j] >= g->c.nvar || (recv_vids[j] >= g->c.own_begin && recv_vids[j] < g->c.own_end))
            return fail(NSK_E_INDEX, "receive list names a variable this handle owns or does not hold");
        rv[(size_t)j] = g->c.iid[recv_vids[j]];
    }
    // the lists of a previous set-up go first; from here to commit() the handle is "not set up" (a closing wait +
    // unpack still pending would read them: the set-up that replaces the lists drops it, as the import always did)
    HIPCHECK(hipStreamSynchronize(g->stream));
    nsk_drop_sweep_graph(g);
    NskP2P &x = g->p2p;
    dev_free(g, x.send_iid); dev_free(g, x.recv_iid);
    x.reset();
    int rc;
    if ((rc = ensure_w_start(g))) return rc;
    if (!x.err) {
        if ((rc = dev_alloc(g, &x.err, 4))) return rc;
        HIPCHECK(hipMemsetAsync(x.err, 0, 4 * sizeof(unsigned int), g->stream));
    }
    int32_t *send_iid = nullptr, *recv_iid = nullptr;
    NskRollback rb(g->mem, nsk_free_raw);
    if ((rc = dev_upload(g, &send_iid, sv))) return rc;
    if ((rc = dev_upload(g, &recv_iid, rv))) return rc;
    HIPCHECK(hipStreamSynchronize(g->stream));
    rb.commit();
    x.world = world; x.rank = rank; x.nsend = nsend; x.nrecv = nrecv;
    x.send_iid = send_iid; x.recv_iid = recv_iid;
    x.soff.assign(send_off, send_off + world + 1);
    x.roff.assign(recv_off, recv_off + world + 1);
    x.dbase.assign(peer_base, peer_base + world);
    x.dtotal.assign(peer_total, peer_total + world);
    for (int q = 0; q < world; q++)             // symmetric: q is a peer when either side reads from the other
        if (q != rank && (send_off[q + 1] > send_off[q] || recv_off[q + 1] > recv_off[q])) x.peer_mask |= 1u << q;
    x.send_host.swap(sv);
    x.recv_host.swap(rv);
    if (const char *t = getenv("NSK_P2P_TIMEOUT_S")) {
        const double sec = atof(t);
        if (sec > 0) x.timeout_ticks = (unsigned long long)(sec * 1e8);
    }
    return NSK_OK;
}

int nsk_p2p_export(nsk_graph *g, void *handle64, void **base) {
    if (!g) return fail(NSK_E_INVALID, "null argument");
    if (g->p2p.world == 0) return fail(NSK_E_INVALID, "nsk_p2p_setup has not been called");
    HIPCHECK(hipSetDevice(g->device));
    const size_t vb = (size_t)g->c.vbytes, nw = (size_t)g->c.nweight;
    const size_t bytes = nsk_p2p_bytes(g->p2p.world, (size_t)g->p2p.nrecv, vb, nw);
    if (g->p2p.base && g->p2p.bytes < bytes) {          // a later set-up with longer lists: a new allocation
        HIPCHECK(hipStreamSynchronize(g->stream));
        dev_free(g, g->p2p.base);
        g->p2p.base = nullptr;
    }
    if (!g->p2p.base) {
        // fine-grained: a peer's stores and this rank's polling loads are coherent while kernels run
        uint8_t *base8 = nullptr;
        int rc = dev_alloc(g, &base8, bytes, true);
        if (rc) return rc;
        g->p2p.base = base8;
        g->p2p.bytes = bytes;
    }
    HIPCHECK(hipMemsetAsync(g->p2p.base, 0, g->p2p.bytes, g->stream));
    HIPCHECK(hipMemsetAsync(g->p2p.err, 0, 4 * sizeof(unsigned int), g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    g->p2p.tag = 0;
    g->p2p.ready = false;
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
    if (handle64) {
        hipIpcMemHandle_t h;
        HIPCHECK(hipIpcGetMemHandle(&h, g->p2p.base));
        memcpy(handle64, &h, 64);
    }
    if (base) *base = g->p2p.base;
    return NSK_OK;
}

}  // extern "C"

// Fused boundary exchange (nsk_internal.h NskP2P::fused): decide whether the handle qualifies and build the push map.
// Conditions: every sampled variable in a table segment; the receive list is the run of ghost ids in order (the
// compiler numbers the ghosts a handle reads first and ascending, so the receive block IS the ghost array); every
// boundary value has exactly one reader (range shards of a grid; a value read by several ranks keeps the
// exchange kernels).
static int p2p_fuse_plan(nsk_graph *g) {
    g->p2p.fused = false;
    g->p2p.border_tiles.clear();
    if (nsk::diag_env("NSK_NO_P2P_FUSE") || !nsk_tables_only(g)) return NSK_OK;
    const nsk::Compiled &c = g->c;
    const std::vector<int32_t> &sv = g->p2p.send_host, &rv = g->p2p.recv_host;
    if (rv.empty() && sv.empty()) return NSK_OK;
    const uint32_t ghost_lo = rv.empty() ? (uint32_t)c.nid : (uint32_t)rv[0];
    for (size_t j = 0; j < rv.size(); j++) if ((uint32_t)rv[j] != ghost_lo + (uint32_t)j) return NSK_OK;
    if (ghost_lo < (uint32_t)c.npos) return NSK_OK;
    for (int q = 0; q < g->p2p.world; q++) if (g->p2p.dtotal[q] >= (1ll << 28)) return NSK_OK;
    // tiles that read a ghost: slot bases of the implicit adjacency, or the stream words
    std::vector<int32_t> tiles;
    for (int32_t p : sv) tiles.push_back(p >> 6);
    for (const nsk::Compiled::Segment &sg : c.segments) {
        const int nch = sg.nslots > 4 ? 2 : 1;
        for (int64_t t = 0; t < sg.ntiles; t++) {
            bool reads = false;
            const uint32_t *ab = sg.aff >= 0 ? &c.seg_aff[((size_t)sg.aff + (size_t)t * nch) * 4] : nullptr;
            if (ab && ab[0] != 0xFFFFFFFFu) {
                for (int j = 0; j < 4 * nch && !reads; j++) reads = ab[j] + 63u >= ghost_lo && ab[j] < ghost_lo + (uint32_t)rv.size();
            } else {
                const uint32_t *w = &c.adj[((size_t)sg.adj_off + (size_t)t * 64 * nch) * 4];
                for (int i = 0; i < 256 * nch && !reads; i++) reads = w[i] - ghost_lo < (uint32_t)rv.size();
            }
            if (reads) tiles.push_back((int32_t)(sg.pos0 / 64 + t));
        }
    }
    std::sort(tiles.begin(), tiles.end());
    tiles.erase(std::unique(tiles.begin(), tiles.end()), tiles.end());
    // fewer, longer runs (a launch carries at most NSK_SEG_MAX segment entries): a short segment with a border
    // tile is border as a whole, and so are gaps of a few tiles between border tiles of one segment -- such a tile
    // pushes nothing (its row of the map is empty), it only waits and counts like its neighbours
    {
        std::vector<int32_t> extra;
        for (const nsk::Compiled::Segment &sg : c.segments) {
            const int32_t f = (int32_t)(sg.pos0 / 64), e = f + sg.ntiles;
            auto lo = std::lower_bound(tiles.begin(), tiles.end(), f), hi = std::lower_bound(tiles.begin(), tiles.end(), e);
            if (lo == hi) continue;
            if (sg.ntiles <= 64) { for (int32_t t = f; t < e; t++) extra.push_back(t); continue; }
            for (auto it = lo; it + 1 < hi; ++it)
                if (it[1] - it[0] > 1 && it[1] - it[0] <= 16) for (int32_t t = it[0] + 1; t < it[1]; t++) extra.push_back(t);
        }
        tiles.insert(tiles.end(), extra.begin(), extra.end());
        std::sort(tiles.begin(), tiles.end());
        tiles.erase(std::unique(tiles.begin(), tiles.end()), tiles.end());
    }
    std::vector<uint32_t> pm(tiles.size() * 64, 0xFFFFFFFFu);
    for (int q = 0; q < g->p2p.world; q++)
        for (int64_t k = g->p2p.soff[q]; k < g->p2p.soff[q + 1]; k++) {
            const int32_t pos = sv[(size_t)k];
            const size_t row = (size_t)(std::lower_bound(tiles.begin(), tiles.end(), pos >> 6) - tiles.begin());
            uint32_t &e = pm[row * 64 + (size_t)(pos & 63)];
            if (e != 0xFFFFFFFFu) return NSK_OK;                                     // a second reader
            e = ((uint32_t)q << 28) | (uint32_t)(g->p2p.dbase[q] + (k - g->p2p.soff[q]));
        }
    dev_free(g, g->p2p.push_map);
    g->p2p.push_map = nullptr;
    int rc = dev_upload(g, &g->p2p.push_map, pm);
    if (rc) return rc;
    g->p2p.border_tiles.swap(tiles);
    g->p2p.ghost_lo = ghost_lo;
    g->p2p.fused = true;
    g->seg_plans_valid = false;          // the segment plans split at the border tiles
    return NSK_OK;
}

extern "C" {

static int p2p_finish_import(nsk_graph *g) {
    if (g->c.nweight)       // the weights every rank starts the next learning epoch from
        HIPCHECK(hipMemcpyAsync(g->w_start, g->w, (size_t)g->c.nweight * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
    int rc = p2p_fuse_plan(g);
    if (rc) return rc;
    HIPCHECK(hipStreamSynchronize(g->stream));
    nsk_drop_sweep_graph(g);
    g->p2p.tag = 0;
    g->p2p.close_pending = false;
    g->p2p.ready = true;
    return NSK_OK;
}

int nsk_p2p_import(nsk_graph *g, const void *all_handles) {
    if (!g || !all_handles) return fail(NSK_E_INVALID, "null argument");
    if (!g->p2p.base) return fail(NSK_E_INVALID, "nsk_p2p_export first");
    HIPCHECK(hipSetDevice(g->device));
    p2p_close_peers(g);
    for (int q = 0; q < g->p2p.world; q++) {
        if (q == g->p2p.rank) { g->p2p.peer_base[q] = g->p2p.base; continue; }
        hipIpcMemHandle_t h;
        memcpy(&h, (const char *)all_handles + (size_t)q * 64, 64);
        HIPCHECK(hipIpcOpenMemHandle(&g->p2p.peer_base[q], h, hipIpcMemLazyEnablePeerAccess));
        g->p2p.peer_ipc[q] = true;
    }
    return p2p_finish_import(g);
}

int nsk_p2p_import_local(nsk_graph *g, void *const *bases) {
    if (!g || !bases) return fail(NSK_E_INVALID, "null argument");
    if (!g->p2p.base) return fail(NSK_E_INVALID, "nsk_p2p_export first");
    HIPCHECK(hipSetDevice(g->device));
    p2p_close_peers(g);
    for (int q = 0; q < g->p2p.world; q++) {
        if (q != g->p2p.rank && !bases[q]) return fail(NSK_E_INVALID, "null peer allocation");
        g->p2p.peer_base[q] = q == g->p2p.rank ? g->p2p.base : bases[q];
    }
    return p2p_finish_import(g);
}

}  // extern "C"

// the kernels' view of the pairwise lists: the peers' blocks, this rank's segments in its lists and in the readers' blocks
static P2PPlan p2p_plan(const nsk_graph *g) {
    const NskP2P &x = g->p2p;
    P2PPlan plan;
    memset(&plan, 0, sizeof(plan));
    for (int q = 0; q < x.world; q++) {
        plan.base[q] = x.peer_base[q];
        plan.soff[q] = (unsigned long long)x.soff[q];
        plan.roff[q] = (unsigned long long)x.roff[q];
        plan.dbase[q] = (unsigned long long)x.dbase[q];
        plan.dtotal[q] = (unsigned long long)x.dtotal[q];
    }
    for (int q = x.world; q <= 16; q++) { plan.soff[q] = (unsigned long long)x.nsend; plan.roff[q] = (unsigned long long)x.nrecv; }
    return plan;
}

// part 0 = one whole exchange (the sweep loops); 1 = the pushes, 2 = wait + unpack (+ the owner's half of the
// weight merge), 3 = the closing half of the weight merge -- the parts on their own serve the tests that drive
// several handles from one process (issued breadth-first) and the phase timings
template <typename VT>
static int p2p_exchange(nsk_graph *g, const unsigned long long *tag_base, unsigned int tag_off, bool learn, int part, int selftest = 0) {
    const int world = g->p2p.world, me = g->p2p.rank;
    const int nw = (int)g->c.nweight;
    if ((part == 0 || part == 1) && !tag_base) ++g->p2p.tag;
    const unsigned int tag = tag_base ? tag_off : g->p2p.tag;
    const bool weights = learn && nw > 0 && world > 1;
    // a learning epoch's weight deltas go to every rank, so every rank is a peer of every other
    const unsigned int mask = weights ? (((1u << world) - 1u) & ~(1u << me)) : g->p2p.peer_mask;
    if (!mask) return NSK_OK;
    const P2PPlan plan = p2p_plan(g);
    P2PWeights pw;
    // big: lists beyond 2^16 values or tables beyond 2^16 weights -- many-block launches with one-wave flag kernels
    // between them (k_p2p_push_big); otherwise one or two <= 64-block launches that raise and poll themselves
    const char *big_env = nsk::diag_env("NSK_P2P_BIG_MIN");             // (diagnostic; read per exchange so that tests can set it)
    const int64_t big_min = big_env ? atoll(big_env) : 65536;
    const bool big = std::max(g->p2p.nsend, g->p2p.nrecv) > big_min || (weights && nw > big_min);
    pw.w = weights ? g->w : nullptr; pw.w_start = weights ? g->w_start : nullptr; pw.nw = weights ? nw : 0;
    const int64_t wwork = weights ? ((int64_t)nw + 3) / 4 : 0;          // (a block's threads take a few weights each)
    auto blocks = [&](int64_t work) { return (int)std::max<int64_t>(1, std::min<int64_t>(64, (work + 4 * NSK_BLOCK - 1) / (4 * NSK_BLOCK))); };
    auto many = [&](int64_t work) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (work + NSK_BLOCK - 1) / NSK_BLOCK))); };
    VT *val = (VT *)g->val, *val_evid = (VT *)g->val_evid;
    const int both = learn ? 1 : 0;
    auto push_big = [&]() {
        k_p2p_push_big<VT><<<many(std::max<int64_t>(g->p2p.nsend, pw.nw)), dim3(NSK_BLOCK), 0, g->stream>>>(
            val, val_evid, both, g->p2p.send_iid, (long long)g->p2p.nsend, plan, pw, world, me, tag, tag_base, selftest);
        k_p2p_raise<<<dim3(1), dim3(64), 0, g->stream>>>(plan, 0, world, me, mask, tag, tag_base);
    };
    auto unpack_big = [&]() {
        k_p2p_wait<<<dim3(1), dim3(64), 0, g->stream>>>(g->p2p.base, 0, world, mask, tag, tag_base, g->p2p.err, g->p2p.timeout_ticks);
        k_p2p_unpack_big<VT><<<many(std::max<int64_t>(g->p2p.nrecv, (pw.nw + world - 1) / world)), dim3(NSK_BLOCK), 0, g->stream>>>(
            val, val_evid, both, g->p2p.recv_iid, (long long)g->p2p.nrecv, g->p2p.base, plan, pw, world, me, tag, tag_base, g->p2p.err, selftest);
        if (weights) k_p2p_raise<<<dim3(1), dim3(64), 0, g->stream>>>(plan, 1, world, me, mask, tag, tag_base);
    };
    auto gather = [&]() {
        if (!weights) return;
        if (big) k_p2p_wait<<<dim3(1), dim3(64), 0, g->stream>>>(g->p2p.base, 1, world, mask, tag, tag_base, g->p2p.err, g->p2p.timeout_ticks);
        k_p2p_gather_w<VT><<<big ? many(nw) : dim3((unsigned)blocks(wwork)), dim3(NSK_BLOCK), 0, g->stream>>>(
            g->w, g->w_start, nw, g->p2p.base, (long long)g->p2p.nrecv, world, mask, tag, g->p2p.err, g->p2p.timeout_ticks, selftest, big ? 1 : 0);
        if (!selftest) g->weights_dirty = true;
    };
    if ((part == 0 || part == 1) && g->p2p.npf > 0 && !selftest)         // the partial-factor aggregates this rank's readers take
        k_pf_compute<VT><<<dim3((unsigned)((g->p2p.npf + NSK_BLOCK - 1) / NSK_BLOCK)), dim3(NSK_BLOCK), 0, g->stream>>>(
            val, val_evid, both, g->p2p.pf_op, g->p2p.pf_off, g->p2p.pf_mem, (int)g->p2p.npf, (long long)g->c.nid);
    if (part == 0) {                            // the sweep loops: push, flags, wait and unpack in one launch
        if (big) { push_big(); unpack_big(); }
        else {
            const int nb = blocks(std::max(std::max(g->p2p.nsend, g->p2p.nrecv), wwork));
            k_p2p_exchange<VT, true><<<dim3(nb), dim3(NSK_BLOCK), 0, g->stream>>>(
                val, val_evid, both, g->p2p.send_iid, (long long)g->p2p.nsend, plan, pw, g->p2p.recv_iid,
                (long long)g->p2p.nrecv, g->p2p.base, world, me, mask, g->p2p.err + 1, tag, g->p2p.err, tag_base, g->p2p.timeout_ticks, selftest);
        }
        gather();
    } else if (part == 1) {
        if (big) push_big();
        else {
            // at most 64 blocks (grid-stride): the closing ticket adds must not queue up
            const int nb = blocks(std::max(g->p2p.nsend, wwork));
            k_p2p_push<VT><<<dim3(nb), dim3(NSK_BLOCK), 0, g->stream>>>(val, val_evid, both, g->p2p.send_iid, (long long)g->p2p.nsend, plan, pw, world, me,
                                                                       mask, g->p2p.err + 1, tag, tag_base, selftest);
        }
    } else if (part == 2) {
        if (big) unpack_big();
        else {
            const int nb = blocks(std::max(g->p2p.nrecv, wwork));
            k_p2p_exchange<VT, false><<<dim3(nb), dim3(NSK_BLOCK), 0, g->stream>>>(
                val, val_evid, both, g->p2p.send_iid, (long long)g->p2p.nsend, plan, pw, g->p2p.recv_iid,
                (long long)g->p2p.nrecv, g->p2p.base, world, me, mask, g->p2p.err + 1, tag, g->p2p.err, tag_base, g->p2p.timeout_ticks, selftest);
        }
    } else {
        gather();
    }
    HIPCHECK(hipGetLastError());
    return NSK_OK;
}

int nsk_p2p_enqueue(nsk_graph *g, const unsigned long long *tag_base, unsigned int tag_off, bool learn, int part) {
    return NSK_BY_VT(g, p2p_exchange, g, tag_base, tag_off, learn, part);
}

// kernel argument of a fused table launch
void nsk_p2p_fill(nsk_graph *g, nsk::TabP2P &px, const unsigned long long *tag_base, unsigned int tag, bool wait) {
    memset(&px, 0, sizeof(px));
    px.wait = wait ? 1 : 0;
    px.mine = g->p2p.base;
    for (int q = 0; q < g->p2p.world; q++) { px.peer[q] = g->p2p.peer_base[q]; px.dtotal[q] = (unsigned long long)g->p2p.dtotal[q]; }
    px.push_map = g->p2p.push_map;
    px.counter = g->p2p.err + 3;
    px.err = g->p2p.err;
    px.tag_base = tag_base;
    px.timeout_ticks = g->p2p.timeout_ticks;
    px.ghost_lo = g->p2p.ghost_lo;
    px.nrecv = (uint32_t)g->p2p.nrecv;
    px.border_total = g->p2p.border_total;
    px.tag = tag;
    px.peer_mask = g->p2p.peer_mask;
    px.world = g->p2p.world;
    px.me = g->p2p.rank;
}

// the ghost values of the value array into the receive block of the LAST exchange's parity: what the first fused
// sweep of a call reads (the caller may have uploaded a state since)
template <typename VT>
static __global__ __launch_bounds__(NSK_BLOCK) void k_p2p_ghost_pack(const VT *val, const int32_t *recv_iid, long long nrecv, void *mine,
                                                                      int world, unsigned int tag) {
    VT *rb = (VT *)((char *)mine + nsk_p2p_recv_off(world)) + (size_t)(tag & 1u) * 2 * (size_t)nrecv;
    for (long long j = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; j < nrecv; j += (long long)gridDim.x * NSK_BLOCK)
        rb[j] = val[recv_iid[j]];
}
template <typename VT>
static int p2p_ghost_pack(nsk_graph *g) {
    const int nb = (int)std::min<int64_t>(64, (g->p2p.nrecv + NSK_BLOCK - 1) / NSK_BLOCK);
    k_p2p_ghost_pack<VT><<<dim3(nb), dim3(NSK_BLOCK), 0, g->stream>>>((const VT *)g->val, g->p2p.recv_iid, (long long)g->p2p.nrecv,
                                                                      g->p2p.base, g->p2p.world, g->p2p.tag);
    HIPCHECK(hipGetLastError());
    return NSK_OK;
}
int nsk_p2p_ghost_pack(nsk_graph *g) { return g->p2p.nrecv == 0 ? NSK_OK : NSK_BY_VT(g, p2p_ghost_pack, g); }

// A fused sweep sequence ends with its last class launch; the wait for the peers' last flags and the copy of the
// received values into the value array's ghost ids (what downloads, the other kernels and the next call's pack
// read) is enqueued lazily -- before the next thing that needs it -- so that a caller driving several ranks from
// one process can issue every rank's sweeps before any rank's wait.
int nsk_p2p_flush(nsk_graph *g) {
    if (!g || !g->p2p.close_pending) return NSK_OK;
    g->p2p.close_pending = false;
    return nsk_p2p_enqueue(g, nullptr, 0, false, 2);          // wait for tag p2p_tag + unpack
}

extern "C" {

int nsk_p2p_check(nsk_graph *g) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!g->p2p.err) return NSK_OK;
    HIPCHECK(hipSetDevice(g->device));
    { int frc = nsk_p2p_flush(g); if (frc) return frc; }
    unsigned int err = 0;
    HIPCHECK(hipMemcpyAsync(&err, g->p2p.err, sizeof(err), hipMemcpyDeviceToHost, g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    if (err) {
        HIPCHECK(hipMemsetAsync(g->p2p.err, 0, sizeof(unsigned int), g->stream));      // reported once
        if (err & NSK_P2P_ERR_PAYLOAD)
            return fail(NSK_E_DEVICE, "peer-to-peer self-test: a peer's flag arrived but the payload read back differs from "
                                      "what the peer wrote (peer writes are not visible to this device's kernels)");
        return fail(NSK_E_DEVICE, "peer-to-peer exchange: a peer's boundary values did not arrive within "
                                  "NSK_P2P_TIMEOUT_S; the ghost values of this handle are incomplete");
    }
    return NSK_OK;
}

}  // extern "C"

// learn == 2: the memory protocol of the fused exchange (k_p2p_fused_selftest)
template <typename VT>
static int p2p_fused_selftest(nsk_graph *g, int part) {
    if (!g->p2p.peer_mask) return NSK_OK;
    if (part != 2) ++g->p2p.tag;
    const P2PPlan plan = p2p_plan(g);
    k_p2p_fused_selftest<VT><<<dim3(1), dim3(NSK_BLOCK), 0, g->stream>>>((long long)g->p2p.nsend, (long long)g->p2p.nrecv, plan, g->p2p.base,
                                                                         g->p2p.world, g->p2p.rank, g->p2p.peer_mask, g->p2p.tag, g->p2p.err,
                                                                         g->p2p.timeout_ticks, part);
    HIPCHECK(hipGetLastError());
    return NSK_OK;
}

extern "C" {

int nsk_p2p_selftest(nsk_graph *g, int learn, int part) {
    int rc = p2p_enter(g, P2P_FLUSH, bad_part(part));
    if (rc) return rc;
    if (learn == 2) return part == 3 ? NSK_OK : NSK_BY_VT(g, p2p_fused_selftest, g, part);
    return NSK_BY_VT(g, p2p_exchange, g, nullptr, 0, learn != 0, part, 1);
}

int nsk_p2p_fuse(nsk_graph *g, int on) {
    int rc = p2p_enter(g, P2P_FLUSH);
    if (rc) return rc;
    if (on) {
        if ((rc = p2p_fuse_plan(g))) return rc;
    } else if (g->p2p.fused) {
        g->p2p.fused = false;
        g->p2p.border_tiles.clear();
        g->seg_plans_valid = false;
    }
    nsk_drop_sweep_graph(g);
    return g->p2p.fused ? 1 : 0;
}

int nsk_p2p_reset(nsk_graph *g) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!g->p2p.base) return fail(NSK_E_INVALID, "nsk_p2p_setup / nsk_p2p_export first");
    HIPCHECK(hipSetDevice(g->device));
    { int frc = nsk_p2p_flush(g); if (frc) return frc; }
    HIPCHECK(hipStreamSynchronize(g->stream));
    nsk_drop_sweep_graph(g);
    HIPCHECK(hipMemsetAsync(g->p2p.base, 0, g->p2p.bytes, g->stream));
    HIPCHECK(hipMemsetAsync(g->p2p.err, 0, 4 * sizeof(unsigned int), g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    g->p2p.tag = 0;
    g->p2p.close_pending = false;
    return NSK_OK;
}

int nsk_p2p_exchange(nsk_graph *g, int learn, int part) {
    int rc = p2p_enter(g, P2P_NO_TRACE | P2P_FLUSH, bad_part(part));
    return rc ? rc : nsk_p2p_enqueue(g, nullptr, 0, learn != 0, part);
}

int nsk_gibbs_sweeps_p2p(nsk_graph *g, int64_t nsweeps, int sample_evidence, int burnin) {
    int rc = p2p_enter(g, P2P_NO_TRACE, bad_sweeps(nsweeps));
    if (rc) return rc;
    HIPCHECK(hipSetDevice(g->device));
    return nsk_gibbs_run(g, nsweeps, sample_evidence, burnin, true);      // (flushes a pending close unless it continues it)
}

int nsk_learn_sweeps_p2p(nsk_graph *g, int64_t nsweeps, double step, double decay, int regularization,
                         double reg_param, int64_t truncation, int learn_non_evidence) {
    int rc = p2p_enter(g, P2P_NO_TRACE | P2P_FLUSH, bad_sweeps(nsweeps));
    if (rc) return rc;
    const int nw = (int)g->c.nweight;
    // the caller may have written the weight buffer since the last epoch: this call starts from what is there
    if (nw && nsweeps) HIPCHECK(hipMemcpyAsync(g->w_start, g->w, (size_t)nw * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
    for (int64_t s = 0; s < nsweeps; s++) {
        if ((rc = nsk_learn_sweeps(g, 1, step, 1.0, regularization, reg_param, truncation, learn_non_evidence))) return rc;
        if ((rc = nsk_p2p_enqueue(g, nullptr, 0, true, 0))) return rc;     // values of both chains + weight deltas; w_start = merged w
        step *= decay;
    }
    return NSK_OK;
}

// ---- native RCCL loop -----------------------------------------------------------------------------
static int load_rccl(const char *path) {
    if (g_rccl.lib) return NSK_OK;
    void *h = dlopen(path && path[0] ? path : "librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(NSK_E_DEVICE, std::string("dlopen(librccl): ") + dlerror());
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(h, "ncclCommInitRank");
    g_rccl.AllGather = (decltype(g_rccl.AllGather))dlsym(h, "ncclAllGather");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(h, "ncclAllReduce");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(h, "ncclCommDestroy");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.AllReduce || !g_rccl.CommDestroy)
        return fail(NSK_E_DEVICE, "librccl lacks the expected symbols");
    g_rccl.lib = h;
    return NSK_OK;
}

#define RCCLCHECK(expr)                                                                         \
    do {                                                                                        \
        ncclResult_t r_ = (expr);                                                               \
        if (r_ != ncclSuccess)                                                                  \
            return fail(NSK_E_DEVICE, std::string(#expr) + ": " +                              \
                        (g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "rccl error"));    \
    } while (0)

int nsk_comm_unique_id(const char *librccl_path, void *id128) {
    if (!id128) return fail(NSK_E_INVALID, "null argument");
    int rc = load_rccl(librccl_path);
    if (rc) return rc;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    RCCLCHECK(g_rccl.GetUniqueId((ncclUniqueId *)id128));
    return NSK_OK;
}

int nsk_comm_init(nsk_graph *g, int world, int rank, const void *id128, const char *librccl_path) {
    if (!g || !id128 || world < 1 || rank < 0 || rank >= world) return fail(NSK_E_INVALID, "bad argument");
    NSK_ONE_CHAIN(g, "nsk_comm_init");
    int rc = load_rccl(librccl_path);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(g->device));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclComm_t comm = nullptr;
    RCCLCHECK(g_rccl.CommInitRank(&comm, world, id, rank));
    g->gather.comm = comm;
    return NSK_OK;
}

static int native_exchange(nsk_graph *g, int which) {
    int rc = exchange_step(g, which, true);
    if (rc) return rc;
    const void *sb = which == NSK_BUF_VALUE ? g->gather.send : g->gather.send_evid;
    void *rb = which == NSK_BUF_VALUE ? g->gather.recv : g->gather.recv_evid;
    if (g->gather.slot > 0)
        RCCLCHECK(g_rccl.AllGather(sb, rb, (size_t)g->gather.slot, g->c.vbytes == 1 ? ncclInt8 : ncclInt32,
                                   (ncclComm_t)g->gather.comm, g->stream));
    return exchange_step(g, which, false);
}

int nsk_gibbs_sweeps_exchange(nsk_graph *g, int64_t nsweeps, int sample_evidence, int burnin) {
    int rc = gather_enter(g, true);
    if (rc) return rc;
    for (int64_t s = 0; s < nsweeps; s++) {
        if ((rc = nsk_gibbs_sweeps(g, 1, sample_evidence, burnin))) return rc;
        if ((rc = native_exchange(g, NSK_BUF_VALUE))) return rc;
    }
    return NSK_OK;
}

int nsk_learn_sweeps_exchange(nsk_graph *g, int64_t nsweeps, double step, double decay, int regularization,
                              double reg_param, int64_t truncation, int learn_non_evidence) {
    int rc = gather_enter(g, true);
    if (rc) return rc;
    const int nw = (int)g->c.nweight;
    for (int64_t s = 0; s < nsweeps; s++) {
        HIPCHECK(hipSetDevice(g->device));
        if (nw) HIPCHECK(hipMemcpyAsync(g->w_start, g->w, (size_t)nw * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
        if ((rc = nsk_learn_sweeps(g, 1, step, 1.0, regularization, reg_param, truncation, learn_non_evidence))) return rc;
        if ((rc = native_exchange(g, NSK_BUF_VALUE))) return rc;
        if ((rc = native_exchange(g, NSK_BUF_VALUE_EVID))) return rc;
        if (nw) {       // w = w_start + sum over ranks of (w - w_start): numbskull_master.py:223-224
            const dim3 grid((nw + NSK_BLOCK - 1) / NSK_BLOCK), block(NSK_BLOCK);
            k_weight_delta<<<grid, block, 0, g->stream>>>(g->w, g->w_start, g->w_delta, nw);
            RCCLCHECK(g_rccl.AllReduce(g->w_delta, g->w_delta, (size_t)nw, ncclDouble, ncclSum,
                                       (ncclComm_t)g->gather.comm, g->stream));
            k_weight_merge<<<grid, block, 0, g->stream>>>(g->w, g->w_start, g->w_delta, nw);
            g->weights_dirty = true;
        }
        step *= decay;
    }
    return NSK_OK;
}

}  // extern "C"
