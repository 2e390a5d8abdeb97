// nsk_api.hip -- the C-ABI entry points of include/numbskull_amd.h: handle life cycle, state transfer, chains, info
// (sweep drivers: nsk_gibbs.hip / nsk_learn.hip; boundary exchange: nsk_exchange.hip; diagnostics: nsk_trace.hip,
// nsk_energy.hip, nsk_wstats.hip).
//
// Replaces the callee side of the reference's three run_pool(...) call sites
// (numbskull/factorgraph.py:141,163,202): gibbsthread (inference.py:10-33) and
// learnthread/sample_and_sgd (learning.py:12-125).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "nsk_internal.h"
#include "nsk_class_plan.h"
#include "nsk_kernels_learn.h"
#include "nsk_kernels_misc.h"

using namespace nsk;

// =============================================================================================
// host side
// =============================================================================================
static thread_local std::string g_err;

namespace nsk {
int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
void set_error(const std::string &m) { g_err = m; }
}

// May this device keep XCD-private accumulators (workgroup-scope atomics in the issuing XCD's L2,
// private copies picked by HW_REG_XCC_ID)?  gfx942 / gfx950 by architecture name AND a self-test, run
// once per device and process: 2048 x 256 threads add to the slot of their XCD (k_xcd_selftest); the
// slots, read back after the kernel boundary, must add up to the number of threads, with ids < 8.
static bool xcd_private_ok(nsk_graph *g) {
    static std::mutex mu;
    static std::map<int, bool> verdict;
    std::lock_guard<std::mutex> lk(mu);
    auto it = verdict.find(g->device);
    if (it != verdict.end()) return it->second;
    bool ok = false;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, g->device) == hipSuccess &&
        (strstr(prop.gcnArchName, "gfx950") || strstr(prop.gcnArchName, "gfx942"))) {
        unsigned int *d = nullptr, h[17];
        const unsigned int nblocks = 2048, nthreads = 256;
        if (hipMalloc((void **)&d, sizeof(h)) == hipSuccess) {
            bool ran = hipMemsetAsync(d, 0, sizeof(h), g->stream) == hipSuccess;
            if (ran) {
                k_xcd_selftest<<<dim3(nblocks), dim3(nthreads), 0, g->stream>>>(d);
                ran = hipGetLastError() == hipSuccess &&
                      hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, g->stream) == hipSuccess &&
                      hipStreamSynchronize(g->stream) == hipSuccess;
            }
            if (ran) {
                unsigned long long sum = 0;
                for (int i = 0; i < 16; i++) sum += h[i];
                ok = sum == (unsigned long long)nblocks * nthreads && h[16] != 0u && (h[16] >> NSK_XCDS) == 0u;
            }
            (void)hipFree(d);
        }
        if (!ok && getenv("NSK_VERBOSE")) fprintf(stderr, "[nsk] XCD-private accumulators: self-test failed, one shared copy\n");
    }
    verdict[g->device] = ok;
    return ok;
}

// narrow int32 host values to the device value type (int8 / int32) and upload
static int upload_values(nsk_graph *g, void *dst, const int32_t *src, size_t n) {
    if (g->c.vbytes == 4) {
        if (n) HIPCHECK(hipMemcpyAsync(dst, src, n * 4, hipMemcpyHostToDevice, g->stream));
        HIPCHECK(hipStreamSynchronize(g->stream));
        return NSK_OK;
    }
    std::vector<int8_t> tmp(n);
    for (size_t i = 0; i < n; i++) tmp[i] = (int8_t)src[i];
    if (n) HIPCHECK(hipMemcpyAsync(dst, tmp.data(), n, hipMemcpyHostToDevice, g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    return NSK_OK;
}

static void mt_seed_numpy(MTState &s, uint32_t seed) {      // np.random.seed(int): init_genrand
    s.mt[0] = seed;
    for (int i = 1; i < 624; i++) s.mt[i] = 1812433253u * (s.mt[i - 1] ^ (s.mt[i - 1] >> 30)) + (uint32_t)i;
    s.idx = 624;
}

static void mt_seed_python(MTState &s, uint64_t seed) {     // random.seed(int): init_by_array
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    int keylen = key[1] ? 2 : 1;
    mt_seed_numpy(s, 19650218u);
    int i = 1, j = 0;
    for (int k = 624; k; k--) {
        s.mt[i] = (s.mt[i] ^ ((s.mt[i - 1] ^ (s.mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
        i++; j++;
        if (i >= 624) { s.mt[0] = s.mt[623]; i = 1; }
        if (j >= keylen) j = 0;
    }
    for (int k = 623; k; k--) {
        s.mt[i] = (s.mt[i] ^ ((s.mt[i - 1] ^ (s.mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
        i++;
        if (i >= 624) { s.mt[0] = s.mt[623]; i = 1; }
    }
    s.mt[0] = 0x80000000u;
    s.idx = 624;
}


extern "C" {

const char *nsk_last_error(void) { return g_err.c_str(); }
const char *nsk_version(void) { return "numbskull_amd 0.1.1 (gfx950)"; }

int nsk_device_count(int *count) {
    if (!count) return fail(NSK_E_INVALID, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(NSK_E_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
    *count = n;
    return NSK_OK;
}

int nsk_graph_destroy(nsk_graph *g) {
    if (!g) return NSK_OK;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    nsk_exchange_release(g);
    for (const NskLedger::Entry &e : g->mem.entries) nsk_free_raw(e.raw);
    for (int k = 0; k < 2; k++) if (g->xfer_host[k]) (void)hipHostFree(g->xfer_host[k]);
    if (g->cnt_host) (void)hipHostFree(g->cnt_host);
    nsk_drop_sweep_graph(g);
    if (g->ev0) (void)hipEventDestroy(g->ev0);
    if (g->ev1) (void)hipEventDestroy(g->ev1);
    if (g->own_stream && g->stream) (void)hipStreamDestroy(g->stream);
    for (int i = 0; i < 3; i++) {
        if (g->side[i]) (void)hipStreamDestroy(g->side[i]);
        if (g->ev_join[i]) (void)hipEventDestroy(g->ev_join[i]);
    }
    if (g->ev_fork) (void)hipEventDestroy(g->ev_fork);
    delete g;
    return NSK_OK;
}

// upload the generic-path arrays (once; the ones the log-potential put there already stay, energy_ensure)
int nsk_ensure_generic(nsk_graph *g) {
    if (g->generic_uploaded) return NSK_OK;
    Compiled &c = g->c;
    int rc;
    HIPCHECK(hipSetDevice(g->device));
#define UP(name) do { if (!g->name) { rc = dev_upload(g, &g->name, c.name); if (rc) return rc; } } while (0)
    UP(p_slot); UP(slot_off); UP(fidx); UP(gstream); UP(gs_off);
    UP(f_rec); UP(f_feat); UP(m_rec); UP(v_pos);
#undef UP
    if (!g->v_card) { rc = dev_upload(g, &g->v_card, c.v_card_i); if (rc) return rc; }
    if (c.literal_heads && !g->iid_of_vid) { rc = dev_upload(g, &g->iid_of_vid, c.iid); if (rc) return rc; }
    HIPCHECK(hipStreamSynchronize(g->stream));
    g->generic_uploaded = true;
    return NSK_OK;
}

static int create_impl(const nsk_graph_desc *desc, nsk_graph *g) {
    std::string err;
    const auto t_compile = std::chrono::steady_clock::now();
    int rc = compile_graph(desc, g->c, err);
    if (rc) return fail(rc, err);
    g->compile_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_compile).count();
    g->values_regular = g->chain_regular[0] = g->chain_regular[1] = g->c.values_regular;
    g->rng_tag = (uint32_t)g->c.own_begin;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(NSK_E_DEVICE, "no HIP device available: the Gibbs sweep runs on the GPU only "
                                  "(there is no CPU fallback)");
    if (desc->device < 0 || desc->device >= ndev) return fail(NSK_E_INVALID, "device ordinal out of range");
    g->device = desc->device;
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    g->own_stream = true;
    for (int i = 0; i < 3; i++) {
        HIPCHECK(hipStreamCreateWithFlags(&g->side[i], hipStreamNonBlocking));
        HIPCHECK(hipEventCreateWithFlags(&g->ev_join[i], hipEventDisableTiming));
    }
    HIPCHECK(hipEventCreateWithFlags(&g->ev_fork, hipEventDisableTiming));
    HIPCHECK(hipEventCreate(&g->ev0));
    HIPCHECK(hipEventCreate(&g->ev1));
    Compiled &c = g->c;
#define UP(name) do { rc = dev_upload(g, &g->name, c.name); if (rc) return rc; } while (0)
    if (const char *padn = nsk::diag_env("NSK_ALLOC_PAD"))          // (diagnostic: n tiny allocations in front of the arrays)
        for (int i = 0; i < atoi(padn); i++) { uint32_t *dummy = nullptr; rc = dev_alloc(g, &dummy, 1); if (rc) return rc; }
    UP(p_vid); UP(p_info); UP(p_cnt);
    // the CSR-style arrays serve the generic kernels, the hub waves, the per-lane-header tiles and
    // the sequential validation scan only: a graph that lives entirely in tiles (the Ising grids:
    // 1.4 GB of them at 10M variables) uploads them when the sequential scan is first selected
    {
        bool generic_needed = c.phase_dyn_base.size() > 0 && c.phase_dyn_base.back() > 0;
        for (size_t k = 0; k + 1 < c.phase_start.size(); k++)
            if (c.phase_end[k] > c.phase_fast_end[k]) generic_needed = true;
        if (generic_needed || nsk::diag_env("NSK_EAGER_GENERIC")) { rc = nsk_ensure_generic(g); if (rc) return rc; }
    }
    UP(w_fixed); UP(logtab); UP(adj); UP(seg_aff); UP(seg_wide); UP(wide_exc); UP(hub_desc); UP(hub_adj); UP(ep_desc); UP(ep_adj); UP(ep_wrow); UP(ep_kstat); UP(bighub_pos); UP(tiles); UP(tile_hdr); UP(dyn_tiles); UP(rest_tiles); UP(learn_rest_tiles); UP(tile_wrow);
#undef UP
    // (value windows, -DNSK_EP_WIN builds only: no allocation otherwise -- the default build's sequence of device
    // allocations is round 4's, address for address)
    if (!c.ep_win.empty()) {
        rc = dev_upload(g, &g->ep_win, c.ep_win); if (rc) return rc;
        rc = dev_upload(g, &g->ep_win_off, c.ep_win_off); if (rc) return rc;
    }
    rc = dev_upload(g, &g->w, c.w_init); if (rc) return rc;
    if (c.ndirect > 0) {
        rc = dev_upload(g, &g->w_direct, c.w_direct); if (rc) return rc;
        rc = dev_upload(g, &g->multi_wids, c.multi_wids); if (rc) return rc;
    }
    const size_t nvar = (size_t)c.nvar, npos = (size_t)c.npos, vb = (size_t)c.vbytes, nid = (size_t)c.nid;
    uint8_t *tmp = nullptr;
    rc = dev_alloc(g, &tmp, npos * vb); if (rc) return rc; g->p_init = tmp;
    // (+ 16 bytes with value windows: they are copied in whole 16-byte chunks)
    const size_t vpad = c.ep_win.empty() ? 0 : 16;
    rc = dev_alloc(g, &tmp, nid * vb + vpad + 16); if (rc) return rc; g->val = tmp;      // (+ 16: k_unpack_tally walks 16-byte chunks)
    rc = dev_alloc(g, &tmp, nid * vb + vpad + 16); if (rc) return rc; g->val_evid = tmp;
    rc = upload_values(g, g->p_init, c.p_init.data(), npos); if (rc) return rc;
    {   // values live at internal ids (padding positions hold 0 and are never read as a variable)
        std::vector<int32_t> init_i(nid, 0);
        for (size_t v = 0; v < nvar; v++) init_i[c.iid[v]] = c.v_init[v];
        rc = upload_values(g, g->val, init_i.data(), nid); if (rc) return rc;
        rc = upload_values(g, g->val_evid, init_i.data(), nid); if (rc) return rc;
    }
    rc = dev_alloc(g, &g->cnt, (size_t)c.ncount); if (rc) return rc;
    rc = dev_alloc(g, &g->cnt_total, (size_t)c.ncount); if (rc) return rc;
    rc = dev_alloc(g, &g->cnt_pos, (size_t)c.npos + 16); if (rc) return rc;
    rc = dev_alloc(g, &g->prog_w, 2 * c.tile_hdr.size()); if (rc) return rc;
    rc = dev_alloc(g, &g->adj_wt, (size_t)c.nwrows * 64); if (rc) return rc;
    rc = dev_alloc(g, &g->ztab, (size_t)c.nztab); if (rc) return rc;
    rc = dev_alloc(g, &g->ep_wt, (size_t)(c.ep_wrow.empty() ? 0 : c.ep_wrow.back()) * 64); if (rc) return rc;
    rc = dev_alloc(g, &g->sink, 1024); if (rc) return rc;
    if (getenv("NSK_VERBOSE"))
        fprintf(stderr, "[nsk] device arrays: val %p val_evid %p cnt_pos %p seg_aff %p adj %p ztab %p p_init %p (mod 2 MB: %zx %zx %zx %zx)\n",
                g->val, g->val_evid, (void *)g->cnt_pos, (void *)g->seg_aff, (void *)g->adj, (void *)g->ztab, g->p_init,
                (size_t)((uintptr_t)g->val & 0x1FFFFF), (size_t)((uintptr_t)g->cnt_pos & 0x1FFFFF), (size_t)((uintptr_t)g->seg_aff & 0x1FFFFF),
                (size_t)((uintptr_t)g->val_evid & 0x1FFFFF));
    {
        std::vector<ZProgDev> zp(c.zprogs.size());
        for (size_t i = 0; i < zp.size(); i++) zp[i] = {c.zprogs[i].prog, c.zprogs[i].nslots, c.zprogs[i].off, 0u};
        rc = dev_upload(g, &g->zprogs, zp); if (rc) return rc;
    }
    g->smallw = c.nweight > 0 && c.nweight <= NSK_SMALLW;
    if (g->smallw) {
        const size_t cells = (size_t)NSK_LEARN_BINS * (size_t)c.nweight;     // binned partial sums
        rc = dev_alloc(g, &g->part_G, cells); if (rc) return rc;
        rc = dev_alloc(g, &g->part_K, cells); if (rc) return rc;
        rc = dev_alloc(g, &g->part_T, cells); if (rc) return rc;
        HIPCHECK(hipMemsetAsync(g->part_G, 0, cells * sizeof(long long), g->stream));
        HIPCHECK(hipMemsetAsync(g->part_K, 0, cells * sizeof(uint32_t), g->stream));
        HIPCHECK(hipMemsetAsync(g->part_T, 0, cells * sizeof(uint32_t), g->stream));
    }
    HIPCHECK(hipMemsetAsync(g->cnt_pos, 0, (size_t)c.npos + 16, g->stream));
    // global learning accumulators: one private copy per XCD (nsk_device.h sink_add); graphs with few
    // weights accumulate in LDS and never touch them.  A private copy pays while it stays in its XCD's L2
    // (4 MB): up to 2^18 weights (2 MB of sums).  Beyond, the adds miss the L2 either way and eight copies only
    // multiply the update launch's reads -- 50M LR graph, 10^6 weights (tools/sessions/history/r4_s22.sh): eight copies
    // 5.22e9 updates/s, one copy with agent-scope adds 5.47e9; 5M LR graph, 10^5 weights: copies 262 us per
    // class against 300.
    g->acc_copies = (!g->smallw && c.nweight <= (1 << 18)) ? NSK_XCDS : 1;
    {   // the XCD-private copies rely on global atomics executing in the issuing XCD's own L2 and on
        // HW_REG_XCC_ID (nsk_device.h sink_add): true on gfx942 / gfx950 -- and checked once per device by
        // xcd_private_ok -- so any other architecture, a failed check (or NSK_DIAG=1 NSK_ONE_ACC=1) keeps
        // ONE copy updated with agent-scope atomics
        const bool known = xcd_private_ok(g);
        if (!known || nsk::diag_env("NSK_ONE_ACC")) g->acc_copies = 1;
        g->bins_xcd = (known && !nsk::diag_env("NSK_ONE_ACC")) ? 1 : 0;
    }
    const size_t nacc = (size_t)g->acc_copies * (size_t)(c.nweight ? c.nweight : 1);
    rc = dev_alloc(g, &g->G, nacc); if (rc) return rc;
    rc = dev_alloc(g, &g->K, nacc); if (rc) return rc;
    rc = dev_alloc(g, &g->T, nacc); if (rc) return rc;
    rc = dev_alloc(g, &g->clip_count, 1); if (rc) return rc;
    rc = dev_alloc(g, &g->d_counters, 4); if (rc) return rc;
    HIPCHECK(hipMemsetAsync(g->clip_count, 0, sizeof(unsigned int), g->stream));
    rc = dev_alloc(g, &g->mt_np, 1); if (rc) return rc;
    rc = dev_alloc(g, &g->mt_py, 1); if (rc) return rc;
    HIPCHECK(hipMemsetAsync(g->cnt, 0, (c.ncount ? c.ncount : 1) * sizeof(int32_t), g->stream));
    HIPCHECK(hipMemsetAsync(g->cnt_total, 0, (c.ncount ? c.ncount : 1) * sizeof(long long), g->stream));
    HIPCHECK(hipMemsetAsync(g->G, 0, nacc * sizeof(long long), g->stream));
    HIPCHECK(hipMemsetAsync(g->K, 0, nacc * sizeof(uint32_t), g->stream));
    HIPCHECK(hipMemsetAsync(g->T, 0, nacc * sizeof(uint32_t), g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    return nsk_set_seed(g, 0, 0);
}

int nsk_graph_create(const nsk_graph_desc *desc, nsk_graph **out) {
    if (!desc || !out) return fail(NSK_E_INVALID, "null argument");
    *out = nullptr;
    nsk_graph *g = new nsk_graph();
    int rc = create_impl(desc, g);
    if (rc) {
        std::string keep = g_err;
        nsk_graph_destroy(g);
        g_err = keep;
        return rc;
    }
    *out = g;
    return NSK_OK;
}

int nsk_set_seed(nsk_graph *g, uint64_t seed, uint64_t sweep0) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    HIPCHECK(hipSetDevice(g->device));
    g->seed = seed;
    g->sweep = sweep0;
    MTState a, b;
    mt_seed_numpy(a, (uint32_t)seed);
    mt_seed_python(b, seed);
    HIPCHECK(hipMemcpyAsync(g->mt_np, &a, sizeof(MTState), hipMemcpyHostToDevice, g->stream));
    HIPCHECK(hipMemcpyAsync(g->mt_py, &b, sizeof(MTState), hipMemcpyHostToDevice, g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    return NSK_OK;
}

int nsk_set_rng_tag(nsk_graph *g, uint32_t tag) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    g->rng_tag = tag;
    return NSK_OK;
}

int nsk_set_learn_cap(nsk_graph *g, double cap) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (cap != cap) return fail(NSK_E_INVALID, "cap is NaN");
    g->learn_cap = cap;
    return NSK_OK;
}

int nsk_set_learn_lag(nsk_graph *g, int lag) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    g->learn_lag = lag != 0;
    return NSK_OK;
}

int nsk_set_scan(nsk_graph *g, int scan) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (scan != NSK_SCAN_CHROMATIC && scan != NSK_SCAN_SEQUENTIAL) return fail(NSK_E_INVALID, "unknown scan order");
    if (scan == NSK_SCAN_SEQUENTIAL && (g->c.own_begin != 0 || g->c.own_end != g->c.nvar))
        return fail(NSK_E_INVALID, "sequential scan needs the whole graph on one handle");
    if (scan == NSK_SCAN_SEQUENTIAL) NSK_ONE_CHAIN(g, "nsk_set_scan(NSK_SCAN_SEQUENTIAL)");
    if (scan == NSK_SCAN_SEQUENTIAL) { int rc = nsk_ensure_generic(g); if (rc) return rc; }
    g->scan = scan;
    return NSK_OK;
}

int nsk_set_stream(nsk_graph *g, void *hip_stream) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    if (g->own_stream) { HIPCHECK(hipStreamDestroy(g->stream)); g->own_stream = false; }
    g->stream = (hipStream_t)hip_stream;
    return NSK_OK;
}

int nsk_synchronize(nsk_graph *g) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    HIPCHECK(hipSetDevice(g->device));
    { int frc = nsk_p2p_flush(g); if (frc) return frc; }
    HIPCHECK(hipStreamSynchronize(g->stream));
    return NSK_OK;
}

}  // extern "C"

// the fast path reads weights through prog_w: rebuild it whenever weights may have changed (start
// of every sweep call -- the host may have written the weight buffer -- and after every update)
void nsk_refresh_ztab(nsk_graph *g, int set, hipStream_t st) {
    if (!g->c.zprogs.empty())
        k_refresh_ztab<<<dim3((unsigned)g->c.zprogs.size()), dim3(NSK_BLOCK), 0, st ? st : g->stream>>>(
            g->zprogs, g->tile_hdr, set ? g->prog_w1 : g->prog_w, set ? g->ztab1 : g->ztab);
}

int nsk_ensure_lag_sets(nsk_graph *g) {
    if (g->G1) return NSK_OK;
    const Compiled &c = g->c;
    int rc;
    HIPCHECK(hipSetDevice(g->device));
    if ((rc = dev_alloc(g, &g->w1, (size_t)c.nweight))) return rc;
    if ((rc = dev_alloc(g, &g->prog_w1, 2 * c.tile_hdr.size()))) return rc;
    if ((rc = dev_alloc(g, &g->ztab1, (size_t)c.nztab))) return rc;
    if (g->smallw) {
        const size_t cells = (size_t)NSK_LEARN_BINS * (size_t)c.nweight;
        if ((rc = dev_alloc(g, &g->part_G1, cells))) return rc;
        if ((rc = dev_alloc(g, &g->part_K1, cells))) return rc;
        if ((rc = dev_alloc(g, &g->part_T1, cells))) return rc;
        HIPCHECK(hipMemsetAsync(g->part_G1, 0, cells * sizeof(long long), g->stream));
        HIPCHECK(hipMemsetAsync(g->part_K1, 0, cells * sizeof(uint32_t), g->stream));
        HIPCHECK(hipMemsetAsync(g->part_T1, 0, cells * sizeof(uint32_t), g->stream));
    }
    const size_t nacc = (size_t)g->acc_copies * (size_t)(c.nweight ? c.nweight : 1);
    if ((rc = dev_alloc(g, &g->G1, nacc))) return rc;
    if ((rc = dev_alloc(g, &g->K1, nacc))) return rc;
    if ((rc = dev_alloc(g, &g->T1, nacc))) return rc;
    HIPCHECK(hipMemsetAsync(g->G1, 0, nacc * sizeof(long long), g->stream));
    HIPCHECK(hipMemsetAsync(g->K1, 0, nacc * sizeof(uint32_t), g->stream));
    HIPCHECK(hipMemsetAsync(g->T1, 0, nacc * sizeof(uint32_t), g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    return NSK_OK;
}

void nsk_refresh_prog_weights(nsk_graph *g, bool force) {
    if (!force && !g->weights_dirty && !g->weights_exposed) return;
    g->weights_dirty = false;
    const int n = (int)g->c.tile_hdr.size();
    if (n > 0 && g->c.nfast > 0 && g->c.nweight > 0) {
        k_refresh_prog_weights<<<dim3((n + NSK_BLOCK - 1) / NSK_BLOCK), dim3(NSK_BLOCK), 0, g->stream>>>(
            g->tile_hdr, g->w, g->prog_w, n);
        nsk_refresh_ztab(g);
    }
    const int neg = (int)g->c.ep_wrow.size() - 1;
    if (neg > 0 && !g->adj_wt_skip)          // materialised weights of the entry-parallel groups (inference)
        k_refresh_ep_weights<<<dim3((unsigned)neg), dim3(NSK_BLOCK), 0, g->stream>>>(
            (const uint4 *)g->ep_desc, g->ep_adj, g->ep_wrow, g->w, g->ep_wt);
    const int nt = (int)(g->c.tiles.size() / 4) - 1;
    if (g->c.nwrows > 0 && nt > 0 && !g->adj_wt_skip)
        k_refresh_shape_weights<<<dim3((nt + 3) / 4), dim3(NSK_BLOCK), 0, g->stream>>>(
            (const uint4 *)g->tiles, (const uint4 *)g->adj, g->tile_hdr, g->tile_wrow, g->w, g->adj_wt, nt);
}

// the tally a packed-mode sweep sequence left inside the value bytes (nsk_gibbs.hip pack_tally) back into cnt_pos
int nsk_unpack_tally(nsk_graph *g) {
    if (g->packed_sweeps == 0) return NSK_OK;
    const long long n16 = ((long long)g->c.npos + 15) / 16;
    if (n16 > 0)
        k_unpack_tally<<<dim3((unsigned)((n16 + NSK_BLOCK - 1) / NSK_BLOCK)), dim3(NSK_BLOCK), 0, g->stream>>>((uint4 *)g->val, (uint4 *)g->cnt_pos, n16);
    g->packed_sweeps = 0;
    return NSK_OK;
}

int nsk_fold_position_tally(nsk_graph *g) {
    if (g->nchains > 1 && !g->chain_swapped) {          // every chain's tally (they sweep in step)
        const int pts = g->pos_tally_sweeps;
        for (int r = 0; r < g->nchains; r++) { ChainSwap cs(g, r); g->pos_tally_sweeps = pts; (void)nsk_fold_position_tally(g); }
        g->pos_tally_sweeps = 0;
        return NSK_OK;
    }
    (void)nsk_unpack_tally(g);
    const int np = (int)g->c.npos;
    if (np > 0 && g->c.nfast > 0 && g->pos_tally_sweeps > 0)
        k_fold_counts_pos<<<dim3((np + NSK_BLOCK - 1) / NSK_BLOCK), dim3(NSK_BLOCK), 0, g->stream>>>(
            g->cnt_pos, g->p_cnt, g->p_vid, g->cnt_total, np);
    g->pos_tally_sweeps = 0;
    return NSK_OK;
}

extern "C" {

static int fold_counts(nsk_graph *g) {
    if (!g->cnt_dirty) return NSK_OK;
    const int n = (int)g->c.ncount;
    for (int r = 0; r < g->nchains; r++)
        if (n > 0)
            k_fold_counts<<<dim3((n + NSK_BLOCK - 1) / NSK_BLOCK), dim3(NSK_BLOCK), 0, g->stream>>>(
                g->cnt + (size_t)r * (size_t)n, g->cnt_total + (size_t)r * (size_t)n, n);
    nsk_fold_position_tally(g);
    HIPCHECK(hipGetLastError());
    g->cnt_dirty = false;
    return NSK_OK;
}

}  // extern "C"



static int xfer_ensure(nsk_graph *g) {
    if (g->xfer_dev) return NSK_OK;
    const size_t bytes = (size_t)std::max<int64_t>(g->c.nvar, 1) * (size_t)g->c.vbytes;
    // (non-coherent = cacheable on the host: the host threads READ these buffers after a download, and reads of
    //  the default, uncached mapping ran at ~1 GB/s)
    for (int k = 0; k < 2; k++) HIPCHECK(hipHostMalloc(&g->xfer_host[k], bytes, hipHostMallocNonCoherent));
    uint8_t *t = nullptr;
    int rc = dev_alloc(g, &t, bytes);
    if (rc) return rc;
    g->xfer_dev = t;
    if (g->iid_of_vid) { g->xfer_iid = g->iid_of_vid; return NSK_OK; }
    return dev_upload(g, &g->xfer_iid, g->c.iid);
}

// validate the caller's int64 values and narrow them to the device value type, in the caller's order
// (host threads over index blocks); bad: 0 fine, 1 a value does not fit the value type; *regular: every
// value lies in [0, cardinality)
template <typename VT>
static void narrow_values(const nsk_graph *g, const int64_t *src, VT *dst, int *bad, bool *regular) {
    const int64_t lo = sizeof(VT) == 1 ? -128 : INT32_MIN, hi = sizeof(VT) == 1 ? 127 : INT32_MAX;
    const int32_t *card = g->c.v_card.data();
    std::vector<int> tbad((size_t)nsk::compile_threads(), 0), tirr((size_t)nsk::compile_threads(), 0);
    nsk::parallel_for(g->c.nvar, [&](int64_t b0, int64_t b1, int t) {
        int bd = 0, ir = 0;
        for (int64_t i = b0; i < b1; i++) {
            const int64_t x = src[i];
            bd |= (x < lo || x > hi) ? 1 : 0;
            ir |= (x < 0 || x >= (int64_t)card[i]) ? 1 : 0;
            dst[i] = (VT)x;
        }
        tbad[(size_t)t] = bd; tirr[(size_t)t] = ir;
    });
    *bad = 0; *regular = true;
    for (int x : tbad) *bad |= x;
    for (int x : tirr) if (x) *regular = false;
}

template <typename VT>
static void narrow_values_unchecked(const nsk_graph *g, const int64_t *src, VT *dst) {
    nsk::parallel_for(g->c.nvar, [&](int64_t b0, int64_t b1, int) { for (int64_t i = b0; i < b1; i++) dst[i] = (VT)src[i]; });
}

extern "C" {


int nsk_state_upload(nsk_graph *g, const int64_t *var_value, const int64_t *var_value_evid,
                     const double *weight_value, const int64_t *count) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    HIPCHECK(hipSetDevice(g->device));
    { int frc = nsk_p2p_flush(g); if (frc) return frc; }
    const int64_t nvar = g->c.nvar;
    const size_t vb = (size_t)g->c.vbytes;
    const int64_t *srcs[2] = {var_value, var_value_evid};
    void *dsts[2] = {g->val, g->val_evid};
    if ((var_value || var_value_evid) && nvar) {
        int rc = xfer_ensure(g);
        if (rc) return rc;
        // validate BOTH chains before anything is copied: an error must leave the device state as it was
        bool regular[2] = {g->chain_regular[0], g->chain_regular[1]};
        for (int k = 0; k < 2; k++) {
            if (!srcs[k]) continue;
            int bad = 0;
            bool reg = true;
            if (vb == 1) narrow_values<int8_t>(g, srcs[k], (int8_t *)g->xfer_host[k], &bad, &reg);
            else narrow_values<int32_t>(g, srcs[k], (int32_t *)g->xfer_host[k], &bad, &reg);
            if (bad) return fail(NSK_E_RANGE, "variable value does not fit the device value type");
            // UFO (inference.py:398-405) uses the first member's value as an index into the factor's
            // member list: the reference reads a neighbouring factor's edge (or faults); refuse
            if (!reg && g->c.has_ufo)
                return fail(NSK_E_RANGE, "a variable value lies outside its domain on a graph with UFO factors "
                                         "(the value indexes the factor's member list)");
            regular[k] = reg;
        }
        const int nb = (int)std::min<int64_t>(4096, (nvar + NSK_BLOCK - 1) / NSK_BLOCK);
        for (int k = 0; k < 2; k++) {
            if (!srcs[k]) continue;
            g->chain_regular[k] = regular[k];
            g->values_regular = g->chain_regular[0] && g->chain_regular[1] && g->chains_regular;
            HIPCHECK(hipMemcpyAsync(g->xfer_dev, g->xfer_host[k], (size_t)nvar * vb, hipMemcpyHostToDevice, g->stream));
            if (vb == 1) k_state_scatter<int8_t><<<dim3(nb), dim3(NSK_BLOCK), 0, g->stream>>>((int8_t *)dsts[k], g->xfer_iid, (const int8_t *)g->xfer_dev, nvar);
            else k_state_scatter<int32_t><<<dim3(nb), dim3(NSK_BLOCK), 0, g->stream>>>((int32_t *)dsts[k], g->xfer_iid, (const int32_t *)g->xfer_dev, nvar);
        }
    }
    if (weight_value && g->c.nweight) {
        const double *src = weight_value;
        if (!g->c.wuser.empty()) {      // the device table is in slot order (nsk_compile.h wmap)
            g->w_stage.resize((size_t)g->c.nweight);
            const int32_t *wuser = g->c.wuser.data();
            double *st = g->w_stage.data();
            nsk::parallel_for(g->c.nweight, [&](int64_t b0, int64_t b1, int) { for (int64_t i = b0; i < b1; i++) st[i] = weight_value[wuser[i]]; });
            src = st;
        }
        HIPCHECK(hipMemcpyAsync(g->w, src, (size_t)g->c.nweight * sizeof(double), hipMemcpyHostToDevice, g->stream));
        if (src != weight_value) HIPCHECK(hipStreamSynchronize(g->stream));
        g->weights_dirty = true;
    }
    if (count && g->c.ncount) {
        if (g->nchains > 1) { int rc = fold_counts(g); if (rc) return rc; }     // (the other chains' tallies stay theirs)
        HIPCHECK(hipMemcpyAsync(g->cnt_total, count, (size_t)g->c.ncount * sizeof(int64_t), hipMemcpyHostToDevice, g->stream));
        HIPCHECK(hipMemsetAsync(g->cnt, 0, (size_t)g->c.ncount * sizeof(int32_t), g->stream));
        if (g->c.npos) HIPCHECK(hipMemsetAsync(g->cnt_pos, 0, (size_t)g->c.npos, g->stream));
        g->pos_tally_sweeps = 0;
        g->cnt_dirty = false;
    }
    HIPCHECK(hipStreamSynchronize(g->stream));
    return NSK_OK;
}

// device values of one chain -> the caller's int64 array: gather into the caller's order on the device, one
// narrow copy over PCIe, widened by the host threads (internal, not in the public header: nsk_temper.hip downloads its
// kept states through it)
int nsk_download_values(nsk_graph *g, const void *src, int64_t *dst, int k) {
    const int64_t nvar = g->c.nvar;
    if (!nvar) return NSK_OK;
    int rc = xfer_ensure(g);
    if (rc) return rc;
    const size_t vb = (size_t)g->c.vbytes;
    const int nb = (int)std::min<int64_t>(4096, (nvar + NSK_BLOCK - 1) / NSK_BLOCK);
    if (vb == 1) k_state_gather<int8_t><<<dim3(nb), dim3(NSK_BLOCK), 0, g->stream>>>((const int8_t *)src, g->xfer_iid, (int8_t *)g->xfer_dev, nvar);
    else k_state_gather<int32_t><<<dim3(nb), dim3(NSK_BLOCK), 0, g->stream>>>((const int32_t *)src, g->xfer_iid, (int32_t *)g->xfer_dev, nvar);
    HIPCHECK(hipMemcpyAsync(g->xfer_host[k], g->xfer_dev, (size_t)nvar * vb, hipMemcpyDeviceToHost, g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    const void *h = g->xfer_host[k];
    nsk::parallel_for(nvar, [&](int64_t b0, int64_t b1, int) {
        if (vb == 1) for (int64_t i = b0; i < b1; i++) dst[i] = ((const int8_t *)h)[i];
        else for (int64_t i = b0; i < b1; i++) dst[i] = ((const int32_t *)h)[i];
    });
    return NSK_OK;
}

int nsk_state_download(nsk_graph *g, int64_t *var_value, int64_t *var_value_evid, double *weight_value,
                       int64_t *count) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    HIPCHECK(hipSetDevice(g->device));
    { int frc = nsk_p2p_flush(g); if (frc) return frc; }
    int rc;
    if (var_value && (rc = nsk_download_values(g, g->val, var_value, 0))) return rc;
    if (var_value_evid && (rc = nsk_download_values(g, g->val_evid, var_value_evid, 1))) return rc;
    if (weight_value && g->c.nweight) {
        if (!g->c.wuser.empty()) {      // slot order on the device, the caller's order in `weight_value`
            g->w_stage.resize((size_t)g->c.nweight);
            HIPCHECK(hipMemcpyAsync(g->w_stage.data(), g->w, (size_t)g->c.nweight * sizeof(double), hipMemcpyDeviceToHost, g->stream));
            HIPCHECK(hipStreamSynchronize(g->stream));
            const int32_t *wmap = g->c.wmap.data();
            const double *st = g->w_stage.data();
            nsk::parallel_for(g->c.nweight, [&](int64_t b0, int64_t b1, int) { for (int64_t i = b0; i < b1; i++) weight_value[i] = st[wmap[i]]; });
        } else {
            HIPCHECK(hipMemcpyAsync(weight_value, g->w, (size_t)g->c.nweight * sizeof(double), hipMemcpyDeviceToHost, g->stream));
        }
    }
    if (count) {
        if ((rc = fold_counts(g))) return rc;
        const int64_t nc = g->c.ncount;
        bool done = false;
        if (nc >= (1 << 16)) {          // large tallies cross PCIe as int32 (pinned staging, widened by the host threads)
            if (!g->cnt_dev32) {
                HIPCHECK(hipHostMalloc(&g->cnt_host, (size_t)nc * 4, hipHostMallocNonCoherent));
                if ((rc = dev_alloc(g, &g->cnt_dev32, (size_t)nc))) return rc;
                if ((rc = dev_alloc(g, &g->cnt_wide, 1))) return rc;
            }
            unsigned int wide = 0;
            HIPCHECK(hipMemsetAsync(g->cnt_wide, 0, sizeof(unsigned int), g->stream));
            k_count_narrow<<<dim3((unsigned)std::min<int64_t>(4096, (nc + NSK_BLOCK - 1) / NSK_BLOCK)), dim3(NSK_BLOCK), 0, g->stream>>>(
                g->cnt_total, g->cnt_dev32, nc, g->cnt_wide);
            HIPCHECK(hipMemcpyAsync(g->cnt_host, g->cnt_dev32, (size_t)nc * 4, hipMemcpyDeviceToHost, g->stream));
            HIPCHECK(hipMemcpyAsync(&wide, g->cnt_wide, sizeof(wide), hipMemcpyDeviceToHost, g->stream));
            HIPCHECK(hipStreamSynchronize(g->stream));
            if (!wide) {
                const int32_t *h32 = (const int32_t *)g->cnt_host;
                nsk::parallel_for(nc, [&](int64_t b0, int64_t b1, int) { for (int64_t i = b0; i < b1; i++) count[i] = h32[i]; });
                done = true;
            }
        }
        if (!done && nc)
            HIPCHECK(hipMemcpyAsync(count, g->cnt_total, (size_t)nc * sizeof(int64_t), hipMemcpyDeviceToHost, g->stream));
    }
    // a peer-to-peer exchange that timed out since the last check left ghost values (and merged weights)
    // incomplete: the state handed back is then not a result -- say so here too, not only in nsk_p2p_check
    unsigned int p2p_err = 0;
    if (g->p2p.err) HIPCHECK(hipMemcpyAsync(&p2p_err, g->p2p.err, sizeof(p2p_err), hipMemcpyDeviceToHost, g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    if (p2p_err) {
        HIPCHECK(hipMemsetAsync(g->p2p.err, 0, sizeof(unsigned int), g->stream));          // reported once
        return fail(NSK_E_DEVICE, "peer-to-peer exchange: a peer's boundary values did not arrive within "
                                  "NSK_P2P_TIMEOUT_S; the downloaded state is incomplete");
    }
    return NSK_OK;
}

// ---- several chains (nsk_set_chains) ---------------------------------------------------------------------------
int nsk_set_chains(nsk_graph *g, int nchains) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (nchains < 1 || nchains > NSK_MAX_CHAINS) return fail(NSK_E_INVALID, "nsk_set_chains: the chain count must lie in [1, 1024]");
    if (nchains == g->nchains) return NSK_OK;
    NSK_NO_TRACE(g, "nsk_set_chains with another count");       // (its rows hold one share per chain)
    if (nchains > 1) {
        if (g->scan != NSK_SCAN_CHROMATIC) return fail(NSK_E_INVALID, "several chains: the sequential scan samples one chain");
        if ((g->c.flags & NSK_FLAG_PARTITION) || g->c.own_begin != 0 || g->c.own_end != g->c.nvar)
            return fail(NSK_E_INVALID, "several chains: the handle must own the whole graph (no own_range / NSK_FLAG_PARTITION)");
        if (g->gather.world > 0 || g->p2p.world > 0 || g->gather.comm)
            return fail(NSK_E_INVALID, "several chains: the handle exchanges a boundary (exchange, RCCL or peer-to-peer set up)");
    }
    HIPCHECK(hipSetDevice(g->device));
    int rc = fold_counts(g);                 // every tally in its master: the chains keep them across the move
    if (rc) return rc;
    const Compiled &c = g->c;
    const size_t vb = (size_t)c.vbytes, nid = (size_t)c.nid, npos = (size_t)c.npos, nc = (size_t)c.ncount;
    const size_t vpad = c.ep_win.empty() ? 0 : 16;
    const size_t half = (std::max(nid * vb + vpad + 16, npos + 16) + 255) / 256 * 256;     // values | position tally
    const size_t stride = 2 * half, R = (size_t)nchains;
    if (stride / 256 * (R - 1) >= ((size_t)1 << 31)) return fail(NSK_E_NOMEM, "nsk_set_chains: the chains' state does not fit");
    uint8_t *slab = nullptr;
    int32_t *cnt = nullptr;
    long long *tot = nullptr;
    NskRollback rb(g->mem, nsk_free_raw);       // (an early return below leaves none of the three behind)
    if ((rc = dev_alloc(g, &slab, R * stride))) return rc;
    if ((rc = dev_alloc(g, &cnt, R * std::max<size_t>(nc, 1)))) return rc;
    if ((rc = dev_alloc(g, &tot, R * std::max<size_t>(nc, 1)))) return rc;
    HIPCHECK(hipMemsetAsync(slab, 0, R * stride, g->stream));
    HIPCHECK(hipMemsetAsync(cnt, 0, R * std::max<size_t>(nc, 1) * sizeof(int32_t), g->stream));
    HIPCHECK(hipMemsetAsync(tot, 0, R * std::max<size_t>(nc, 1) * sizeof(long long), g->stream));
    // the chains both counts have keep their values and tallies; new ones start as nsk_graph_create leaves a handle
    const int keep = std::min(nchains, g->nchains);
    for (int r = 0; r < keep; r++) {
        const size_t off = (size_t)r * g->chain_stride, o2 = (size_t)r * nc;
        HIPCHECK(hipMemcpyAsync(slab + (size_t)r * stride, (char *)g->val + off, nid * vb + vpad + 16, hipMemcpyDeviceToDevice, g->stream));
        if (nc) HIPCHECK(hipMemcpyAsync(tot + (size_t)r * nc, g->cnt_total + o2, nc * sizeof(long long), hipMemcpyDeviceToDevice, g->stream));
    }
    bool regular = keep > 1 ? g->chains_regular : true;
    if (nchains > keep) {
        std::vector<int32_t> init_i(nid, 0);
        for (size_t v = 0; v < (size_t)c.nvar; v++) init_i[c.iid[v]] = c.v_init[v];
        for (int r = keep; r < nchains; r++)
            if ((rc = upload_values(g, slab + (size_t)r * stride, init_i.data(), nid))) return rc;
        regular = regular && c.values_regular;
    }
    HIPCHECK(hipStreamSynchronize(g->stream));
    rb.commit();
    // the arrays of the previous layout go (a one-chain handle's first call frees the ones nsk_graph_create made)
    dev_free(g, g->val); dev_free(g, g->cnt); dev_free(g, g->cnt_total);
    if (!g->chain_stride) dev_free(g, g->cnt_pos);                  // (inside the old slab once the chain count was set)
    g->val = slab; g->cnt_pos = slab + half; g->cnt = cnt; g->cnt_total = tot;
    g->chain_stride = stride;
    g->nchains = nchains;
    g->chains_regular = nchains > 1 ? regular : true;
    g->values_regular = g->chain_regular[0] && g->chain_regular[1] && g->chains_regular;
    g->pos_tally_sweeps = 0;
    g->cnt_dirty = false;
    g->seg_plans_valid = false;                  // (the plans check the arrays' offsets from the value array)
    nsk_drop_sweep_graph(g);                // (captured launches hold the old arrays' addresses)
    return NSK_OK;
}

int nsk_get_chains(nsk_graph *g) { return g ? g->nchains : 0; }

int nsk_chains_upload(nsk_graph *g, const int64_t *var_value, const int64_t *count) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    HIPCHECK(hipSetDevice(g->device));
    const int64_t nvar = g->c.nvar;
    const size_t vb = (size_t)g->c.vbytes, R = (size_t)g->nchains, nc = (size_t)g->c.ncount;
    if (var_value && nvar) {
        int rc = xfer_ensure(g);
        if (rc) return rc;
        // validate every chain before anything is copied: an error leaves the device state as it was
        bool reg_rest = true, reg0 = true;
        for (size_t r = 0; r < R; r++) {
            int bad = 0;
            bool reg = true;
            if (vb == 1) narrow_values<int8_t>(g, var_value + r * (size_t)nvar, (int8_t *)g->xfer_host[0], &bad, &reg);
            else narrow_values<int32_t>(g, var_value + r * (size_t)nvar, (int32_t *)g->xfer_host[0], &bad, &reg);
            if (bad) return fail(NSK_E_RANGE, "variable value does not fit the device value type");
            if (!reg && g->c.has_ufo)
                return fail(NSK_E_RANGE, "a variable value lies outside its domain on a graph with UFO factors "
                                         "(the value indexes the factor's member list)");
            if (r == 0) reg0 = reg; else reg_rest = reg_rest && reg;
        }
        const int nb = (int)std::min<int64_t>(4096, (nvar + NSK_BLOCK - 1) / NSK_BLOCK);
        for (size_t r = 0; r < R; r++) {
            if (vb == 1) narrow_values_unchecked<int8_t>(g, var_value + r * (size_t)nvar, (int8_t *)g->xfer_host[0]);
            else narrow_values_unchecked<int32_t>(g, var_value + r * (size_t)nvar, (int32_t *)g->xfer_host[0]);
            void *dst = (char *)g->val + r * g->chain_stride;
            HIPCHECK(hipMemcpyAsync(g->xfer_dev, g->xfer_host[0], (size_t)nvar * vb, hipMemcpyHostToDevice, g->stream));
            if (vb == 1) k_state_scatter<int8_t><<<dim3(nb), dim3(NSK_BLOCK), 0, g->stream>>>((int8_t *)dst, g->xfer_iid, (const int8_t *)g->xfer_dev, nvar);
            else k_state_scatter<int32_t><<<dim3(nb), dim3(NSK_BLOCK), 0, g->stream>>>((int32_t *)dst, g->xfer_iid, (const int32_t *)g->xfer_dev, nvar);
            HIPCHECK(hipStreamSynchronize(g->stream));          // (the staging buffer serves the next chain)
        }
        g->chain_regular[0] = reg0;
        if (R > 1) g->chains_regular = reg_rest;
        g->values_regular = g->chain_regular[0] && g->chain_regular[1] && g->chains_regular;
    }
    if (count && nc) {
        int rc = fold_counts(g);
        if (rc) return rc;
        HIPCHECK(hipMemcpyAsync(g->cnt_total, count, R * nc * sizeof(int64_t), hipMemcpyHostToDevice, g->stream));
        HIPCHECK(hipMemsetAsync(g->cnt, 0, R * nc * sizeof(int32_t), g->stream));
        if (g->c.npos)
            for (size_t r = 0; r < R; r++) HIPCHECK(hipMemsetAsync(g->cnt_pos + r * g->chain_stride, 0, (size_t)g->c.npos, g->stream));
        g->pos_tally_sweeps = 0;
        g->cnt_dirty = false;
    }
    HIPCHECK(hipStreamSynchronize(g->stream));
    return NSK_OK;
}

int nsk_chains_download(nsk_graph *g, int64_t *var_value, int64_t *count) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    HIPCHECK(hipSetDevice(g->device));
    const size_t R = (size_t)g->nchains, nc = (size_t)g->c.ncount, nvar = (size_t)g->c.nvar;
    int rc;
    if (var_value)
        for (size_t r = 0; r < R; r++)
            if ((rc = nsk_download_values(g, (const char *)g->val + r * g->chain_stride, var_value + r * nvar, 0))) return rc;
    if (count && nc) {
        if ((rc = fold_counts(g))) return rc;
        HIPCHECK(hipMemcpyAsync(count, g->cnt_total, R * nc * sizeof(int64_t), hipMemcpyDeviceToHost, g->stream));
    }
    HIPCHECK(hipStreamSynchronize(g->stream));
    return NSK_OK;
}

// (have: the tile / group counters when the caller has counted them already, else they are counted here)
static void fill_info(const Compiled &c, nsk_graph_info *info, const RouteCounts *have = nullptr) {
    info->nvar = c.nvar;
    info->nowned = c.nsampled;
    info->ncolors = (int64_t)c.phase_start.size() - 1;
    info->value_bytes = c.vbytes;
    info->device_bytes = 0;
    info->nfast = c.nfast;
    info->ngeneric = c.nsampled - c.nfast;
    info->alg_bytes_inference = c.alg_bytes_inference;
    info->alg_bytes_learning = c.alg_bytes_learning;
    info->sweeps_done = 0;
    info->layout_bytes_inference = c.layout_bytes_inference;
    info->layout_bytes_learning = c.layout_bytes_learning;
    info->ztab_entries = c.nztab;
    info->compile_seconds = 0;
    info->learn_cap = 0.5;
    info->learn_clipped = 0;
    info->grad_shift = c.grad_shift;
    info->acc_copies = 0;
    info->learn_lag = (c.nweight > 0 && c.nweight <= NSK_SMALLW) ? 1 : 0;
    info->direct_weights = c.ndirect;
    info->weight_slots = c.wmap.empty() ? 0 : 1;
    info->layout_hash = getenv("NSK_LAYOUT_HASH") ? layout_hash(c) : 0;
    info->p2p_fused = 0;
    info->tab_quads = c.ntab_quads;
    info->wide_quads = c.nwide_quads;
    info->hubs = 0;
    for (size_t k = 0; k < c.phase_heavy_end.size(); k++)
        for (int64_t p = c.phase_fast_end[k]; p < c.phase_heavy_end[k]; p++) info->hubs += c.p_vid[(size_t)p] >= 0;
    info->hubs_ep = c.nhub_ep;
    info->hubs_block = c.phase_bighub_base.empty() ? 0 : c.phase_bighub_base.back();   // (bighub_pos is padded when empty)
    RouteCounts rc;
    if (have) rc = *have;
    else compiled_routes(c, nullptr, &rc);
    info->tiles_shape = rc.tiles_shape;
    info->tiles_shape_padded = rc.tiles_shape_padded;
    info->tiles_lane = rc.tiles_lane;
    info->tiles_general = rc.tiles_general;
    info->tiles_general_roles = rc.tiles_general_roles;
    info->ep_groups = rc.ep_groups;
    info->ep_groups_two_pass = rc.ep_groups_two_pass;
}

int nsk_graph_get_info(nsk_graph *g, nsk_graph_info *info) {
    if (!g || !info) return fail(NSK_E_INVALID, "null argument");
    if (!g->have_route_counts) { compiled_routes(g->c, nullptr, &g->route_counts); g->have_route_counts = true; }
    fill_info(g->c, info, &g->route_counts);
    info->device_bytes = g->mem.total;
    info->sweeps_done = g->sweeps_done;
    info->learn_cap = g->learn_cap;
    if (g->clip_count) {
        unsigned int n = 0;
        (void)hipSetDevice(g->device);
        (void)hipStreamSynchronize(g->stream);
        if (hipMemcpy(&n, g->clip_count, sizeof(n), hipMemcpyDeviceToHost) == hipSuccess) info->learn_clipped = (int64_t)n;
    }
    info->compile_seconds = g->compile_seconds;
    info->acc_copies = g->acc_copies + (g->bins_xcd ? 16 : 0);
    info->learn_lag = (g->learn_lag && g->smallw) ? 1 : 0;
    info->p2p_fused = g->p2p.fused ? 1 : 0;
    return NSK_OK;
}

int nsk_graph_plan(const nsk_graph_desc *desc, int32_t *color, nsk_graph_info *info) {
    if (!desc) return fail(NSK_E_INVALID, "null argument");
    Compiled c;
    std::string err;
    int rc = compile_graph(desc, c, err);
    if (rc) return fail(rc, err);
    if (color && c.nvar) memcpy(color, c.color.data(), (size_t)c.nvar * sizeof(int32_t));
    if (info) fill_info(c, info);
    return NSK_OK;
}

int nsk_graph_plan_routes(const nsk_graph_desc *desc, int32_t *route) {
    if (!desc || (!route && desc->nvar)) return fail(NSK_E_INVALID, "null argument");
    Compiled c;
    std::string err;
    int rc = compile_graph(desc, c, err);
    if (rc) return fail(rc, err);
    compiled_routes(c, route, nullptr);
    return NSK_OK;
}

int nsk_graph_plan_classes(const nsk_graph_desc *desc, int learning, int regularization, int grid_cap, int32_t *rec, int64_t *nclass) {
    if (!desc || !nclass || grid_cap < 0) return fail(NSK_E_INVALID, "null argument or negative grid cap");
    Compiled c;
    std::string err;
    int rc = compile_graph(desc, c, err);
    if (rc) return fail(rc, err);
    *nclass = c.phase_start.empty() ? 0 : (int64_t)c.phase_start.size() - 1;
    if (!rec) return NSK_OK;
    // what gibbs_impl / nsk_learn_chromatic put into the options (nsk_gibbs.hip, nsk_learn.hip), from the layout alone
    PlanOpts opts;
    opts.overlap = nsk::diag_env("NSK_NO_OVERLAP") == nullptr;
    opts.ep_per_cu = plan_per_cu(nsk::diag_env("NSK_EP_PER_CU"));
    opts.grid_cap = std::min(grid_cap, 1 << 20);
    if (learning) {
        opts.smallw = c.nweight > 0 && c.nweight <= NSK_SMALLW;
        opts.nweight = c.nweight;
        opts.has_kstat = !c.ep_kstat.empty();
        opts.regularization = regularization;
    } else {
        opts.value_bytes = (size_t)c.nid * (size_t)c.vbytes;
    }
    compiled_class_records(c, learning != 0, opts, rec);
    return NSK_OK;
}

int nsk_graph_get_routes(nsk_graph *g, int32_t *route) {
    if (!g || (!route && g->c.nvar)) return fail(NSK_E_INVALID, "null argument");
    compiled_routes(g->c, route, nullptr);
    return NSK_OK;
}

int nsk_graph_plan_needs(const nsk_graph_desc *desc, int64_t *count, int32_t *vids) {
    if (!desc || !count) return fail(NSK_E_INVALID, "null argument");
    Compiled c;
    std::string err;
    int rc = compile_graph(desc, c, err);
    if (rc) return fail(rc, err);
    *count = (int64_t)c.ghost_needs.size();
    if (vids && *count) memcpy(vids, c.ghost_needs.data(), (size_t)*count * sizeof(int32_t));
    return NSK_OK;
}

int nsk_graph_get_layout(nsk_graph *g, int32_t *iid, int64_t *nid) {
    if (!g) return fail(NSK_E_INVALID, "null argument");
    if (iid && g->c.nvar) memcpy(iid, g->c.iid.data(), (size_t)g->c.nvar * sizeof(int32_t));
    if (nid) *nid = g->c.nid;
    return NSK_OK;
}

int nsk_graph_get_generators(nsk_graph *g, int64_t *gen) {
    if (!g || !gen) return fail(NSK_E_INVALID, "null argument");
    const Compiled &c = g->c;
    std::vector<uint8_t> quad((size_t)c.npos, 0);
    for (const Compiled::Segment &sg : c.segments)
        if (sg.ztab >= 0) {
            for (int64_t p = sg.pos0; p < sg.pos0 + (int64_t)sg.ntiles * 64 && p < c.npos; p++) quad[(size_t)p] = 1;
            if (sg.wide < 0) continue;
            const int stride = NSK_WIDE_STRIDE(sg.nslots > 4 ? 2 : 1);
            const int64_t q0 = sg.pos0 >> 8, nq = ((sg.pos0 + 64 * (int64_t)sg.ntiles + 255) >> 8) - q0;
            for (int64_t qi = 0; qi < nq; qi++)
                if (c.seg_wide[(size_t)sg.wide + (size_t)qi * stride] != 0xFFFFFFFFu)
                    for (int64_t p = (q0 + qi) << 8; p < ((q0 + qi + 1) << 8) && p < c.npos; p++) quad[(size_t)p] = 2;
        }
    for (int64_t v = 0; v < c.nvar; v++) {
        const int64_t p = c.color[v] >= 0 ? (int64_t)c.iid[v] : -1;
        const int sch = (p >= 0 && p < c.npos) ? quad[(size_t)p] : 0;
        gen[v] = p < 0 ? -1 : (p | (sch == 1 ? (1ll << 40) : sch == 2 ? (1ll << 41) : 0ll));
    }
    return NSK_OK;
}

int nsk_graph_get_weight_slots(nsk_graph *g, int64_t *slot) {
    if (!g || (!slot && g->c.nweight)) return fail(NSK_E_INVALID, "null argument");
    const Compiled &c = g->c;
    for (int64_t w = 0; w < c.nweight; w++) slot[w] = c.wmap.empty() ? w : (int64_t)c.wmap[(size_t)w];
    return c.wmap.empty() ? 0 : 1;
}

int nsk_graph_get_colors(nsk_graph *g, int32_t *color) {
    if (!g || !color) return fail(NSK_E_INVALID, "null argument");
    if (g->c.nvar) memcpy(color, g->c.color.data(), (size_t)g->c.nvar * sizeof(int32_t));
    return NSK_OK;
}

int nsk_profile_begin(nsk_graph *g) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    HIPCHECK(hipSetDevice(g->device));
    g->launches_at_begin = g->launches;
    HIPCHECK(hipEventRecord(g->ev0, g->stream));
    return NSK_OK;
}

int nsk_profile_end(nsk_graph *g, double *elapsed_ms, int64_t *kernel_launches) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipEventRecord(g->ev1, g->stream));
    HIPCHECK(hipEventSynchronize(g->ev1));
    float ms = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms, g->ev0, g->ev1));
    if (elapsed_ms) *elapsed_ms = (double)ms;
    if (kernel_launches) *kernel_launches = g->launches - g->launches_at_begin;
    return NSK_OK;
}

int nsk_profile_mark(nsk_graph *g) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipEventRecord(g->ev1, g->stream));
    return NSK_OK;
}

int nsk_profile_read(nsk_graph *g, double *elapsed_ms, int64_t *kernel_launches) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipEventSynchronize(g->ev1));
    float ms = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms, g->ev0, g->ev1));
    if (elapsed_ms) *elapsed_ms = (double)ms;
    if (kernel_launches) *kernel_launches = g->launches - g->launches_at_begin;
    return NSK_OK;
}

int nsk_device_buffer(nsk_graph *g, int which, void **ptr, int64_t *nbytes) {
    if (!g || !ptr) return fail(NSK_E_INVALID, "null argument");
    switch (which) {
    case NSK_BUF_VALUE: *ptr = g->val; if (nbytes) *nbytes = g->c.nid * g->c.vbytes; return NSK_OK;
    case NSK_BUF_VALUE_EVID: *ptr = g->val_evid; if (nbytes) *nbytes = g->c.nid * g->c.vbytes; return NSK_OK;
    case NSK_BUF_WEIGHT: *ptr = g->w; if (nbytes) *nbytes = g->c.nweight * 8; g->weights_exposed = true; return NSK_OK;
    case NSK_BUF_SEND: *ptr = g->gather.send; if (nbytes) *nbytes = g->gather.slot * g->c.vbytes; return NSK_OK;
    case NSK_BUF_RECV: *ptr = g->gather.recv; if (nbytes) *nbytes = g->gather.slot * g->c.vbytes * g->gather.world; return NSK_OK;
    case NSK_BUF_SEND_EVID: *ptr = g->gather.send_evid; if (nbytes) *nbytes = g->gather.slot * g->c.vbytes; return NSK_OK;
    case NSK_BUF_RECV_EVID: *ptr = g->gather.recv_evid; if (nbytes) *nbytes = g->gather.slot * g->c.vbytes * g->gather.world; return NSK_OK;
    default: return fail(NSK_E_INVALID, "unknown buffer id");
    }
}

int nsk_selftest_exp(int device, const double *x, double *y, int64_t n) {
    if (n < 0 || (n && (!x || !y))) return fail(NSK_E_INVALID, "bad argument");
    if (n == 0) return NSK_OK;
    HIPCHECK(hipSetDevice(device));
    double *dx = nullptr, *dy = nullptr;
    HIPCHECK(hipMalloc((void **)&dx, n * sizeof(double)));
    HIPCHECK(hipMalloc((void **)&dy, n * sizeof(double)));
    HIPCHECK(hipMemcpy(dx, x, n * sizeof(double), hipMemcpyHostToDevice));
    k_selftest_exp<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(dx, dy, n);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpy(y, dy, n * sizeof(double), hipMemcpyDeviceToHost));
    (void)hipFree(dx); (void)hipFree(dy);
    return NSK_OK;
}

int nsk_selftest_philox(int device, uint64_t seed, uint64_t sweep, uint32_t stream, int64_t n,
                        uint32_t *out) {
    if (n < 0 || (n && !out)) return fail(NSK_E_INVALID, "bad argument");
    if (n == 0) return NSK_OK;
    HIPCHECK(hipSetDevice(device));
    uint32_t *d = nullptr;
    HIPCHECK(hipMalloc((void **)&d, 4 * n * sizeof(uint32_t)));
    k_selftest_philox<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(
        (uint32_t)seed, (uint32_t)(seed >> 32), stream, (uint32_t)sweep, (uint32_t)(sweep >> 32), n, d);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpy(out, d, 4 * n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    (void)hipFree(d);
    return NSK_OK;
}

int nsk_selftest_stream(int device, int64_t nbytes, int width, int iters, double *gbytes_per_s) {
    // width 4 / 16: plain grid-stride copy (the counter-calibration workload); width 64: the
    // bandwidth ceiling -- 4 x 16-byte non-temporal loads in flight per lane, non-temporal stores
    if (nbytes < 4096 || (width != 4 && width != 16 && width != 64) || iters < 1 || !gbytes_per_s) return fail(NSK_E_INVALID, "bad argument");
    HIPCHECK(hipSetDevice(device));
    nbytes &= ~(int64_t)4095;
    void *a = nullptr, *b = nullptr;
    HIPCHECK(hipMalloc(&a, nbytes));
    HIPCHECK(hipMalloc(&b, nbytes));
    HIPCHECK(hipMemset(a, 1, nbytes));
    hipEvent_t e0, e1;
    HIPCHECK(hipEventCreate(&e0));
    HIPCHECK(hipEventCreate(&e1));
    const long long n = nbytes / (width == 64 ? 16 : width);
    const int grid = 256 * 8;
    for (int it = -1; it < iters; it++) {
        if (it == 0) HIPCHECK(hipEventRecord(e0, 0));
        if (width == 4) k_stream_copy<uint32_t><<<dim3(grid), dim3(NSK_BLOCK)>>>((const uint32_t *)a, (uint32_t *)b, n);
        else if (width == 16) k_stream_copy<uint4><<<dim3(grid), dim3(NSK_BLOCK)>>>((const uint4 *)a, (uint4 *)b, n);
        else k_stream_copy_nt<4><<<dim3(grid * 2), dim3(NSK_BLOCK)>>>((const uint4 *)a, (uint4 *)b, n);
    }
    HIPCHECK(hipEventRecord(e1, 0));
    HIPCHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
    *gbytes_per_s = 2.0 * (double)nbytes * iters / ((double)ms * 1e-3) / 1e9;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(a); (void)hipFree(b);
    return NSK_OK;
}

}  // extern "C"
