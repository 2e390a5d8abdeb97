// nsk_sw.hip -- Swendsen-Wang cluster updates of pairwise binary graphs (nsk_internal.h NskSw, nsk_kernels_sw.h):
// nsk_sw_setup takes the structure of one state from nsk_sw_plan.h (the classification and the tables' layout are
// bp_plan's; bonds, fields, the breadth-first tiles, the tiles' bond lists and the cross list: pure host arithmetic),
// uploads it, fills theta with k_bp_tables itself -- the bits of nsk_bp_download(NSK_BP_THETA) -- and derives J, q, h and
// H from it; the range rule is checked on a download of J and h, set-up not being the hot path.  nsk_sw_sweeps enqueues,
// per step, the five launches of one cluster update of every chain (tile, cross, flatten, decide, flip) and the ordinary
// sweeps behind it through nsk_gibbs_sweeps, without a host wait, and copies the counts back once.  The launches of an
// update are not counted by the profiling bracket.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "nsk_class_plan.h"         // plan_grid_cap
#include "nsk_internal.h"
#include "nsk_kernels_sw.h"
#include "nsk_sw_plan.h"

using namespace nsk;

namespace {

// (diagnostic, NSK_DIAG=1 NSK_SW_GRID_CAP=blocks, read at each call: small grids, later trips)
unsigned int sw_blocks(long long items, long long per_block, long long limit) {
    const int cap = plan_grid_cap(nsk::diag_env("NSK_SW_GRID_CAP"));
    if (cap > 0 && cap < limit) limit = cap;
    return (unsigned int)std::max<long long>(1, std::min((items + per_block - 1) / per_block, limit));
}
unsigned int sw_blocks(long long items) { return sw_blocks(items, NSK_BLOCK, NSK_SW_MAX_BLOCKS); }

int sw_tile_size() {
    const char *env = nsk::diag_env("NSK_SW_TILE");
    const int n = env ? atoi(env) : 0;
    return n >= 32 && n <= NSK_SW_TILE ? n : NSK_SW_TILE;
}

void sw_free(nsk_graph *g, NskSw &s) {
    for (void *p : s.owned) dev_free(g, p);
    s = NskSw();
}

template <typename T>
int sw_upload(nsk_graph *g, NskSw &s, T **ptr, const std::vector<T> &h) {
    int rc = dev_upload(g, ptr, h);
    if (!rc) s.owned.push_back(*ptr);
    return rc;
}
template <typename T>
int sw_alloc(nsk_graph *g, NskSw &s, T **ptr, size_t n) {
    int rc = dev_alloc(g, ptr, n);
    if (!rc) s.owned.push_back(*ptr);
    return rc;
}

int sw_common(nsk_graph *g, const char *what, bool need_setup) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    int rc = energy_whole_graph(g, what);
    if (rc) return rc;
    if (need_setup && !g->sw.ready) return fail(NSK_E_INVALID, std::string(what) + ": no cluster update is set up (nsk_sw_setup)");
    return NSK_OK;
}

// what k_bp_tables and k_bp_refresh read of the set-up: the table side of a BpArgs, nothing of the messages
BpArgs sw_bp_args(const nsk_graph *g, const NskSw &s) {
    BpArgs a = {};
    a.f_rec = (const uint4 *)g->f_rec; a.mrec = (const int2 *)s.mrec; a.pm_off = s.pm_off;
    a.slot_off = s.slot_off; a.slot_rec = (const int2 *)s.slot_rec; a.tab_off = s.tab_off; a.edge_off = s.edge_off;
    a.v_card = g->v_card; a.w = g->w; a.logtab = g->logtab;
    a.theta = s.theta; a.feat = s.feat;
    a.nfactor = (long long)g->c.nfactor; a.ntable = (long long)s.ntable; a.nid = (long long)g->c.nid;
    a.nedge = (int32_t)s.nedge;
    return a;
}

SwTabArgs sw_tab_args(const nsk_graph *g, const NskSw &s, double *J, double *qs, double *h, long long *H) {
    SwTabArgs t = {};
    t.theta = s.theta; t.tab_off = s.tab_off; t.edge_off = s.edge_off; t.f_bond = s.f_bond; t.ve_off = s.ve_off; t.ve_edge = s.ve_edge;
    t.g = s.gfield; t.J = J; t.qs = qs; t.h = h; t.H = H;
    t.nfactor = (long long)g->c.nfactor; t.nvars = (int32_t)s.info.nvars;
    return t;
}

// J, q, h and H from theta as it stands, into the arrays named; then the range rule on a download of J and h.
// Synchronises.  NSK_E_RANGE leaves the arrays named in an unspecified state: the caller drops them.
int sw_tables(nsk_graph *g, const NskSw &s, const char *who, double *J, double *qs, double *h, long long *H) {
    const size_t nb = (size_t)s.info.nbonds, nv = (size_t)s.info.nvars;
    const SwTabArgs t = sw_tab_args(g, s, J, qs, h, H);
    if (t.nfactor > 0) k_sw_factor<<<dim3(sw_blocks(t.nfactor)), dim3(NSK_BLOCK), 0, g->stream>>>(t);
    if (nv > 0) k_sw_field<<<dim3(sw_blocks((long long)nv)), dim3(NSK_BLOCK), 0, g->stream>>>(t);
    hipError_t e = hipGetLastError();
    std::vector<double> hJ(nb), hh(nv);
    if (e == hipSuccess && nb) e = hipMemcpyAsync(hJ.data(), J, nb * 8, hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess && nv) e = hipMemcpyAsync(hh.data(), h, nv * 8, hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);
    HIPCHECK(e);
    HIPCHECK(e2);
    for (size_t b = 0; b < nb; b++)
        if (!std::isfinite(hJ[b]))
            return fail(NSK_E_RANGE, std::string(who) + ": the coupling of factor " + std::to_string((long long)s.bond_fac[b]) + " is not finite");
    double total = 0.0;             // (integers below 2^31 each, at most 2^31 of them: exact in a double)
    for (size_t o = 0; o < nv; o++) {
        if (!std::isfinite(hh[o]) || std::fabs(hh[o]) >= 2147483648.0)
            return fail(NSK_E_RANGE, std::string(who) + ": the field of variable " + std::to_string((long long)g->c.p_vid[(size_t)s.ord_id[o]]) +
                                     " is not finite or reaches 2^31");
        total += std::ceil(std::fabs(hh[o]));
    }
    if (total >= 2147483648.0)
        return fail(NSK_E_RANGE, std::string(who) + ": the fields' magnitudes, each rounded up, sum to 2^31 or more: a cluster's int64 sum could wrap");
    return NSK_OK;
}

// parents, accumulators and decisions for the handle's chains as they are now; labels of another chain count are dropped
int sw_state_ensure(nsk_graph *g) {
    NskSw &s = g->sw;
    if (s.state_chains == g->nchains) return NSK_OK;
    for (void *p : {(void *)s.parent, (void *)s.acc, (void *)s.flip})
        if (p) { dev_free(g, p); s.owned.erase(std::find(s.owned.begin(), s.owned.end(), p)); }
    s.parent = nullptr; s.acc = nullptr; s.flip = nullptr;
    s.state_chains = 0;
    s.have_labels = false;
    const size_t n = (size_t)g->nchains * (size_t)s.info.nvars;
    int rc = sw_alloc(g, s, &s.parent, n);
    if (!rc) rc = sw_alloc(g, s, &s.acc, 2 * n);
    if (!rc) rc = sw_alloc(g, s, &s.flip, n);
    if (rc) {
        if (rc != NSK_E_NOMEM) return rc;
        return fail(NSK_E_NOMEM, "nsk_sw_sweeps: parents, accumulators and decisions (" + std::to_string((long long)(21 * n)) +
                                 " bytes) do not fit on the device");
    }
    s.state_chains = g->nchains;
    return NSK_OK;
}

template <typename VT>
void sw_update_enqueue(nsk_graph *g, const SwArgs &a, int R) {
    const dim3 block(NSK_BLOCK);
    const unsigned int lanes = sw_blocks(a.nvars);
    k_sw_tile<VT><<<dim3(sw_blocks(a.ntiles, 1, 1 << 16), (unsigned)R), block, 0, g->stream>>>(a);
    if (a.ncross > 0) k_sw_cross<VT><<<dim3(sw_blocks(a.ncross), (unsigned)R), block, 0, g->stream>>>(a);
    k_sw_flatten<VT><<<dim3(lanes, (unsigned)R), block, 0, g->stream>>>(a);
    k_sw_decide<<<dim3(lanes, (unsigned)R), block, 0, g->stream>>>(a);
    k_sw_flip<VT><<<dim3(lanes, (unsigned)R), block, 0, g->stream>>>(a);
}

}  // namespace

extern "C" {

int nsk_sw_plan(const nsk_graph_desc *desc, int sample_evidence, int tile, nsk_sw_info *info, int64_t *order, int64_t *bond_factor,
                int64_t *bond_ends, int64_t *bond_tile) {
    if (!desc) return fail(NSK_E_INVALID, "null argument");
    if (tile < 32 || tile > NSK_SW_TILE) return fail(NSK_E_INVALID, "nsk_sw_plan: tile must lie in [32, 1024]");
    Compiled c;
    std::string err;
    int rc = compile_graph(desc, c, err);
    if (rc) return fail(rc, err);
    SwPlan pl;
    const std::string why = sw_plan(c, sample_evidence, NSK_BP_MAX_MEMBERS, NSK_BP_MAX_TABLE, NSK_ZLOCAL, tile, pl);
    if (!why.empty()) return fail(NSK_E_INVALID, why);
    if (info) *info = pl.info;
    const size_t nv = (size_t)pl.info.nvars, nb = (size_t)pl.info.nbonds;
    for (size_t o = 0; order && o < nv; o++) order[o] = c.p_vid[(size_t)pl.ord_id[o]];
    for (size_t b = 0; b < nb; b++) {
        if (bond_factor) bond_factor[b] = pl.bond_fac[b];
        if (bond_ends) { bond_ends[2 * b] = pl.bond_ends[2 * b]; bond_ends[2 * b + 1] = pl.bond_ends[2 * b + 1]; }
        if (bond_tile) bond_tile[b] = -1;
    }
    for (size_t t = 0; bond_tile && t < (size_t)pl.info.ntiles; t++)
        for (int32_t i = pl.tb_off[t]; i < pl.tb_off[t + 1]; i++) bond_tile[pl.tb_rec[2 * (size_t)i + 1]] = (int64_t)t;
    return NSK_OK;
}

int nsk_sw_setup(nsk_graph *g, int which, int64_t chain, int sample_evidence, nsk_sw_info *info_out) {
    const char *who = "nsk_sw_setup";
    int rc = sw_common(g, who, false);
    if (rc) return rc;
    if ((rc = chain_select(g, which, chain, 1, who, true))) return rc;
    // ---- the structure: every refusal names the lowest offending factor and precedes any allocation
    const Compiled &c = g->c;
    SwPlan pl;
    const std::string why = sw_plan(c, sample_evidence, NSK_BP_MAX_MEMBERS, NSK_BP_MAX_TABLE, NSK_ZLOCAL, sw_tile_size(), pl);
    if (!why.empty()) return fail(NSK_E_INVALID, why);
    HIPCHECK(hipSetDevice(g->device));
    if ((rc = energy_ensure(g, 0, who))) return rc;
    if ((rc = nsk_unpack_tally(g))) return rc;
    HIPCHECK(hipStreamSynchronize(g->stream));
    // ---- a new set-up beside the resident one, which stays until this one stands
    NskSw n;
    n.info = pl.info; n.sample_evidence = sample_evidence ? 1 : 0;
    n.ntable = pl.bp.info.ntable; n.nedge = pl.bp.info.nedges;
    const size_t nv = (size_t)n.info.nvars, nb = (size_t)n.info.nbonds;
    const int64_t before = g->mem.total;
    rc = sw_upload(g, n, &n.pm_off, pl.bp.pm_off);
    if (!rc) rc = sw_upload(g, n, &n.tab_off, pl.bp.tab_off);
    if (!rc) rc = sw_upload(g, n, &n.slot_off, pl.bp.slot_off);
    if (!rc) rc = sw_upload(g, n, &n.edge_off, pl.bp.edge_off);
    if (!rc) rc = sw_upload(g, n, &n.mrec, pl.bp.mrec);
    if (!rc) rc = sw_upload(g, n, &n.slot_rec, pl.bp.slot_rec);
    if (!rc) rc = sw_upload(g, n, &n.f_bond, pl.f_bond);
    if (!rc) rc = sw_upload(g, n, &n.ve_off, pl.ve_off);
    if (!rc) rc = sw_upload(g, n, &n.ve_edge, pl.ve_edge);
    if (!rc) rc = sw_upload(g, n, &n.d_ord_id, pl.ord_id);
    if (!rc) rc = sw_upload(g, n, &n.tile_off, pl.tile_off);
    if (!rc) rc = sw_upload(g, n, &n.tb_off, pl.tb_off);
    if (!rc) rc = sw_upload(g, n, &n.tb_rec, pl.tb_rec);
    if (!rc) rc = sw_upload(g, n, &n.cross, pl.cross);
    if (!rc) rc = sw_alloc(g, n, &n.theta, (size_t)n.ntable);
    if (!rc) rc = sw_alloc(g, n, &n.feat, (size_t)n.ntable);
    if (!rc) rc = sw_alloc(g, n, &n.gfield, (size_t)n.nedge);
    if (!rc) rc = sw_alloc(g, n, &n.J, nb);
    if (!rc) rc = sw_alloc(g, n, &n.qs, nb);
    if (!rc) rc = sw_alloc(g, n, &n.h, nv);
    if (!rc) rc = sw_alloc(g, n, &n.H, nv);
    if (rc) {
        (void)hipStreamSynchronize(g->stream);
        sw_free(g, n);
        if (rc != NSK_E_NOMEM) return rc;
        return fail(NSK_E_NOMEM, "nsk_sw_setup: structure and tables (" +
                                 std::to_string(24ll * n.ntable + 24ll * (long long)nb + 16ll * n.info.ncross + 8ll * n.nedge + 28ll * (long long)nv) +
                                 " bytes and the tables' structure) do not fit on the device");
    }
    n.info.device_bytes = g->mem.total - before;
    n.ord_id.swap(pl.ord_id); n.bond_fac.swap(pl.bond_fac); n.bond_ends.swap(pl.bond_ends);
    const BpArgs a = sw_bp_args(g, n);
    const char *val = chain_val(g, which, chain);
    if (a.nfactor > 0) {
        const dim3 grid(sw_blocks(a.ntable)), block(NSK_BLOCK);
        if (c.vbytes == 4) k_bp_tables<int32_t><<<grid, block, 0, g->stream>>>(a, (const int32_t *)val);
        else k_bp_tables<int8_t><<<grid, block, 0, g->stream>>>(a, (const int8_t *)val);
    }
    rc = sw_tables(g, n, who, n.J, n.qs, n.h, n.H);    // (its synchronisation: the uploads read the vectors of this scope)
    if (rc) {
        (void)hipStreamSynchronize(g->stream);
        sw_free(g, n);
        return rc;
    }
    sw_free(g, g->sw);
    g->sw = std::move(n);
    g->sw.ready = true;
    if (info_out) *info_out = g->sw.info;
    return NSK_OK;
}

int nsk_sw_layout(nsk_graph *g, int64_t *order, int64_t *bond_factor, int64_t *bond_ends) {
    int rc = sw_common(g, "nsk_sw_layout", true);
    if (rc) return rc;
    const NskSw &s = g->sw;
    for (size_t o = 0; order && o < s.ord_id.size(); o++) order[o] = g->c.p_vid[(size_t)s.ord_id[o]];      // (a free variable has a position)
    for (size_t b = 0; bond_factor && b < s.bond_fac.size(); b++) bond_factor[b] = s.bond_fac[b];
    for (size_t i = 0; bond_ends && i < s.bond_ends.size(); i++) bond_ends[i] = s.bond_ends[i];
    return NSK_OK;
}

int nsk_sw_download(nsk_graph *g, int what, double *out) {
    int rc = sw_common(g, "nsk_sw_download", true);
    if (rc) return rc;
    if (what < NSK_SW_J || what > NSK_SW_H) return fail(NSK_E_INVALID, "nsk_sw_download: what must be NSK_SW_J, NSK_SW_Q or NSK_SW_H");
    const NskSw &s = g->sw;
    const size_t n = (size_t)(what == NSK_SW_H ? s.info.nvars : s.info.nbonds);
    if (n == 0) return NSK_OK;
    if (!out) return fail(NSK_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    HIPCHECK(hipMemcpy(out, what == NSK_SW_J ? (const void *)s.J : (what == NSK_SW_Q ? (const void *)s.qs : (const void *)s.H), n * 8, hipMemcpyDeviceToHost));
    for (size_t b = 0; what == NSK_SW_Q && b < n; b++) out[b] = std::fabs(out[b]);       // (the sign bit is J's)
    return NSK_OK;
}

int nsk_sw_labels(nsk_graph *g, int64_t chain, int32_t *out) {
    int rc = sw_common(g, "nsk_sw_labels", true);
    if (rc) return rc;
    const NskSw &s = g->sw;
    if (!s.have_labels) return fail(NSK_E_INVALID, "nsk_sw_labels: no cluster update has run on this set-up");
    if (chain < 0 || chain >= s.state_chains) return fail(NSK_E_INVALID, "nsk_sw_labels: chain outside those the last update served");
    const size_t nv = (size_t)s.info.nvars;
    if (nv == 0) return NSK_OK;
    if (!out) return fail(NSK_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    HIPCHECK(hipMemcpy(out, s.parent + (size_t)chain * nv, nv * 4, hipMemcpyDeviceToHost));
    return NSK_OK;
}

int nsk_sw_refresh(nsk_graph *g) {
    const char *who = "nsk_sw_refresh";
    int rc = sw_common(g, who, true);
    if (rc) return rc;
    NskSw &s = g->sw;
    const size_t nb = (size_t)s.info.nbonds, nv = (size_t)s.info.nvars;
    HIPCHECK(hipSetDevice(g->device));
    // the new tables beside the resident ones, which they replace once they passed the range rule (theta is scratch)
    double *J = nullptr, *qs = nullptr, *h = nullptr;
    long long *H = nullptr;
    rc = call_alloc(g, &J, nb, who, "the couplings, 8 bytes a bond");
    if (!rc) rc = call_alloc(g, &qs, nb, who, "the bond probabilities, 8 bytes a bond");
    if (!rc) rc = call_alloc(g, &h, nv, who, "the fields, 8 bytes a variable");
    if (!rc) rc = call_alloc(g, &H, nv, who, "the fixed-point fields, 8 bytes a variable");
    if (!rc) {
        const BpArgs a = sw_bp_args(g, s);
        if (a.nfactor > 0) k_bp_refresh<<<dim3(sw_blocks(a.ntable)), dim3(NSK_BLOCK), 0, g->stream>>>(a);
        rc = sw_tables(g, s, who, J, qs, h, H);
    }
    hipError_t e = hipSuccess;
    if (!rc && nb) e = hipMemcpyAsync(s.J, J, nb * 8, hipMemcpyDeviceToDevice, g->stream);
    if (!rc && nb && e == hipSuccess) e = hipMemcpyAsync(s.qs, qs, nb * 8, hipMemcpyDeviceToDevice, g->stream);
    if (!rc && nv && e == hipSuccess) e = hipMemcpyAsync(s.h, h, nv * 8, hipMemcpyDeviceToDevice, g->stream);
    if (!rc && nv && e == hipSuccess) e = hipMemcpyAsync(s.H, H, nv * 8, hipMemcpyDeviceToDevice, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);
    dev_free(g, H); dev_free(g, h); dev_free(g, qs); dev_free(g, J);
    if (rc) return rc;
    HIPCHECK(e);
    HIPCHECK(e2);
    return NSK_OK;
}

int nsk_sw_clear(nsk_graph *g) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!g->sw.ready) return NSK_OK;
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    sw_free(g, g->sw);
    return NSK_OK;
}

int nsk_sw_sweeps(nsk_graph *g, int64_t nsteps, int64_t gibbs_per_step, int burnin, int64_t *clusters, int64_t *largest, int64_t *flipped) {
    const char *who = "nsk_sw_sweeps";
    int rc = sw_common(g, who, true);
    if (rc) return rc;
    if (nsteps < 1 || nsteps > 65536) return fail(NSK_E_INVALID, "nsk_sw_sweeps: nsteps must lie in [1, 65536]");
    if (gibbs_per_step < 0 || 1 + gibbs_per_step > INT32_MAX / nsteps)
        return fail(NSK_E_INVALID, "nsk_sw_sweeps: gibbs_per_step must be at least 0 and nsteps x (1 + gibbs_per_step) at most 2^31 - 1");
    if (g->scan != NSK_SCAN_CHROMATIC) return fail(NSK_E_INVALID, "nsk_sw_sweeps: the sequential scan is not served");
    if (!burnin && gibbs_per_step > 0) NSK_NO_TRACE(g, who);
    HIPCHECK(hipSetDevice(g->device));
    if ((rc = sw_state_ensure(g))) return rc;
    NskSw &s = g->sw;
    const int R = g->nchains;
    const size_t T = (size_t)nsteps, n = 3 * T * (size_t)R;
    unsigned long long *out = nullptr;              // [nsteps][chains][3], for this call only
    if ((rc = call_alloc(g, &out, n, who, "the counts, 24 bytes a step and chain"))) return rc;
    // a tally kept in bits 1-7 of the value bytes goes back to its array first: the update sees plain values
    if ((rc = nsk_unpack_tally(g))) { dev_free(g, out); return rc; }
    hipError_t e = hipMemsetAsync(out, 0, n * 8, g->stream);

    SwArgs a = {};
    a.chain_stride = (long long)g->chain_stride;
    a.ord_id = s.d_ord_id; a.tile_off = s.tile_off; a.tb_off = s.tb_off; a.tb_rec = (const int2 *)s.tb_rec; a.cross = (const int4 *)s.cross;
    a.qs = s.qs; a.H = s.H; a.parent = s.parent; a.acc = s.acc; a.flip = s.flip;
    a.nvars = (int32_t)s.info.nvars; a.ntiles = (int32_t)s.info.ntiles; a.ncross = (int32_t)s.info.ncross;
    a.k0 = (uint32_t)g->seed; a.k1 = (uint32_t)(g->seed >> 32);
    for (size_t t = 0; t < T && !rc && e == hipSuccess; t++) {
        // 1. the cluster update, under a sweep index of its own (the values' address is read here: nsk_set_chains moves it)
        a.val = (char *)g->val;
        a.out = out + 3 * t * (size_t)R;
        a.s_lo = (uint32_t)g->sweep; a.s_hi = nsk_sweep_hi(g);
        if (a.nvars > 0) {
            if (g->c.vbytes == 4) sw_update_enqueue<int32_t>(g, a, R);
            else sw_update_enqueue<int8_t>(g, a, R);
            s.have_labels = true;
        }
        g->sweep += 1;
        e = hipGetLastError();
        // 2. the ordinary sweeps, as nsk_gibbs_sweeps enqueues, tallies and counts them
        if (e == hipSuccess && gibbs_per_step > 0) rc = nsk_gibbs_sweeps(g, gibbs_per_step, s.sample_evidence, burnin);
    }
    std::vector<unsigned long long> host(n);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(host.data(), out, n * 8, hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);
    dev_free(g, out);
    if (rc) return rc;
    HIPCHECK(e);
    HIPCHECK(e2);
    for (size_t i = 0; i < T * (size_t)R; i++) {
        if (clusters) clusters[i] = (int64_t)host[3 * i];
        if (largest) largest[i] = (int64_t)host[3 * i + 1];
        if (flipped) flipped[i] = (int64_t)host[3 * i + 2];
    }
    return NSK_OK;
}

}  // extern "C"
