// nsk_bp_dual.hip -- dual MAP bounds on the selected resident set-up (nsk_internal.h NskBp, nsk_kernels_bpdual.h): max-sum
// diffusion in its variable-centred form, one launch per route and colour class.  The first dual call on a set-up plans
// the classes and routes (nsk_bp_dual_plan.h, host only; a refusal of the plan is kept and returned every time); the first
// nsk_bp_dual_run on a set-up uploads the two item lists and allocates D, M, the terms and Bv, which the set-up owns from
// then on (nsk_bp_clear, a replacing set-up and nsk_graph_destroy free them with the rest).  nsk_bp_dual_run enqueues
// every sweep on the handle's stream without a synchronisation between them, the early exit on the device as in
// nsk_bp_run, and copies the residuals back once.  Of the sum-product set-up it reads theta and the structure and writes
// nothing.  The launches are not counted by the profiling bracket.
#include <hip/hip_runtime.h>

#include "nsk_internal.h"
#include "nsk_kernels_bpdual.h"

using namespace nsk;

static int dual_common(nsk_graph *g, const char *what) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    int rc = energy_whole_graph(g, what);
    if (rc) return rc;
    if (!g->bp.ready) return fail(NSK_E_INVALID, std::string(what) + ": no belief propagation is set up (nsk_bp_setup)");
    return bp_refuse_wide(g->bp, what);
}
// ... and its classes and routes, planned when a dual call first asks: the set-up's own plan made again from the compiled
// records (host only; a set-up whose user never asks pays nothing).  The plan's refusal is kept and returned every time.
static int dual_planned(nsk_graph *g, const char *what) {
    int rc = dual_common(g, what);
    if (rc) return rc;
    NskBp &b = g->bp;
    if (!b.du_planned) {
        BpPlan pl;
        b.du_why = bp_plan(g->c, b.du_sev, NSK_BP_MAX_MEMBERS, NSK_BP_MAX_TABLE, NSK_ZLOCAL, pl);
        if (b.du_why.empty()) b.du_why = bp_dual_plan(g->c, pl, NSK_ZLOCAL, trw_lane_max(nsk::diag_env("NSK_DUAL_LANE_MAX")), b.du_plan);
        b.du_planned = true;
    }
    return refuse(b.du_why);
}
// ... and the arrays of a run
static int dual_ran(nsk_graph *g, const char *what) {
    int rc = dual_common(g, what);
    if (rc) return rc;
    if (!g->bp.du_d) return fail(NSK_E_INVALID, std::string(what) + ": no dual run on this set-up (nsk_bp_dual_run)");
    return NSK_OK;
}

static DualArgs dual_args(const nsk_graph *g) {
    const NskBp &b = g->bp;
    DualArgs m = {};
    m.b = bp_args(g, b);
    m.D = b.du_d; m.M = b.du_m; m.tf = b.du_tf; m.tv = b.du_tv; m.bv = b.du_bv;
    m.lane_ids = b.du_lane; m.wave_ids = b.du_wave;
    m.wave_lds = (int32_t)b.du_plan.wave_lds;
    return m;
}

// bytes of dynamic LDS of a wave-route launch
static size_t dual_lds_bytes(const NskBp &b) { return (size_t)dual_block_waves(b.du_plan.wave_lds) * (size_t)b.du_plan.wave_lds * 8; }

// the arrays of the first run on a set-up; on a failure none of them stays
static int dual_ensure(nsk_graph *g, bool &fresh) {
    NskBp &b = g->bp;
    fresh = false;
    if (b.du_d) return NSK_OK;
    const BpDualPlan &r = b.du_plan;
    const size_t nmsg = (size_t)b.info.nmsg, nbel = (size_t)b.info.nbelief, F = (size_t)g->c.nfactor, nid = (size_t)g->c.nid, at = b.owned.size();
    auto keep = [&](int rc, void *p) { if (!rc) b.owned.push_back(p); return rc; };
    int rc = keep(dev_alloc(g, &b.du_d, nmsg), b.du_d);
    if (!rc) rc = keep(dev_alloc(g, &b.du_m, nmsg), b.du_m);
    if (!rc) rc = keep(dev_alloc(g, &b.du_bv, nbel), b.du_bv);
    if (!rc) rc = keep(dev_alloc(g, &b.du_tf, F), b.du_tf);
    if (!rc) rc = keep(dev_alloc(g, &b.du_tv, nid), b.du_tv);
    if (!rc) rc = keep(dev_upload(g, &b.du_lane, r.lane), b.du_lane);
    if (!rc) rc = keep(dev_upload(g, &b.du_wave, r.wave), b.du_wave);
    if (rc) {
        (void)hipStreamSynchronize(g->stream);      // (an upload may still read its list)
        for (size_t i = at; i < b.owned.size(); i++) dev_free(g, b.owned[i]);
        b.owned.resize(at);
        b.du_d = b.du_m = b.du_bv = b.du_tf = b.du_tv = nullptr;
        b.du_lane = b.du_wave = nullptr;
        if (rc != NSK_E_NOMEM) return rc;
        const long long bytes = 16ll * (long long)nmsg + 8ll * (long long)(nbel + F + nid) + 4ll * (long long)(r.lane.size() + r.wave.size());
        return fail(NSK_E_NOMEM, "nsk_bp_dual_run: D, M, the reparametrised unaries, the terms and the item lists (" + std::to_string(bytes) +
                                 " bytes) do not fit on the device");
    }
    fresh = true;
    return NSK_OK;
}

// tf, tv and Bv from D as it stands
static hipError_t dual_terms_enqueue(nsk_graph *g, const DualArgs &m) {
    const long long items = std::max<long long>((long long)m.b.nfactor, (long long)m.b.nvlist);
    k_bp_dual_terms<<<dim3(bp_blocks(items, NSK_BLOCK)), dim3(NSK_BLOCK), 0, g->stream>>>(m);
    return hipGetLastError();
}

extern "C" {

int nsk_bp_dual_run(nsk_graph *g, int64_t max_sweeps, double tol, int warm, int64_t *sweeps, double *residual) {
    int rc = dual_planned(g, "nsk_bp_dual_run");
    if (rc) return rc;
    if (!sweeps) return fail(NSK_E_INVALID, "null argument");
    if (max_sweeps < 1 || max_sweeps > 4096) return fail(NSK_E_INVALID, "nsk_bp_dual_run: max_sweeps must lie in [1, 4096]");
    if (!(tol >= 0.0)) return fail(NSK_E_INVALID, "nsk_bp_dual_run: tol must be at least 0");
    if (warm != 0 && warm != 1) return fail(NSK_E_INVALID, "nsk_bp_dual_run: warm must be 0 or 1");
    HIPCHECK(hipSetDevice(g->device));
    NskBp &b = g->bp;
    // more LDS than a launch may ask for unannounced: announced by every call, since the attribute is the kernel's and
    // another set-up's call may have set a smaller size since
    if (b.du_plan.counts[1] > 0 && dual_lds_bytes(b) > 65536) {
        hipError_t ea = hipFuncSetAttribute((const void *)k_dual_wave, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dual_lds_bytes(b));
        if (ea != hipSuccess)
            return fail(NSK_E_DEVICE, "nsk_bp_dual_run: the wave route needs " + std::to_string((long long)dual_lds_bytes(b)) +
                                      " bytes of LDS a block, which the device refuses: " + hipGetErrorString(ea));
    }
    bool fresh = false;
    if ((rc = dual_ensure(g, fresh))) return rc;
    const size_t S = (size_t)max_sweeps;
    unsigned long long *res = nullptr;              // [max_sweeps] bit patterns, for this call only
    if ((rc = dev_alloc(g, &res, S))) {
        if (fresh) (void)hipStreamSynchronize(g->stream);
        if (rc != NSK_E_NOMEM) return rc;
        return fail(NSK_E_NOMEM, "nsk_bp_dual_run: the residuals (" + std::to_string((long long)(S * 8)) + " bytes) do not fit on the device");
    }
    const DualArgs m = dual_args(g);
    const BpArgs &a = m.b;
    const BpDualPlan &pl = b.du_plan;
    const int W = dual_block_waves(pl.wave_lds);
    const size_t lds = dual_lds_bytes(b), ncls = pl.lane_off.size() - 1;
    const dim3 block(NSK_BLOCK), wblock((unsigned)W * 64);
    hipError_t e = hipMemsetAsync(res, 0, S * 8, g->stream);
    if (e == hipSuccess && (!b.du_reset || !warm)) {        // a cold start; arrays never reset start cold whatever the caller says
        k_dual_reset<<<dim3(bp_blocks(std::max<long long>(a.nedge, a.nid), NSK_BLOCK)), block, 0, g->stream>>>(m);
        e = hipGetLastError();
        if (e == hipSuccess) b.du_reset = true;
    }
    if (a.nedge > 0)
        for (size_t t = 0; t < S && e == hipSuccess; t++)
            for (size_t k = 0; k < ncls && e == hipSuccess; k++) {
                const int l0 = pl.lane_off[k], l1 = pl.lane_off[k + 1], w0 = pl.wave_off[k], w1 = pl.wave_off[k + 1];
                if (l1 > l0) k_dual_lane<<<dim3(bp_blocks(l1 - l0, NSK_BLOCK)), block, 0, g->stream>>>(m, l0, l1, (int)t, tol, res);
                if (w1 > w0) k_dual_wave<<<dim3(bp_blocks(w1 - w0, W)), wblock, lds, g->stream>>>(m, w0, w1, (int)t, tol, res);
                e = hipGetLastError();
            }
    std::vector<double> host(S);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), res, S * 8, hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);      // (also: the uploads of a first run have read their lists)
    dev_free(g, res);
    if (fresh) { b.du_plan.lane = {}; b.du_plan.wave = {}; }    // (the offsets, the counts and the LDS size stay)
    HIPCHECK(e);
    HIPCHECK(e2);
    int64_t ran = -max_sweeps;
    for (size_t t = 0; t < S; t++) {
        if (residual) residual[t] = host[t];
        if (ran < 0 && host[t] <= tol) ran = (int64_t)t + 1;
    }
    *sweeps = ran;
    return NSK_OK;
}

int nsk_bp_dual_download(nsk_graph *g, int what, double *out) {
    int rc = dual_ran(g, "nsk_bp_dual_download");
    if (rc) return rc;
    if (what < NSK_BP_DUAL_D || what > NSK_BP_DUAL_BV) return fail(NSK_E_INVALID, "nsk_bp_dual_download: what must be NSK_BP_DUAL_D .. NSK_BP_DUAL_BV");
    const NskBp &b = g->bp;
    const Compiled &c = g->c;
    const size_t nmsg = (size_t)b.info.nmsg, F = (size_t)c.nfactor, nvar = (size_t)c.nvar, nid = (size_t)c.nid, nbel = (size_t)b.info.nbelief;
    const size_t n = what <= NSK_BP_DUAL_M ? nmsg : (what == NSK_BP_DUAL_TERMS ? F + nvar : nbel);
    if (n == 0) return NSK_OK;
    if (!out) return fail(NSK_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(g->device));
    if (what <= NSK_BP_DUAL_M) {
        HIPCHECK(hipStreamSynchronize(g->stream));
        HIPCHECK(hipMemcpy(out, what == NSK_BP_DUAL_D ? b.du_d : b.du_m, n * 8, hipMemcpyDeviceToHost));
        return NSK_OK;
    }
    hipError_t e = dual_terms_enqueue(g, dual_args(g));
    std::vector<double> dev(what == NSK_BP_DUAL_TERMS ? nid : nbel);
    if (what == NSK_BP_DUAL_TERMS) {                // per factor in the caller's order, then per variable in the caller's order
        if (e == hipSuccess && F > 0) e = hipMemcpyAsync(out, b.du_tf, F * 8, hipMemcpyDeviceToHost, g->stream);
        if (e == hipSuccess && nid > 0) e = hipMemcpyAsync(dev.data(), b.du_tv, nid * 8, hipMemcpyDeviceToHost, g->stream);
    } else if (e == hipSuccess) e = hipMemcpyAsync(dev.data(), b.du_bv, nbel * 8, hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);
    HIPCHECK(e);
    HIPCHECK(e2);
    if (what == NSK_BP_DUAL_TERMS) {
        for (size_t v = 0; v < nvar; v++) out[F + v] = dev[(size_t)c.iid[v]];
        return NSK_OK;
    }
    size_t o = 0;                                   // the "full" layout of nsk_bp_beliefs
    for (size_t v = 0; v < nvar; v++) {
        const size_t id = (size_t)c.iid[v];
        for (long long k = b.b_off[id]; k < b.b_off[id + 1]; k++) out[o++] = dev[(size_t)k];
    }
    return NSK_OK;
}

int nsk_bp_dual_decode(nsk_graph *g, int which, int64_t chain, int64_t *ties) {
    int rc = dual_ran(g, "nsk_bp_dual_decode");
    if (rc) return rc;
    if ((rc = chain_select(g, which, chain, 1, "nsk_bp_dual_decode", true))) return rc;
    HIPCHECK(hipSetDevice(g->device));
    // the kernel writes plain values: a tally kept in the value bytes goes back to its array first, as in nsk_icm
    if ((rc = nsk_unpack_tally(g))) return rc;
    unsigned long long *cnt = nullptr;              // for this call only
    if ((rc = call_alloc(g, &cnt, 1, "nsk_bp_dual_decode", "the tie counter"))) return rc;
    const DualArgs m = dual_args(g);
    MsArgs ms = {};                                 // nsk_bp_map_decode's scan, over Bv
    ms.b = m.b; ms.mm = m.bv;
    char *val = chain_val(g, which, chain);
    unsigned long long host = 0;
    hipError_t e = hipMemsetAsync(cnt, 0, sizeof(unsigned long long), g->stream);
    if (e == hipSuccess) e = dual_terms_enqueue(g, m);
    if (e == hipSuccess && m.b.nvlist > 0) {
        const dim3 grid(bp_blocks(m.b.nvlist, NSK_BLOCK)), block(NSK_BLOCK);
        if (g->c.vbytes == 4) k_ms_decode<int32_t><<<grid, block, 0, g->stream>>>(ms, (int32_t *)val, cnt);
        else k_ms_decode<int8_t><<<grid, block, 0, g->stream>>>(ms, (int8_t *)val, cnt);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);
    dev_free(g, cnt);
    HIPCHECK(e);
    HIPCHECK(e2);
    if (ties) *ties = (int64_t)host;
    return NSK_OK;
}

int nsk_bp_dual_routes(nsk_graph *g, int64_t *counts) {
    int rc = dual_planned(g, "nsk_bp_dual_routes");
    if (rc) return rc;
    if (!counts) return fail(NSK_E_INVALID, "null argument");
    counts[0] = g->bp.du_plan.counts[0]; counts[1] = g->bp.du_plan.counts[1];
    return NSK_OK;
}

int nsk_bp_dual_classes(nsk_graph *g, int32_t *cls) {
    int rc = dual_planned(g, "nsk_bp_dual_classes");
    if (rc) return rc;
    if (g->c.nvar > 0 && !cls) return fail(NSK_E_INVALID, "null argument");
    for (int64_t v = 0; v < g->c.nvar; v++) cls[v] = g->bp.du_plan.cls[(size_t)g->c.iid[(size_t)v]];
    return NSK_OK;
}

// host only: no device is touched
int nsk_bp_dual_plan(const nsk_graph_desc *desc, int sample_evidence, int64_t *counts, int32_t *route, int32_t *cls, int64_t *wave_lds) {
    if (!desc) return fail(NSK_E_INVALID, "null argument");
    Compiled c;
    std::string err;
    int rc = compile_graph(desc, c, err);
    if (rc) return fail(rc, err);
    BpPlan pl;
    std::string why = bp_plan(c, sample_evidence, NSK_BP_MAX_MEMBERS, NSK_BP_MAX_TABLE, NSK_ZLOCAL, pl);
    if (!why.empty()) return fail(NSK_E_INVALID, why);
    BpDualPlan r;
    why = bp_dual_plan(c, pl, NSK_ZLOCAL, trw_lane_max(nsk::diag_env("NSK_DUAL_LANE_MAX")), r);
    if (!why.empty()) return fail(NSK_E_INVALID, why);
    if (counts) { counts[0] = r.counts[0]; counts[1] = r.counts[1]; }
    if (wave_lds) *wave_lds = r.wave_lds;
    std::vector<int32_t> by_id((size_t)c.nid, -1);
    for (int32_t i : r.lane) by_id[(size_t)pl.v_list[(size_t)i]] = 0;
    for (int32_t i : r.wave) by_id[(size_t)pl.v_list[(size_t)i]] = 1;
    for (int64_t v = 0; v < c.nvar; v++) {
        if (route) route[v] = by_id[(size_t)c.iid[(size_t)v]];
        if (cls) cls[v] = r.cls[(size_t)c.iid[(size_t)v]];
    }
    return NSK_OK;
}

}  // extern "C"
