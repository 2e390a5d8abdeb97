// nsk_bp_trw.hip -- tree-reweighted belief propagation on the selected resident set-up (nsk_internal.h NskBp,
// nsk_kernels_bptrw.h): fractional BP with one weight rho_f a factor, whose free energy bounds log Z from above for rho
// in the spanning-tree polytope of a pairwise graph.  The set-up (nsk_bp.hip) plans which route serves which factor
// (nsk_bp_trw_plan.h); the first nsk_bp_trw_run on a set-up uploads the two lists and allocates rho, psi_rho, the three
// message arrays, the beliefs and the two term arrays, which the set-up owns from then on (nsk_bp_clear, a replacing
// set-up and nsk_graph_destroy free them with the rest).  nsk_bp_trw_run enqueues psi_rho and every iteration on the
// handle's stream -- per iteration one factor-phase launch per populated route, then the variable phase -- without a
// synchronisation between them, the early exit on the device as in nsk_bp_run, and copies the residuals back once.  Of the
// sum-product set-up it reads theta, the structure and the clamped variables' indicator beliefs and writes nothing; wk,
// the scratch of the large cardinalities, is shared.  The launches are not counted by the profiling bracket.
#include <hip/hip_runtime.h>

#include "nsk_internal.h"
#include "nsk_kernels_bptrw.h"

using namespace nsk;

static int trw_common(nsk_graph *g, const char *what) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    int rc = energy_whole_graph(g, what);
    if (rc) return rc;
    if (!g->bp.ready) return fail(NSK_E_INVALID, std::string(what) + ": no belief propagation is set up (nsk_bp_setup)");
    return NSK_OK;
}
// ... and the arrays of a run
static int trw_ran(nsk_graph *g, const char *what) {
    int rc = trw_common(g, what);
    if (rc) return rc;
    if (!g->bp.tw_lf) return fail(NSK_E_INVALID, std::string(what) + ": no tree-reweighted run on this set-up (nsk_bp_trw_run)");
    return NSK_OK;
}

static TrwArgs trw_args(const nsk_graph *g) {
    const NskBp &b = g->bp;
    TrwArgs t = {};
    t.b = bp_args(g, b);
    t.rho = b.tw_rho; t.psi = b.tw_psi; t.LF = b.tw_lf; t.LN = b.tw_ln; t.EN = b.tw_en; t.bel = b.tw_bel; t.tf = b.tw_tf; t.tv = b.tw_tv;
    t.lane_ids = b.tw_lane; t.wave_ids = b.tw_wave;
    t.nlane = b.tw_nlane; t.nwave = b.tw_nwave; t.wave_lds = (int32_t)b.tw_routes.wave_lds;
    return t;
}

// bytes of dynamic LDS of a wave-route launch
static size_t trw_lds_bytes(const NskBp &b) { return (size_t)trw_block_waves(b.tw_routes.wave_lds) * (size_t)b.tw_routes.wave_lds * 8; }

// the arrays of the first run on a set-up; on a failure none of them stays
static int trw_ensure(nsk_graph *g, bool &fresh) {
    NskBp &b = g->bp;
    fresh = false;
    if (b.tw_lf) return NSK_OK;
    const BpTrwRoutes &r = b.tw_routes;
    if (!r.wave.empty() && trw_lds_bytes(b) > 65536) {      // beyond what a launch may ask for unannounced
        hipError_t e = hipFuncSetAttribute((const void *)k_trw_wave, hipFuncAttributeMaxDynamicSharedMemorySize, (int)trw_lds_bytes(b));
        if (e != hipSuccess)
            return fail(NSK_E_DEVICE, "nsk_bp_trw_run: the wave route needs " + std::to_string((long long)trw_lds_bytes(b)) +
                                      " bytes of LDS a block, which the device refuses: " + hipGetErrorString(e));
    }
    const size_t nmsg = (size_t)b.info.nmsg, nbel = (size_t)b.info.nbelief, ntab = (size_t)b.info.ntable, F = (size_t)g->c.nfactor,
                 nid = (size_t)g->c.nid, at = b.owned.size();
    auto keep = [&](int rc, void *p) { if (!rc) b.owned.push_back(p); return rc; };
    int rc = keep(dev_alloc(g, &b.tw_lf, nmsg), b.tw_lf);
    if (!rc) rc = keep(dev_alloc(g, &b.tw_ln, nmsg), b.tw_ln);
    if (!rc) rc = keep(dev_alloc(g, &b.tw_en, nmsg), b.tw_en);
    if (!rc) rc = keep(dev_alloc(g, &b.tw_psi, ntab), b.tw_psi);
    if (!rc) rc = keep(dev_alloc(g, &b.tw_bel, nbel), b.tw_bel);
    if (!rc) rc = keep(dev_alloc(g, &b.tw_rho, F), b.tw_rho);
    if (!rc) rc = keep(dev_alloc(g, &b.tw_tf, F), b.tw_tf);
    if (!rc) rc = keep(dev_alloc(g, &b.tw_tv, nid), b.tw_tv);
    if (!rc) rc = keep(dev_upload(g, &b.tw_lane, r.lane), b.tw_lane);
    if (!rc) rc = keep(dev_upload(g, &b.tw_wave, r.wave), b.tw_wave);
    if (rc) {
        (void)hipStreamSynchronize(g->stream);      // (an upload may still read its list)
        for (size_t i = at; i < b.owned.size(); i++) dev_free(g, b.owned[i]);
        b.owned.resize(at);
        b.tw_lf = b.tw_ln = b.tw_en = b.tw_psi = b.tw_bel = b.tw_rho = b.tw_tf = b.tw_tv = nullptr;
        b.tw_lane = b.tw_wave = nullptr;
        if (rc != NSK_E_NOMEM) return rc;
        const long long bytes = 24ll * (long long)nmsg + 8ll * (long long)(ntab + nbel + nid) + 16ll * (long long)F +
                                4ll * (long long)(r.lane.size() + r.wave.size());
        return fail(NSK_E_NOMEM, "nsk_bp_trw_run: the three message arrays, psi_rho, the beliefs, rho, the terms and the route lists (" +
                                 std::to_string(bytes) + " bytes) do not fit on the device");
    }
    b.tw_nlane = (int32_t)r.lane.size(); b.tw_nwave = (int32_t)r.wave.size();
    fresh = true;
    return NSK_OK;
}

extern "C" {

int nsk_bp_trw_run(nsk_graph *g, const double *rho, int64_t max_iters, double damping, double tol, int warm, int64_t *iters,
                   double *residual) {
    int rc = trw_common(g, "nsk_bp_trw_run");
    if (rc) return rc;
    if ((rc = bp_refuse_wide(g->bp, "nsk_bp_trw_run"))) return rc;
    if (!iters || !rho) return fail(NSK_E_INVALID, "null argument");
    if (max_iters < 1 || max_iters > 4096) return fail(NSK_E_INVALID, "nsk_bp_trw_run: max_iters must lie in [1, 4096]");
    if (!(damping >= 0.0 && damping < 1.0)) return fail(NSK_E_INVALID, "nsk_bp_trw_run: damping must lie in [0, 1)");
    if (!(tol >= 0.0)) return fail(NSK_E_INVALID, "nsk_bp_trw_run: tol must be at least 0");
    if (warm != 0 && warm != 1) return fail(NSK_E_INVALID, "nsk_bp_trw_run: warm must be 0 or 1");
    if ((rc = refuse(trw_check_rho(rho, g->c.nfactor)))) return rc;
    HIPCHECK(hipSetDevice(g->device));
    bool fresh = false;
    if ((rc = trw_ensure(g, fresh))) return rc;
    NskBp &b = g->bp;
    const size_t S = (size_t)max_iters, F = (size_t)g->c.nfactor;
    unsigned long long *res = nullptr;              // [max_iters] bit patterns, for this call only
    if ((rc = dev_alloc(g, &res, S))) {
        if (fresh) (void)hipStreamSynchronize(g->stream);
        if (rc != NSK_E_NOMEM) return rc;
        return fail(NSK_E_NOMEM, "nsk_bp_trw_run: the residuals (" + std::to_string((long long)(S * 8)) + " bytes) do not fit on the device");
    }
    const TrwArgs t = trw_args(g);
    const BpArgs &a = t.b;
    const double oml = 1.0 - damping;
    const int nbin = b.nvbin, nall = a.nvlist, W = trw_block_waves(b.tw_routes.wave_lds);
    const size_t lds = trw_lds_bytes(b);
    const dim3 block(NSK_BLOCK), wblock((unsigned)W * 64), vblock(NSK_BP_VAR_BLOCK);
    const int npair = (int)b.tw_routes.npair;
    const dim3 gp(bp_blocks(npair, NSK_BLOCK)), gl(bp_blocks(t.nlane - npair, NSK_BLOCK)), gw(bp_blocks(t.nwave, W)), gb(bp_blocks(nbin, NSK_BP_VAR_BLOCK)),
               gr(bp_blocks(nall - nbin, NSK_BP_VAR_BLOCK));
    hipError_t e = hipMemsetAsync(res, 0, S * 8, g->stream);
    // rho and the tables under it: theta or rho may have changed since the last call
    if (e == hipSuccess && F > 0) e = hipMemcpyAsync(b.tw_rho, rho, F * 8, hipMemcpyHostToDevice, g->stream);
    if (e == hipSuccess && F > 0) {
        k_trw_psi<<<dim3(bp_blocks((long long)F, NSK_BLOCK)), block, 0, g->stream>>>(t);
        e = hipGetLastError();
    }
    if (e == hipSuccess && (fresh || !warm)) {      // a cold start; new arrays start cold whatever the caller says
        k_trw_reset<<<dim3(bp_blocks(std::max<long long>(a.nedge, a.nid), NSK_BLOCK)), block, 0, g->stream>>>(t);
        e = hipGetLastError();
    }
    if (a.nedge > 0)
        for (size_t it = 0; it < S && e == hipSuccess; it++) {
            if (npair > 0) k_trw_lane<true><<<gp, block, 0, g->stream>>>(t, 0, npair, (int)it, tol, damping, oml, res);
            if (t.nlane > npair) k_trw_lane<false><<<gl, block, 0, g->stream>>>(t, npair, t.nlane, (int)it, tol, damping, oml, res);
            if (t.nwave > 0) k_trw_wave<<<gw, wblock, lds, g->stream>>>(t, (int)it, tol, damping, oml, res);
            if (nbin > 0) k_trw_var<true><<<gb, vblock, 0, g->stream>>>(t, 0, nbin, (int)it, tol, res);
            if (nall > nbin) k_trw_var<false><<<gr, vblock, 0, g->stream>>>(t, nbin, nall, (int)it, tol, res);
            e = hipGetLastError();
        }
    std::vector<double> host(S);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), res, S * 8, hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);      // (also: rho and the uploads of a first run have been read)
    dev_free(g, res);
    if (fresh) { b.tw_routes.lane = {}; b.tw_routes.wave = {}; }        // (the counts and the LDS size stay)
    HIPCHECK(e);
    HIPCHECK(e2);
    int64_t ran = -max_iters;
    for (size_t i = 0; i < S; i++) {
        if (residual) residual[i] = host[i];
        if (ran < 0 && host[i] <= tol) ran = (int64_t)i + 1;
    }
    *iters = ran;
    return NSK_OK;
}

int nsk_bp_trw_beliefs(nsk_graph *g, const int64_t *vids, int64_t nvids, double *out) {
    int rc = trw_ran(g, "nsk_bp_trw_beliefs");
    if (rc) return rc;
    const Compiled &c = g->c;
    if (nvids < 0 || (!vids && nvids != 0)) return fail(NSK_E_INVALID, "nsk_bp_trw_beliefs: a null selection with a count, or a negative count");
    if (vids && nvids == 0) return NSK_OK;
    const int64_t n = vids ? nvids : c.nvar;
    for (int64_t i = 0; vids && i < n; i++)
        if (vids[i] < 0 || vids[i] >= c.nvar) return fail(NSK_E_INDEX, "nsk_bp_trw_beliefs: variable id out of range");
    const NskBp &b = g->bp;
    if (b.info.nbelief == 0) return NSK_OK;
    if (!out) return fail(NSK_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    std::vector<double> all((size_t)b.info.nbelief);
    HIPCHECK(hipMemcpy(all.data(), b.tw_bel, all.size() * 8, hipMemcpyDeviceToHost));
    size_t o = 0;
    for (int64_t i = 0; i < n; i++) {
        const size_t id = (size_t)c.iid[(size_t)(vids ? vids[i] : i)];
        for (long long k = b.b_off[id]; k < b.b_off[id + 1]; k++) out[o++] = all[(size_t)k];
    }
    return NSK_OK;
}

int nsk_bp_trw_download(nsk_graph *g, int what, double *out) {
    int rc = trw_ran(g, "nsk_bp_trw_download");
    if (rc) return rc;
    if (what < NSK_BP_TRW_LF || what > NSK_BP_TRW_TERMS) return fail(NSK_E_INVALID, "nsk_bp_trw_download: what must be NSK_BP_TRW_LF .. NSK_BP_TRW_TERMS");
    const NskBp &b = g->bp;
    const Compiled &c = g->c;
    const size_t nmsg = (size_t)b.info.nmsg, ntab = (size_t)b.info.ntable, F = (size_t)c.nfactor, nvar = (size_t)c.nvar, nid = (size_t)c.nid;
    const size_t n = what <= NSK_BP_TRW_LN ? nmsg : (what == NSK_BP_TRW_FACTOR_BELIEFS ? ntab : F + nvar);
    if (n == 0) return NSK_OK;
    if (!out) return fail(NSK_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(g->device));
    const TrwArgs t = trw_args(g);
    if (what <= NSK_BP_TRW_LN) {
        HIPCHECK(hipStreamSynchronize(g->stream));
        HIPCHECK(hipMemcpy(out, what == NSK_BP_TRW_LF ? b.tw_lf : b.tw_ln, n * 8, hipMemcpyDeviceToHost));
        return NSK_OK;
    }
    if (what == NSK_BP_TRW_TERMS) {                 // per factor in the caller's order, then per variable in the caller's order
        k_trw_energy<<<dim3(bp_blocks((long long)std::max<size_t>(F, (size_t)t.b.nvlist), NSK_BLOCK)), dim3(NSK_BLOCK), 0, g->stream>>>(t);
        hipError_t e = hipGetLastError();
        std::vector<double> tv(nid);
        if (e == hipSuccess && F > 0) e = hipMemcpyAsync(out, b.tw_tf, F * 8, hipMemcpyDeviceToHost, g->stream);
        if (e == hipSuccess && nid > 0) e = hipMemcpyAsync(tv.data(), b.tw_tv, nid * 8, hipMemcpyDeviceToHost, g->stream);
        const hipError_t e2 = hipStreamSynchronize(g->stream);
        HIPCHECK(e);
        HIPCHECK(e2);
        for (size_t v = 0; v < nvar; v++) out[F + v] = tv[(size_t)c.iid[v]];
        return NSK_OK;
    }
    double *fb = nullptr;                           // for this call only
    if ((rc = call_alloc(g, &fb, n, "nsk_bp_trw_download", "the factor beliefs"))) return rc;
    k_trw_fbelief<<<dim3(bp_blocks((long long)F, NSK_BLOCK)), dim3(NSK_BLOCK), 0, g->stream>>>(t, fb);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, fb, n * 8, hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);
    dev_free(g, fb);
    HIPCHECK(e);
    HIPCHECK(e2);
    return NSK_OK;
}

int nsk_bp_trw_routes(nsk_graph *g, int64_t *counts) {
    int rc = trw_common(g, "nsk_bp_trw_routes");
    if (rc) return rc;
    if (!counts) return fail(NSK_E_INVALID, "null argument");
    counts[0] = g->bp.tw_routes.counts[0]; counts[1] = g->bp.tw_routes.counts[1];
    return NSK_OK;
}

// host only: no device is touched
int nsk_bp_trw_plan(const nsk_graph_desc *desc, int sample_evidence, int64_t *counts, int32_t *route, int64_t *wave_lds) {
    if (!desc) return fail(NSK_E_INVALID, "null argument");
    Compiled c;
    std::string err;
    int rc = compile_graph(desc, c, err);
    if (rc) return fail(rc, err);
    BpPlan pl;
    const std::string why = bp_plan(c, sample_evidence, NSK_BP_MAX_MEMBERS, NSK_BP_MAX_TABLE, NSK_ZLOCAL, pl);
    if (!why.empty()) return fail(NSK_E_INVALID, why);
    BpTrwRoutes r;
    bp_trw_routes(pl, NSK_ZLOCAL, trw_lane_max(nsk::diag_env("NSK_TRW_LANE_MAX")), r);
    if (counts) { counts[0] = r.counts[0]; counts[1] = r.counts[1]; }
    if (wave_lds) *wave_lds = r.wave_lds;
    if (route) {
        for (int64_t f = 0; f < c.nfactor; f++) route[f] = -1;
        for (int32_t f : r.lane) route[f] = 0;
        for (int32_t f : r.wave) route[f] = 1;
    }
    return NSK_OK;
}

}  // extern "C"
