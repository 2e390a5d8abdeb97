// nsk_bp_map.hip -- max-product belief propagation on the selected resident set-up (nsk_internal.h NskBp,
// nsk_kernels_bpmap.h): MAP decoding over the (max, +) semiring.  The set-up (nsk_bp.hip) plans which kernel serves
// which factor (nsk_bp_map_plan.h); the first nsk_bp_map_run on a set-up uploads the three lists and allocates both
// message arrays and the max-marginals, which the set-up owns from then on (nsk_bp_clear, a replacing set-up and
// nsk_graph_destroy free them with the rest).  nsk_bp_map_run enqueues every iteration on the handle's stream -- per
// iteration one factor-phase launch per populated route, then the variable phase -- without a synchronisation between
// them, the early exit on the device as in nsk_bp_run, and copies the residuals back once.  The sum-product arrays of
// the set-up are read (theta, the structure, the clamped variables' indicator beliefs) and never written; wk, the
// scratch of the large cardinalities, is shared.  The launches are not counted by the profiling bracket.
#include <hip/hip_runtime.h>

#include "nsk_internal.h"
#include "nsk_kernels_bpmap.h"

using namespace nsk;

static int ms_common(nsk_graph *g, const char *what) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    int rc = energy_whole_graph(g, what);
    if (rc) return rc;
    if (!g->bp.ready) return fail(NSK_E_INVALID, std::string(what) + ": no belief propagation is set up (nsk_bp_setup)");
    return NSK_OK;
}
// ... and the arrays of a run
static int ms_ran(nsk_graph *g, const char *what) {
    int rc = ms_common(g, what);
    if (rc) return rc;
    if (!g->bp.ms_f) return fail(NSK_E_INVALID, std::string(what) + ": no max-product run on this set-up (nsk_bp_map_run)");
    return NSK_OK;
}

static MsArgs ms_args(const nsk_graph *g) {
    const NskBp &b = g->bp;
    MsArgs m = {};
    m.b = bp_args(g, b);
    m.F = b.ms_f; m.V = b.ms_v; m.mm = b.ms_mm;
    m.lane_ids = b.ms_lane; m.wave_ids = b.ms_wave; m.edge_ids = b.ms_edge;
    m.nlane = b.ms_nlane; m.nwave = b.ms_nwave; m.nedge_r = b.ms_nedge;
    return m;
}

// the arrays of the first run on a set-up; on a failure none of them stays
static int ms_ensure(nsk_graph *g, bool &fresh) {
    NskBp &b = g->bp;
    fresh = false;
    if (b.ms_f) return NSK_OK;
    const BpMapRoutes &r = b.ms_routes;
    const size_t nmsg = (size_t)b.info.nmsg, nbel = (size_t)b.info.nbelief, at = b.owned.size();
    auto keep = [&](int rc, void *p) { if (!rc) b.owned.push_back(p); return rc; };
    int rc = keep(dev_alloc(g, &b.ms_f, nmsg), b.ms_f);
    if (!rc) rc = keep(dev_alloc(g, &b.ms_v, nmsg), b.ms_v);
    if (!rc) rc = keep(dev_alloc(g, &b.ms_mm, nbel), b.ms_mm);
    if (!rc) rc = keep(dev_upload(g, &b.ms_lane, r.lane), b.ms_lane);
    if (!rc) rc = keep(dev_upload(g, &b.ms_wave, r.wave), b.ms_wave);
    if (!rc) rc = keep(dev_upload(g, &b.ms_edge, r.edge), b.ms_edge);
    if (rc) {
        (void)hipStreamSynchronize(g->stream);      // (an upload may still read its list)
        for (size_t i = at; i < b.owned.size(); i++) dev_free(g, b.owned[i]);
        b.owned.resize(at);
        b.ms_f = b.ms_v = b.ms_mm = nullptr;
        b.ms_lane = b.ms_wave = b.ms_edge = nullptr;
        if (rc != NSK_E_NOMEM) return rc;
        const long long bytes = 16ll * (long long)nmsg + 8ll * (long long)nbel + 4ll * (long long)(r.lane.size() + r.wave.size() + r.edge.size());
        return fail(NSK_E_NOMEM, "nsk_bp_map_run: both message arrays, the max-marginals and the route lists (" + std::to_string(bytes) +
                                 " bytes) do not fit on the device");
    }
    b.ms_nlane = (int32_t)r.lane.size(); b.ms_nwave = (int32_t)r.wave.size(); b.ms_nedge = (int32_t)r.edge.size();
    fresh = true;
    return NSK_OK;
}

extern "C" {

int nsk_bp_map_run(nsk_graph *g, int64_t max_iters, double damping, double tol, int warm, int64_t *iters, double *residual) {
    int rc = ms_common(g, "nsk_bp_map_run");
    if (rc) return rc;
    if ((rc = bp_refuse_wide(g->bp, "nsk_bp_map_run"))) return rc;
    if (!iters) return fail(NSK_E_INVALID, "null argument");
    if (max_iters < 1 || max_iters > 4096) return fail(NSK_E_INVALID, "nsk_bp_map_run: max_iters must lie in [1, 4096]");
    if (!(damping >= 0.0 && damping < 1.0)) return fail(NSK_E_INVALID, "nsk_bp_map_run: damping must lie in [0, 1)");
    if (!(tol >= 0.0)) return fail(NSK_E_INVALID, "nsk_bp_map_run: tol must be at least 0");
    if (warm != 0 && warm != 1) return fail(NSK_E_INVALID, "nsk_bp_map_run: warm must be 0 or 1");
    HIPCHECK(hipSetDevice(g->device));
    bool fresh = false;
    if ((rc = ms_ensure(g, fresh))) return rc;
    NskBp &b = g->bp;
    const size_t S = (size_t)max_iters;
    unsigned long long *res = nullptr;              // [max_iters] bit patterns, for this call only
    if ((rc = dev_alloc(g, &res, S))) {
        if (fresh) (void)hipStreamSynchronize(g->stream);
        if (rc != NSK_E_NOMEM) return rc;
        return fail(NSK_E_NOMEM, "nsk_bp_map_run: the residuals (" + std::to_string((long long)(S * 8)) + " bytes) do not fit on the device");
    }
    const MsArgs m = ms_args(g);
    const BpArgs &a = m.b;
    const double oml = 1.0 - damping;
    const int nbin = b.nvbin, nall = a.nvlist;
    const dim3 block(NSK_BLOCK), wblock(NSK_MS_WAVES * 64), vblock(NSK_BP_VAR_BLOCK);
    const dim3 gl(bp_blocks(m.nlane, NSK_BLOCK)), gw(bp_blocks(m.nwave, NSK_MS_WAVES)), ge(bp_blocks(m.nedge_r, NSK_BLOCK)),
               gb(bp_blocks(nbin, NSK_BP_VAR_BLOCK)), gr(bp_blocks(nall - nbin, NSK_BP_VAR_BLOCK));
    hipError_t e = hipMemsetAsync(res, 0, S * 8, g->stream);
    if (e == hipSuccess && (fresh || !warm)) {      // a cold start; new arrays start cold whatever the caller says
        k_ms_reset<<<dim3(bp_blocks(std::max<long long>(a.nedge, a.nid), NSK_BLOCK)), block, 0, g->stream>>>(m);
        e = hipGetLastError();
    }
    if (a.nedge > 0)
        for (size_t t = 0; t < S && e == hipSuccess; t++) {
            if (m.nlane > 0) k_ms_lane<<<gl, block, 0, g->stream>>>(m, (int)t, tol, damping, oml, res);
            if (m.nwave > 0) k_ms_wave<<<gw, wblock, 0, g->stream>>>(m, (int)t, tol, damping, oml, res);
            if (m.nedge_r > 0) k_ms_edge<<<ge, block, 0, g->stream>>>(m, (int)t, tol, damping, oml, res);
            if (nbin > 0) k_ms_var<true><<<gb, vblock, 0, g->stream>>>(m, 0, nbin, (int)t, tol, res);
            if (nall > nbin) k_ms_var<false><<<gr, vblock, 0, g->stream>>>(m, nbin, nall, (int)t, tol, res);
            e = hipGetLastError();
        }
    std::vector<double> host(S);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), res, S * 8, hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);      // (also: the uploads of a first run have read their lists)
    dev_free(g, res);
    if (fresh) { b.ms_routes.lane = {}; b.ms_routes.wave = {}; b.ms_routes.edge = {}; }     // (the counts stay)
    HIPCHECK(e);
    HIPCHECK(e2);
    int64_t ran = -max_iters;
    for (size_t t = 0; t < S; t++) {
        if (residual) residual[t] = host[t];
        if (ran < 0 && host[t] <= tol) ran = (int64_t)t + 1;
    }
    *iters = ran;
    return NSK_OK;
}

int nsk_bp_map_marginals(nsk_graph *g, const int64_t *vids, int64_t nvids, double *out) {
    int rc = ms_ran(g, "nsk_bp_map_marginals");
    if (rc) return rc;
    const Compiled &c = g->c;
    if (nvids < 0 || (!vids && nvids != 0)) return fail(NSK_E_INVALID, "nsk_bp_map_marginals: a null selection with a count, or a negative count");
    if (vids && nvids == 0) return NSK_OK;
    const int64_t n = vids ? nvids : c.nvar;
    for (int64_t i = 0; vids && i < n; i++)
        if (vids[i] < 0 || vids[i] >= c.nvar) return fail(NSK_E_INDEX, "nsk_bp_map_marginals: variable id out of range");
    const NskBp &b = g->bp;
    if (b.info.nbelief == 0) return NSK_OK;
    if (!out) return fail(NSK_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    std::vector<double> all((size_t)b.info.nbelief);
    HIPCHECK(hipMemcpy(all.data(), b.ms_mm, all.size() * 8, hipMemcpyDeviceToHost));
    size_t o = 0;
    for (int64_t i = 0; i < n; i++) {
        const size_t id = (size_t)c.iid[(size_t)(vids ? vids[i] : i)];
        for (long long k = b.b_off[id]; k < b.b_off[id + 1]; k++) out[o++] = all[(size_t)k];
    }
    return NSK_OK;
}

int nsk_bp_map_download(nsk_graph *g, int what, double *out) {
    int rc = ms_ran(g, "nsk_bp_map_download");
    if (rc) return rc;
    if (what != 0 && what != 1) return fail(NSK_E_INVALID, "nsk_bp_map_download: what must be 0 (factor to variable) or 1 (variable to factor)");
    const NskBp &b = g->bp;
    const size_t n = (size_t)b.info.nmsg;
    if (n == 0) return NSK_OK;
    if (!out) return fail(NSK_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    HIPCHECK(hipMemcpy(out, what == 0 ? b.ms_f : b.ms_v, n * 8, hipMemcpyDeviceToHost));
    return NSK_OK;
}

int nsk_bp_map_decode(nsk_graph *g, int which, int64_t chain, int64_t *ties) {
    int rc = ms_ran(g, "nsk_bp_map_decode");
    if (rc) return rc;
    if ((rc = chain_select(g, which, chain, 1, "nsk_bp_map_decode", true))) return rc;
    HIPCHECK(hipSetDevice(g->device));
    // the kernel writes plain values: a tally kept in the value bytes goes back to its array first, as in nsk_icm
    if ((rc = nsk_unpack_tally(g))) return rc;
    unsigned long long *cnt = nullptr;              // for this call only
    if ((rc = call_alloc(g, &cnt, 1, "nsk_bp_map_decode", "the tie counter"))) return rc;
    const MsArgs m = ms_args(g);
    char *val = chain_val(g, which, chain);
    unsigned long long host = 0;
    hipError_t e = hipMemsetAsync(cnt, 0, sizeof(unsigned long long), g->stream);
    if (e == hipSuccess && m.b.nvlist > 0) {
        const dim3 grid(bp_blocks(m.b.nvlist, NSK_BLOCK)), block(NSK_BLOCK);
        if (g->c.vbytes == 4) k_ms_decode<int32_t><<<grid, block, 0, g->stream>>>(m, (int32_t *)val, cnt);
        else k_ms_decode<int8_t><<<grid, block, 0, g->stream>>>(m, (int8_t *)val, cnt);
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

int nsk_bp_map_routes(nsk_graph *g, int64_t *counts) {
    int rc = ms_common(g, "nsk_bp_map_routes");
    if (rc) return rc;
    if (!counts) return fail(NSK_E_INVALID, "null argument");
    for (int i = 0; i < 3; i++) counts[i] = g->bp.ms_routes.counts[i];
    return NSK_OK;
}

}  // extern "C"
