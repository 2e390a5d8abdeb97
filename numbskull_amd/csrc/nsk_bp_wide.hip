// nsk_bp_wide.hip -- belief propagation through wide logical factors (nsk_bp_wide_plan.h, nsk_kernels_bpwide.h):
// nsk_bp_setup_wide is nsk_bp_setup (nsk_bp.hip bp_setup) with the wide route on; the wide factors' records, positions
// and the list of the table route's edges hang off the selected set-up, are on the ledger and go with it
// (nsk_bp_clear).  In a set-up that has wide factors nsk_bp_run's factor phase is k_bp_factor_narrow over the table
// route's edges and k_bp_wide over the wide factors, on one residual word; a set-up without them launches what it always
// launched.  nsk_bp_wide_terms evaluates the wide factors' Bethe terms.
#include <hip/hip_runtime.h>

#include "nsk_bp_wide_plan.h"
#include "nsk_internal.h"
#include "nsk_kernels_bpwide.h"

using namespace nsk;

static BpWideArgs bp_wide_args(const NskBp &b, const double *w) {
    BpWideArgs q = {};
    q.msg_off = b.msg_off; q.w = w; q.v2f = b.v2f; q.f2v = b.f2v;
    q.rec = (const int4 *)b.wd_rec; q.pos_off = b.wd_pos_off; q.pos = b.wd_pos; q.narrow = b.wd_narrow;
    q.nwide = (int32_t)b.winfo.nwide; q.nnarrow = b.wd_nnarrow; q.wave_lds = (int32_t)bp_wide_wave_lds(b.winfo.max_positions);
    return q;
}

template <typename T>
static int wide_upload(nsk_graph *g, T **ptr, const std::vector<T> &h) {
    int rc = dev_upload(g, ptr, h);
    if (!rc) g->bp.owned.push_back(*ptr);
    return rc;
}

// (nsk_bp.hip bp_setup waits for the stream before wp leaves its scope, and frees everything on a failure)
int bp_wide_attach(nsk_graph *g, BpWidePlan &wp, const char *val) {
    NskBp &b = g->bp;
    const int64_t before = g->mem.total;
    b.wd_nnarrow = (int32_t)wp.narrow.size();
    if (wp.narrow.empty()) wp.narrow.push_back(0);          // (no empty upload; nnarrow says 0)
    int rc = wide_upload(g, &b.wd_rec, wp.rec);
    if (!rc) rc = wide_upload(g, &b.wd_pos_off, wp.pos_off);
    if (!rc) rc = wide_upload(g, &b.wd_pos, wp.pos);
    if (!rc) rc = wide_upload(g, &b.wd_narrow, wp.narrow);
    if (rc) return rc;
    b.wd_factors.clear();
    for (int64_t k = 0; k < wp.nwide; k++) b.wd_factors.push_back(wp.rec[4 * (size_t)k]);
    b.winfo.nwide = wp.nwide; b.winfo.wide_positions = (int64_t)wp.pos.size(); b.winfo.max_positions = wp.max_positions;
    b.winfo.lds_bytes = bp_wide_block_waves(wp.max_positions) * bp_wide_wave_lds(wp.max_positions) * 8;
    b.winfo.device_bytes = g->mem.total - before;
    const int npos = (int)wp.pos.size();
    const dim3 grid(bp_blocks(npos, NSK_BLOCK)), block(NSK_BLOCK);
    if (g->c.vbytes == 4) k_bp_wide_clamp<int32_t><<<grid, block, 0, g->stream>>>(b.wd_pos, npos, (const int32_t *)val);
    else k_bp_wide_clamp<int8_t><<<grid, block, 0, g->stream>>>(b.wd_pos, npos, (const int8_t *)val);
    return hipGetLastError() == hipSuccess ? NSK_OK : fail(NSK_E_DEVICE, "nsk_bp_setup_wide: the clamped positions' launch failed");
}

void bp_wide_factor_enqueue(nsk_graph *g, const BpArgs &a, int t, double tol, double damping, double oml, unsigned long long *res) {
    const NskBp &b = g->bp;
    const BpWideArgs q = bp_wide_args(b, g->w);
    const int waves = bp_wide_block_waves(b.winfo.max_positions);
    if (q.nnarrow > 0) k_bp_factor_narrow<<<dim3(bp_blocks(q.nnarrow, NSK_BLOCK)), dim3(NSK_BLOCK), 0, g->stream>>>(a, q, t, tol, damping, oml, res);
    k_bp_wide<<<dim3(bp_blocks(q.nwide, waves)), dim3(64 * waves), (size_t)b.winfo.lds_bytes, g->stream>>>(q, t, tol, damping, oml, res);
}

extern "C" {

int nsk_bp_setup_wide(nsk_graph *g, int which, int64_t chain, int sample_evidence, nsk_bp_info *info, nsk_bp_wide_info *winfo) {
    int wide_min = NSK_BP_MAX_MEMBERS + 1;
    if (const char *env = nsk::diag_env("NSK_BP_WIDE_MIN")) wide_min = std::max(1, atoi(env));
    int rc = bp_setup(g, "nsk_bp_setup_wide", which, chain, sample_evidence, wide_min, info);
    if (!rc && winfo) *winfo = g->bp.winfo;
    return rc;
}

int nsk_bp_wide_terms(nsk_graph *g, int64_t *factor_ids, double *terms) {
    const char *who = "nsk_bp_wide_terms";
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!g->bp.ready) return fail(NSK_E_INVALID, std::string(who) + ": no belief propagation is set up (nsk_bp_setup)");
    const NskBp &b = g->bp;
    const size_t n = (size_t)b.winfo.nwide;
    if (n == 0) return NSK_OK;
    for (size_t k = 0; factor_ids && k < n; k++) factor_ids[k] = b.wd_factors[k];
    if (!terms) return NSK_OK;
    HIPCHECK(hipSetDevice(g->device));
    double *d = nullptr;                        // for this call only
    int rc = call_alloc(g, &d, n, who, "the terms, 8 bytes a wide factor");
    if (rc) return rc;
    const int waves = bp_wide_block_waves(b.winfo.max_positions);
    k_bp_wide_terms<<<dim3(bp_blocks((long long)n, waves)), dim3(64 * waves), (size_t)b.winfo.lds_bytes, g->stream>>>(bp_wide_args(b, g->w), d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(terms, d, n * 8, hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);
    dev_free(g, d);
    HIPCHECK(e);
    HIPCHECK(e2);
    return NSK_OK;
}

// host only: no device is touched
int nsk_bp_wide_plan(const nsk_graph_desc *desc, int sample_evidence, nsk_bp_info *info, nsk_bp_wide_info *winfo, int32_t *route) {
    if (!desc) return fail(NSK_E_INVALID, "null argument");
    Compiled c;
    std::string err;
    int rc = compile_graph(desc, c, err);
    if (rc) return fail(rc, err);
    int wide_min = NSK_BP_MAX_MEMBERS + 1;
    if (const char *env = nsk::diag_env("NSK_BP_WIDE_MIN")) wide_min = std::max(1, atoi(env));
    BpPlan pl;
    BpWidePlan wp;
    const std::string why = bp_plan_wide(c, sample_evidence, NSK_BP_MAX_MEMBERS, NSK_BP_MAX_TABLE, NSK_ZLOCAL, wide_min, NSK_BP_WIDE_MAX_MEMBERS, pl, wp);
    if (!why.empty()) return fail(NSK_E_INVALID, why);
    if (info) *info = pl.info;
    if (winfo) {
        *winfo = nsk_bp_wide_info();
        winfo->nwide = wp.nwide; winfo->wide_positions = (int64_t)wp.pos.size(); winfo->max_positions = wp.max_positions;
        winfo->lds_bytes = wp.nwide ? bp_wide_block_waves(wp.max_positions) * bp_wide_wave_lds(wp.max_positions) * 8 : 0;
    }
    if (route) {
        for (int64_t f = 0; f < c.nfactor; f++) route[f] = 0;
        for (int64_t k = 0; k < wp.nwide; k++) route[wp.rec[4 * (size_t)k]] = 1;
    }
    return NSK_OK;
}

}  // extern "C"
