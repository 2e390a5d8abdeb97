// nsk_wstats.hip -- the per-weight statistics (nsk_internal.h NskWstats): the entry points (nsk_weight_stats, the sample
// trace's stats column), the by-weight list, the plans, and the launches of the kernels (nsk_kernels_wstats.h) on the
// handle's stream; the sample trace calls nsk_wstats_enqueue behind every record launch when its stats column is on.
#include <hip/hip_runtime.h>

#include "nsk_internal.h"
#include "nsk_kernels_wstats.h"

using namespace nsk;

// whole rounds of XCDs, one item per lane (shorts) or wave (pieces) up to the cap
static unsigned int wstats_blocks(long long items, long long per_block) {
    const long long need = (items + per_block - 1) / per_block;
    return (unsigned int)(need >= NSK_WSTATS_MAX_BLOCKS ? NSK_WSTATS_MAX_BLOCKS : (need + 7) / 8 * 8);
}

template <typename VT>
static void wstats_launch(nsk_graph *g, const WstatsArgs &a, const void *val, unsigned int R, double *out, double *partial) {
    const dim3 block(NSK_BLOCK);
    if (a.nshort > 0)
        k_wstats_short<VT><<<dim3(wstats_blocks(a.nshort, NSK_BLOCK), R), block, 0, g->stream>>>(a, (const VT *)val, out);
    if (a.npiece > 0)
        k_wstats_piece<VT><<<dim3(wstats_blocks(a.npiece, NSK_BLOCK / 64), R), block, 0, g->stream>>>(a, (const VT *)val, out, partial);
}

// Up to three launches behind whatever the stream holds; not counted by the profiling bracket (sweep kernels only).
int nsk_wstats_enqueue(nsk_graph *g, const NskWstatsPlan &plan, const void *val, int nchains, bool packed_bytes, bool scaled,
                       double *out, int64_t out_stride) {
    const NskWstats &ws = g->wstats;
    if (!g->energy.ready || !ws.ready || nchains < 1 || (plan.npartial > 0 && nchains > plan.partial_chains) || (scaled && !g->f_feat))
        return fail(NSK_E_INVALID, "weight statistics: the by-weight list is not set up");
    WstatsArgs a;
    a.e = energy_args(g);
    a.wf_idx = ws.wf_idx;
    a.feat = scaled ? g->f_feat : nullptr;
    a.shorts = plan.shorts; a.pieces = plan.pieces; a.multi = plan.multi;
    for (int k = 0; k < NSK_WSTATS_SHORT; k++) a.len_end[k] = plan.len_end[k];
    a.nshort = plan.nshort; a.npiece = plan.npiece; a.nmulti = plan.nmulti; a.npartial = plan.npartial;
    a.out_stride = (long long)out_stride;
    const unsigned int R = (unsigned int)nchains;
    if (g->c.vbytes == 4) wstats_launch<int32_t>(g, a, val, R, out, plan.partial);
    else if (packed_bytes) wstats_launch<PackedByte>(g, a, val, R, out, plan.partial);
    else wstats_launch<int8_t>(g, a, val, R, out, plan.partial);
    if (a.nmulti > 0)
        k_wstats_reduce<<<dim3((unsigned int)((a.nmulti + NSK_BLOCK / 64 - 1) / (NSK_BLOCK / 64)), R), dim3(NSK_BLOCK), 0, g->stream>>>(a, plan.partial, out);
    HIPCHECK(hipGetLastError());
    return NSK_OK;
}

// ---- per-weight statistics (nsk_internal.h NskWstats, nsk_kernels_wstats.h) -----------------------------------------
// The by-weight index list at the first use (after energy_ensure: every factor's weight slot was checked), and the
// feature values when a scaled sum asks for them (nsk_pcd.hip reads the list too)
int nsk_wstats_ensure(nsk_graph *g, bool scaled, const char *what) {
    NskWstats &ws = g->wstats;
    Compiled &c = g->c;
    HIPCHECK(hipSetDevice(g->device));
    if (!ws.ready) {
        const size_t nw = (size_t)c.nweight, nf = (size_t)c.nfactor;
        std::vector<uint32_t> off(nw + 1, 0);
        for (size_t f = 0; f < nf; f++) off[(size_t)c.f_rec[4 * f + 2] + 1]++;
        for (size_t w = 0; w < nw; w++) off[w + 1] += off[w];
        std::vector<int32_t> idx(nf);
        std::vector<uint32_t> at(off.begin(), off.end() - 1);
        for (size_t f = 0; f < nf; f++) idx[at[(size_t)c.f_rec[4 * f + 2]]++] = (int32_t)f;     // ascending inside a weight
        NskRollback rb(g->mem, nsk_free_raw);
        int32_t *dev = nullptr;
        int rc = dev_upload(g, &dev, idx);
        if (!rc && hipStreamSynchronize(g->stream) != hipSuccess) rc = fail(NSK_E_DEVICE, "hipStreamSynchronize failed");
        if (rc) {
            if (rc != NSK_E_NOMEM) return rc;
            return fail(NSK_E_NOMEM, std::string(what) + ": the by-weight factor list (" + std::to_string((long long)(nf * 4 / 1048576)) +
                                     " MB) does not fit on the device");
        }
        rb.commit();
        ws.wf_off = std::move(off); ws.wf_first.resize(nw);
        for (size_t w = 0; w < nw; w++) ws.wf_first[w] = ws.wf_off[w] < ws.wf_off[w + 1] ? idx[ws.wf_off[w]] : 0;
        ws.wf_idx = dev;
        ws.ready = true;
    }
    if (scaled && !g->f_feat) {
        NskRollback rb(g->mem, nsk_free_raw);
        double *feat = nullptr;
        int rc = dev_upload(g, &feat, c.f_feat);
        if (!rc && hipStreamSynchronize(g->stream) != hipSuccess) rc = fail(NSK_E_DEVICE, "hipStreamSynchronize failed");
        if (rc) {
            if (rc != NSK_E_NOMEM) return rc;
            return fail(NSK_E_NOMEM, std::string(what) + ": the feature values (" + std::to_string((long long)(c.f_feat.size() * 8 / 1048576)) +
                                     " MB) do not fit on the device");
        }
        rb.commit();
        g->f_feat = feat;
    }
    return NSK_OK;
}

// partial sums of the plan's weights of several pieces, for `chains` chains (grown when more ask)
static int wstats_partial_ensure(nsk_graph *g, NskWstatsPlan &plan, int chains) {
    if (plan.npartial == 0 || chains <= plan.partial_chains) return NSK_OK;
    double *partial = nullptr;
    int rc = dev_alloc(g, &partial, (size_t)chains * (size_t)plan.npartial);
    if (rc) return rc;
    HIPCHECK(hipStreamSynchronize(g->stream));      // (launches that write the buffer that goes)
    dev_free(g, plan.partial);
    plan.partial = partial; plan.partial_chains = chains;
    return NSK_OK;
}

// The work list of the weights whose SLOTS are slot[0 .. ncols): column j of the output is weight slot[j]'s sum.  How a
// weight is cut is a function of its own length (nsk_kernels_wstats.h); a weight named twice is evaluated twice.
static int wstats_plan_build(nsk_graph *g, NskWstatsPlan &plan, const int32_t *slot, int64_t ncols, int chains, const char *what) {
    const NskWstats &ws = g->wstats;
    NskWstatsPlan p;
    p.ncols = ncols;
    // the cut and its items (nsk_steps.h; a weight without a factor reads 0: the output is zeroed where it is allocated)
    static_assert(sizeof(WeightCutShort) == sizeof(uint2) && sizeof(WeightItem) == sizeof(uint4), "the items are uploaded as they are");
    const WeightCut cut = weight_cut(ws.wf_off, ws.wf_first, slot, (size_t)ncols, NSK_WSTATS_SHORT);
    const WstatsItems it = wstats_items(cut, NSK_WSTATS_PIECE);
    std::copy(cut.len_end.begin(), cut.len_end.end(), p.len_end);
    p.nshort = (int64_t)cut.shorts.size(); p.npiece = (int64_t)it.pieces.size(); p.nmulti = (int64_t)it.multi.size(); p.npartial = it.npartial;
    NskRollback rb(g->mem, nsk_free_raw);
    int rc = NSK_OK;
    if (p.nshort) rc = dev_upload(g, (WeightCutShort **)&p.shorts, cut.shorts);
    if (!rc && p.npiece) rc = dev_upload(g, (WeightItem **)&p.pieces, it.pieces);
    if (!rc && p.nmulti) rc = dev_upload(g, (WeightItem **)&p.multi, it.multi);
    if (!rc && hipStreamSynchronize(g->stream) != hipSuccess) rc = fail(NSK_E_DEVICE, "hipStreamSynchronize failed");
    if (!rc) rc = wstats_partial_ensure(g, p, chains);
    if (rc) {
        if (rc != NSK_E_NOMEM) return rc;
        const double mb = ((double)p.nshort * 8 + (double)p.npiece * 16 + (double)p.nmulti * 16 + (double)p.npartial * 8 * chains) / 1048576.0;
        return fail(NSK_E_NOMEM, std::string(what) + ": the work list of the weights (" + std::to_string((long long)mb) + " MB) does not fit on the device");
    }
    rb.commit();
    plan = p;
    return NSK_OK;
}

void wstats_plan_free(nsk_graph *g, NskWstatsPlan &plan) {
    dev_free(g, plan.shorts); dev_free(g, plan.pieces); dev_free(g, plan.multi); dev_free(g, plan.partial);
    plan = NskWstatsPlan();
}

// slot of the caller's weight id
static inline int32_t wstats_slot(const Compiled &c, int64_t wid) { return c.wmap.empty() ? (int32_t)wid : c.wmap[(size_t)wid]; }

extern "C" {

int nsk_weight_stats(nsk_graph *g, int which, int64_t first_chain, int64_t nchains, int scaled, double *out) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!out) return fail(NSK_E_INVALID, "null argument");
    int rc = chain_select(g, which, first_chain, nchains, "nsk_weight_stats");
    if (!rc) rc = energy_whole_graph(g, "nsk_weight_stats");
    if (rc) return rc;
    const Compiled &c = g->c;
    if (c.nweight == 0) return NSK_OK;
    if ((rc = energy_ensure(g, 0, "nsk_weight_stats"))) return rc;
    if ((rc = nsk_wstats_ensure(g, scaled != 0, "nsk_weight_stats"))) return rc;
    NskWstats &ws = g->wstats;
    if (!ws.all_ready) {
        std::vector<int32_t> slot((size_t)c.nweight);
        for (int64_t w = 0; w < c.nweight; w++) slot[(size_t)w] = wstats_slot(c, w);
        if ((rc = wstats_plan_build(g, ws.all, slot.data(), c.nweight, (int)nchains, "nsk_weight_stats"))) return rc;
        ws.all_ready = true;
    }
    if ((rc = wstats_partial_ensure(g, ws.all, (int)nchains))) return rc;
    if (nchains > ws.result_chains) {
        double *result = nullptr;
        const size_t n = (size_t)nchains * (size_t)c.nweight;
        if ((rc = dev_alloc(g, &result, n)))
            return fail(NSK_E_NOMEM, "nsk_weight_stats: one double per chain and weight (" + std::to_string((long long)(n * 8 / 1048576)) + " MB) does not fit on the device");
        HIPCHECK(hipStreamSynchronize(g->stream));
        dev_free(g, ws.result);
        HIPCHECK(hipMemsetAsync(result, 0, n * sizeof(double), g->stream));     // (weights without a factor are never written)
        ws.result = result; ws.result_chains = (int)nchains;
    }
    if ((rc = nsk_wstats_enqueue(g, ws.all, chain_val(g, which, first_chain),(int)nchains, g->packed_sweeps > 0, scaled != 0, ws.result, c.nweight))) return rc;
    HIPCHECK(hipMemcpyAsync(out, ws.result, (size_t)nchains * (size_t)c.nweight * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    return NSK_OK;
}

int nsk_trace_weight_stats(nsk_graph *g, const int64_t *wids, int64_t nwids, int scaled) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    NskTrace &t = g->trace;
    if (t.capacity == 0) return fail(NSK_E_INVALID, "nsk_trace_weight_stats: no trace is set up");
    const Compiled &c = g->c;
    if (nwids >= 0 && (wids ? nwids < 1 : nwids != 0))
        return fail(NSK_E_INVALID, "nsk_trace_weight_stats: a list of weight ids needs at least one (NULL with 0: all weights)");
    if (nwids > 0)
        for (int64_t j = 0; j < nwids; j++)
            if (wids[j] < 0 || wids[j] >= c.nweight) return fail(NSK_E_INDEX, "nsk_trace_weight_stats: weight id out of range");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    int rc = NSK_OK;
    if (nwids >= 0) {       // (before the column that stands goes)
        if ((rc = energy_whole_graph(g, "nsk_trace_weight_stats"))) return rc;
        if ((rc = energy_ensure(g, 0, "nsk_trace_weight_stats"))) return rc;
        if ((rc = nsk_wstats_ensure(g, scaled != 0, "nsk_trace_weight_stats"))) return rc;
    }
    dev_free(g, t.ws);
    t.ws = nullptr; t.ws_scaled = false;
    wstats_plan_free(g, t.ws_plan);
    if (nwids < 0) return NSK_OK;
    const int64_t ncols = wids ? nwids : c.nweight;
    const double total = (double)t.capacity * (double)t.chains * (double)ncols;
    if (total >= 35184372088832.0) return fail(NSK_E_NOMEM, "nsk_trace_weight_stats: the column does not fit");
    std::vector<int32_t> slot((size_t)ncols);
    for (int64_t j = 0; j < ncols; j++) slot[(size_t)j] = wstats_slot(c, wids ? wids[j] : j);
    NskRollback rb(g->mem, nsk_free_raw);
    NskWstatsPlan plan;
    if ((rc = wstats_plan_build(g, plan, slot.data(), ncols, t.chains, "nsk_trace_weight_stats"))) return rc;
    double *col = nullptr;
    const size_t n = (size_t)t.capacity * (size_t)t.chains * (size_t)ncols;
    if ((rc = dev_alloc(g, &col, n)))
        return fail(NSK_E_NOMEM, "nsk_trace_weight_stats: capacity x chains x weights doubles (" + std::to_string((long long)(n * 8 / 1048576)) + " MB) do not fit on the device");
    HIPCHECK(hipMemsetAsync(col, 0, (n ? n : 1) * sizeof(double), g->stream));     // (weights without a factor, rows recorded while it was off)
    rb.commit();
    t.ws_plan = plan;
    t.ws = col;
    t.ws_scaled = scaled != 0;
    return NSK_OK;
}

int nsk_trace_download_weight_stats(nsk_graph *g, int64_t first_row, int64_t nrows, double *out) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    const NskTrace &t = g->trace;
    if (t.capacity == 0) return fail(NSK_E_INVALID, "nsk_trace_download_weight_stats: no trace is set up");
    if (!t.ws) return fail(NSK_E_INVALID, "nsk_trace_download_weight_stats: the trace keeps no stats column (nsk_trace_weight_stats)");
    if (first_row < 0 || nrows < 0 || first_row + nrows > t.rows) return fail(NSK_E_INVALID, "nsk_trace_download_weight_stats: rows beyond those recorded");
    const size_t row = (size_t)t.chains * (size_t)t.ws_plan.ncols;
    if (nrows > 0 && row > 0 && !out) return fail(NSK_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    if (nrows > 0 && row > 0)
        HIPCHECK(hipMemcpy(out, t.ws + (size_t)first_row * row, (size_t)nrows * row * sizeof(double), hipMemcpyDeviceToHost));
    return NSK_OK;
}

}  // extern "C"
