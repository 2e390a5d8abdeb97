// nsk_wstats.hip -- launches of the per-weight statistics (nsk_kernels_wstats.h) on the handle's stream.  The entry
// points (nsk_weight_stats, nsk_trace_weight_stats), the by-weight list and the plans live in nsk_api.hip; the sample
// trace calls nsk_wstats_enqueue behind every record launch when its stats column is on.
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
    a.e.f_rec = (const uint4 *)g->f_rec; a.e.m_rec = (const int2 *)g->m_rec;
    a.e.v_card = g->v_card; a.e.iid_of_vid = g->iid_of_vid;
    a.e.w = g->w; a.e.logtab = g->logtab;
    a.e.nfactor = (long long)g->c.nfactor;
    a.e.chain_stride = (long long)g->chain_stride;
    a.e.head_by_vid = (g->c.flags & NSK_FLAG_HEAD_BY_VID) ? 1 : 0;
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
