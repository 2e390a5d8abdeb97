// nsk_energy.hip -- launches of the factor-parallel log-potential (nsk_kernels_energy.h) on the handle's stream.
// The entry points (nsk_log_potential, nsk_factor_values, nsk_trace_log_potential) and the lazily uploaded arrays live
// in nsk_api.hip; the sample trace calls nsk_energy_enqueue behind every record launch when its lp column is on.
#include <hip/hip_runtime.h>

#include "nsk_internal.h"
#include "nsk_kernels_energy.h"

using namespace nsk;

static EnergyArgs energy_args(const nsk_graph *g) {
    EnergyArgs a;
    a.f_rec = (const uint4 *)g->f_rec; a.m_rec = (const int2 *)g->m_rec;
    a.v_card = g->v_card; a.iid_of_vid = g->iid_of_vid;
    a.w = g->w; a.logtab = g->logtab;
    a.nfactor = (long long)g->c.nfactor;
    a.chain_stride = (long long)g->chain_stride;
    a.head_by_vid = (g->c.flags & NSK_FLAG_HEAD_BY_VID) ? 1 : 0;
    return a;
}

// out[r] = log-potential of chain r, r < nchains, of the chains that start at `val` (device pointers; nchains at most
// the chains the partials were sized for, nsk_api.hip energy_ensure).  packed_bytes: the value is bit 0 of a value byte.
// Two launches behind whatever the stream holds; not counted by the profiling bracket (sweep kernels only).
int nsk_energy_enqueue(nsk_graph *g, const void *val, int nchains, bool packed_bytes, double *out) {
    const NskEnergy &en = g->energy;
    if (!en.ready || nchains < 1 || nchains > en.chains) return fail(NSK_E_INVALID, "log-potential: the factor records are not set up");
    const EnergyArgs a = energy_args(g);
    const unsigned int nb = nsk_energy_blocks(a.nfactor);
    const dim3 grid(nb, (unsigned)nchains), block(NSK_BLOCK);
    if (g->c.vbytes == 4) k_energy_partial<int32_t><<<grid, block, 0, g->stream>>>(a, (const int32_t *)val, en.partial);
    else if (packed_bytes) k_energy_partial<PackedByte><<<grid, block, 0, g->stream>>>(a, (const PackedByte *)val, en.partial);
    else k_energy_partial<int8_t><<<grid, block, 0, g->stream>>>(a, (const int8_t *)val, en.partial);
    k_energy_reduce<<<dim3((unsigned)nchains), block, 0, g->stream>>>(en.partial, (int)nb, out);
    HIPCHECK(hipGetLastError());
    return NSK_OK;
}

// out[f] = eval_factor(f) on the state at `val` (one chain), f in the caller's factor order
int nsk_factor_values_enqueue(nsk_graph *g, const void *val, double *out) {
    if (!g->energy.ready) return fail(NSK_E_INVALID, "factor values: the factor records are not set up");
    const EnergyArgs a = energy_args(g);
    const dim3 grid(nsk_energy_blocks(a.nfactor)), block(NSK_BLOCK);
    if (g->c.vbytes == 4) k_factor_values<int32_t><<<grid, block, 0, g->stream>>>(a, (const int32_t *)val, out);
    else k_factor_values<int8_t><<<grid, block, 0, g->stream>>>(a, (const int8_t *)val, out);
    HIPCHECK(hipGetLastError());
    return NSK_OK;
}
