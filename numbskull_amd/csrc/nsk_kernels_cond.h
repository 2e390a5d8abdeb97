// nsk_kernels_cond.h -- the conditionals the sampler draws from (nsk_conditionals / the accumulators of a sample trace,
// nsk_trace_conditionals): for a selected variable v of cardinality C at position p and a state x,
//   p_k = potential(v, k, x), k = 0 .. C - 1: the walk of list slot p_slot[p] + k * (dataType == 1) that draw_sample
//         performs (nsk_device.h; one walk of the shared list for a binary dataType-0 variable, potential2),
//   e_k = nsk_exp(p_k), unshifted;  Z = e_0, Z + e_1, ... in k order;  P_k = e_k / Z, one IEEE division.
// Z = 0, infinite or NaN gives what IEEE gives -- the sampler's own degenerate case, not treated specially.  Above
// NSK_ZLOCAL values the potentials are computed twice (Z, then the quotients), as draw_sample does; no scratch memory.
//
// One lane per selected device column (selections are sorted by position, so neighbouring lanes gather neighbouring
// values), grid-stride; blockIdx.y = chain: chain r's values lie at val + r * chain_stride BYTES, its output at
// out + r * total.  Column i owns the doubles [off[i], off[i + 1]) of a chain's output; no two lanes share one, so the
// accumulating flavour (S = S + P_k, once per launch) needs no atomics and its sums are reproducible.
#pragma once

#include "nsk_device.h"
#include "nsk_kernels_energy.h"     // PackedByte
#include "nsk_kernels_gibbs.h"      // NSK_BLOCK

namespace nsk {

enum : int { COND_POTENTIALS = 0, COND_PROBABILITIES = 1, COND_ACCUMULATE = 2 };

// what the walk reads of a handle, and the selection
struct CondArgs {
    const uint32_t *p_info;
    const int32_t *p_slot, *slot_off, *fidx;
    const uint4 *f_rec;
    const int2 *m_rec;
    const int32_t *v_card, *iid_of_vid;     // iid_of_vid: null unless a reachable factor reads its head at the literal edge index
    double *w;
    const double *logtab;
    const int32_t *sel;                     // [nsel] device column -> position, ascending
    const long long *off;                   // [nsel + 1] its first double in a chain's output
    long long nsel, total, chain_stride;
    int head_by_vid;
};

template <typename VT>
__device__ __forceinline__ DevGraph<VT> cond_view(const CondArgs &a) {
    DevGraph<VT> g = {};
    g.p_info = a.p_info; g.p_slot = a.p_slot; g.slot_off = a.slot_off; g.fidx = a.fidx;
    g.f_rec = a.f_rec; g.m_rec = a.m_rec; g.v_card = a.v_card; g.w = a.w; g.logtab = a.logtab;
    g.iid_of_vid = a.iid_of_vid; g.head_by_vid = a.head_by_vid;
    return g;
}

template <int MODE>
__device__ __forceinline__ void cond_store(double *d, double x) {
    if (MODE == COND_ACCUMULATE) *d = *d + x;
    else *d = x;
}

template <typename VT, int MODE>
__global__ __launch_bounds__(NSK_BLOCK) void k_cond(const CondArgs a, const VT *val, double *out) {
    const DevGraph<VT> g = cond_view<VT>(a);
    const VT *v = (const VT *)((const char *)val + (long long)blockIdx.y * a.chain_stride);
    double *o = out + (long long)blockIdx.y * a.total;
    for (long long i = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; i < a.nsel; i += (long long)gridDim.x * NSK_BLOCK) {
        const int p = a.sel[i];
        const uint32_t info = g.p_info[p];
        const int card = NSK_INFO_CARD(info), step = (int)NSK_INFO_DT1(info), slot0 = g.p_slot[p];
        double *d = o + a.off[i];           // (the host has checked off[i + 1] - off[i] == card)
        if (card == 2 && !step) {
            double p0, p1;
            potential2(g, p, slot0, v, p0, p1);
            if (MODE == COND_POTENTIALS) { d[0] = p0; d[1] = p1; continue; }
            const double e0 = nsk_exp(p0), e1 = nsk_exp(p1);
            const double z = e0 + e1;
            cond_store<MODE>(d, e0 / z);
            cond_store<MODE>(d + 1, e1 / z);
            continue;
        }
        if (MODE == COND_POTENTIALS) {
            for (int k = 0; k < card; k++) d[k] = potential(g, p, k, slot0 + step * k, v);
            continue;
        }
        if (card <= NSK_ZLOCAL) {
            double E[NSK_ZLOCAL];
            double z = 0.0;
            for (int k = 0; k < card; k++) {
                const double ek = nsk_exp(potential(g, p, k, slot0 + step * k, v));
                z = (k == 0) ? ek : z + ek;
                E[k] = ek;
            }
            for (int k = 0; k < card; k++) cond_store<MODE>(d + k, E[k] / z);
            continue;
        }
        // large domains: two passes, the second recomputes the identical potentials
        double z = 0.0;
        for (int k = 0; k < card; k++) {
            const double ek = nsk_exp(potential(g, p, k, slot0 + step * k, v));
            z = (k == 0) ? ek : z + ek;
        }
        for (int k = 0; k < card; k++) {
            const double ek = nsk_exp(potential(g, p, k, slot0 + step * k, v));
            cond_store<MODE>(d + k, ek / z);
        }
    }
}

}  // namespace nsk
