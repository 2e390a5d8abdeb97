// nsk_kernels_icm.h -- iterated conditional modes (nsk_icm): greedy coordinate ascent on the potentials the sampler
// exponentiates, deterministic, no random numbers, no exponential.
//
// The rule.  One ICM sweep visits the colour classes in colour order, as the chromatic scan does; inside a class every
// eligible variable is decided in parallel -- a variable reads none of its own class, so the parallel decision is the
// sequential one.  A position p is eligible when p_vid[p] >= 0 and NSK_INFO_EV(p_info[p]) == 0 || sample_evidence (the
// test of the sweep kernels).  For an eligible variable v of cardinality C with current value cur:
//   p_k = potential(v, k, x), k = 0 .. C - 1: the doubles nsk_conditionals(what = 0) returns, by the same walk
//         (nsk_device.h; both potentials of a binary dataType-0 variable from one potential2 walk);
//   best = cur, best_p = p_cur when 0 <= cur < C, else best = 0, best_p = p_0;
//   for k ascending: if (p_k > best_p) { best = k; best_p = p_k; }
// so a move happens on strict improvement only, the smallest k wins among several maxima, and a NaN potential never
// wins (nor is a NaN incumbent ever left: no comparison with it holds).  One pass serves any cardinality: nothing is
// kept per value.  (The incumbent's own k is skipped in the loop: best_p never falls below p_cur, so its comparison
// cannot hold.)  The lane stores best only where it differs from cur -- a plain store of the value type, the only
// thing written besides the counter -- and counts the change.
//
// One lane per position of the class's range [lo, hi), grid-stride; blockIdx.y = chain: chain r's values lie at
// val + r * chain_stride BYTES.  Changes: the lanes' counts are added over the wave (butterfly) and the block (LDS), and
// the block adds its total to cur[chain] with at most ONE integer atomicAdd -- integers, so the order does not matter.
// Early exit without the host: prev != null is the counter row of the sweep before; where prev[chain] == 0 that chain
// has reached its fixed point, no later sweep can change it, and the block returns after that one scalar load
// (block-uniform, before any barrier).  Its own counter then stays 0, which ends the sweeps after it the same way.
#pragma once

#include "nsk_kernels_cond.h"       // CondArgs, cond_view: what the walk reads of a handle

namespace nsk {

template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_icm(const CondArgs a, const int32_t *p_vid, VT *val, long long lo, long long hi,
                                                   int sample_evidence, const long long *prev, unsigned long long *cur) {
    __shared__ int lds[NSK_BLOCK / 64];
    if (prev && prev[blockIdx.y] == 0) return;
    const DevGraph<VT> g = cond_view<VT>(a);
    VT *v = (VT *)((char *)val + (long long)blockIdx.y * a.chain_stride);
    int nchanged = 0;
    for (long long i = lo + (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; i < hi; i += (long long)gridDim.x * NSK_BLOCK) {
        const int p = (int)i;
        if (p_vid[p] < 0) continue;
        const uint32_t info = g.p_info[p];
        if (!(NSK_INFO_EV(info) == 0 || sample_evidence)) continue;
        const int card = NSK_INFO_CARD(info), step = (int)NSK_INFO_DT1(info), slot0 = g.p_slot[p];
        const int x = (int)v[p];
        const int first = (x >= 0 && x < card) ? x : 0;
        int best = first;
        if (card == 2 && !step) {
            double p0, p1;
            potential2(g, p, slot0, v, p0, p1);
            double best_p = first ? p1 : p0;
            if (p0 > best_p) { best = 0; best_p = p0; }
            if (p1 > best_p) { best = 1; best_p = p1; }
        } else {
            double best_p = potential(g, p, first, slot0 + step * first, v);
            for (int k = 0; k < card; k++) {
                if (k == first) continue;
                const double pk = potential(g, p, k, slot0 + step * k, v);
                if (pk > best_p) { best = k; best_p = pk; }
            }
        }
        if (best != x) { v[p] = (VT)best; nchanged++; }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) nchanged += __shfl_xor(nchanged, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = nchanged;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = lds[0];
#pragma unroll
        for (int k = 1; k < NSK_BLOCK / 64; k++) s += lds[k];
        if (s > 0) atomicAdd(cur + blockIdx.y, (unsigned long long)s);
    }
}

}  // namespace nsk
