// nsk_kernels_wstats.h -- per-weight sufficient statistics of a state, S_w = sum over the factors f with weightId == w of
// e_f (nsk_weight_stats / the stats column of a sample trace): the log-potential's sum, split by weight.
//
// e_f is energy_factor (nsk_kernels_energy.h): the factor as its first member sees it.  With `feat` set every term is
// the ONE rounded product feat[f] * e_f (-ffp-contract=off).  The factors of a weight are read through the by-weight
// index list wf_idx (factor ids ascending inside a weight); a PLAN (nsk_internal.h NskWstatsPlan) names the work:
//
//   shorts   one LANE per weight of at most NSK_WSTATS_SHORT factors: the lane adds its entries in ascending order and
//            stores the sum.  The items are sorted by length (len_end[k] = items of length <= k + 1), so the lanes of
//            a wave finish together, and by first factor id inside a length, so neighbouring lanes read neighbouring
//            records.
//   pieces   one WAVE per piece of at most NSK_WSTATS_PIECE entries of ONE longer weight: lane l adds the entries
//            l, l + 64, ... in ascending order, then the six rounds of x + partner of energy_block_sum's butterfly
//            (every lane performs the same additions).  A weight of one piece stores its sum, a piece of a longer
//            weight its partial.
//   multi    one wave per weight of several pieces (k_wstats_reduce, a second launch): lane l adds the partials
//            l, l + 64, ... in piece order, then the same butterfly.
//
// How a weight is cut depends on its own length alone, so S_w is a function of graph, state and `feat` only: the same
// bits for any chain, chain count, selection of weights, query or trace row, run, CU or XCD.  No floating-point
// atomics, no constant taken from the device.  blockIdx.y = chain: values at val + r * chain_stride BYTES, sums at
// out + r * out_stride, partials at partial + r * npartial.
#pragma once

#include "nsk_internal.h"          // NSK_WSTATS_SHORT, NSK_WSTATS_PIECE
#include "nsk_kernels_energy.h"

namespace nsk {

struct WstatsArgs {
    EnergyArgs e;
    const int32_t *wf_idx;          // factor ids by weight
    const double *feat;             // featureValue per factor, or null: the terms are e_f
    const uint2 *shorts;            // {first entry in wf_idx, output column}
    const uint4 *pieces;            // {first entry, entries, output column or partial index, 1: partial}
    const uint4 *multi;             // {first partial, partials, output column, 0}
    unsigned int len_end[NSK_WSTATS_SHORT];     // shorts [len_end[k - 1], len_end[k]) have k + 1 entries
    long long nshort, npiece, nmulti, npartial, out_stride;
};

template <typename VT>
__device__ __forceinline__ double wstats_term(const WstatsArgs &a, const DevGraph<VT> &g, const VT *v, long long entry) {
    const int f = a.wf_idx[entry];
    const double e = energy_factor(g, a.e.f_rec[f], a.e.m_rec, v);
    return a.feat ? a.feat[f] * e : e;
}

__device__ __forceinline__ double wstats_wave_sum(double x) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) x = x + __shfl_xor(x, off, 64);
    return x;
}

// gridDim.x is a multiple of 8: every XCD walks one contiguous eighth of each round of the items (xcd_logical_block)
template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_wstats_short(const WstatsArgs a, const VT *val, double *out) {
    const DevGraph<VT> g = energy_view<VT>(a.e);
    const VT *v = (const VT *)((const char *)val + (long long)blockIdx.y * a.e.chain_stride);
    double *o = out + (long long)blockIdx.y * a.out_stride;
    const long long lb = xcd_logical_block((int)blockIdx.x, (int)gridDim.x);
    for (long long i = lb * NSK_BLOCK + threadIdx.x; i < a.nshort; i += (long long)gridDim.x * NSK_BLOCK) {
        const uint2 it = a.shorts[i];
        int len = 1;
#pragma unroll
        for (int k = 0; k < NSK_WSTATS_SHORT - 1; k++) len += i >= (long long)a.len_end[k] ? 1 : 0;
        double acc = 0.0;
        for (int k = 0; k < len; k++) acc = acc + wstats_term(a, g, v, (long long)it.x + k);
        o[it.y] = acc;
    }
}

template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_wstats_piece(const WstatsArgs a, const VT *val, double *out, double *partial) {
    const DevGraph<VT> g = energy_view<VT>(a.e);
    const VT *v = (const VT *)((const char *)val + (long long)blockIdx.y * a.e.chain_stride);
    const long long lb = xcd_logical_block((int)blockIdx.x, (int)gridDim.x);
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int per = NSK_BLOCK / 64;
    for (long long p = lb * per + wave; p < a.npiece; p += (long long)gridDim.x * per) {
        const uint4 it = a.pieces[p];
        double acc = 0.0;
        for (unsigned int k = (unsigned int)lane; k < it.y; k += 64u) acc = acc + wstats_term(a, g, v, (long long)it.x + k);
        const double s = wstats_wave_sum(acc);
        if (lane == 0) {
            if (it.w) partial[(long long)blockIdx.y * a.npartial + it.z] = s;
            else out[(long long)blockIdx.y * a.out_stride + it.z] = s;
        }
    }
}

static __global__ __launch_bounds__(NSK_BLOCK) void k_wstats_reduce(const WstatsArgs a, const double *partial, double *out) {
    const int lane = (int)(threadIdx.x & 63);
    const long long m = (long long)blockIdx.x * (NSK_BLOCK / 64) + (threadIdx.x >> 6);
    if (m >= a.nmulti) return;
    const uint4 it = a.multi[m];
    const double *p = partial + (long long)blockIdx.y * a.npartial + it.x;
    double acc = 0.0;
    for (unsigned int k = (unsigned int)lane; k < it.y; k += 64u) acc = acc + p[k];
    const double s = wstats_wave_sum(acc);
    if (lane == 0) out[(long long)blockIdx.y * a.out_stride + it.z] = s;
}

}  // namespace nsk
