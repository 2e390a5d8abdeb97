// nsk_kernels_energy.h -- the log-potential of a state, sum over ALL factors of weight[f.weightId] * eval_factor(f, state)
// (nsk_log_potential / nsk_factor_values / the lp column of a sample trace), evaluated factor by factor.
//
// One lane per factor, grid-stride in ascending factor id: f_rec[f] (16 bytes, coalesced), the factor's m_rec entries, the
// members' values, and eval_factor -- the very function the sweep kernels call -- as the factor's FIRST member sees it
// at its current value (var_samp = that member, value = its value; no member: var_samp = -1, and no internal id is
// negative).  Every member reads as it is either way; the one place where the asker matters is the reference's literal
// head lookup (head_member): a factor whose head IS its first member takes the head's value from the variable, not
// from var_value[edge index], exactly as it does whenever that variable is sampled.  The term is ONE rounded product
// w[rec.z] * e_f (the library is compiled with -ffp-contract=off), as in potential().
//
// The sum is reproducible: a function of graph, weights and state only.  The grid is a function of nfactor alone
// (nsk_internal.h nsk_energy_blocks); a lane adds its own factors in ascending order, the wave adds its lanes in a
// butterfly (every lane performs the same six rounds of x + partner, so all end with the same double), the block adds
// its four waves in wave order through LDS, and k_energy_reduce adds the block partials the same way: thread t the partials t, t + 256, ... in
// ascending order, butterfly, waves in order.  No floating-point atomics; nothing depends on which CU or XCD ran what.
// blockIdx.y = chain: chain r's values lie at val + r * chain_stride BYTES, its partials at partial + r * gridDim.x.
#pragma once

#include "nsk_device.h"
#include "nsk_kernels_gibbs.h"      // NSK_BLOCK

namespace nsk {

// A value byte of a handle that keeps its tally in bits 1-7 of the value bytes while a traced call runs (k_unpack_tally):
// bit 0 is the value.  eval_factor<PackedByte> reads members through the conversion.
struct PackedByte {
    signed char b;
    __device__ __forceinline__ operator int() const { return (int)(b & 1); }
};

// what the walk reads of a handle
struct EnergyArgs {
    const uint4 *f_rec;
    const int2 *m_rec;
    const int32_t *v_card, *iid_of_vid;     // iid_of_vid: null unless a factor reads its head at the literal edge index
    const double *w, *logtab;
    long long nfactor, chain_stride;
    int head_by_vid;
};

template <typename VT>
__device__ __forceinline__ DevGraph<VT> energy_view(const EnergyArgs &a) {
    DevGraph<VT> g = {};
    g.m_rec = a.m_rec; g.v_card = a.v_card; g.iid_of_vid = a.iid_of_vid; g.logtab = a.logtab;
    g.head_by_vid = a.head_by_vid;
    return g;
}

// the value of factor `rec` on the state `val`, as its first member sees it (above)
template <typename VT>
__device__ __forceinline__ double energy_factor(const DevGraph<VT> &g, const uint4 rec, const int2 *mb, const VT *val) {
    int var_samp = -1, value = 0;
    if (NSK_FHEAD_ARITY(rec.x) > 0 && NSK_FHEAD_FUNC(rec.x) != F_NOOP) {
        var_samp = mb[(int)rec.y].x;
        value = (int)val[var_samp];
    }
    return eval_factor(g, rec, mb, var_samp, value, val);
}

// sum of the block's 256 values, the same double in every thread of wave 0 (thread 0 stores it)
__device__ __forceinline__ double energy_block_sum(double x, double *lds) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) x = x + __shfl_xor(x, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = lds[0];
#pragma unroll
    for (int k = 1; k < NSK_BLOCK / 64; k++) s = s + lds[k];
    return s;
}

// The blocks are dealt round-robin to the 8 XCDs: every XCD walks one contiguous eighth of each round of the grid, so the
// value lines neighbouring factors share are fetched into one L2 (xcd_logical_block; gridDim.x is a multiple of 8).
template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_energy_partial(const EnergyArgs a, const VT *val, double *partial) {
    __shared__ double lds[NSK_BLOCK / 64];
    const DevGraph<VT> g = energy_view<VT>(a);
    const VT *v = (const VT *)((const char *)val + (long long)blockIdx.y * a.chain_stride);
    const long long lb = xcd_logical_block((int)blockIdx.x, (int)gridDim.x);
    double acc = 0.0;
    for (long long f = lb * NSK_BLOCK + threadIdx.x; f < a.nfactor; f += (long long)gridDim.x * NSK_BLOCK) {
        const uint4 rec = a.f_rec[f];
        const double t = a.w[rec.z] * energy_factor(g, rec, a.m_rec, v);
        acc = acc + t;
    }
    const double s = energy_block_sum(acc, lds);
    if (threadIdx.x == 0) partial[(long long)blockIdx.y * gridDim.x + lb] = s;
}

// one block per chain: out[chain] = the sum of the chain's nparts block partials
static __global__ __launch_bounds__(NSK_BLOCK) void k_energy_reduce(const double *partial, int nparts, double *out) {
    __shared__ double lds[NSK_BLOCK / 64];
    const double *p = partial + (long long)blockIdx.x * nparts;
    double acc = 0.0;
    for (int i = (int)threadIdx.x; i < nparts; i += NSK_BLOCK) acc = acc + p[i];
    const double s = energy_block_sum(acc, lds);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// the same walk, e_f of every factor stored instead of summed (one chain)
template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_factor_values(const EnergyArgs a, const VT *val, double *out) {
    const DevGraph<VT> g = energy_view<VT>(a);
    for (long long f = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; f < a.nfactor; f += (long long)gridDim.x * NSK_BLOCK)
        out[f] = energy_factor(g, a.f_rec[f], a.m_rec, val);
}

}  // namespace nsk
