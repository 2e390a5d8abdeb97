// nsk_kernels_pcd.h -- the chain-summed per-weight moments in fixed point (nsk_weight_moments) and the full-batch
// maximum-likelihood learner built on them, persistent contrastive divergence (nsk_pcd_steps).
//
// The rule.  For a state x and a factor f, e_f is energy_factor (nsk_kernels_energy.h): the factor as its first member
// sees it, what nsk_log_potential and nsk_weight_stats evaluate.  Then
//   q_f = __double2ll_rn(e_f * 2^32)         round to nearest even (the scaling is exact)
//   M[weight slot of f] += q_f               int64, over every factor of every chain named
// The sums are integers: no order of execution changes a bit, and one accumulator of nweight x 8 bytes serves any number
// of chains.  The host has checked that no sum can leave int64 (nsk_pcd.hip: B_w * nchains < 2^30).
//
// The factors of a weight are read through the by-weight list of the statistics (NskWstats::wf_idx), cut the way the
// statistics cut them (NSK_WSTATS_SHORT, NSK_WSTATS_PIECE), by weight SLOT:
//   k_moments_short   one LANE per weight of at most NSK_WSTATS_SHORT factors; the items are sorted by length and by first
//                     factor, as the statistics' are.  The lane adds its weight's factors -- every record read once,
//                     evaluated on the chains blockIdx.y, blockIdx.y + gridDim.y, ... -- in a register and issues ONE
//                     global atomic.
//   k_moments_piece   one WAVE per piece of at most NSK_WSTATS_PIECE entries of one longer weight: lane l adds the entries
//                     l, l + 64, ... of the same chains, the wave adds its lanes' integers in a butterfly.  A wave walks
//                     its pieces in ascending order (the grid is capped, nsk_moments_blocks) and keeps adding in a
//                     register while consecutive pieces name one slot; what a block's waves hold at the end meets in LDS
//                     and equal slots leave as one atomic.  So a wave issues at most one global atomic per weight it
//                     holds, and a single-weight graph of any size at most one per block and chain group.
// gridDim.y = the chain groups (nsk_moments_chain_groups): every chain its own while the items are few, fewer groups
// once the items alone fill the device, so that the atomics do not multiply with the chains.
//
// k_pcd_update: one lane per weight slot, not for a fixed weight.  Every line is one rounded IEEE operation:
//   m = ((double)M * 2^-32) / n              one conversion, an exact scaling, one division: the model's mean over n chains
//   g = pos - m;  if (normalize) g = g / n_w
//   w = step_weight(w, g, step, reg_param)   the rule of every learner (nsk_kernels_step.h)
// pos is target[slot], or with the sums Mc of a clamped population (latent variables) ((double)Mc * 2^-32) / nclamped.
// gmax = the largest |g| over those weights: |g| is a non-negative finite double, whose bit pattern orders as an
// unsigned integer (step_block_max).  With `mout` the step's sums are kept: M, or Mc then M.
//
// Latent variables (nsk_pcd_latent_steps): k_pcd_clamp writes the initial values of the evidence variables into the
// clamped chains.
#pragma once

#include "nsk_internal.h"          // NSK_WSTATS_SHORT, NSK_WSTATS_PIECE
#include "nsk_kernels_energy.h"
#include "nsk_kernels_step.h"

namespace nsk {

// The grids: one item per lane (shorts) or wave (pieces) up to NSK_MOMENTS_MAX_BLOCKS blocks (8 per CU), whole rounds of
// XCDs (xcd_logical_block); more items loop.  cap > 0 (diagnostic, NSK_MOMENTS_GRID_CAP, blocks): at most that many,
// rounded down to whole rounds of XCDs but at least one -- the later trips at small shapes.
#define NSK_MOMENTS_MAX_BLOCKS 2048
static inline unsigned int nsk_moments_blocks(long long items, long long per_block, int cap) {
    const long long need = ((items + per_block - 1) / per_block + 7) / 8 * 8;
    const long long limit = cap > 0 ? std::max(8ll, std::min<long long>(NSK_MOMENTS_MAX_BLOCKS, cap / 8 * 8)) : NSK_MOMENTS_MAX_BLOCKS;
    return (unsigned int)std::max(8ll, std::min(need, limit));
}
static inline long long nsk_moments_trips(long long items, long long per_block, int cap) {
    const long long per_trip = (long long)nsk_moments_blocks(items, per_block, cap) * per_block;
    return (items + per_trip - 1) / per_trip;
}
// chain groups of a launch of `blocks` blocks: as many as keep about NSK_MOMENTS_MAX_BLOCKS blocks in flight
static inline unsigned int nsk_moments_chain_groups(unsigned int blocks, long long nchains) {
    const long long want = (NSK_MOMENTS_MAX_BLOCKS + blocks - 1) / blocks;
    return (unsigned int)std::max(1ll, std::min(nchains, want));
}

struct MomentsArgs {
    EnergyArgs e;
    const int32_t *wf_idx;          // factor ids by weight slot
    const uint2 *shorts;            // {first entry in wf_idx, weight slot}
    const uint4 *pieces;            // {first entry, entries, weight slot, 0}, ascending by slot and entry
    unsigned int len_end[NSK_WSTATS_SHORT];     // shorts [len_end[k - 1], len_end[k]) have k + 1 entries
    long long nshort, npiece;
    int nchains;
};

// the terms of one entry of the by-weight list over the chains r0, r0 + dr, ...: the record is read once, and the
// chains' value loads are independent of one another
template <typename VT>
__device__ __forceinline__ long long moments_term(const MomentsArgs &a, const DevGraph<VT> &g, const VT *val, long long entry, int r0, int dr) {
    const uint4 rec = a.e.f_rec[a.wf_idx[entry]];
    long long acc = 0;
    for (int r = r0; r < a.nchains; r += dr) {
        const VT *v = (const VT *)((const char *)val + (long long)r * a.e.chain_stride);
        acc += __double2ll_rn(energy_factor(g, rec, a.e.m_rec, v) * NSK_GRAD_SCALE);
    }
    return acc;
}

__device__ __forceinline__ void moments_add(unsigned long long *M, unsigned int slot, long long x) {
    if (x != 0) (void)__hip_atomic_fetch_add(M + slot, (unsigned long long)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_moments_short(const MomentsArgs a, const VT *val, unsigned long long *M) {
    const DevGraph<VT> g = energy_view<VT>(a.e);
    const long long lb = xcd_logical_block((int)blockIdx.x, (int)gridDim.x);
    for (long long i = lb * NSK_BLOCK + threadIdx.x; i < a.nshort; i += (long long)gridDim.x * NSK_BLOCK) {
        const uint2 it = a.shorts[i];
        int len = 1;
#pragma unroll
        for (int k = 0; k < NSK_WSTATS_SHORT - 1; k++) len += i >= (long long)a.len_end[k] ? 1 : 0;
        long long acc = 0;
        for (int k = 0; k < len; k++) acc += moments_term(a, g, val, (long long)it.x + k, (int)blockIdx.y, (int)gridDim.y);
        moments_add(M, it.y, acc);
    }
}

template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_moments_piece(const MomentsArgs a, const VT *val, unsigned long long *M) {
    __shared__ long long lds_run[NSK_BLOCK / 64];
    __shared__ int lds_slot[NSK_BLOCK / 64];
    const DevGraph<VT> g = energy_view<VT>(a.e);
    const long long lb = xcd_logical_block((int)blockIdx.x, (int)gridDim.x);
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int per = NSK_BLOCK / 64;
    int slot = -1;                  // the slot of the running sum (wave-uniform; -1: none yet)
    long long run = 0;              // ... which every lane holds alike
    for (long long p = lb * per + wave; p < a.npiece; p += (long long)gridDim.x * per) {
        const uint4 it = a.pieces[p];
        long long acc = 0;
        for (unsigned int k = (unsigned int)lane; k < it.y; k += 64u) acc += moments_term(a, g, val, (long long)it.x + k, (int)blockIdx.y, (int)gridDim.y);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off, 64);
        if ((int)it.z != slot) {
            if (lane == 0 && slot >= 0) moments_add(M, (unsigned int)slot, run);
            slot = (int)it.z; run = 0;
        }
        run += acc;
    }
    if (lane == 0) { lds_slot[wave] = slot; lds_run[wave] = run; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < per; k++) {
            const int s = lds_slot[k];
            if (s < 0) continue;
            long long x = lds_run[k];
            for (int j = k + 1; j < per; j++)
                if (lds_slot[j] == s) { x += lds_run[j]; lds_slot[j] = -1; }
            moments_add(M, (unsigned int)s, x);
        }
    }
}

// One step's update (see the top of the file): M, Mc (null: target is read), target, nfac by slot; gmax this step's
// output, zeroed by the host; mout (may be null) this step's row(s) of the kept moments
static __global__ __launch_bounds__(NSK_BLOCK) void k_pcd_update(const long long *M, double nchains, const long long *Mc, double nclamped,
                                                                 const double *target, const double *nfac, int nweight, double *w,
                                                                 const uint8_t *w_fixed, int normalize, double step, double reg_param,
                                                                 unsigned long long *gmax, long long *mout) {
    const int s = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x);
    unsigned long long mag = 0ull;
    if (s < nweight) {
        const long long S = M[s], Sc = Mc ? Mc[s] : 0;
        if (mout) {
            if (Mc) { mout[s] = Sc; mout[nweight + s] = S; }
            else mout[s] = S;
        }
        if (!w_fixed[s]) {
            const double pos = Mc ? ((double)Sc * (1.0 / NSK_GRAD_SCALE)) / nclamped : target[s];
            const double m = ((double)S * (1.0 / NSK_GRAD_SCALE)) / nchains;
            double gr = pos - m;
            if (normalize) gr = gr / nfac[s];
            w[s] = step_weight(w[s], gr, step, reg_param);
            mag = (unsigned long long)__double_as_longlong(fabs(gr));
        }
    }
    step_block_max<NSK_BLOCK>(mag, gmax);
}

// ---- latent variables (nsk_pcd_latent_steps): a clamped and a free population of chains ----
// The clamp: pairs = {internal id, value} of every variable with isEvidence 1, 2 or 3, built by the host for the call;
// chain r < nchains of the chains that start at `val` gets every value written.  One lane per pair and chain group
// (blockIdx.y, as the moment launches), more pairs loop.
template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_pcd_clamp(VT *val, long long chain_stride, int nchains, const int2 *pairs, long long npairs) {
    for (long long i = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; i < npairs; i += (long long)gridDim.x * NSK_BLOCK) {
        const int2 p = pairs[i];
        for (int r = (int)blockIdx.y; r < nchains; r += (int)gridDim.y)
            ((VT *)((char *)val + (long long)r * chain_stride))[p.x] = (VT)p.y;
    }
}

}  // namespace nsk
