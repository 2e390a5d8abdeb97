// nsk_kernels_plgrad.h -- the gradient of the log-pseudo-likelihood with respect to the weights (nsk_pl_gradient) and the
// deterministic learner built on it, maximum pseudo-likelihood (nsk_mple_steps).
//
// The rule.  For a state x, the weight table w and a selected variable v at position p, cardinality C, own value
// cur = x_v: P_k, k = 0 .. C - 1, are the very bits nsk_conditionals(what = 1) returns for v -- the same walk (potential2
// for a binary dataType-0 variable, potential otherwise), the same unshifted nsk_exp, the same running Z in k order, one
// IEEE division (nsk_kernels_cond.h; up to NSK_ZLOCAL values the exponentials wait in registers, above that the
// potentials are computed twice).  The variable is SKIPPED -- it adds nothing, and one to the chain's `skipped` -- when
// cur lies outside [0, C) or Z is not a finite positive number.  Otherwise, for k = 0 .. C - 1 and every entry j of list
// slot p_slot[p] + k * (dataType == 1), f = fidx[j]:
//   c_k = (k == cur ? 1.0 : 0.0) - P_k       one rounded subtraction
//   e   = eval_factor(f, v, k, x)            as potential() calls it, head quirks included
//   t   = c_k * e                            one rounded product
//   q   = __double2ll_rn(t * 2^32)           round to nearest even (the scaling is exact)
//   G[chain][weight slot of f] += q          int64
// G * 2^-32 is the derivative of sum_v log P(x_v | the others) over the selection, to within 2^-33 per term.  Fixed
// weights get their sum like any other; featureValue plays no part, as in potential().  With the literal head lookup
// (IMPLY_MLN-type functions without NSK_FLAG_HEAD_BY_VID) this is the derivative of the sum of the SAMPLER'S OWN
// conditionals, which are then not the conditionals of one joint energy -- the limit nsk_icm states.
// The sums are integers: no order of execution changes a bit.  (A binary dataType-0 variable's two values share one
// list, walked once with both terms per entry -- the same integers in another order.)
//
// k_plgrad: one lane per selected position (the selection is sorted by position), grid-stride (nsk_plgrad_blocks),
// blockIdx.y = chain: chain r's values lie at val + r * chain_stride BYTES, its sums at G + r * nweight.  A lane adds in
// a register while consecutive entries name the same weight slot and flushes on a change of slot: with at most
// NSK_PLGRAD_BINS weights into int64 bins in LDS (64-bit ds adds), which the block adds to G after a barrier, one global
// 64-bit atomic per non-zero bin; with more weights straight to G (the contention is spread then).  Both paths give the
// same integers.  The host has checked that no sum can leave int64 (nsk_plgrad.hip: B_w * nchains < 2^30).  skipped:
// the lanes' counts are added over the wave and the block, one integer atomic per block and chain.
//
// k_mple_update: one lane per weight slot.  S = the int64 sum of G[r][slot] over the call's chains (exact);
//   gbar = ((double)S * 2^-32) / N           one conversion, an exact scaling, one rounded division
//   w = step_weight(w, gbar, step, reg_param)                          the rule of every learner (nsk_kernels_step.h); not for a fixed weight
// and gmax = the largest |S| over the weights that are not fixed (step_block_max).
#pragma once

#include "nsk_kernels_cond.h"       // CondArgs, cond_view: what the walk reads of a handle
#include "nsk_kernels_step.h"

namespace nsk {

#define NSK_PLGRAD_BINS 256         // handles with at most this many weights accumulate per block in LDS
// The grid of k_plgrad, per chain: one position per lane until every CU has a block (NSK_PLGRAD_CU_BLOCKS); from there on
// lanes take a second position before the grid grows -- a lane's run of equal weight slots and its block's flush of the
// bins are shared by what it serves -- up to NSK_PLGRAD_MAX_BLOCKS blocks (8 per CU); a longer selection loops further.
// (10M grid, one chain: 1.1-1.4 ms at 2048 blocks against 2.5 ms at 256; 10 000 variables: 20 us with one position per
// lane against 34 us with two -- DESIGN.md section 4)
#define NSK_PLGRAD_CU_BLOCKS 256
#define NSK_PLGRAD_MAX_BLOCKS 2048
static inline unsigned int nsk_plgrad_blocks(long long nsel) {
    const long long one = (nsel + NSK_BLOCK - 1) / NSK_BLOCK, two = (one + 1) / 2;
    if (one <= NSK_PLGRAD_CU_BLOCKS) return (unsigned int)(one < 1 ? 1 : one);
    return (unsigned int)(two < NSK_PLGRAD_CU_BLOCKS ? NSK_PLGRAD_CU_BLOCKS : (two > NSK_PLGRAD_MAX_BLOCKS ? NSK_PLGRAD_MAX_BLOCKS : two));
}

struct PlgradSink {
    unsigned long long *bins;       // LDS bins, or null: straight to G
    unsigned long long *G;          // this chain's sums
    int slot;                       // the weight slot of the running sum (-1: none yet)
    long long run;
    __device__ __forceinline__ void flush() {
        if (slot < 0 || run == 0) return;
        if (bins) (void)__hip_atomic_fetch_add(bins + slot, (unsigned long long)run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else (void)__hip_atomic_fetch_add(G + slot, (unsigned long long)run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void add(int s, long long q) {
        if (s != slot) { flush(); slot = s; run = 0; }
        run += q;
    }
};

__device__ __forceinline__ long long plgrad_term(double ck, double e) {
    const double t = ck * e;
    return __double2ll_rn(t * NSK_GRAD_SCALE);
}

// the terms of value k: the walk of one list slot
template <typename VT>
__device__ __forceinline__ void plgrad_walk(const DevGraph<VT> &g, int p, int k, int slot, const VT *v, double ck, PlgradSink &sk) {
    const int b = g.slot_off[slot], e = g.slot_off[slot + 1];
    for (int j = b; j < e; j++) {
        const uint4 rec = g.f_rec[g.fidx[j]];
        sk.add((int)rec.z, plgrad_term(ck, eval_factor(g, rec, g.m_rec, p, k, v)));
    }
}

template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_plgrad(const CondArgs a, const VT *val, int nweight, unsigned long long *G,
                                                      unsigned long long *skipped) {
    __shared__ unsigned long long bins[NSK_PLGRAD_BINS];
    __shared__ int lds[NSK_BLOCK / 64];
    const bool binned = nweight <= NSK_PLGRAD_BINS;         // (block-uniform)
    if (binned) {
        for (int i = threadIdx.x; i < NSK_PLGRAD_BINS; i += NSK_BLOCK) bins[i] = 0ull;
        __syncthreads();
    }
    const DevGraph<VT> g = cond_view<VT>(a);
    const VT *v = (const VT *)((const char *)val + (long long)blockIdx.y * a.chain_stride);
    PlgradSink sk;
    sk.bins = binned ? bins : nullptr;
    sk.G = G + (long long)blockIdx.y * nweight;
    sk.slot = -1; sk.run = 0;
    int nskipped = 0;
    for (long long i = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; i < a.nsel; i += (long long)gridDim.x * NSK_BLOCK) {
        const int p = a.sel[i];
        const uint32_t info = g.p_info[p];
        const int card = NSK_INFO_CARD(info), step = (int)NSK_INFO_DT1(info), slot0 = g.p_slot[p];
        const int cur = (int)v[p];
        if (cur < 0 || cur >= card) { nskipped++; continue; }
        if (card == 2 && !step) {
            double p0, p1;
            potential2(g, p, slot0, v, p0, p1);
            const double e0 = nsk_exp(p0), e1 = nsk_exp(p1);
            const double z = e0 + e1;
            if (!(z > 0.0 && z < __longlong_as_double(0x7ff0000000000000LL))) { nskipped++; continue; }
            const double c0 = (cur == 0 ? 1.0 : 0.0) - e0 / z, c1 = (cur == 1 ? 1.0 : 0.0) - e1 / z;
            const int b = g.slot_off[slot0], e = g.slot_off[slot0 + 1];
            for (int j = b; j < e; j++) {
                const uint4 rec = g.f_rec[g.fidx[j]];
                const long long q0 = plgrad_term(c0, eval_factor(g, rec, g.m_rec, p, 0, v));
                const long long q1 = plgrad_term(c1, eval_factor(g, rec, g.m_rec, p, 1, v));
                sk.add((int)rec.z, q0 + q1);
            }
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
            if (!(z > 0.0 && z < __longlong_as_double(0x7ff0000000000000LL))) { nskipped++; continue; }
            for (int k = 0; k < card; k++)
                plgrad_walk(g, p, k, slot0 + step * k, v, (k == cur ? 1.0 : 0.0) - E[k] / z, sk);
            continue;
        }
        // large domains: the second pass recomputes the identical potentials
        double z = 0.0;
        for (int k = 0; k < card; k++) {
            const double ek = nsk_exp(potential(g, p, k, slot0 + step * k, v));
            z = (k == 0) ? ek : z + ek;
        }
        if (!(z > 0.0 && z < __longlong_as_double(0x7ff0000000000000LL))) { nskipped++; continue; }
        for (int k = 0; k < card; k++) {
            const double ek = nsk_exp(potential(g, p, k, slot0 + step * k, v));
            plgrad_walk(g, p, k, slot0 + step * k, v, (k == cur ? 1.0 : 0.0) - ek / z, sk);
        }
    }
    sk.flush();
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) nskipped += __shfl_xor(nskipped, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = nskipped;
    __syncthreads();                                        // (also: every lane's bin adds are done)
    if (threadIdx.x == 0) {
        int s = lds[0];
#pragma unroll
        for (int k = 1; k < NSK_BLOCK / 64; k++) s += lds[k];
        if (s > 0) atomicAdd(skipped + blockIdx.y, (unsigned long long)s);
    }
    if (binned)
        for (int i = threadIdx.x; i < nweight; i += NSK_BLOCK) {
            const unsigned long long x = bins[i];
            if (x) (void)__hip_atomic_fetch_add(sk.G + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
}

// One MPLE step (see the top of the file): G = nchains x nweight sums by slot, gmax / skipped_out this step's outputs,
// skipped_in the chains' skip counts of the step's k_plgrad launch
__global__ __launch_bounds__(NSK_BLOCK) void k_mple_update(const long long *G, int nchains, int nweight, double *w, const uint8_t *w_fixed,
                                                           double n, double step, double reg_param, long long *gmax,
                                                           const unsigned long long *skipped_in, long long *skipped_out) {
    const int s = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x);
    long long mag = 0;
    if (s < nweight) {
        long long S = 0;
        for (int r = 0; r < nchains; r++) S += G[(long long)r * nweight + s];
        if (!w_fixed[s]) {
            const double gbar = ((double)S * (1.0 / NSK_GRAD_SCALE)) / n;
            w[s] = step_weight(w[s], gbar, step, reg_param);
            mag = S < 0 ? -S : S;
        }
    }
    // (|S| is not negative and gmax starts at 0: the unsigned maximum stores the bits the signed one would)
    step_block_max<NSK_BLOCK>((unsigned long long)mag, (unsigned long long *)gmax);
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        long long k = 0;
        for (int r = 0; r < nchains; r++) k += (long long)skipped_in[r];
        *skipped_out = k;
    }
}

}  // namespace nsk
