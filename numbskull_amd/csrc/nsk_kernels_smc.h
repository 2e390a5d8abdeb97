// nsk_kernels_smc.h -- the two kernels nsk_smc_sweeps (nsk_smc.hip) puts behind the fold of a step: population annealing,
// the resampling step of sequential Monte Carlo, on the folded log-weights of the handle's chains.
//
//   k_smc_decide  ONE block for the whole population (R <= 1024 chains, thread r = chain r).  Keeps the row of log-weights
//                 as the caller's logw_pre, takes w_r = nsk_exp(log_weight[r] - max), lets ONE lane add the running sums
//                 c_r = c_{r-1} + w_r and q_r = q_{r-1} + w_r * w_r in chain order over LDS -- the only arithmetic here
//                 whose order matters -- and resamples iff S * S < thrR * Q (the effective sample size S^2 / Q fell below
//                 threshold * R).  Systematic resampling with the caller's one uniform: lane i searches c for
//                 target_i = ((double)i + offset) * (S / R), counts arrive in LDS by integer atomics, and the ancestors
//                 are dealt so that the copy is in place: a chain with offspring keeps its slot, the dead slots in
//                 ascending order take the surplus offspring in ascending order (two integer prefix sums and a search).
//                 Every product, sum and quotient is one rounded float64 operation (-ffp-contract=off);
//                 numbskull_amd.diagnostics.smc_resample is the same rule in numpy.
//   k_smc_copy    grid (blocks, chains), as k_temper_keep: a block loads its chain's ancestor (the address depends on
//                 blockIdx alone: a scalar load and a uniform branch) and returns when the chain keeps its own state, or
//                 copies its grid-stride share of the ancestor's value bytes over the chain's with 16-byte loads and
//                 stores; block 0 copies the bytes behind the last whole 16.  Every source is a chain that kept its slot,
//                 so nobody writes what another block reads: no second buffer.
#pragma once

#include "nsk_device.h"
#include "nsk_kernels_gibbs.h"      // NSK_BLOCK

#define NSK_SMC_MAX 1024            // chains one decide block serves: the most a handle holds

namespace nsk {

struct SmcDecide {
    double *log_weight;             // [R] the folded log-weights; 0.0 after a resampling
    double *logw_pre;               // [R] row t of the caller's logw_pre, or null
    int32_t *anc;                   // [R] row t of the ancestors
    int32_t *resampled;             // the flag of step t
    double thrR;                    // threshold * (double)R, the host's one rounded product
    double offset;                  // the step's uniform in [0, 1)
    int R;
};

// inclusive prefix sum over the block (blockDim.x a multiple of 64, at most 1024): shuffles inside a wave, the waves'
// totals through LDS
__device__ __forceinline__ int smc_block_scan(int v, int *wsum) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(v, off, 64);
        if (lane >= off) v += u;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    int base = 0;
    for (int k = 0; k < wave; k++) base += wsum[k];
    __syncthreads();                // wsum is free again
    return base + v;
}

// the number of j < n with x[j] <= key, x ascending
template <typename T>
__device__ __forceinline__ int smc_count_le(const T *x, int n, T key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] <= key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one block of R rounded up to whole waves
static __global__ __launch_bounds__(NSK_SMC_MAX) void k_smc_decide(const SmcDecide a) {
    __shared__ double c[NSK_SMC_MAX];           // w_r, then the running sums c_r in place
    __shared__ int n[NSK_SMC_MAX];              // offspring counts
    __shared__ int x[NSK_SMC_MAX];              // inclusive prefix of the surplus offspring max(n_j - 1, 0)
    __shared__ double wmax[NSK_SMC_MAX / 64], sq[2];
    __shared__ int wsum[NSK_SMC_MAX / 64];
    const int r = (int)threadIdx.x, R = a.R, nwaves = (int)blockDim.x >> 6;
    const bool live = r < R;
    const double ninf = __longlong_as_double(0xfff0000000000000LL);
    const double lw = live ? a.log_weight[r] : ninf;
    if (live && a.logw_pre) a.logw_pre[r] = lw;
    const int any_nan = __syncthreads_or(lw != lw);
    // the maximum (fmax: order-free; a NaN row never gets as far as using it)
    double m = lw;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if ((r & 63) == 0) wmax[r >> 6] = m;
    n[r] = 0;
    __syncthreads();
    m = wmax[0];
    for (int k = 1; k < nwaves; k++) m = fmax(m, wmax[k]);
    bool go = !any_nan && m - m == 0.0;         // m finite
    if (go) {                                   // (uniform: every thread holds the same flag and the same m)
        c[r] = live ? nsk_exp(lw - m) : 0.0;
        __syncthreads();
        if (r == 0) {
            double cs = c[0], qs = c[0] * c[0];
            for (int j = 1; j < R; j++) {
                const double w = c[j], w2 = w * w;
                cs = cs + w;
                qs = qs + w2;
                c[j] = cs;
            }
            sq[0] = cs;
            sq[1] = qs;
        }
        __syncthreads();
        go = sq[0] * sq[0] < a.thrR * sq[1];
    }
    if (!go) {
        if (live) a.anc[r] = r;
        if (r == 0) *a.resampled = 0;
        return;
    }
    // systematic resampling: a_i = #{j : c_j <= target_i}, at most R - 1
    if (live) {
        const double step = sq[0] / (double)R;
        const double target = ((double)r + a.offset) * step;
        atomicAdd(&n[min(smc_count_le(c, R, target), R - 1)], 1);
    }
    __syncthreads();
    const int nj = live ? n[r] : 1;
    const int dead = smc_block_scan(nj == 0 ? 1 : 0, wsum);         // this slot included
    x[r] = smc_block_scan(nj > 1 ? nj - 1 : 0, wsum);
    __syncthreads();
    if (!live) return;
    // the dead slot of rank k takes the k-th surplus offspring: the first j whose prefix passes k (the counts sum to R, so
    // there are as many surplus offspring as dead slots; the clamp keeps the copy inside the slab come what may)
    a.anc[r] = nj == 0 ? min(smc_count_le(x, R, dead - 1), R - 1) : r;
    a.log_weight[r] = 0.0;
    if (r == 0) *a.resampled = 1;
}

// chain r's values lie at val + r * chain_stride BYTES, 16-byte aligned; nbytes of them are values
static __global__ __launch_bounds__(NSK_BLOCK) void k_smc_copy(const int32_t *anc, char *val, long long chain_stride, long long nbytes) {
    const int src = anc[blockIdx.y];
    if (src == (int)blockIdx.y) return;
    const char *s = val + (long long)src * chain_stride;
    char *d = val + (long long)blockIdx.y * chain_stride;
    const long long n16 = nbytes >> 4;
    for (long long i = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; i < n16; i += (long long)gridDim.x * NSK_BLOCK)
        ((uint4 *)d)[i] = ((const uint4 *)s)[i];
    const long long tail = n16 << 4;
    if (blockIdx.x == 0 && tail + (long long)threadIdx.x < nbytes) d[tail + threadIdx.x] = s[tail + threadIdx.x];
}

}  // namespace nsk
