// nsk_kernels_step.h -- what every full-batch learner's update kernel shares (k_pcd_update in nsk_kernels_pcd.h, which
// nsk_bp.hip launches too, and k_mple_update in nsk_kernels_plgrad.h): the weight step and the largest magnitude of a
// launch.  This is the one place of the rule; the kernels say where g comes from.
#pragma once

#include "nsk_device.h"

namespace nsk {

// The weight step: w moves along g with an L2 penalty.  Every line is ONE rounded IEEE operation (the translation units
// are built with -ffp-contract=off), in this order.
__device__ __forceinline__ double step_weight(double w, double g, double step, double reg_param) {
    const double a = reg_param * w;
    const double b = g - a;
    const double c = step * b;
    return w + c;
}

// The largest `mag` over a launch of blocks of BLOCK lanes, into *out (zeroed by the host): a butterfly over the wave,
// the waves' maxima through LDS, and from lane 0 of the block ONE 64-bit integer atomic max when the block's is not 0.
// mag is a non-negative magnitude as an unsigned integer -- a non-negative int64, or the bit pattern of a non-negative
// finite double, which orders as one.  Every lane of the block calls it (there is a barrier inside).
template <int BLOCK>
__device__ __forceinline__ void step_block_max(unsigned long long mag, unsigned long long *out) {
    __shared__ unsigned long long lds[BLOCK / 64];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const unsigned long long o = __shfl_xor(mag, off, 64); mag = o > mag ? o : mag; }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = mag;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = lds[0];
#pragma unroll
        for (int k = 1; k < BLOCK / 64; k++) m = lds[k] > m ? lds[k] : m;
        if (m > 0ull) (void)__hip_atomic_fetch_max(out, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace nsk
