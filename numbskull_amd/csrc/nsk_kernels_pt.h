// nsk_kernels_pt.h -- the two kernels nsk_pt_sweeps (nsk_pt.hip) puts behind the score of a step: parallel tempering,
// replica exchange between the handle's chains.  Chain r stays at betas[r]; STATES travel between the chains.
//
//   k_pt_decide   ONE block (R - 1 <= 1023 pairs, thread r = the pair of the chains r and r + 1).  The pair is proposed at
//                 step t iff r and t have the same parity (deterministic even-odd scheme: the proposed pairs of a step
//                 are disjoint).  d = (betas[r] - betas[r + 1]) * (U[r + 1] - U[r]) -- two rounded differences, one
//                 rounded product (-ffp-contract=off) -- and the swap is accepted iff d >= 0.0, or d >= -745.0 and the
//                 pair's uniform lies below nsk_exp(d); a NaN d compares false everywhere and rejects.  accepted[r] is
//                 1, 0, or -1 for a pair not proposed; partner[c] is the chain whose state chain c takes (c itself where
//                 nothing moves): the thread of a proposed pair writes both its chains' words, the threads of the pairs
//                 not proposed write the words of the end chains that no proposed pair holds.
//                 numbskull_amd.diagnostics.pt_swap_rule is the same rule in numpy.
//   k_pt_swap     grid (blocks, proposed pairs), as k_smc_copy: a block loads the partner word of its pair's lower chain
//                 (the address depends on blockIdx and the step's parity alone: a scalar load and a uniform branch) and
//                 returns when the pair was rejected, or exchanges its grid-stride share of the two chains' value bytes
//                 in place -- both 16-byte loads are issued before either store; block 0 exchanges the bytes behind the
//                 last whole 16.  The pairs of a step are disjoint, so nobody touches what another block reads or
//                 writes: no second buffer.
#pragma once

#include "nsk_device.h"
#include "nsk_kernels_gibbs.h"      // NSK_BLOCK

#define NSK_PT_MAX 1024             // chains one decide block serves: the most a handle holds

namespace nsk {

struct PtDecide {
    const double *betas;            // [R] the chains' inverse temperatures
    const double *U;                // [R] the log-potentials of the chains' states under the base weights
    const double *uniforms;         // [R - 1] row t of the caller's uniforms, each in [0, 1)
    int32_t *accepted;              // [R - 1] row t of the decisions
    int32_t *partner;               // [R] whose state each chain takes
    int R;
    int parity;                     // t & 1
};

// one block of R - 1 rounded up to whole waves; R >= 2
static __global__ __launch_bounds__(NSK_PT_MAX) void k_pt_decide(const PtDecide a) {
    const int r = (int)threadIdx.x, R = a.R;
    if (r + 1 >= R) return;
    if ((r & 1) != a.parity) {
        a.accepted[r] = -1;
        // the chains r and r + 1 belong to the pairs r - 1 and r + 1 of this step, where those exist
        if (r == 0) a.partner[0] = 0;
        if (r + 2 >= R) a.partner[r + 1] = r + 1;
        return;
    }
    const double db = a.betas[r] - a.betas[r + 1];
    const double du = a.U[r + 1] - a.U[r];
    const double d = db * du;
    const bool acc = d >= 0.0 || (d >= -745.0 && a.uniforms[r] < nsk_exp(d));
    a.accepted[r] = acc ? 1 : 0;
    a.partner[r] = acc ? r + 1 : r;
    a.partner[r + 1] = acc ? r : r + 1;
}

// chain r's values lie at val + r * chain_stride BYTES, 16-byte aligned; nbytes of them are values.  Block row y serves
// the pair of the chains parity + 2 y and parity + 2 y + 1.
static __global__ __launch_bounds__(NSK_BLOCK) void k_pt_swap(const int32_t *partner, char *val, long long chain_stride, long long nbytes,
                                                              int parity) {
    const int lo = parity + 2 * (int)blockIdx.y;
    if (partner[lo] != lo + 1) return;
    char *p = val + (long long)lo * chain_stride;
    char *q = p + chain_stride;
    const long long n16 = nbytes >> 4;
    for (long long i = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; i < n16; i += (long long)gridDim.x * NSK_BLOCK) {
        const uint4 x = ((const uint4 *)p)[i], y = ((const uint4 *)q)[i];
        ((uint4 *)p)[i] = y;
        ((uint4 *)q)[i] = x;
    }
    const long long tail = n16 << 4;
    if (blockIdx.x == 0 && tail + (long long)threadIdx.x < nbytes) {
        const char x = p[tail + threadIdx.x], y = q[tail + threadIdx.x];
        p[tail + threadIdx.x] = y;
        q[tail + threadIdx.x] = x;
    }
}

}  // namespace nsk
