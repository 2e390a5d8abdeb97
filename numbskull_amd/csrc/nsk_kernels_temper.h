// nsk_kernels_temper.h -- the three kernels nsk_tempered_sweeps (nsk_temper.hip) puts around the sweep and log-potential
// launches of a step.  potential() is linear in the weights, so sampling at the inverse temperature beta is sampling under
// the weight table beta * w: the sweep kernels, their draw tables and their plans are used as they are.
//
//   k_temper_scale  w[s] = beta * base[s], one lane per slot: ONE rounded float64 product (the library is compiled with
//                   -ffp-contract=off), fixed weights included.
//   k_temper_fold   one block per chain, behind k_energy_partial: the block adds the chain's block partials exactly as
//                   k_energy_reduce does (thread t the partials t, t + 256, ... in ascending order, butterfly, waves in
//                   order: energy_block_sum), so U has the bits of nsk_log_potential; thread 0 -- the one lane that owns
//                   the chain's sums -- writes the lp row, folds the AIS weight and decides whether the state is the best
//                   so far.
//   k_temper_keep   grid (blocks, chains): a block loads its chain's flag (the address depends on blockIdx alone: a
//                   scalar load and a uniform branch) and returns, or copies its grid-stride share of the chain's value
//                   bytes with 16-byte loads and stores; block 0 copies the bytes behind the last whole 16.
#pragma once

#include "nsk_internal.h"
#include "nsk_kernels_energy.h"

namespace nsk {

static __global__ __launch_bounds__(NSK_BLOCK) void k_temper_scale(const double *base, double beta, double *w, long long n) {
    const long long i = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x;
    if (i < n) w[i] = beta * base[i];
}

// what the fold keeps per chain; a null pointer switches its part off
struct TemperFold {
    double *lp_row;             // [chains] row t of the lp matrix
    double *log_weight;         // [chains] running AIS log-weights
    double *best_u;             // [chains] the largest U so far
    unsigned int *improved;     // [chains] 1: this step's state replaces the kept one (k_temper_keep)
    double dbeta;               // betas[t + 1] - betas[t], one rounded difference (the host's)
    int fold;                   // a step follows this one: log_weight += dbeta * U
    int first;                  // step 0: the state and U are taken unconditionally
};

static __global__ __launch_bounds__(NSK_BLOCK) void k_temper_fold(const double *partial, int nparts, const TemperFold a) {
    __shared__ double lds[NSK_BLOCK / 64];
    const double *p = partial + (long long)blockIdx.x * nparts;
    double acc = 0.0;
    for (int i = (int)threadIdx.x; i < nparts; i += NSK_BLOCK) acc = acc + p[i];
    const double u = energy_block_sum(acc, lds);
    if (threadIdx.x != 0) return;
    const unsigned int r = blockIdx.x;
    if (a.lp_row) a.lp_row[r] = u;
    if (a.log_weight && a.fold) {
        const double term = a.dbeta * u;                // one rounded product, one rounded addition
        a.log_weight[r] = a.log_weight[r] + term;
    }
    if (a.improved) {
        // strictly larger only: the earliest maximum stays, and a NaN compares false
        const bool take = a.first || u > a.best_u[r];
        if (take) a.best_u[r] = u;
        a.improved[r] = take ? 1u : 0u;
    }
}

// chain r's values lie at src + r * src_stride BYTES, its kept state at dst + r * dst_stride; both 16-byte aligned
static __global__ __launch_bounds__(NSK_BLOCK) void k_temper_keep(const unsigned int *improved, const char *src, long long src_stride,
                                                                  char *dst, long long dst_stride, long long nbytes) {
    if (improved[blockIdx.y] == 0) return;
    const char *s = src + (long long)blockIdx.y * src_stride;
    char *d = dst + (long long)blockIdx.y * dst_stride;
    const long long n16 = nbytes >> 4;
    for (long long i = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; i < n16; i += (long long)gridDim.x * NSK_BLOCK)
        ((uint4 *)d)[i] = ((const uint4 *)s)[i];
    const long long tail = n16 << 4;
    if (blockIdx.x == 0 && tail + (long long)threadIdx.x < nbytes) d[tail + threadIdx.x] = s[tail + threadIdx.x];
}

}  // namespace nsk

// ------------------------------------------------------------------------------------------
// the host side of a step that nsk_tempered_sweeps (nsk_temper.hip) and nsk_smc_sweeps (nsk_smc.hip) share: one place,
// so that "the same launches, the same bits" holds by construction
// ------------------------------------------------------------------------------------------
// a buffer of one call through the ledger; NSK_E_NOMEM names the entry point `who` and the size of what does not fit
template <typename T>
static int temper_alloc(nsk_graph *g, T **ptr, size_t n, const char *who, const char *what) {
    const int rc = dev_alloc(g, ptr, n);
    if (rc != NSK_E_NOMEM) return rc;
    return nsk::fail(NSK_E_NOMEM, std::string(who) + ": " + what + " (" + std::to_string((long long)((n ? n : 1) * sizeof(T))) +
                                  " bytes) do not fit on the device");
}

// the log-potential of every chain under the weights `w`, folded behind the walk (nsk_energy_enqueue with k_temper_fold in
// the place of k_energy_reduce: the same grid, the same partials, the same order)
template <typename VT>
static void temper_score(nsk_graph *g, const double *w, int nchains, const nsk::TemperFold &fold) {
    nsk::EnergyArgs a = energy_args(g);
    a.w = w;
    const unsigned int nb = nsk_energy_blocks(a.nfactor);
    nsk::k_energy_partial<VT><<<dim3(nb, (unsigned)nchains), dim3(NSK_BLOCK), 0, g->stream>>>(a, (const VT *)g->val, g->energy.partial);
    nsk::k_temper_fold<<<dim3((unsigned)nchains), dim3(NSK_BLOCK), 0, g->stream>>>(g->energy.partial, (int)nb, fold);
}
