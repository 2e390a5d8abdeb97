// nsk_kernels_tracepairs.h -- co-occurrence counts of pairs of columns of a bit-packed sample trace
// (nsk_trace_pair_counts; DESIGN.md section 4 "Pairwise joint marginals from the trace").
//
// The trace keeps a row's columns side by side (bit = column); a pair's count wants a column's rows side by side.
// k_trace_transpose turns the window, rows first .. first + s - 1 of R chains (not split), nb = ceil(s / 64) blocks of 64
// rows, into T[slot][b][chain][blk]: bit i of that word is x(first + 64 blk + i) of column b of the slot's word, 0 beyond
// the window -- the R nb time-major words of one column lie together.  A wave takes one word of the selection and 8
// neighbouring blocks of one chain: lane i loads the word of row 64 blk + i for each of them (the loads in flight
// together), transpose64 (nsk_kernels_tracestat.h) turns each tile, and lane b ends with the 8 words of column b that
// are neighbours in T -- its 8 stores fill one run of 64 bytes.  The 8 waves of a workgroup take 8 neighbouring slots,
// as in k_trace_autocov: where the selection's words are neighbours the 64-byte line a row's load touches is consumed
// whole.
// k_trace_pair_counts: one wave per pair (a, b).  The lanes walk the R nb words of both columns and count
// n11 += popcll(Ta & Tb), n1a += popcll(Ta), n1b += popcll(Tb) in int64.  G = min(64, nb rounded up to a power of two)
// lanes share one chain, 64 / G chains go by at a time; an xor butterfly inside the G lanes sums them and the first lane
// of every group writes the three counts of (pair, chain).  Integers only, no atomics: the order cannot show.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "nsk_kernels_tracestat.h"

#define NSK_TRACEPAIRS_TBLOCK 512   // k_trace_transpose: 8 waves, 8 slots
#define NSK_TRACEPAIRS_TBLKS 8      // ... and 8 row blocks a wave: 64 bytes of T a lane
#define NSK_TRACEPAIRS_PBLOCK 256   // k_trace_pair_counts: 4 waves, 4 pairs

namespace nsk {

struct TracePairsArgs {
    const unsigned long long *rows;    // the word 0 of chain 0 of the first row
    const int32_t *words;              // the words the selection touches, sorted, each once
    long long nslots;                  // ... how many
    long long nwords;                  // words a chain
    long long chains;                  // R
    long long nrows;                   // s
    long long nb;                      // ceil(s / 64)
    long long bgroups;                 // ceil(nb / NSK_TRACEPAIRS_TBLKS)
    unsigned long long *T;             // [slot][bit][chain][blk]
    const long long *pairs;            // per pair the two columns of T (slot * 64 + bit)
    long long npairs;
    int G;                             // lanes a chain in k_trace_pair_counts: a power of two, 1 .. 64
    long long *counts;                 // [pair][chain][n11, n1a, n1b]
};

// block index = (slot group * R + chain) * bgroups + block group
__global__ __launch_bounds__(NSK_TRACEPAIRS_TBLOCK) void k_trace_transpose(const TracePairsArgs a) {
    const long long bg = (long long)blockIdx.x % a.bgroups, rest = (long long)blockIdx.x / a.bgroups;
    const long long chain = rest % a.chains, slot = (rest / a.chains) * (NSK_TRACEPAIRS_TBLOCK / 64) + (threadIdx.x >> 6);
    if (slot >= a.nslots) return;                       // (whole waves)
    const int lane = (int)(threadIdx.x & 63);
    const long long w = (long long)a.words[slot], row_words = a.chains * a.nwords, blk0 = bg * NSK_TRACEPAIRS_TBLKS;
    const unsigned long long *src = a.rows + chain * a.nwords + w;
    unsigned long long x[NSK_TRACEPAIRS_TBLKS];
#pragma unroll
    for (int k = 0; k < NSK_TRACEPAIRS_TBLKS; k++) {
        const long long t = ((blk0 + k) << 6) + lane;
        x[k] = t < a.nrows ? src[t * row_words] : 0ull;
    }
    unsigned long long *dst = a.T + ((slot * 64 + lane) * a.chains + chain) * a.nb + blk0;
#pragma unroll
    for (int k = 0; k < NSK_TRACEPAIRS_TBLKS; k++) {
        const unsigned long long c = transpose64(x[k], lane);
        if (blk0 + k < a.nb) dst[k] = c;
    }
}

__global__ __launch_bounds__(NSK_TRACEPAIRS_PBLOCK) void k_trace_pair_counts(const TracePairsArgs a) {
    const long long j = (long long)blockIdx.x * (NSK_TRACEPAIRS_PBLOCK / 64) + (threadIdx.x >> 6);
    if (j >= a.npairs) return;                          // (whole waves)
    const int lane = (int)(threadIdx.x & 63), G = a.G, sub = lane & (G - 1), per = 64 / G;
    const long long per_col = a.chains * a.nb;
    const unsigned long long *Ta = a.T + a.pairs[2 * j] * per_col, *Tb = a.T + a.pairs[2 * j + 1] * per_col;
    for (long long r0 = 0; r0 < a.chains; r0 += per) {
        const long long r = r0 + lane / G;
        long long n11 = 0, n1a = 0, n1b = 0;
        if (r < a.chains)
            for (long long blk = sub; blk < a.nb; blk += G) {
                const unsigned long long ta = Ta[r * a.nb + blk], tb = Tb[r * a.nb + blk];
                n11 += __popcll(ta & tb);
                n1a += __popcll(ta);
                n1b += __popcll(tb);
            }
        for (int off = G >> 1; off > 0; off >>= 1) {    // (every lane of the wave is here: G and the trip counts are uniform)
            n11 += __shfl_xor(n11, off);
            n1a += __shfl_xor(n1a, off);
            n1b += __shfl_xor(n1b, off);
        }
        if (sub == 0 && r < a.chains) {
            long long *o = a.counts + (j * a.chains + r) * 3;
            o[0] = n11; o[1] = n1a; o[2] = n1b;
        }
    }
}

}  // namespace nsk
