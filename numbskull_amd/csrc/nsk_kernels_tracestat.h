// nsk_kernels_tracestat.h -- per-column autocovariance counts and effective sample size of a bit-packed sample trace
// (nsk_trace_ess / nsk_trace_autocov_counts; DESIGN.md section 4 "Effective sample size from the trace").
//
// One wave per 64-column word of the row, lane = column.  Rows first .. first + s - 1 of R chains are split as
// diagnostics._split splits them: n = s / 2, half-chains rows [0, n) and [s - n, s) of every chain, H = 2 R of them.
// A half-chain goes by in blocks of 64 rows: lane i loads the word of row t0 + i (0 beyond the half-chain: the partial
// last block needs no other mask) and the 64 x 64 bit tile is transposed (transpose64: what 64 ballots would give, lane b
// keeping ballot b) -- bit i of lane b is x(t0 + i) of its column.  With the previous block's tile the products
// x(t) x(t - k) of lag k are the bits of
// cur & (cur << k | prev >> (64 - k)) (formed in 32-bit halves, one funnel shift each); popcounts give c_h(k) = sum over t < n - k of x(t) x(t + k).  Behind a
// half-chain, with S_h = c_h(0), the sums of its first and last k rows F and E (head_h(k) = S_h - E, tail_h(k) = S_h - F),
//     A(k) += n^2 c_h(k) - n S_h (head_h(k) + tail_h(k)) + (n - k) S_h^2,      S1 += S_h,     S2 += S_h^2
// in int64 (the host refuses a call whose 4 H n^3 could reach 2^63).  The lag loops are unrolled over the compile-time
// bound LB (15 / 31 / 63: the accumulators stay in registers); lags beyond the call's L are computed and dropped.
// The 8 waves of a workgroup take 8 neighbouring words: the 64-byte line a row's load touches is consumed whole.
// The counting itself -- the lag products of a tile, the fold behind a half-chain, the epilogue -- is AutocovLane, which
// k_trace_autocov_planes (nsk_kernels_tracevalues.h: lane = one value of a categorical column) shares.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#define NSK_TRACESTAT_BLOCK 512     // 8 waves, 8 words of the row: one 64-byte line per row and chain

namespace nsk {

struct TraceStatArgs {
    const unsigned long long *rows;    // the word 0 of chain 0 of the first row
    const int32_t *words;              // the words to serve (nullptr: every word, slot = word)
    long long nslots;                  // ... how many
    long long nwords;                  // words a chain
    long long chains;                  // R
    long long n;                       // rows of a half-chain
    long long second;                  // s - n: the first row of the second halves
    int L;                             // lags 0 .. L
    // the epilogue's constants, rounded on the host as the specification orders them
    double D, Bden, c1, Hn;            // H n n (n - 1);  H (H - 1) n n;  (n - 1) / n;  H n
    // counts: [slot][lane][A(0 .. L), S1, S2]
    long long *counts;
    // summary, by device column (nwords * 64 each)
    double *mean, *tau, *rhat2;
    unsigned char *truncated;
};

// The 64 x 64 bit tile a wave holds one row a lane, transposed: lane b comes out with bit i = bit b of lane i's word --
// what 64 ballots give, in six exchanges: at every scale j = 32 .. 1 the tile is 2 x 2 blocks of j x j sub-tiles and the
// two off-diagonal ones change places (a lane and its partner lane ^ j swap the halves the mask keeps apart).
static __device__ __forceinline__ unsigned long long transpose64(unsigned long long x, int lane) {
    const unsigned long long mask[6] = {0x00000000FFFFFFFFull, 0x0000FFFF0000FFFFull, 0x00FF00FF00FF00FFull,
                                        0x0F0F0F0F0F0F0F0Full, 0x3333333333333333ull, 0x5555555555555555ull};
#pragma unroll
    for (int r = 0; r < 6; r++) {
        const int j = 32 >> r;
        const unsigned long long m = mask[r], p = __shfl_xor(x, j);
        x = (lane & j) ? ((x & ~m) | ((p & ~m) >> j)) : ((x & m) | ((p & m) << j));
    }
    return x;
}

// The counting both estimator kernels share (k_trace_autocov here, k_trace_autocov_planes of nsk_kernels_tracevalues.h):
// a lane's series goes by as time-major 64-row words, half-chain after half-chain; `tile` takes the next word, `fold`
// closes a half-chain, `store` writes the integers or the summary.
template <int LB>
struct AutocovLane {
    long long A[LB + 1];
    unsigned int c[LB + 1];
    long long S1, S2;
    unsigned long long prev, first;

    __device__ __forceinline__ void init() {
#pragma unroll
        for (int k = 0; k <= LB; k++) { A[k] = 0; c[k] = 0; }
        S1 = S2 = 0;
        prev = first = 0;
    }

    // block `blk` of a half-chain of n rows in nb blocks, the last of them m rows: bit i of cur is x(64 blk + i), 0 beyond row n
    __device__ __forceinline__ void tile(const unsigned long long cur, const long long blk, const long long nb, const int m, const long long n) {
        if (blk == 0) { first = cur; prev = 0; }
        c[0] += (unsigned int)__popcll(cur);
        // (cur << k | prev >> (64 - k)) & cur in 32-bit halves: one funnel shift a half over the words prev.lo, prev.hi, cur.lo, cur.hi
        const unsigned int w0 = (unsigned int)prev, w1 = (unsigned int)(prev >> 32), w2 = (unsigned int)cur, w3 = (unsigned int)(cur >> 32);
#pragma unroll
        for (int k = 1; k <= LB; k++) {
            const unsigned int lo = k < 32 ? __funnelshift_l(w1, w2, k) : k == 32 ? w1 : __funnelshift_l(w0, w1, k - 32);
            const unsigned int hi = k < 32 ? __funnelshift_l(w2, w3, k) : k == 32 ? w2 : __funnelshift_l(w1, w2, k - 32);
            c[k] += (unsigned int)__popc(lo & w2) + (unsigned int)__popc(hi & w3);
        }
        if (blk == nb - 1) {                            // the half-chain is through: fold it
            const unsigned long long last = m == 64 ? cur : ((cur << (64 - m)) | (prev >> m));     // rows n - 64 .. n - 1 (bit 63 the last)
            const long long S = (long long)c[0], SS = S * S, nS = n * S, n2 = n * n;
            S1 += S; S2 += SS;
            A[0] += n2 * S - n * SS;                    // head(0) + tail(0) = 2 S
            c[0] = 0;
#pragma unroll
            for (int k = 1; k <= LB; k++) {
                const long long F = (long long)__popcll(first & ((1ull << k) - 1ull)), E = (long long)__popcll(last >> (64 - k));
                A[k] += n2 * (long long)c[k] - nS * (2 * S - F - E) + (n - k) * SS;
                c[k] = 0;
            }
        }
        prev = cur;
    }

    // the integers to a.counts + at * (L + 3), or the summary to element `at` of the four arrays
    template <bool SUMMARY>
    __device__ __forceinline__ void store(const TraceStatArgs &a, const long long at) const {
        if (!SUMMARY) {
            long long *o = a.counts + at * (long long)(a.L + 3);
#pragma unroll
            for (int k = 0; k <= LB; k++)
                if (k <= a.L) o[k] = A[k];
            o[a.L + 1] = S1;
            o[a.L + 2] = S2;
            return;
        }
        // The epilogue (float64, one rounded operation a step, -ffp-contract=off; diagnostics.ess_from_counts restates it)
        const long long H = 2 * a.chains;
        const double W = (double)A[0] / a.D;
        const double B = (double)(H * S2 - S1 * S1) / a.Bden;
        const double V = a.c1 * W + B;
        const bool ok = V > 0.0;
        bool run = ok;
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < (LB + 1) / 2; j++)
            if (2 * j + 1 <= a.L) {
                const double r0 = 1.0 - ((double)(A[0] - A[2 * j]) / a.D) / V;
                const double r1 = 1.0 - ((double)(A[0] - A[2 * j + 1]) / a.D) / V;
                const double P = r0 + r1;
                if (run && P > 0.0) sum = sum + P; else run = false;
            }
        const double tau = -1.0 + 2.0 * sum;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        a.mean[at] = (double)S1 / a.Hn;
        a.tau[at] = ok && tau > 0.0 ? tau : nan;
        a.rhat2[at] = ok ? V / W : nan;
        a.truncated[at] = run && (long long)a.L < a.n - 1 ? 1 : 0;
    }
};

template <int LB, bool SUMMARY>
__global__ __launch_bounds__(NSK_TRACESTAT_BLOCK) void k_trace_autocov(const TraceStatArgs a) {
    const long long slot = (long long)blockIdx.x * (NSK_TRACESTAT_BLOCK / 64) + (threadIdx.x >> 6);
    if (slot >= a.nslots) return;                       // (whole waves)
    const int lane = (int)(threadIdx.x & 63);
    const long long w = a.words ? (long long)a.words[slot] : slot;
    const long long n = a.n, nb = (n + 63) >> 6, H = 2 * a.chains, row_words = a.chains * a.nwords;
    const int m = (int)(n - ((nb - 1) << 6));           // rows of the last block: 1 .. 64

    AutocovLane<LB> acc;
    acc.init();

    // row t of half-chain h (h < R: the first half of chain h; else the second half of chain h - R)
    const auto load = [&](long long h, long long blk) -> unsigned long long {
        const long long t = (blk << 6) + lane;
        if (t >= n) return 0ull;
        const long long chain = h < a.chains ? h : h - a.chains, row = (h < a.chains ? 0 : a.second) + t;
        return a.rows[row * row_words + chain * a.nwords + w];
    };

    unsigned long long next = load(0, 0);
    long long h = 0, blk = 0;
    for (long long it = 0; it < H * nb; it++) {
        const unsigned long long wd = next;
        long long h1 = h, blk1 = blk + 1;
        if (blk1 == nb) { blk1 = 0; h1++; }
        if (h1 < H) next = load(h1, blk1);              // (in flight while this tile is counted)
        acc.tile(transpose64(wd, lane), blk, nb, m, n);
        h = h1; blk = blk1;
    }
    if (SUMMARY) acc.template store<true>(a, w * 64 + lane);
    else acc.template store<false>(a, slot * 64 + lane);
}

}  // namespace nsk
