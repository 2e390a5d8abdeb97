// nsk_kernels_tracevalues.h -- the trace statistics for categorical columns (nsk_trace_value_ess /
// nsk_trace_value_autocov_counts / nsk_trace_value_pair_counts; DESIGN.md section 4 "Indicators of a plain trace").
//
// A plain trace keeps one element (int8 or int32) per row, chain and device column.  An INDICATOR is a pair (device
// column, value); its series is the 0 / 1 sequence x(t) == value.  k_trace_onehot writes the indicators of a window as
// time-major bit words -- planes -- and from there on the packed trace's counting applies: AutocovLane
// (nsk_kernels_tracestat.h) through k_trace_autocov_planes, and k_trace_pair_counts (nsk_kernels_tracepairs.h) as it is.
//
// k_trace_onehot<VT>: a workgroup of 4 waves takes one 64-row block of one segment (chain, first row, length) and one
// tile of 64 neighbouring device columns that has indicators (the host lists those tiles with their runs of the sorted
// indicator list).  The tile comes in by rows -- a wave's load is 64 neighbouring elements of one row, 16 rows a wave --
// and is staged in LDS, one row a pitch of 64 elements and a pad that spreads a column over the banks; every touched
// trace byte is read from memory once, whatever the number of values asked of a column.  Then the waves share the
// tile's indicators in runs of 64: lane = row reads its element of the indicator's column from LDS, one __ballot
// (x == value, rows beyond the segment and the wave's every lane voting) a indicator, lane b keeping ballot b, and the
// run leaves as one store a lane: out[indicator * s_ind + segment * s_seg + blk * s_blk].  Bits beyond the segment are 0.
// The elements are loaded one by one (a row has no padding: with int8 values and an odd column count no row base is
// aligned).
//
// k_trace_autocov_planes<LB, SUMMARY>: k_trace_autocov with lane = indicator.  One wave serves 64 neighbouring
// indicators of planes laid out [half-chain][blk][indicator, padded to a multiple of 64] -- a wave's load is one run of
// 512 bytes -- and counts them with AutocovLane: the integers and the epilogue are k_trace_autocov's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "nsk_kernels_tracestat.h"

#define NSK_TRACEVALUES_OBLOCK 256  // k_trace_onehot: 4 waves a tile, 16 rows each to load
#define NSK_TRACEVALUES_ABLOCK 256  // k_trace_autocov_planes: 4 waves, 256 neighbouring indicators

namespace nsk {

struct TraceOnehotArgs {
    const void *buf;                   // row 0 of the trace: element (row, chain, col) at ((row * chains + chain) * ndev + col)
    long long chains, ndev;
    const int32_t *ind;                // the indicators, sorted by (device column, value), each once: (column, value)
    const int32_t *tiles;              // per column tile with indicators: (tile = column / 64, first indicator, one past the last)
    long long ntiles;
    const long long *segs;             // per segment: (chain, first row, length)
    long long nsegs;
    long long nb;                      // blocks of 64 rows a segment: ceil(the longest length / 64)
    unsigned long long *out;
    long long s_ind, s_seg, s_blk;     // the strides of out, in words
};

struct TraceValuesArgs {
    TraceStatArgs s;                   // chains, n, L, the epilogue's constants; counts [indicator][L + 3]; the summary by indicator
    const unsigned long long *planes;  // [half-chain][blk][indicator < npad]
    long long nind, npad;              // indicators; rounded up to a multiple of 64
};

// block index = (tile * nsegs + segment) * nb + blk
template <typename VT>
__global__ __launch_bounds__(NSK_TRACEVALUES_OBLOCK) void k_trace_onehot(const TraceOnehotArgs a) {
    constexpr int PITCH = 64 + (sizeof(VT) == 1 ? 4 : 1);      // 17 or 65 dwords a row: a column's 64 rows fall on distinct banks
    __shared__ VT tile[64 * PITCH];
    const long long blk = (long long)blockIdx.x % a.nb, rest = (long long)blockIdx.x / a.nb;
    const long long seg = rest % a.nsegs, ti = rest / a.nsegs;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const long long chain = a.segs[3 * seg], first = a.segs[3 * seg + 1], length = a.segs[3 * seg + 2];
    const long long c0 = (long long)a.tiles[3 * ti] * 64;
    const int i0 = a.tiles[3 * ti + 1], i1 = a.tiles[3 * ti + 2];
    const long long t0 = blk << 6;
    const long long left = length - t0;                         // rows of this block: <= 0 where a shorter segment has none
    const VT *src = (const VT *)a.buf;
    // the tile by rows: row r of the block, column c0 + lane
#pragma unroll 4
    for (int r = wave; r < 64; r += NSK_TRACEVALUES_OBLOCK / 64) {
        VT x = 0;
        if (r < left && c0 + lane < a.ndev) x = src[((first + t0 + r) * a.chains + chain) * a.ndev + c0 + lane];
        tile[r * PITCH + lane] = x;
    }
    __syncthreads();
    const bool live = lane < left;
    for (int j0 = i0 + wave * 64; j0 < i1; j0 += NSK_TRACEVALUES_OBLOCK) {     // (whole waves: j0, i1 are the wave's)
        const int cnt = i1 - j0 < 64 ? i1 - j0 : 64;
        unsigned long long keep = 0;
        for (int b = 0; b < cnt; b++) {
            const int col = a.ind[2 * (j0 + b)], value = a.ind[2 * (j0 + b) + 1];
            const int x = (int)tile[lane * PITCH + (int)(col - c0)];
            const unsigned long long m = __ballot(live && x == value);
            if (lane == b) keep = m;
        }
        if (lane < cnt) a.out[(long long)(j0 + lane) * a.s_ind + seg * a.s_seg + blk * a.s_blk] = keep;
    }
}

template <int LB, bool SUMMARY>
__global__ __launch_bounds__(NSK_TRACEVALUES_ABLOCK) void k_trace_autocov_planes(const TraceValuesArgs a) {
    const long long ind = ((long long)blockIdx.x * (NSK_TRACEVALUES_ABLOCK / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    if ((ind & ~63ll) >= a.nind) return;                // (whole waves)
    const bool mine = ind < a.nind;                     // the last wave's lanes beyond the list count zeros and store nothing
    const long long n = a.s.n, nb = (n + 63) >> 6, H = 2 * a.s.chains;
    const int m = (int)(n - ((nb - 1) << 6));           // rows of the last block: 1 .. 64

    AutocovLane<LB> acc;
    acc.init();
    const unsigned long long *src = a.planes + ind;
    unsigned long long next = mine ? src[0] : 0ull;
    long long blk = 0;
    for (long long it = 0; it < H * nb; it++) {
        const unsigned long long cur = next;
        if (it + 1 < H * nb) next = mine ? src[(it + 1) * a.npad] : 0ull;     // (in flight while this tile is counted)
        acc.tile(cur, blk, nb, m, n);
        if (++blk == nb) blk = 0;
    }
    if (!mine) return;
    if (SUMMARY) acc.template store<true>(a.s, ind);
    else acc.template store<false>(a.s, ind);
}

}  // namespace nsk
