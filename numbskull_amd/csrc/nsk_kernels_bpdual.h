// nsk_kernels_bpdual.h -- max-sum diffusion, variable-centred and chromatic, on the resident set-up of nsk_kernels_bp.h: the
// kernels of nsk_bp_dual_run / nsk_bp_dual_download / nsk_bp_dual_decode (nsk_bp_dual.hip; the rule is stated in
// include/numbskull_amd.h and restated in numpy by numbskull_amd.diagnostics.msd_iterate / msd_terms -- device and numpy
// agree bit for bit).  A block-coordinate descent on the dual of the MAP linear relaxation: D[e][k] is what factor f(e)
// has handed to value k of its variable; r_f(a) = theta_f(a) - the D entries of f's free slots at the digits of a is the
// reparametrised table, Bv[k] = the sum of v's D entries the reparametrised unary.  The update of variable v takes the
// max-marginals M of every incident r_f onto v, adds them to Bv and shares the total evenly among the d factors and v
// itself: the bound sum_f max r_f + sum_v max Bv never goes up.  Variables of one colour class share no factor
// (nsk_bp_dual_plan.h checks it), so one launch updates a class: it reads the D of other classes and writes its own.
//
//   k_dual_reset   one lane per directed edge: D and M +0.0; one lane per value: Bv 0; one per variable: tv 0
//   k_dual_lane    the LANE route: one lane per variable; see there
//   k_dual_wave    the WAVE route: one wave per variable; see there
//   k_bp_dual_terms  tf with one lane a small factor and one wave a large one; tv and Bv with one lane a variable
//   (decode: k_ms_decode of nsk_kernels_bpmap.h over Bv -- the scan is the same)
//
// Every SUM is taken in the order the rule writes.  A MAXIMUM over table entries may be taken in any order: ms_max passes
// over NaNs and the wave route's integer maxima never meet one, and the rule adds +0.0 to the result, after which a zero
// is +0.0 whichever of -0.0 and +0.0 the order preferred.
#pragma once

#include "nsk_bp_dual_plan.h"
#include "nsk_kernels_bpmap.h"      // ms_max, ms_key, ms_unkey, ms_done, ms_residual, ms_wave_sync, k_ms_decode

namespace nsk {

// what the kernels read beside the set-up
struct DualArgs {
    BpArgs b;
    double *D, *M;                  // msg_off's layout
    double *tf, *tv, *bv;           // [nfactor], [nid], b_off's layout
    const int32_t *lane_ids, *wave_ids;     // items (indices into v_list), class-major
    int32_t wave_lds;               // doubles of LDS a wave owns
};

__device__ __forceinline__ double dual_change(double nw, double old) {
    const double d = fabs(nw - old);
    return d == d ? d : __longlong_as_double(0x7ff0000000000000LL);
}

static __global__ __launch_bounds__(NSK_BLOCK) void k_dual_reset(const DualArgs m) {
    const BpArgs &a = m.b;
    for (int e = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); e < a.nedge; e += (int)(gridDim.x * NSK_BLOCK))
        for (long long i = a.msg_off[e]; i < a.msg_off[e + 1]; i++) { m.D[i] = 0.0; m.M[i] = 0.0; }
    for (long long id = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; id < a.nid; id += (long long)gridDim.x * NSK_BLOCK) {
        m.tv[id] = 0.0;
        for (long long i = a.b_off[id]; i < a.b_off[id + 1]; i++) m.bv[i] = 0.0;
    }
}

// ---- one lane, one edge: mk[k] = MAX over the entries a of f(e)'s table whose digit for e's slot is k of r_f(a), the
// table walked once, ascending; r_f(a) = ((theta - D[(f,0)][a_0]) - D[(f,1)][a_1]) - .., the co-members' entries read
// where they lie.  n <= NSK_ZLOCAL values.  A unary table has one entry a value; a 2 x 2 table is taken in registers.
__device__ __forceinline__ void dual_lane_edge(const DualArgs &m, int e, int n, double *mk) {
    const BpArgs &a = m.b;
    const int f = a.e_fac[e], e0 = a.edge_off[f], A = a.edge_off[f + 1] - e0, j = e - e0;
    const long long t0 = a.tab_off[f], mo0 = a.msg_off[e0];
    const int T = (int)(a.tab_off[f + 1] - t0);
    const double *D = m.D + mo0;
    if (A == 1) {
        for (int k = 0; k < n; k++) mk[k] = a.theta[t0 + k] - D[k];
        return;
    }
    if (A == 2 && T == 4 && a.msg_off[e0 + 1] - mo0 == 2) {         // entry a = 2 a_0 + a_1
        const double d0 = D[0], d1 = D[1], u0 = D[2], u1 = D[3];
        const double r0 = (a.theta[t0] - d0) - u0, r1 = (a.theta[t0 + 1] - d0) - u1;
        const double r2 = (a.theta[t0 + 2] - d1) - u0, r3 = (a.theta[t0 + 3] - d1) - u1;
        mk[0] = j == 0 ? ms_max(r0, r1) : ms_max(r0, r2);
        mk[1] = j == 0 ? ms_max(r2, r3) : ms_max(r1, r3);
        return;
    }
    for (int k = 0; k < n; k++) mk[k] = ms_nan();
    for (int ai = 0; ai < T; ai++) {
        double r = a.theta[t0 + ai];
        int st = T, kj = 0;
        for (int h = 0; h < A; h++) {
            const int oh = (int)(a.msg_off[e0 + h] - mo0), ch = (int)(a.msg_off[e0 + h + 1] - mo0) - oh;
            st /= ch;
            const int dg = (ai / st) % ch;
            r = r - D[oh + dg];
            if (h == j) kj = dg;
        }
        mk[kj & (NSK_ZLOCAL - 1)] = ms_max(mk[kj & (NSK_ZLOCAL - 1)], r);
    }
}

// ---- the lane route: n <= NSK_ZLOCAL, small tables, few edges.  tot[] and the maxima of the edge under way are
// lane-private.  First pass: Bv, then per edge M (stored) and tot; second pass: D from D, M and the share.
static __global__ __launch_bounds__(NSK_BLOCK) void k_dual_lane(const DualArgs m, int lo, int hi, int t, double tol, unsigned long long *residual) {
    if (ms_done(residual, t, tol)) return;          // block-uniform, before the barrier
    const BpArgs &a = m.b;
    double res = 0.0;
    for (int q = lo + (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); q < hi; q += (int)(gridDim.x * NSK_BLOCK)) {
        const int i = m.lane_ids[q], id = a.v_list[i];
        const int q0 = a.v_eoff[i], d = a.v_eoff[i + 1] - q0;
        int n = (int)(a.b_off[id + 1] - a.b_off[id]);
        n = n > NSK_ZLOCAL ? NSK_ZLOCAL : n;        // (the plan routes no other variable here)
        const int32_t *edges = a.v_edges + q0;
        double tot[NSK_ZLOCAL], mk[NSK_ZLOCAL];
        for (int k = 0; k < n; k++) tot[k] = 0.0;
        for (int x = 0; x < d; x++) {
            const long long mo = a.msg_off[edges[x]];
            for (int k = 0; k < n; k++) tot[k] = tot[k] + m.D[mo + k];
        }
        for (int x = 0; x < d; x++) {
            const int e = edges[x];
            const long long mo = a.msg_off[e];
            dual_lane_edge(m, e, n, mk);
            for (int k = 0; k < n; k++) {
                const double mv = mk[k] + 0.0;
                m.M[mo + k] = mv;
                tot[k] = tot[k] + mv;
            }
        }
        const double parts = (double)(d + 1);
        for (int k = 0; k < n; k++) tot[k] = tot[k] / parts;
        for (int x = 0; x < d; x++) {
            const long long mo = a.msg_off[edges[x]];
            for (int k = 0; k < n; k++) {
                const double old = m.D[mo + k], nw = (old + m.M[mo + k]) - tot[k];
                m.D[mo + k] = nw;
                res = fmax(res, dual_change(nw, old));
            }
        }
    }
    ms_residual<NSK_BLOCK>(res, residual + t);
}

// ---- the wave route.  Dynamic LDS: wave w of a block owns m.wave_lds doubles, the largest 2 n + C of the route's
// variables (nsk_bp_dual_plan.h), laid out as tot[n], acc[n], vin[C].  Per variable, wave-uniform throughout:
//   A. where n <= NSK_ZLOCAL the lanes take the edges of small tables one each (dual_lane_edge) -- a hub of 1200
//      unary factors is nineteen trips;
//   B. the other edges one after the other: the wave stages the D vectors of the factor's free slots, neighbours in
//      msg_off's layout, in vin; the lanes take the entries a = lane + 64 * trip, so the theta reads coalesce, decode the
//      digits arithmetically (a shift for a binary axis), form r_f(a) by the rule's left fold out of vin and offer it to
//      acc[digit of v's slot] -- the order-preserving key of nsk_kernels_bpmap.h under an integer atomicMax on LDS; lane
//      k then stores M[e][k] = acc[k] + 0.0;
//   C. lane k sums Bv[k] and tot[k] over the edges in order and leaves the share in tot[k];
//   D. the lanes take the (edge, k) pairs: D from D, M and the share, the residual.
// M crosses from A and B to C and D through global memory within the wave: the wave fences order it.
static __global__ __launch_bounds__(NSK_DUAL_WAVES * 64) void k_dual_wave(const DualArgs m, int lo, int hi, int t, double tol,
                                                                         unsigned long long *residual) {
    extern __shared__ double dual_lds[];
    __shared__ double red[NSK_DUAL_WAVES];
    if (ms_done(residual, t, tol)) return;          // block-uniform, before the barrier
    const BpArgs &a = m.b;
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6), W = (int)(blockDim.x >> 6);
    double *tot = dual_lds + (size_t)w * (size_t)m.wave_lds;
    double res = 0.0;
    for (int idx = lo + (int)blockIdx.x * W + w; idx < hi; idx += (int)gridDim.x * W) {
        const int i = __builtin_amdgcn_readfirstlane(m.wave_ids[idx]);      // wave-uniform: what follows is scalar
        const int id = a.v_list[i], q0 = a.v_eoff[i], d = a.v_eoff[i + 1] - q0;
        const int n = (int)(a.b_off[id + 1] - a.b_off[id]);
        if (2ll * n > (long long)m.wave_lds) continue;                      // (the plan routes no such variable here)
        const int32_t *edges = a.v_edges + q0;
        unsigned long long *acc = (unsigned long long *)(tot + n);
        double *vin = tot + 2 * n;
        const bool small = n <= NSK_ZLOCAL;
        if (small)
            for (int x = lane; x < d; x += 64) {
                const int e = edges[x], f = a.e_fac[e];
                if (a.tab_off[f + 1] - a.tab_off[f] > NSK_DUAL_LANE_TABLE) continue;
                double mk[NSK_ZLOCAL];
                dual_lane_edge(m, e, n, mk);
                const long long mo = a.msg_off[e];
                for (int k = 0; k < n; k++) m.M[mo + k] = mk[k] + 0.0;
            }
        for (int x = 0; x < d; x++) {
            const int e = __builtin_amdgcn_readfirstlane(edges[x]);
            const int f = a.e_fac[e], e0 = a.edge_off[f];
            const long long t0 = a.tab_off[f], mo0 = a.msg_off[e0];
            const int T = (int)(a.tab_off[f + 1] - t0);
            if (small && T <= NSK_DUAL_LANE_TABLE) continue;
            int A = a.edge_off[f + 1] - e0;
            A = A > NSK_BP_MAX_MEMBERS ? NSK_BP_MAX_MEMBERS : A;
            const int j = e - e0, C = (int)(a.msg_off[e0 + A] - mo0);
            if (2ll * n + C > (long long)m.wave_lds) continue;              // (nor such a factor)
            int ox[NSK_BP_MAX_MEMBERS], cx[NSK_BP_MAX_MEMBERS];
#pragma unroll
            for (int h = 0; h < NSK_BP_MAX_MEMBERS; h++) {
                ox[h] = 0; cx[h] = 1;
                if (h < A) { ox[h] = (int)(a.msg_off[e0 + h] - mo0); cx[h] = (int)(a.msg_off[e0 + h + 1] - mo0) - ox[h]; }
            }
            ms_wave_sync();                         // the last edge's accumulators have been read
            for (int c = lane; c < C; c += 64) vin[c] = m.D[mo0 + c];
            for (int k = lane; k < n; k += 64) acc[k] = 0ull;
            ms_wave_sync();
            for (int ai = lane; ai < T; ai += 64) {
                int kx[NSK_BP_MAX_MEMBERS];
                unsigned int r = (unsigned int)ai, kj = 0;
#pragma unroll
                for (int h = NSK_BP_MAX_MEMBERS - 1; h >= 0; h--) {
                    kx[h] = 0;
                    if (h < A) {
                        unsigned int dg;
                        if (cx[h] == 2) { dg = r & 1u; r >>= 1; }
                        else { const unsigned int qq = r / (unsigned int)cx[h]; dg = r - qq * (unsigned int)cx[h]; r = qq; }
                        kx[h] = ox[h] + (int)dg;
                        if (h == j) kj = dg;
                    }
                }
                double s = a.theta[t0 + ai];
#pragma unroll
                for (int h = 0; h < NSK_BP_MAX_MEMBERS; h++)
                    if (h < A) s = s - vin[kx[h]];
                if (s == s) atomicMax(acc + kj, ms_key(s));
            }
            ms_wave_sync();
            const long long mo = a.msg_off[e];
            for (int k = lane; k < n; k += 64) m.M[mo + k] = ms_unkey(acc[k]) + 0.0;
        }
        ms_wave_sync();                             // M is written; the last variable's shares have been read
        const double parts = (double)(d + 1);
        for (int k = lane; k < n; k += 64) {
            double s = 0.0;
            for (int x = 0; x < d; x++) s = s + m.D[a.msg_off[edges[x]] + k];
            for (int x = 0; x < d; x++) s = s + m.M[a.msg_off[edges[x]] + k];
            tot[k] = s / parts;
        }
        ms_wave_sync();
        for (long long x = lane; x < (long long)d * n; x += 64) {
            const int xe = (int)(x / n), k = (int)(x - (long long)xe * n);
            const long long mo = a.msg_off[edges[xe]];
            const double old = m.D[mo + k], nw = (old + m.M[mo + k]) - tot[k];
            m.D[mo + k] = nw;
            res = fmax(res, dual_change(nw, old));
        }
    }
    // the block's residual as ms_residual reduces it, over the waves this launch has
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) res = fmax(res, __shfl_xor(res, off, 64));
    if (lane == 0) red[w] = res;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < W; k++) res = fmax(res, red[k]);
        if (res > 0.0) atomicMax(residual + t, (unsigned long long)__double_as_longlong(res));
    }
}

// ---- the terms of the bound.  r_f(ai) read where the entries lie; one lane, ascending
__device__ __forceinline__ double dual_entry(const DualArgs &m, long long t0, int T, int e0, int A, int ai) {
    const BpArgs &a = m.b;
    double r = a.theta[t0 + ai];
    int st = T;
    for (int h = 0; h < A; h++) {
        const long long mo = a.msg_off[e0 + h];
        const int ch = (int)(a.msg_off[e0 + h + 1] - mo);
        st /= ch;
        r = r - m.D[mo + (ai / st) % ch];
    }
    return r;
}

// A wave takes 64 factors: every lane folds its own where the table is small; the large ones the wave takes one after the
// other, the lanes striding over the entries, their maxima met by shuffles of the order-preserving keys.  tf = MAX + 0.0.
// Then one lane per free variable with an edge: Bv in edge order, tv its maximum in k order.
static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_dual_terms(const DualArgs m) {
    const BpArgs &a = m.b;
    const int lane = (int)(threadIdx.x & 63);
    for (long long base = (long long)blockIdx.x * NSK_BLOCK + (threadIdx.x & ~63u); base < a.nfactor; base += (long long)gridDim.x * NSK_BLOCK) {
        const long long f = base + lane;
        int T = 0;
        if (f < a.nfactor) {
            const long long t0 = a.tab_off[f];
            const int e0 = a.edge_off[f], A = a.edge_off[f + 1] - e0;
            T = (int)(a.tab_off[f + 1] - t0);
            if (T <= NSK_DUAL_LANE_TABLE) {
                double mx = ms_nan();
                for (int ai = 0; ai < T; ai++) mx = ms_max(mx, dual_entry(m, t0, T, e0, A, ai));
                m.tf[f] = mx + 0.0;
            }
        }
        unsigned long long big = __ballot(T > NSK_DUAL_LANE_TABLE);
        while (big) {
            const int l = __ffsll((long long)big) - 1;
            big &= big - 1;
            const long long g = base + l, t0 = a.tab_off[g];
            const int e0 = a.edge_off[g], A = a.edge_off[g + 1] - e0, Tg = (int)(a.tab_off[g + 1] - t0);
            unsigned long long key = 0ull;
            for (int ai = lane; ai < Tg; ai += 64) {
                const double r = dual_entry(m, t0, Tg, e0, A, ai);
                if (r == r) { const unsigned long long kk = ms_key(r); key = kk > key ? kk : key; }
            }
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned long long o = (unsigned long long)__shfl_xor((long long)key, off, 64);
                key = o > key ? o : key;
            }
            if (lane == 0) m.tf[g] = ms_unkey(key) + 0.0;
        }
    }
    for (int i = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); i < a.nvlist; i += (int)(gridDim.x * NSK_BLOCK)) {
        const int id = a.v_list[i], q0 = a.v_eoff[i], d = a.v_eoff[i + 1] - q0;
        const long long b0 = a.b_off[id];
        const int n = (int)(a.b_off[id + 1] - b0);
        double mx = ms_nan();
        for (int k = 0; k < n; k++) {
            double s = 0.0;
            for (int x = 0; x < d; x++) s = s + m.D[a.msg_off[a.v_edges[q0 + x]] + k];
            m.bv[b0 + k] = s;
            mx = ms_max(mx, s);
        }
        m.tv[id] = mx;
    }
}

}  // namespace nsk
