// nsk_kernels_bptrw.h -- tree-reweighted belief propagation (fractional BP with one weight rho_f a factor) on the resident
// set-up of nsk_kernels_bp.h: the kernels of nsk_bp_trw_run / nsk_bp_trw_download (nsk_bp_trw.hip; the rule is stated in
// include/numbskull_amd.h and restated in numpy by numbskull_amd.diagnostics.trw_iterate).  Messages live in the log
// domain, normalised to a largest entry of 0: LF factor -> variable, LN variable -> factor, and EN = exp(LN), which is
// what the factor phase multiplies.  Every sum is taken in the order the rule writes, so a run is reproducible and both
// routes of the factor phase give the same bits; against numpy only log and exp differ (the device's ocml log and the
// library's nsk_exp), which is why that comparison has a tolerance.
//
//   k_trw_psi      one lane per factor: psi_rho_f(a) = nsk_exp((theta_f(a) - max_a theta_f) / rho_f)
//   k_trw_reset    one lane per directed edge: LF = LN = 0, EN = 1; one lane per variable: the beliefs and the energy
//                  terms the iterations do not write
//   k_trw_lane     the LANE route (nsk_bp_trw_plan.h): one lane per factor, one ascending walk of the table that feeds all
//                  A outgoing vectors; one launch for the 2 x 2 tables, one for the rest; see there
//   k_trw_wave     the WAVE route: one wave per factor, table and incoming vectors staged in LDS; see there
//   k_trw_var      one lane per free variable with an edge: S = sum rho LF, the messages LN = S - LF, EN and the belief
//   k_trw_fbelief  one lane per factor: the factor beliefs, on demand
//   k_trw_energy   one lane per factor and per free variable with an edge: the terms of log Z, on demand
//
// The term of output (j, k) from table entry a is ((psi(a) * EN_0[a_0]) * ..) over the axes i != j ascending -- a left
// fold.  The lane route forms it from the prefix psi * EN_0 * .. * EN_{j-1} that successive j share and the wave route
// from psi(a) directly: the same products in the same order.  Both add the terms of one (j, k) ascending in a, from 0.0.
#pragma once

#include "nsk_bp_trw_plan.h"
#include "nsk_kernels_bpmap.h"      // ms_max, ms_done, ms_residual, ms_wave_sync

namespace nsk {

// what the kernels read beside the set-up
struct TrwArgs {
    BpArgs b;
    const double *rho;              // [nfactor]
    double *psi;                    // [ntable] psi_rho
    double *LF, *LN, *EN;           // msg_off's layout
    double *bel;                    // b_off's layout
    double *tf, *tv;                // [nfactor], [nid]: the terms of log Z
    const int32_t *lane_ids, *wave_ids;
    int32_t nlane, nwave, wave_lds;
};

static __global__ __launch_bounds__(NSK_BLOCK) void k_trw_psi(const TrwArgs t) {
    const BpArgs &a = t.b;
    for (long long f = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; f < a.nfactor; f += (long long)gridDim.x * NSK_BLOCK) {
        const long long t0 = a.tab_off[f], t1 = a.tab_off[f + 1];
        const double r = t.rho[f];
        double mx = a.theta[t0];
        for (long long i = t0 + 1; i < t1; i++) {
            const double th = a.theta[i];
            if (th > mx) mx = th;
        }
        for (long long i = t0; i < t1; i++) t.psi[i] = nsk_exp((a.theta[i] - mx) / r);
    }
}

static __global__ __launch_bounds__(NSK_BLOCK) void k_trw_reset(const TrwArgs t) {
    const BpArgs &a = t.b;
    for (int e = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); e < a.nedge; e += (int)(gridDim.x * NSK_BLOCK))
        for (long long i = a.msg_off[e]; i < a.msg_off[e + 1]; i++) { t.LF[i] = 0.0; t.LN[i] = 0.0; t.EN[i] = 1.0; }
    // a clamped variable: the set-up's indicator belief, no term; a free one: the uniform law and log card, which stay
    // where it has no edge
    for (long long id = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; id < a.nid; id += (long long)gridDim.x * NSK_BLOCK) {
        const int st = a.v_state[id];
        const long long b0 = a.b_off[id], b1 = a.b_off[id + 1];
        const double n = (double)(b1 - b0);
        for (long long i = b0; i < b1; i++) t.bel[i] = st == 2 ? 1.0 / n : a.belief[i];
        t.tv[id] = st == 2 ? log(n) : 0.0;
    }
}

// ---- the factor phase.  The messages of a factor's edges are neighbours in msg_off's layout: entry (j, k) is
// mo0 + o_j + k.  ox / cx: the offsets o_i and cardinalities c_i of the axes, 0 / 1 beyond A; the loops over the axes are
// unrolled over NSK_BP_MAX_MEMBERS under the test i < A, so both arrays are indexed by constants and live in registers.
__device__ __forceinline__ void trw_axes(const BpArgs &a, int e0, int A, long long mo0, int (&ox)[NSK_BP_MAX_MEMBERS], int (&cx)[NSK_BP_MAX_MEMBERS]) {
#pragma unroll
    for (int i = 0; i < NSK_BP_MAX_MEMBERS; i++) {
        ox[i] = 0; cx[i] = 1;
        if (i < A) { ox[i] = (int)(a.msg_off[e0 + i] - mo0); cx[i] = (int)(a.msg_off[e0 + i + 1] - mo0) - ox[i]; }
    }
}

// the axis of message entry c: its index, offset and cardinality
__device__ __forceinline__ void trw_axis_of(const int (&ox)[NSK_BP_MAX_MEMBERS], const int (&cx)[NSK_BP_MAX_MEMBERS], int A, int c, int &j, int &oj, int &cj) {
    j = 0; oj = 0; cj = cx[0];
#pragma unroll
    for (int i = 1; i < NSK_BP_MAX_MEMBERS; i++)
        if (i < A && ox[i] <= c) { j = i; oj = ox[i]; cj = cx[i]; }
}

// s_j[k]: the sum over the table entries a with digit j equal to k, ascending, of psi(a) times the incoming entries of
// the axes i != j ascending.  psi and vin are the factor's own: LDS on the wave route, global memory on the lane route.
__device__ __forceinline__ double trw_entry_sum(const double *psi, const double *vin, const int (&ox)[NSK_BP_MAX_MEMBERS],
                                                const int (&cx)[NSK_BP_MAX_MEMBERS], int A, int T, int j, int cj, int k) {
    int sj = 1;
#pragma unroll
    for (int i = 0; i < NSK_BP_MAX_MEMBERS; i++)
        if (i < A && i > j) sj *= cx[i];
    const int nhi = T / (cj * sj);
    double s = 0.0;
    for (int hi = 0; hi < nhi; hi++)
        for (int lo = 0; lo < sj; lo++) {
            const int ai = (hi * cj + k) * sj + lo;
            unsigned int r = (unsigned int)ai;
            int kx[NSK_BP_MAX_MEMBERS];
#pragma unroll
            for (int i = NSK_BP_MAX_MEMBERS - 1; i >= 0; i--) {
                kx[i] = 0;
                if (i < A) {
                    unsigned int d;
                    if (cx[i] == 2) { d = r & 1u; r >>= 1; }
                    else { const unsigned int q = r / (unsigned int)cx[i]; d = r - q * (unsigned int)cx[i]; r = q; }
                    kx[i] = ox[i] + (int)d;
                }
            }
            double x = psi[ai];
#pragma unroll
            for (int i = 0; i < NSK_BP_MAX_MEMBERS; i++)
                if (i < A && i != j) x = x * vin[kx[i]];
            s = s + x;
        }
    return s;
}

// ---- the lane route.  Three paths, by the factor's shape (uniform over nothing: lanes diverge here):
//   a 2 x 2 table   the four psi, the four incoming entries and the four sums in registers: no array, no loop;
//   C <= NSK_ZLOCAL the incoming vectors are loaded up front into a lane-private array, the table is walked once,
//                   ascending, and entry a adds its A terms to the lane-private sums s_j[a_j];
//   otherwise       (only under the knob NSK_TRW_LANE_MAX) every output entry is summed on its own out of global memory,
//                   twice: the first pass finds the largest logarithm of an axis, the second recomputes the identical
//                   sums and stores -- k_bp_factor's way with large domains.
// The list holds the 2 x 2 tables first (the plan): PAIR serves the entries [lo, hi) that are such tables from a handful of
// registers, the other launch the rest (whose private arrays and axis loops would cost the pairs their occupancy).
template <bool PAIR>
__global__ __launch_bounds__(NSK_BLOCK) void k_trw_lane(const TrwArgs t, int lo, int hi, int it, double tol, double lam, double oml,
                                                       unsigned long long *residual) {
    if (ms_done(residual, it, tol)) return;         // block-uniform, before the barrier
    const BpArgs &a = t.b;
    double res = 0.0;
    for (int i = lo + (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); i < hi; i += (int)(gridDim.x * NSK_BLOCK)) {
        const int f = t.lane_ids[i];
        const int e0 = a.edge_off[f];
        int A = a.edge_off[f + 1] - e0;
        A = A > NSK_BP_MAX_MEMBERS ? NSK_BP_MAX_MEMBERS : A;
        const long long t0 = a.tab_off[f], mo0 = a.msg_off[e0];
        const int T = (int)(a.tab_off[f + 1] - t0);
        const int C = (int)(a.msg_off[e0 + A] - mo0);
        double *Fo = t.LF + mo0;
        if (PAIR) {
            // a pairwise factor of binary variables: entry a = 2 a_0 + a_1; v the incoming of axis 0, u of axis 1
            const double p0 = t.psi[t0], p1 = t.psi[t0 + 1], p2 = t.psi[t0 + 2], p3 = t.psi[t0 + 3];
            const double v0 = t.EN[mo0], v1 = t.EN[mo0 + 1], u0 = t.EN[mo0 + 2], u1 = t.EN[mo0 + 3];
            const double l0 = log(p0 * u0 + p1 * u1), l1 = log(p2 * u0 + p3 * u1);      // axis 0: over a_1
            const double q0 = log(p0 * v0 + p2 * v1), q1 = log(p1 * v0 + p3 * v1);      // axis 1: over a_0
            const double lm = ms_max(l0, l1), qm = ms_max(q0, q1);
            res = fmax(res, bp_store(Fo, l0 - lm, lam, oml));
            res = fmax(res, bp_store(Fo + 1, l1 - lm, lam, oml));
            res = fmax(res, bp_store(Fo + 2, q0 - qm, lam, oml));
            res = fmax(res, bp_store(Fo + 3, q1 - qm, lam, oml));
            continue;
        }
        if (C <= NSK_ZLOCAL) {
            double vin[NSK_ZLOCAL], sk[NSK_ZLOCAL];
            for (int c = 0; c < C; c++) { vin[c] = t.EN[mo0 + c]; sk[c] = 0.0; }
            for (int ai = 0; ai < T; ai++) {
                double pre = t.psi[t0 + ai];        // psi times the incoming entries of the axes below j, left to right
                int stj = T;
                for (int j = 0; j < A; j++) {
                    const int oj = (int)(a.msg_off[e0 + j] - mo0), cj = (int)(a.msg_off[e0 + j + 1] - mo0) - oj;
                    stj /= cj;
                    const int kj = (oj + (ai / stj) % cj) & (NSK_ZLOCAL - 1);
                    double s = pre;
                    int st = stj;
                    for (int h = j + 1; h < A; h++) {
                        const int oh = (int)(a.msg_off[e0 + h] - mo0), ch = (int)(a.msg_off[e0 + h + 1] - mo0) - oh;
                        st /= ch;
                        s = s * vin[(oh + (ai / st) % ch) & (NSK_ZLOCAL - 1)];
                    }
                    sk[kj] = sk[kj] + s;
                    pre = pre * vin[kj];
                }
            }
            for (int c = 0; c < C; c++) sk[c] = log(sk[c]);
            for (int j = 0; j < A; j++) {
                const int oj = (int)(a.msg_off[e0 + j] - mo0), cj = (int)(a.msg_off[e0 + j + 1] - mo0) - oj;
                double mx = sk[oj & (NSK_ZLOCAL - 1)];
                for (int k = 1; k < cj; k++) mx = ms_max(mx, sk[(oj + k) & (NSK_ZLOCAL - 1)]);
                for (int k = 0; k < cj; k++) res = fmax(res, bp_store(Fo + oj + k, sk[(oj + k) & (NSK_ZLOCAL - 1)] - mx, lam, oml));
            }
            continue;
        }
        int ox[NSK_BP_MAX_MEMBERS], cx[NSK_BP_MAX_MEMBERS];
        trw_axes(a, e0, A, mo0, ox, cx);
        for (int j = 0; j < A; j++) {
            const int oj = (int)(a.msg_off[e0 + j] - mo0), cj = (int)(a.msg_off[e0 + j + 1] - mo0) - oj;
            double mx = ms_nan();
            for (int k = 0; k < cj; k++) mx = ms_max(mx, log(trw_entry_sum(t.psi + t0, t.EN + mo0, ox, cx, A, T, j, cj, k)));
            for (int k = 0; k < cj; k++)
                res = fmax(res, bp_store(Fo + oj + k, log(trw_entry_sum(t.psi + t0, t.EN + mo0, ox, cx, A, T, j, cj, k)) - mx, lam, oml));
        }
    }
    ms_residual<NSK_BLOCK>(res, residual + it);
}

// ---- the wave route.  Dynamic LDS: wave w of a block owns t.wave_lds doubles, the largest T + 2 C of the route's
// factors (nsk_bp_trw_plan.h), laid out as psi[T], vin[C], out[C].  The wave copies psi_rho_f and the factor's A incoming
// vectors (neighbours in EN) with coalesced loads; then lane l owns the output entries c = l, l + 64, .. of the C: it
// sums entry (j, k) ascending out of LDS (trw_entry_sum: the order of the lane route) and leaves the logarithm in
// out[c].  Behind a wave barrier the owning lane folds its axis' maximum in k order out of `out`, damps, stores and takes
// the residual.  A table of more than 64 entries an output makes a lane loop; C > 64 gives lanes unequal numbers of
// outputs.  The waves of a block meet only in the residual's reduction; blockDim.x / 64 waves, NSK_TRW_WAVES at most.
static __global__ __launch_bounds__(NSK_TRW_WAVES * 64) void k_trw_wave(const TrwArgs t, int it, double tol, double lam, double oml,
                                                                       unsigned long long *residual) {
    extern __shared__ double trw_lds[];
    __shared__ double red[NSK_TRW_WAVES];
    if (ms_done(residual, it, tol)) return;         // block-uniform, before the barrier
    const BpArgs &a = t.b;
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6), W = (int)(blockDim.x >> 6);
    double *psi = trw_lds + (size_t)w * (size_t)t.wave_lds;
    double res = 0.0;
    for (int idx = (int)blockIdx.x * W + w; idx < t.nwave; idx += (int)gridDim.x * W) {
        const int f = __builtin_amdgcn_readfirstlane(t.wave_ids[idx]);      // wave-uniform: what follows is scalar
        const int e0 = a.edge_off[f];
        int A = a.edge_off[f + 1] - e0;
        A = A > NSK_BP_MAX_MEMBERS ? NSK_BP_MAX_MEMBERS : A;
        const long long t0 = a.tab_off[f], mo0 = a.msg_off[e0];
        const int T = (int)(a.tab_off[f + 1] - t0);
        const int C = (int)(a.msg_off[e0 + A] - mo0);
        if ((long long)T + 2ll * C > (long long)t.wave_lds) continue;      // (the plan routes no such factor here)
        double *vin = psi + T, *out = vin + C;
        int ox[NSK_BP_MAX_MEMBERS], cx[NSK_BP_MAX_MEMBERS];
        trw_axes(a, e0, A, mo0, ox, cx);
        ms_wave_sync();                             // the last factor's `out` has been read
        for (int c = lane; c < T; c += 64) psi[c] = t.psi[t0 + c];
        for (int c = lane; c < C; c += 64) vin[c] = t.EN[mo0 + c];
        ms_wave_sync();
        for (int c = lane; c < C; c += 64) {
            int j, oj, cj;
            trw_axis_of(ox, cx, A, c, j, oj, cj);
            out[c] = log(trw_entry_sum(psi, vin, ox, cx, A, T, j, cj, c - oj));
        }
        ms_wave_sync();
        for (int c = lane; c < C; c += 64) {
            int j, oj, cj;
            trw_axis_of(ox, cx, A, c, j, oj, cj);
            double mx = out[oj];
            for (int k = 1; k < cj; k++) mx = ms_max(mx, out[oj + k]);
            res = fmax(res, bp_store(t.LF + mo0 + c, out[c] - mx, lam, oml));
        }
    }
    // the block's residual as ms_residual reduces it, over the waves this launch has
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) res = fmax(res, __shfl_xor(res, off, 64));
    if (lane == 0) red[w] = res;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < W; k++) res = fmax(res, red[k]);
        if (res > 0.0) atomicMax(residual + it, (unsigned long long)__double_as_longlong(res));
    }
}

// ---- the variable phase.  S[k] = the sum over the variable's edges ascending of rho_f * LF[e][k] (one rounded product,
// one rounded sum), from 0.0; per edge LN[k] = (S[k] - LF[e][k]) - their maximum folded in k order, EN = nsk_exp(LN); the
// belief nsk_exp(S[k] - max S) over its k-ordered sum.
// N == 2: a binary variable, vectors in registers; N == NSK_ZLOCAL: lane-private arrays of n <= N entries; N == 0: S lives
// in the variable's wk slot, the vector under way in the LN slot itself and the unnormalised belief in the belief slot
// (bp_var_lane's homes).
template <int N>
__device__ __forceinline__ void trw_var_lane(const TrwArgs &t, int n, const int32_t *edges, int d, double *bel, double *wk) {
    const BpArgs &a = t.b;
    double Sl[N ? N : 1], Tl[N ? N : 1];
    double *S = N ? Sl : wk;
    if (N == 2) n = 2;
#define NSK_TRW_K for (int k = 0; k < (N == 2 ? 2 : n); k++)
    NSK_TRW_K S[k] = 0.0;
    for (int i = 0; i < d; i++) {
        const int e = edges[i];
        const long long mo = a.msg_off[e];
        const double r = t.rho[a.e_fac[e]];
        NSK_TRW_K S[k] = S[k] + r * t.LF[mo + k];
    }
    for (int i = 0; i < d; i++) {
        const long long mo = a.msg_off[edges[i]];
        double *T = N ? Tl : t.LN + mo;
        NSK_TRW_K T[k] = S[k] - t.LF[mo + k];
        double mt = T[0];
        for (int k = 1; k < (N == 2 ? 2 : n); k++) mt = ms_max(mt, T[k]);
        NSK_TRW_K {
            const double ln = T[k] - mt;
            t.LN[mo + k] = ln;
            t.EN[mo + k] = nsk_exp(ln);
        }
    }
    double mx = S[0];
    for (int k = 1; k < (N == 2 ? 2 : n); k++) mx = ms_max(mx, S[k]);
    double *B = N ? Tl : bel;
    NSK_TRW_K B[k] = nsk_exp(S[k] - mx);
    double Z = B[0];
    for (int k = 1; k < (N == 2 ? 2 : n); k++) Z = Z + B[k];
    NSK_TRW_K bel[k] = B[k] / Z;
#undef NSK_TRW_K
}

// the same arithmetic for a binary variable of at most NSK_BP_VAR_REG edges (bp_var_lane_reg): LF and rho of every edge
// in registers, every message read once and written once, the loads of all edges in flight together
__device__ __forceinline__ void trw_var_lane_reg(const TrwArgs &t, const int32_t *edges, int d, double *bel) {
    const BpArgs &a = t.b;
    long long mo[NSK_BP_VAR_REG];
    int fe[NSK_BP_VAR_REG];
    double f0[NSK_BP_VAR_REG], f1[NSK_BP_VAR_REG], r[NSK_BP_VAR_REG];
#pragma unroll
    for (int i = 0; i < NSK_BP_VAR_REG; i++) {
        const int e = i < d ? edges[i] : 0;
        mo[i] = i < d ? a.msg_off[e] : 0;
        fe[i] = i < d ? a.e_fac[e] : 0;
    }
#pragma unroll
    for (int i = 0; i < NSK_BP_VAR_REG; i++)
        if (i < d) { f0[i] = t.LF[mo[i]]; f1[i] = t.LF[mo[i] + 1]; r[i] = t.rho[fe[i]]; }
    double S0 = 0.0, S1 = 0.0;
#pragma unroll
    for (int i = 0; i < NSK_BP_VAR_REG; i++)
        if (i < d) { S0 = S0 + r[i] * f0[i]; S1 = S1 + r[i] * f1[i]; }
#pragma unroll
    for (int i = 0; i < NSK_BP_VAR_REG; i++)
        if (i < d) {
            const double T0 = S0 - f0[i], T1 = S1 - f1[i], mt = ms_max(T0, T1);
            const double n0 = T0 - mt, n1 = T1 - mt;
            t.LN[mo[i]] = n0; t.LN[mo[i] + 1] = n1;
            t.EN[mo[i]] = nsk_exp(n0); t.EN[mo[i] + 1] = nsk_exp(n1);
        }
    const double mx = ms_max(S0, S1);
    const double b0 = nsk_exp(S0 - mx), b1 = nsk_exp(S1 - mx), Z = b0 + b1;
    bel[0] = b0 / Z; bel[1] = b1 / Z;
}

// iteration `it` over the entries [lo, hi) of v_list, the binary variables first (k_bp_var)
template <bool BIN>
__global__ __launch_bounds__(NSK_BP_VAR_BLOCK) void k_trw_var(const TrwArgs t, int lo, int hi, int it, double tol, const unsigned long long *residual) {
    if (ms_done(residual, it, tol)) return;
    const BpArgs &a = t.b;
    for (int i = lo + (int)(blockIdx.x * NSK_BP_VAR_BLOCK + threadIdx.x); i < hi; i += (int)(gridDim.x * NSK_BP_VAR_BLOCK)) {
        const int id = a.v_list[i];
        const int e0 = a.v_eoff[i], d = a.v_eoff[i + 1] - e0;
        const long long b0 = a.b_off[id];
        const int n = (int)(a.b_off[id + 1] - b0);
        if (BIN && d <= NSK_BP_VAR_REG) trw_var_lane_reg(t, a.v_edges + e0, d, t.bel + b0);
        else if (BIN) trw_var_lane<2>(t, 2, a.v_edges + e0, d, t.bel + b0, nullptr);
        else if (n <= NSK_ZLOCAL) trw_var_lane<NSK_ZLOCAL>(t, n, a.v_edges + e0, d, t.bel + b0, nullptr);
        else trw_var_lane<0>(t, n, a.v_edges + e0, d, t.bel + b0, a.wk + b0);
    }
}

// ---- on demand.  x(a) = ((psi_rho(a) * EN[(f,0)][a_0]) * ..) over the axes ascending
__device__ __forceinline__ double trw_entry_x(const TrwArgs &t, long long t0, int T, int e0, int A, int ai) {
    const BpArgs &a = t.b;
    double x = t.psi[t0 + ai];
    int st = T;
    for (int i = 0; i < A; i++) {
        const long long mo = a.msg_off[e0 + i];
        const int ci = (int)(a.msg_off[e0 + i + 1] - mo);
        st /= ci;
        x = x * t.EN[mo + (ai / st) % ci];
    }
    return x;
}

// b_f(a) = x(a) divided by the a-ordered sum
static __global__ __launch_bounds__(NSK_BLOCK) void k_trw_fbelief(const TrwArgs t, double *fb) {
    const BpArgs &a = t.b;
    for (long long f = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; f < a.nfactor; f += (long long)gridDim.x * NSK_BLOCK) {
        const long long t0 = a.tab_off[f];
        const int T = (int)(a.tab_off[f + 1] - t0);
        const int e0 = a.edge_off[f], A = a.edge_off[f + 1] - e0;
        double Z = 0.0;
        for (int ai = 0; ai < T; ai++) {
            const double x = trw_entry_x(t, t0, T, e0, A, ai);
            fb[t0 + ai] = x;
            Z = ai == 0 ? x : Z + x;
        }
        for (int ai = 0; ai < T; ai++) fb[t0 + ai] = fb[t0 + ai] / Z;
    }
}

// tf[f] = the a-ordered sum of b_f(a) * (theta_f(a) - rho_f * log b_f(a)) over the entries with b_f(a) > 0;
// tv[id] = (the sum of rho over the variable's edges ascending - 1) * the k-ordered sum of b log b over b > 0, for a free
// variable with an edge (k_trw_reset wrote the others).  The host adds the terms with an exactly rounded sum.
static __global__ __launch_bounds__(NSK_BLOCK) void k_trw_energy(const TrwArgs t) {
    const BpArgs &a = t.b;
    for (long long f = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; f < a.nfactor; f += (long long)gridDim.x * NSK_BLOCK) {
        const long long t0 = a.tab_off[f];
        const int T = (int)(a.tab_off[f + 1] - t0);
        const int e0 = a.edge_off[f], A = a.edge_off[f + 1] - e0;
        const double r = t.rho[f];
        double Z = 0.0;
        for (int ai = 0; ai < T; ai++) {
            const double x = trw_entry_x(t, t0, T, e0, A, ai);
            Z = ai == 0 ? x : Z + x;
        }
        double term = 0.0;
        for (int ai = 0; ai < T; ai++) {
            const double b = trw_entry_x(t, t0, T, e0, A, ai) / Z;
            if (b > 0.0) term = term + b * (a.theta[t0 + ai] - r * log(b));
        }
        t.tf[f] = term;
    }
    for (int i = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); i < a.nvlist; i += (int)(gridDim.x * NSK_BLOCK)) {
        const int id = a.v_list[i];
        double R = 0.0, h = 0.0;
        for (int e = a.v_eoff[i]; e < a.v_eoff[i + 1]; e++) R = R + t.rho[a.e_fac[a.v_edges[e]]];
        for (long long k = a.b_off[id]; k < a.b_off[id + 1]; k++) {
            const double b = t.bel[k];
            if (b > 0.0) h = h + b * log(b);
        }
        t.tv[id] = (R - 1.0) * h;
    }
}

}  // namespace nsk
