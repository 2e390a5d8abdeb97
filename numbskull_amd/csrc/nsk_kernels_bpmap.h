// nsk_kernels_bpmap.h -- max-product belief propagation (MAP decoding) on the resident set-up of nsk_kernels_bp.h: the
// kernels of nsk_bp_map_run / nsk_bp_map_decode (nsk_bp_map.hip; the rule is stated in include/numbskull_amd.h and
// restated in numpy by numbskull_amd.diagnostics.ms_iterate / ms_decode -- device and numpy agree bit for bit).  Log
// domain: the tables are the set-up's theta, a message entry is a double <= 0 after the first iteration, products become
// sums and sums become maxima.  Every SUM below is taken in the order the rule writes; a MAXIMUM may be taken in any order
// (see "the order of a maximum"), which is what lets the factor phase split a table across lanes.
//
//   k_ms_reset    one lane per directed edge: both message arrays +0.0; one lane per variable: the max-marginals the
//                 iterations do not write
//   k_ms_lane     the LANE route (nsk_bp_map_plan.h): one lane per factor walks its table once and writes all A outgoing
//                 vectors; the incoming values and the running maxima live in two lane-private arrays of NSK_ZLOCAL
//   k_ms_wave     the WAVE route: one wave per factor, NSK_MS_WAVES factors a block; see there
//   k_ms_edge     the EDGE route: one lane per directed edge, bp_factor_body's walk with (max, +) for (+, *)
//   k_ms_var      one lane per free variable with an edge: prefix and suffix sums, the messages variable -> factor and
//                 the max-marginal (bp_var_lane's walk without the rescale)
//   k_ms_decode   one lane per free variable with an edge: the argmax into the chain row, the ties counted
//
// The order of a maximum.  ms_max(a, b) = b where b > a or a is a NaN, else a: folded from the first entry it passes over
// NaNs as fmax does and, among equal entries, keeps the first -- which matters for the bits only where the equal entries
// are -0.0 and +0.0.  The wave route folds the same entries in no order at all (integer maxima of order-preserving keys,
// in which -0.0 < +0.0), so the two agree bit for bit as long as no maximum over SEVERAL entries meets a -0.0.  None does:
// a V entry is T - max T over finite T, which is +0.0 where equal and negative otherwise, never -0.0 (and +0.0 at a cold
// start); x + V for a V entry that is +0.0 or negative is never -0.0 (x + +0.0 is +0.0 for x = -0.0, x + negative is
// negative or x itself an infinity).  So s_j(a) can be -0.0 only where no V entry is added: A = 1, s_0(a) = theta(a) --
// and there every m_k is the maximum over the single entry a = k.  (The maximum over k that normalises a message, and
// every maximum of the variable phase, is folded by one lane in k order on every route.)  The numpy mirror checks this
// on the test cases: it folds by ms_max and counts the -0.0 among the message entries.
#pragma once

#include "nsk_bp_map_plan.h"
#include "nsk_kernels_bp.h"

namespace nsk {

#define NSK_MS_WAVES 4              // factors (waves) a block of the wave route

// what the kernels read beside the set-up
struct MsArgs {
    BpArgs b;
    double *F, *V, *mm;             // factor -> variable, variable -> factor (msg_off's layout), max-marginals (b_off's)
    const int32_t *lane_ids, *wave_ids;     // factors
    const int32_t *edge_ids;        // directed edges
    int32_t nlane, nwave, nedge_r;
};

__device__ __forceinline__ double ms_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double ms_max(double a, double b) { return (b > a || a != a) ? b : a; }

// the early exit of iteration t, uniform over the grid
__device__ __forceinline__ bool ms_done(const unsigned long long *residual, int t, double tol) {
    return t > 0 && __longlong_as_double((long long)residual[t - 1]) <= tol;
}

// a block's residual as bp_factor_body reduces it: non-negative doubles, +inf for a NaN; every lane of the block comes here
template <int BLOCK>
__device__ __forceinline__ void ms_residual(double res, unsigned long long *slot) {
    __shared__ double lds[BLOCK / 64];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) res = fmax(res, __shfl_xor(res, off, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = res;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < BLOCK / 64; k++) res = fmax(res, lds[k]);
        if (res > 0.0) atomicMax(slot, (unsigned long long)__double_as_longlong(res));
    }
}

static __global__ __launch_bounds__(NSK_BLOCK) void k_ms_reset(const MsArgs m) {
    const BpArgs &a = m.b;
    const double ninf = __longlong_as_double((long long)0xfff0000000000000ULL);
    for (int e = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); e < a.nedge; e += (int)(gridDim.x * NSK_BLOCK))
        for (long long i = a.msg_off[e]; i < a.msg_off[e + 1]; i++) { m.F[i] = 0.0; m.V[i] = 0.0; }
    // a clamped variable: 0 at its value (where the set-up's indicator belief reads 1), -inf elsewhere; a free one: 0
    for (long long id = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; id < a.nid; id += (long long)gridDim.x * NSK_BLOCK) {
        const int st = a.v_state[id];
        for (long long i = a.b_off[id]; i < a.b_off[id + 1]; i++) m.mm[i] = (st == 2 || a.belief[i] == 1.0) ? 0.0 : ninf;
    }
}

// ---- the lane route: T < NSK_MS_LANE_TABLE entries, the axes' cardinalities sum to C <= NSK_ZLOCAL.  The messages of a
// factor's edges are neighbours in msg_off's layout: entry (j, k) is mo0 + o_j + k.
static __global__ __launch_bounds__(NSK_BLOCK) void k_ms_lane(const MsArgs m, int t, double tol, double lam, double oml,
                                                             unsigned long long *residual) {
    if (ms_done(residual, t, tol)) return;          // block-uniform, before the barrier
    const BpArgs &a = m.b;
    double res = 0.0;
    for (int i = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); i < m.nlane; i += (int)(gridDim.x * NSK_BLOCK)) {
        const int f = m.lane_ids[i];
        const int e0 = a.edge_off[f], A = a.edge_off[f + 1] - e0;
        const long long t0 = a.tab_off[f], mo0 = a.msg_off[e0];
        const int T = (int)(a.tab_off[f + 1] - t0);
        double *Fo = m.F + mo0;
        if (A == 2 && T == 4 && a.msg_off[e0 + 1] - mo0 == 2) {
            // a pairwise factor of binary variables, all in registers: entry a = 2 a_0 + a_1
            const double th0 = a.theta[t0], th1 = a.theta[t0 + 1], th2 = a.theta[t0 + 2], th3 = a.theta[t0 + 3];
            const double v0 = m.V[mo0], v1 = m.V[mo0 + 1], u0 = m.V[mo0 + 2], u1 = m.V[mo0 + 3];
            const double p0 = ms_max(th0 + u0, th1 + u1), p1 = ms_max(th2 + u0, th3 + u1);      // axis 0: over a_1
            const double q0 = ms_max(th0 + v0, th2 + v1), q1 = ms_max(th1 + v0, th3 + v1);      // axis 1: over a_0
            const double pm = ms_max(p0, p1), qm = ms_max(q0, q1);
            res = fmax(res, bp_store(Fo, p0 - pm, lam, oml));
            res = fmax(res, bp_store(Fo + 1, p1 - pm, lam, oml));
            res = fmax(res, bp_store(Fo + 2, q0 - qm, lam, oml));
            res = fmax(res, bp_store(Fo + 3, q1 - qm, lam, oml));
            continue;
        }
        double vin[NSK_ZLOCAL], mk[NSK_ZLOCAL];
        int C = (int)(a.msg_off[e0 + A] - mo0);
        C = C > NSK_ZLOCAL ? NSK_ZLOCAL : C;        // (the plan routes no other factor here)
        for (int c = 0; c < C; c++) { vin[c] = m.V[mo0 + c]; mk[c] = ms_nan(); }
        for (int ai = 0; ai < T; ai++) {
            double pre = a.theta[t0 + ai];          // theta + the incoming entries of the axes below j, left to right
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
                    s = s + vin[(oh + (ai / st) % ch) & (NSK_ZLOCAL - 1)];
                }
                mk[kj] = ms_max(mk[kj], s);
                pre = pre + vin[kj];
            }
        }
        for (int j = 0; j < A; j++) {
            const int oj = (int)(a.msg_off[e0 + j] - mo0), cj = (int)(a.msg_off[e0 + j + 1] - mo0) - oj;
            double mx = mk[oj & (NSK_ZLOCAL - 1)];
            for (int k = 1; k < cj; k++) mx = ms_max(mx, mk[(oj + k) & (NSK_ZLOCAL - 1)]);
            for (int k = 0; k < cj; k++) res = fmax(res, bp_store(Fo + oj + k, mk[(oj + k) & (NSK_ZLOCAL - 1)] - mx, lam, oml));
        }
    }
    ms_residual<NSK_BLOCK>(res, residual + t);
}

// ---- the wave route: C <= NSK_MS_LDS.  Per wave 2 x NSK_MS_LDS x 8 bytes of LDS: `vin`, the factor's A incoming vectors
// as they lie in V, and `acc`, one accumulator per outgoing entry (j, k) at the same index.  An accumulator holds the
// order-preserving unsigned key of a double (sign bit set: all bits flipped, else: the sign bit set), 0 = no entry yet,
// and is updated by an integer atomicMax on LDS: the largest key is the largest double, in whichever order the lanes
// arrive.  A NaN is never offered; an accumulator nothing was offered to reads as a NaN.
// Lanes take the entries a = lane + 64 * trip.  A lane decodes the digits of a once (least significant first, a shift for
// a binary axis), gathers the A incoming values from `vin`, and forms s_j(a) for j = 0 .. A - 1 from the left fold
// theta + v_0 + .. + v_{j-1}, which successive j share: s_j(a) is the rule's sum, operation by operation.  The axis
// loops are unrolled over NSK_BP_MAX_MEMBERS under the wave-uniform test i < A, so every array below is indexed by
// constants and lives in registers.  Behind the last trip the lanes normalise: the lane of entry (j, k) folds its axis'
// maximum in k order, damps, stores and takes the residual.  The waves of a block meet only in ms_residual.
__device__ __forceinline__ unsigned long long ms_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ __forceinline__ double ms_unkey(unsigned long long k) {
    if (k == 0ull) return ms_nan();
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k));
}
// the lanes of a wave have written LDS that its other lanes read next
__device__ __forceinline__ void ms_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

static __global__ __launch_bounds__(NSK_MS_WAVES * 64) void k_ms_wave(const MsArgs m, int t, double tol, double lam, double oml,
                                                                     unsigned long long *residual) {
    __shared__ double s_vin[NSK_MS_WAVES][NSK_MS_LDS];
    __shared__ unsigned long long s_acc[NSK_MS_WAVES][NSK_MS_LDS];
    if (ms_done(residual, t, tol)) return;          // block-uniform, before the barrier
    const BpArgs &a = m.b;
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
    double *vin = s_vin[w];
    unsigned long long *acc = s_acc[w];
    double res = 0.0;
    for (int idx = (int)blockIdx.x * NSK_MS_WAVES + w; idx < m.nwave; idx += (int)gridDim.x * NSK_MS_WAVES) {
        const int f = __builtin_amdgcn_readfirstlane(m.wave_ids[idx]);      // wave-uniform: what follows is scalar
        const int e0 = a.edge_off[f];
        int A = a.edge_off[f + 1] - e0;
        A = A > NSK_BP_MAX_MEMBERS ? NSK_BP_MAX_MEMBERS : A;
        const long long t0 = a.tab_off[f], mo0 = a.msg_off[e0];
        const int T = (int)(a.tab_off[f + 1] - t0);
        int C = (int)(a.msg_off[e0 + A] - mo0);
        C = C > NSK_MS_LDS ? NSK_MS_LDS : C;        // (the plan routes no other factor here)
        int ox[NSK_BP_MAX_MEMBERS], cx[NSK_BP_MAX_MEMBERS];
#pragma unroll
        for (int i = 0; i < NSK_BP_MAX_MEMBERS; i++) {
            ox[i] = 0; cx[i] = 1;
            if (i < A) { ox[i] = (int)(a.msg_off[e0 + i] - mo0); cx[i] = (int)(a.msg_off[e0 + i + 1] - mo0) - ox[i]; }
        }
        ms_wave_sync();                             // the last factor's accumulators have been read
        for (int c = lane; c < C; c += 64) { vin[c] = m.V[mo0 + c]; acc[c] = 0ull; }
        ms_wave_sync();
        for (int ai = lane; ai < T; ai += 64) {
            double vv[NSK_BP_MAX_MEMBERS];
            int kx[NSK_BP_MAX_MEMBERS];
            unsigned int r = (unsigned int)ai;
#pragma unroll
            for (int i = NSK_BP_MAX_MEMBERS - 1; i >= 0; i--) {
                kx[i] = 0; vv[i] = 0.0;
                if (i < A) {
                    unsigned int d;
                    if (cx[i] == 2) { d = r & 1u; r >>= 1; }
                    else { const unsigned int q = r / (unsigned int)cx[i]; d = r - q * (unsigned int)cx[i]; r = q; }
                    kx[i] = (ox[i] + (int)d) & (NSK_MS_LDS - 1);
                    vv[i] = vin[kx[i]];
                }
            }
            double pre = a.theta[t0 + ai];
#pragma unroll
            for (int j = 0; j < NSK_BP_MAX_MEMBERS; j++)
                if (j < A) {
                    double s = pre;
#pragma unroll
                    for (int h = j + 1; h < NSK_BP_MAX_MEMBERS; h++)
                        if (h < A) s = s + vv[h];
                    if (s == s) atomicMax(acc + kx[j], ms_key(s));
                    pre = pre + vv[j];
                }
        }
        ms_wave_sync();
        for (int c = lane; c < C; c += 64) {
            int oj = 0, cj = 1;                     // the axis of entry c
#pragma unroll
            for (int i = 0; i < NSK_BP_MAX_MEMBERS; i++)
                if (i < A && ox[i] <= c) { oj = ox[i]; cj = cx[i]; }
            double mx = ms_unkey(acc[oj]);
            for (int k = 1; k < cj; k++) mx = ms_max(mx, ms_unkey(acc[oj + k]));
            res = fmax(res, bp_store(m.F + mo0 + c, ms_unkey(acc[c]) - mx, lam, oml));
        }
    }
    ms_residual<NSK_MS_WAVES * 64>(res, residual + t);
}

// ---- the edge route: the maximum over the table entries with digit j == k, ascending, of theta plus the other axes'
// incoming entries (bp_edge_sum's walk); two passes over k, the second recomputes the identical maxima
__device__ __forceinline__ double ms_edge_max(const MsArgs &m, long long t0, int T, int e0, int A, int j, int cj, int sj, int k) {
    const BpArgs &a = m.b;
    double mk = ms_nan();
    const int nhi = T / (cj * sj);
    for (int hi = 0; hi < nhi; hi++)
        for (int lo = 0; lo < sj; lo++) {
            const int ai = (hi * cj + k) * sj + lo;
            double x = a.theta[t0 + ai];
            int st = T;
            for (int i = 0; i < A; i++) {
                const long long mo = a.msg_off[e0 + i];
                const int ci = (int)(a.msg_off[e0 + i + 1] - mo);
                st /= ci;
                if (i != j) x = x + m.V[mo + (ai / st) % ci];
            }
            mk = ms_max(mk, x);
        }
    return mk;
}

static __global__ __launch_bounds__(NSK_BLOCK) void k_ms_edge(const MsArgs m, int t, double tol, double lam, double oml,
                                                             unsigned long long *residual) {
    if (ms_done(residual, t, tol)) return;          // block-uniform, before the barrier
    const BpArgs &a = m.b;
    double res = 0.0;
    for (int i = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); i < m.nedge_r; i += (int)(gridDim.x * NSK_BLOCK)) {
        const int e = m.edge_ids[i], f = a.e_fac[e];
        const int e0 = a.edge_off[f], A = a.edge_off[f + 1] - e0, j = e - e0;
        const long long t0 = a.tab_off[f], mo = a.msg_off[e];
        const int T = (int)(a.tab_off[f + 1] - t0), cj = (int)(a.msg_off[e + 1] - mo);
        int sj = 1;
        for (int h = A - 1; h > j; h--) sj *= (int)(a.msg_off[e0 + h + 1] - a.msg_off[e0 + h]);
        double mx = ms_nan();
        for (int k = 0; k < cj; k++) mx = ms_max(mx, ms_edge_max(m, t0, T, e0, A, j, cj, sj, k));
        for (int k = 0; k < cj; k++) res = fmax(res, bp_store(m.F + mo + k, ms_edge_max(m, t0, T, e0, A, j, cj, sj, k) - mx, lam, oml));
    }
    ms_residual<NSK_BLOCK>(res, residual + t);
}

// ---- the variable phase.  N == 2: a binary variable, vectors in registers; N == NSK_ZLOCAL: lane-private arrays of
// n <= N entries; N == 0: the prefix sum lives in the variable's max-marginal slot, the suffix sum in its wk slot and the
// vector under way in the V slot itself (bp_var_lane's three homes).
template <int N>
__device__ __forceinline__ void ms_var_lane(const MsArgs &m, int n, const int32_t *edges, int d, double *mm, double *wk) {
    const BpArgs &a = m.b;
    double Pl[N ? N : 1], Sl[N ? N : 1], Tl[N ? N : 1];
    double *P = N ? Pl : mm, *S = N ? Sl : wk;
    if (N == 2) n = 2;
#define NSK_MS_K for (int k = 0; k < (N == 2 ? 2 : n); k++)
    NSK_MS_K P[k] = 0.0;
    for (int i = 0; i < d; i++) {
        const long long mo = a.msg_off[edges[i]];
        NSK_MS_K m.V[mo + k] = P[k];
        NSK_MS_K P[k] = P[k] + m.F[mo + k];
    }
    double mx = P[0];
    for (int k = 1; k < (N == 2 ? 2 : n); k++) mx = ms_max(mx, P[k]);
    NSK_MS_K mm[k] = P[k] - mx;
    NSK_MS_K S[k] = 0.0;
    for (int i = d - 1; i >= 0; i--) {
        const long long mo = a.msg_off[edges[i]];
        double *T = N ? Tl : m.V + mo;
        NSK_MS_K T[k] = m.V[mo + k] + S[k];
        double mt = T[0];
        for (int k = 1; k < (N == 2 ? 2 : n); k++) mt = ms_max(mt, T[k]);
        NSK_MS_K m.V[mo + k] = T[k] - mt;
        NSK_MS_K S[k] = S[k] + m.F[mo + k];
    }
#undef NSK_MS_K
}

// the same arithmetic for a binary variable of at most NSK_BP_VAR_REG edges (bp_var_lane_reg): every message is read
// once and written once, the loads of all edges in flight together
__device__ __forceinline__ void ms_var_lane_reg(const MsArgs &m, const int32_t *edges, int d, double *mm) {
    const BpArgs &a = m.b;
    long long mo[NSK_BP_VAR_REG];
    double f0[NSK_BP_VAR_REG], f1[NSK_BP_VAR_REG], p0[NSK_BP_VAR_REG], p1[NSK_BP_VAR_REG];
#pragma unroll
    for (int i = 0; i < NSK_BP_VAR_REG; i++) mo[i] = i < d ? a.msg_off[edges[i]] : 0;
#pragma unroll
    for (int i = 0; i < NSK_BP_VAR_REG; i++)
        if (i < d) { f0[i] = m.F[mo[i]]; f1[i] = m.F[mo[i] + 1]; }
    double P0 = 0.0, P1 = 0.0;
#pragma unroll
    for (int i = 0; i < NSK_BP_VAR_REG; i++)
        if (i < d) {
            p0[i] = P0; p1[i] = P1;
            P0 = P0 + f0[i]; P1 = P1 + f1[i];
        }
    const double mx = ms_max(P0, P1);
    mm[0] = P0 - mx; mm[1] = P1 - mx;
    double S0 = 0.0, S1 = 0.0;
#pragma unroll
    for (int i = NSK_BP_VAR_REG - 1; i >= 0; i--)
        if (i < d) {
            const double T0 = p0[i] + S0, T1 = p1[i] + S1, mt = ms_max(T0, T1);
            m.V[mo[i]] = T0 - mt; m.V[mo[i] + 1] = T1 - mt;
            S0 = S0 + f0[i]; S1 = S1 + f1[i];
        }
}

// iteration t over the entries [lo, hi) of v_list, the binary variables first (k_bp_var)
template <bool BIN>
__global__ __launch_bounds__(NSK_BP_VAR_BLOCK) void k_ms_var(const MsArgs m, int lo, int hi, int t, double tol, const unsigned long long *residual) {
    if (ms_done(residual, t, tol)) return;
    const BpArgs &a = m.b;
    for (int i = lo + (int)(blockIdx.x * NSK_BP_VAR_BLOCK + threadIdx.x); i < hi; i += (int)(gridDim.x * NSK_BP_VAR_BLOCK)) {
        const int id = a.v_list[i];
        const int e0 = a.v_eoff[i], d = a.v_eoff[i + 1] - e0;
        const long long b0 = a.b_off[id];
        const int n = (int)(a.b_off[id + 1] - b0);
        if (BIN && d <= NSK_BP_VAR_REG) ms_var_lane_reg(m, a.v_edges + e0, d, m.mm + b0);
        else if (BIN) ms_var_lane<2>(m, 2, a.v_edges + e0, d, m.mm + b0, nullptr);
        else if (n <= NSK_ZLOCAL) ms_var_lane<NSK_ZLOCAL>(m, n, a.v_edges + e0, d, m.mm + b0, nullptr);
        else ms_var_lane<0>(m, n, a.v_edges + e0, d, m.mm + b0, a.wk + b0);
    }
}

// ---- decode: per free variable with an edge the comparison of diagnostics.icm_choice from best = 0 -- the smallest k
// among several maxima, a NaN never wins -- written into the chain row by internal id; a tie is a largest max-marginal
// that more than one k attains, a wave's count leaving as one atomic.  Clamped variables and free ones in no table keep
// their values: no lane visits them.
template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_ms_decode(const MsArgs m, VT *val, unsigned long long *ties) {
    const BpArgs &a = m.b;
    for (int base = (int)(blockIdx.x * NSK_BLOCK + (threadIdx.x & ~63u)); base < a.nvlist; base += (int)(gridDim.x * NSK_BLOCK)) {
        const int i = base + (int)(threadIdx.x & 63);
        bool tie = false;
        if (i < a.nvlist) {
            const int id = a.v_list[i];
            const long long b0 = a.b_off[id];
            const int n = (int)(a.b_off[id + 1] - b0);
            int best = 0, hits = 1;
            double pb = m.mm[b0];
            for (int k = 1; k < n; k++) {
                const double pk = m.mm[b0 + k];
                if (pk > pb) { best = k; pb = pk; hits = 1; }
                else if (pk == pb) hits++;
            }
            val[id] = (VT)best;
            tie = hits > 1;
        }
        const unsigned long long mask = __ballot(tie);
        if ((threadIdx.x & 63) == 0 && mask != 0ull)
            (void)__hip_atomic_fetch_add(ties, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace nsk
