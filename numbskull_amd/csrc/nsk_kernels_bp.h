// nsk_kernels_bp.h -- loopy belief propagation (sum-product, flooding schedule) on the factor graph: the kernels of
// nsk_bp_setup / nsk_bp_run / nsk_bp_download (nsk_bp.hip; the rule is stated in include/numbskull_amd.h and restated in
// numpy by numbskull_amd.diagnostics.bp_iterate -- device and numpy agree bit for bit, so every sum and product below is
// taken in the order written there and nothing is reassociated; the library is compiled with -ffp-contract=off).
//
//   k_bp_tables   one lane per (factor, table index): feat_f(a) = eval_factor, the free members at the digits of a, and
//                 theta_f(a) = w * feat_f(a)
//   k_bp_psi      one lane per factor: psi_f(a) = nsk_exp(theta_f(a) - max_a theta_f)
//   k_bp_factor   one lane per directed edge (f, j): the message factor -> variable, damping, the residual
//   k_bp_var      one lane per free variable with an edge: the messages variable -> factor and the belief
//   k_bp_fbelief  one lane per factor: the factor beliefs, on demand
//   k_bp_refresh  one lane per table entry: theta = w * feat from the weights as they stand (nsk_bp_refresh)
//   k_bp_fnorm    one lane per factor: Z_f, the a-ordered sum of k_bp_fbelief (nsk_bp_moments)
//   k_bp_moments  one lane per table entry: the expected per-weight statistics under the factor beliefs, int64 fixed
//                 point, one atomic per run of equal weight slot a wave holds
//   k_bp_*2       refresh, psi, reset, factor, var, fnorm and moments for two set-ups in one launch, blockIdx.y naming the
//                 set-up (nsk_bp_latent_steps): the bodies are shared with the kernels above
//
// A vector over a variable's values (a message, a belief) lives in registers for binary variables, in a lane-private
// array of NSK_ZLOCAL doubles for cardinalities up to NSK_ZLOCAL (runtime-indexed; the compiler keeps it in registers
// with indexed moves, scratch 0 in every kernel here) and in global memory beyond (k_bp_factor recomputes instead: it
// needs no vector at all there).  The digits of a table index are decoded arithmetically, axis 0 the most significant.
#pragma once

#include "nsk_device.h"
#include "nsk_kernels_energy.h"     // energy_factor
#include "nsk_kernels_gibbs.h"      // NSK_BLOCK

namespace nsk {

#define NSK_BP_MAX_BLOCKS 2048      // the lanes of a larger launch loop (8 blocks per CU)
#define NSK_BP_VAR_BLOCK 128        // lanes of a block of the variable phase (a lane walks a variable's whole edge list)

// what the kernels read of a set-up (nsk_internal.h NskBp)
struct BpArgs {
    const uint4 *f_rec;
    const int2 *mrec;               // per factor its own member records {local slot, dense_equal_to} at pm_off[f]
    const long long *pm_off;        // [F + 1]
    const int32_t *slot_off;        // [F + 1] the distinct members of a factor ...
    const int2 *slot_rec;           // ... {internal id, free ? 1 : 0}, in order of first occurrence
    const long long *tab_off;       // [F + 1] table entries
    const int32_t *edge_off;        // [F + 1] directed edges, factor-major
    const int32_t *e_fac;           // [E]
    const long long *msg_off;       // [E + 1] doubles of an edge in f2v / v2f
    const int32_t *v_list, *v_eoff, *v_edges;      // free variables with an edge: internal id, CSR into v_edges (ascending)
    const long long *b_off;         // [nid + 1] doubles of a variable in belief (and wk)
    const uint8_t *v_state;         // [nid] 0: no variable, 1: clamped, 2: free
    const int32_t *v_card;
    const double *w, *logtab;
    double *theta, *psi, *f2v, *v2f, *belief, *wk;
    double *feat;                   // [ntable] eval_factor without the weight: theta = w * feat, one rounded product
    long long nfactor, ntable, nid;
    int32_t nedge, nvlist;
};

// theta: the lane-private value and cardinality arrays are indexed by local slot, and eval_factor reads them through a
// view whose member records name local slots (built once per call: scratch is acceptable here)
template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_bp_tables(const BpArgs a, const VT *val) {
    DevGraph<int32_t> g = {};
    g.logtab = a.logtab;
    g.head_by_vid = 1;              // (local slots: a head is read at its member record; the literal lookup is refused)
    for (long long idx = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; idx < a.ntable; idx += (long long)gridDim.x * NSK_BLOCK) {
        long long lo = 0, hi = a.nfactor;           // tab_off[lo] <= idx < tab_off[hi]; every factor has an entry
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if (a.tab_off[mid] <= idx) lo = mid; else hi = mid;
        }
        const long long f = lo;
        const int ai = (int)(idx - a.tab_off[f]);
        int st = (int)(a.tab_off[f + 1] - a.tab_off[f]);
        int32_t lv[NSK_BP_MAX_MEMBERS], lc[NSK_BP_MAX_MEMBERS];
        const int s0 = a.slot_off[f];
        int ns = a.slot_off[f + 1] - s0;
        ns = ns > NSK_BP_MAX_MEMBERS ? NSK_BP_MAX_MEMBERS : ns;
        for (int s = 0; s < ns; s++) {
            const int2 r = a.slot_rec[s0 + s];
            const int c = a.v_card[r.x];
            lc[s] = c;
            if (r.y) { st /= c; lv[s] = (ai / st) % c; }
            else lv[s] = (int32_t)val[r.x];
        }
        g.v_card = lc;
        uint4 rec = a.f_rec[f];
        const int2 *mb = a.mrec + a.pm_off[f] - (int)rec.y;        // mb[ftv_offset + i] = the factor's own record i
        g.m_rec = mb;
        const double e = energy_factor(g, rec, mb, (const int32_t *)lv);
        a.feat[idx] = e;
        a.theta[idx] = a.w[rec.z] * e;
    }
}

// The bodies of the kernels that nsk_bp_latent_steps launches for two set-ups at once take the set-up and the block's
// index and count: the single kernels pass blockIdx.x and gridDim.x, the pair kernels at the end of the file the same
// with the set-up blockIdx.y names.
__device__ __forceinline__ void bp_psi_body(const BpArgs &a, unsigned int bid, unsigned int nblk) {
    for (long long f = (long long)bid * NSK_BLOCK + threadIdx.x; f < a.nfactor; f += (long long)nblk * NSK_BLOCK) {
        const long long t0 = a.tab_off[f], t1 = a.tab_off[f + 1];
        double mx = a.theta[t0];
        for (long long i = t0 + 1; i < t1; i++) {
            const double th = a.theta[i];
            if (th > mx) mx = th;
        }
        for (long long i = t0; i < t1; i++) a.psi[i] = nsk_exp(a.theta[i] - mx);
    }
}
static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_psi(const BpArgs a) { bp_psi_body(a, blockIdx.x, gridDim.x); }

// every message entry 1 / card
__device__ __forceinline__ void bp_reset_body(const BpArgs &a, unsigned int bid, unsigned int nblk) {
    for (int e = (int)(bid * NSK_BLOCK + threadIdx.x); e < a.nedge; e += (int)(nblk * NSK_BLOCK)) {
        const long long m0 = a.msg_off[e], m1 = a.msg_off[e + 1];
        const double u = 1.0 / (double)(m1 - m0);
        for (long long i = m0; i < m1; i++) { a.f2v[i] = u; a.v2f[i] = u; }
    }
}
static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_reset(const BpArgs a) { bp_reset_body(a, blockIdx.x, gridDim.x); }

// the beliefs the iterations do not write: a clamped variable's indicator, a free variable's uniform law
template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_bp_belief0(const BpArgs a, const VT *val) {
    for (long long id = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; id < a.nid; id += (long long)gridDim.x * NSK_BLOCK) {
        const int st = a.v_state[id];
        if (!st) continue;
        const long long b0 = a.b_off[id], b1 = a.b_off[id + 1];
        const double u = 1.0 / (double)(b1 - b0);
        const long long x = (long long)(int)val[id];
        for (long long i = b0; i < b1; i++) a.belief[i] = st == 2 ? u : (i - b0 == x ? 1.0 : 0.0);
    }
}

// sum over the table entries with digit j == k, ascending, of psi times the other axes' incoming messages
__device__ __forceinline__ double bp_edge_sum(const BpArgs &a, long long t0, int T, int e0, int A, int j, int cj, int sj, int k) {
    double m = 0.0;
    const int nhi = T / (cj * sj);
    for (int hi = 0; hi < nhi; hi++)
        for (int lo = 0; lo < sj; lo++) {
            const int ai = (hi * cj + k) * sj + lo;
            double x = a.psi[t0 + ai];
            int st = T;
            for (int i = 0; i < A; i++) {
                const long long mo = a.msg_off[e0 + i];
                const int ci = (int)(a.msg_off[e0 + i + 1] - mo);
                st /= ci;
                if (i != j) x = x * a.v2f[mo + (ai / st) % ci];
            }
            m = m + x;
        }
    return m;
}

__device__ __forceinline__ double bp_store(double *slot, double nw, double lam, double oml) {
    const double old = *slot;
    if (lam > 0.0) nw = oml * nw + lam * old;
    *slot = nw;
    const double d = fabs(nw - old);
    return d == d ? d : __longlong_as_double(0x7ff0000000000000LL);
}

// iteration t, factor phase.  residual: the bit patterns of non-negative doubles, the order of integer maxima is free.
// (Every lane of the block comes here and, past the exit, to the barrier: a block without an edge of its own loops no
// time.  residual is the set-up's own row.)
__device__ __forceinline__ void bp_factor_body(const BpArgs &a, unsigned int bid, unsigned int nblk, int t, double tol, double lam, double oml,
                                               unsigned long long *residual) {
    __shared__ double lds[NSK_BLOCK / 64];
    if (t > 0 && __longlong_as_double((long long)residual[t - 1]) <= tol) return;      // block-uniform, before the barrier
    double res = 0.0;
    for (int e = (int)(bid * NSK_BLOCK + threadIdx.x); e < a.nedge; e += (int)(nblk * NSK_BLOCK)) {
        const int f = a.e_fac[e];
        const int e0 = a.edge_off[f], A = a.edge_off[f + 1] - e0, j = e - e0;
        const long long t0 = a.tab_off[f];
        const int T = (int)(a.tab_off[f + 1] - t0);
        const long long mo = a.msg_off[e];
        const int cj = (int)(a.msg_off[e + 1] - mo);
        int sj = 1;
        for (int i = A - 1; i > j; i--) sj *= (int)(a.msg_off[e0 + i + 1] - a.msg_off[e0 + i]);
        if (cj == 2) {
            const double m0 = bp_edge_sum(a, t0, T, e0, A, j, 2, sj, 0), m1 = bp_edge_sum(a, t0, T, e0, A, j, 2, sj, 1);
            const double Z = m0 + m1;
            res = fmax(res, bp_store(a.f2v + mo, m0 / Z, lam, oml));
            res = fmax(res, bp_store(a.f2v + mo + 1, m1 / Z, lam, oml));
        } else if (cj <= NSK_ZLOCAL) {
            double m[NSK_ZLOCAL];
            double Z = 0.0;
            for (int k = 0; k < cj; k++) {
                m[k] = bp_edge_sum(a, t0, T, e0, A, j, cj, sj, k);
                Z = k == 0 ? m[0] : Z + m[k];
            }
            for (int k = 0; k < cj; k++) res = fmax(res, bp_store(a.f2v + mo + k, m[k] / Z, lam, oml));
        } else {        // large domains: two passes, the second recomputes the identical sums
            double Z = 0.0;
            for (int k = 0; k < cj; k++) {
                const double mk = bp_edge_sum(a, t0, T, e0, A, j, cj, sj, k);
                Z = k == 0 ? mk : Z + mk;
            }
            for (int k = 0; k < cj; k++) res = fmax(res, bp_store(a.f2v + mo + k, bp_edge_sum(a, t0, T, e0, A, j, cj, sj, k) / Z, lam, oml));
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) res = fmax(res, __shfl_xor(res, off, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = res;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < NSK_BLOCK / 64; k++) res = fmax(res, lds[k]);
        if (res > 0.0) atomicMax(residual + t, (unsigned long long)__double_as_longlong(res));
    }
}
static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_factor(const BpArgs a, int t, double tol, double lam, double oml,
                                                               unsigned long long *residual) {
    bp_factor_body(a, blockIdx.x, gridDim.x, t, tol, lam, oml, residual);
}

// while the largest entry is > 0 and < 2^-512: every entry times 2^512 (exact)
template <int N>
__device__ __forceinline__ void bp_rescale(double *v, int n) {
    const double tiny = __longlong_as_double((long long)(1023 - 512) << 52), big = __longlong_as_double((long long)(1023 + 512) << 52);
    for (;;) {
        double mx = v[0];
        for (int k = 1; k < (N ? N : n); k++) if (v[k] > mx) mx = v[k];
        if (!(mx > 0.0 && mx < tiny)) return;
        for (int k = 0; k < (N ? N : n); k++) v[k] = v[k] * big;
    }
}

// one variable's phase.  N == 2: a binary variable, vectors in registers; N == NSK_ZLOCAL: lane-private arrays of n <= N
// entries; N == 0: the product lives in the variable's belief slot, the running suffix product in its wk slot and the
// vector under way in the v2f slot itself.
template <int N>
__device__ __forceinline__ void bp_var_lane(const BpArgs &a, int n, const int32_t *edges, int d, double *bel, double *wk) {
    double Pl[N ? N : 1], Sl[N ? N : 1], Tl[N ? N : 1];
    double *P = N ? Pl : bel, *S = N ? Sl : wk;
    if (N == 2) n = 2;
#define NSK_BP_K for (int k = 0; k < (N == 2 ? 2 : n); k++)
    NSK_BP_K P[k] = 1.0;
    for (int i = 0; i < d; i++) {
        const long long mo = a.msg_off[edges[i]];
        NSK_BP_K a.v2f[mo + k] = P[k];
        NSK_BP_K P[k] = P[k] * a.f2v[mo + k];
        bp_rescale<N == 2 ? 2 : 0>(P, n);
    }
    double Z = P[0];
    for (int k = 1; k < (N == 2 ? 2 : n); k++) Z = Z + P[k];
    NSK_BP_K bel[k] = P[k] / Z;
    NSK_BP_K S[k] = 1.0;
    for (int i = d - 1; i >= 0; i--) {
        const long long mo = a.msg_off[edges[i]];
        double *T = N ? Tl : a.v2f + mo;
        NSK_BP_K T[k] = a.v2f[mo + k] * S[k];
        bp_rescale<N == 2 ? 2 : 0>(T, n);
        double Zt = T[0];
        for (int k = 1; k < (N == 2 ? 2 : n); k++) Zt = Zt + T[k];
        NSK_BP_K a.v2f[mo + k] = T[k] / Zt;
        NSK_BP_K S[k] = S[k] * a.f2v[mo + k];
        bp_rescale<N == 2 ? 2 : 0>(S, n);
    }
#undef NSK_BP_K
}

// The same arithmetic for a binary variable of at most NSK_BP_VAR_REG edges, its incoming messages and prefix products
// held in registers: every message is read once and written once (the walk above stores the prefixes into v2f and reads
// them back, and reads f2v in both passes), and the loads of all edges are in flight together.
#define NSK_BP_VAR_REG 6
__device__ __forceinline__ void bp_var_lane_reg(const BpArgs &a, const int32_t *edges, int d, double *bel) {
    long long mo[NSK_BP_VAR_REG];
    double f0[NSK_BP_VAR_REG], f1[NSK_BP_VAR_REG], p0[NSK_BP_VAR_REG], p1[NSK_BP_VAR_REG];
#pragma unroll
    for (int i = 0; i < NSK_BP_VAR_REG; i++) mo[i] = i < d ? a.msg_off[edges[i]] : 0;
#pragma unroll
    for (int i = 0; i < NSK_BP_VAR_REG; i++)
        if (i < d) { f0[i] = a.f2v[mo[i]]; f1[i] = a.f2v[mo[i] + 1]; }
    double P[2] = {1.0, 1.0};
#pragma unroll
    for (int i = 0; i < NSK_BP_VAR_REG; i++)
        if (i < d) {
            p0[i] = P[0]; p1[i] = P[1];
            P[0] = P[0] * f0[i]; P[1] = P[1] * f1[i];
            bp_rescale<2>(P, 2);
        }
    const double Z = P[0] + P[1];
    bel[0] = P[0] / Z; bel[1] = P[1] / Z;
    double S[2] = {1.0, 1.0};
#pragma unroll
    for (int i = NSK_BP_VAR_REG - 1; i >= 0; i--)
        if (i < d) {
            double T[2] = {p0[i] * S[0], p1[i] * S[1]};
            bp_rescale<2>(T, 2);
            const double Zt = T[0] + T[1];
            a.v2f[mo[i]] = T[0] / Zt; a.v2f[mo[i] + 1] = T[1] / Zt;
            S[0] = S[0] * f0[i]; S[1] = S[1] * f1[i];
            bp_rescale<2>(S, 2);
        }
}

// iteration t, variable phase over the entries [lo, hi) of v_list.  The list holds the binary variables first: BIN serves
// them from a handful of registers, the other launch the rest (the lane-private vectors of the middle cardinalities cost
// it its occupancy).
template <bool BIN>
__device__ __forceinline__ void bp_var_body(const BpArgs &a, unsigned int bid, unsigned int nblk, int lo, int hi, int t, double tol,
                                            const unsigned long long *residual) {
    if (t > 0 && __longlong_as_double((long long)residual[t - 1]) <= tol) return;
    for (int i = lo + (int)(bid * NSK_BP_VAR_BLOCK + threadIdx.x); i < hi; i += (int)(nblk * NSK_BP_VAR_BLOCK)) {
        const int id = a.v_list[i];
        const int e0 = a.v_eoff[i], d = a.v_eoff[i + 1] - e0;
        const long long b0 = a.b_off[id];
        const int n = (int)(a.b_off[id + 1] - b0);
        if (BIN && d <= NSK_BP_VAR_REG) bp_var_lane_reg(a, a.v_edges + e0, d, a.belief + b0);
        else if (BIN) bp_var_lane<2>(a, 2, a.v_edges + e0, d, a.belief + b0, nullptr);
        else if (n <= NSK_ZLOCAL) bp_var_lane<NSK_ZLOCAL>(a, n, a.v_edges + e0, d, a.belief + b0, nullptr);
        else bp_var_lane<0>(a, n, a.v_edges + e0, d, a.belief + b0, a.wk + b0);
    }
}
template <bool BIN>
__global__ __launch_bounds__(NSK_BP_VAR_BLOCK) void k_bp_var(const BpArgs a, int lo, int hi, int t, double tol, const unsigned long long *residual) {
    bp_var_body<BIN>(a, blockIdx.x, gridDim.x, lo, hi, t, tol, residual);
}

// b_f(a) = psi_f(a) * the incoming messages at the digits of a, divided by their a-ordered sum
static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_fbelief(const BpArgs a, double *fb) {
    for (long long f = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; f < a.nfactor; f += (long long)gridDim.x * NSK_BLOCK) {
        const long long t0 = a.tab_off[f];
        const int T = (int)(a.tab_off[f + 1] - t0);
        const int e0 = a.edge_off[f], A = a.edge_off[f + 1] - e0;
        double Z = 0.0;
        for (int ai = 0; ai < T; ai++) {
            double x = a.psi[t0 + ai];
            int st = T;
            for (int i = 0; i < A; i++) {
                const long long mo = a.msg_off[e0 + i];
                const int ci = (int)(a.msg_off[e0 + i + 1] - mo);
                st /= ci;
                x = x * a.v2f[mo + (ai / st) % ci];
            }
            fb[t0 + ai] = x;
            Z = ai == 0 ? x : Z + x;
        }
        for (int ai = 0; ai < T; ai++) fb[t0 + ai] = fb[t0 + ai] / Z;
    }
}

// ---- learning by belief propagation (nsk_bp_refresh, nsk_bp_moments, nsk_bp_learn_steps) ----
// the factor of a table entry, as k_bp_tables finds it: tab_off[f] <= idx < tab_off[f + 1]; every factor has an entry
__device__ __forceinline__ long long bp_factor_of(const BpArgs &a, long long idx) {
    long long lo = 0, hi = a.nfactor;
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (a.tab_off[mid] <= idx) lo = mid; else hi = mid;
    }
    return lo;
}

// x(a) of k_bp_fbelief: psi times the incoming messages at the digits of a, the axes ascending
__device__ __forceinline__ double bp_entry_x(const BpArgs &a, long long t0, int T, int e0, int A, int ai) {
    double x = a.psi[t0 + ai];
    int st = T;
    for (int i = 0; i < A; i++) {
        const long long mo = a.msg_off[e0 + i];
        const int ci = (int)(a.msg_off[e0 + i + 1] - mo);
        st /= ci;
        x = x * a.v2f[mo + (ai / st) % ci];
    }
    return x;
}

// theta from the device weight table as it stands: one rounded product per entry, the set-up's own (k_bp_psi follows)
__device__ __forceinline__ void bp_refresh_body(const BpArgs &a, unsigned int bid, unsigned int nblk) {
    for (long long idx = (long long)bid * NSK_BLOCK + threadIdx.x; idx < a.ntable; idx += (long long)nblk * NSK_BLOCK)
        a.theta[idx] = a.w[a.f_rec[bp_factor_of(a, idx)].z] * a.feat[idx];
}
static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_refresh(const BpArgs a) { bp_refresh_body(a, blockIdx.x, gridDim.x); }

// Z_f, the a-ordered sum of k_bp_fbelief, one lane per factor.  A factor whose Z_f is not a finite positive number takes
// no part in the moments: it is counted here, a wave's count leaving as one atomic.
__device__ __forceinline__ void bp_fnorm_body(const BpArgs &a, unsigned int bid, unsigned int nblk, double *zf, unsigned long long *skipped) {
    for (long long base = (long long)bid * NSK_BLOCK + (threadIdx.x & ~63u); base < a.nfactor; base += (long long)nblk * NSK_BLOCK) {
        const long long f = base + (threadIdx.x & 63);
        bool skip = false;
        if (f < a.nfactor) {
            const long long t0 = a.tab_off[f];
            const int T = (int)(a.tab_off[f + 1] - t0);
            const int e0 = a.edge_off[f], A = a.edge_off[f + 1] - e0;
            double Z = 0.0;
            for (int ai = 0; ai < T; ai++) {
                const double x = bp_entry_x(a, t0, T, e0, A, ai);
                Z = ai == 0 ? x : Z + x;
            }
            zf[f] = Z;
            skip = !(Z > 0.0 && Z < __longlong_as_double(0x7ff0000000000000LL));
        }
        const unsigned long long m = __ballot(skip);
        if ((threadIdx.x & 63) == 0 && m != 0ull)
            (void)__hip_atomic_fetch_add(skipped, (unsigned long long)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_fnorm(const BpArgs a, double *zf, unsigned long long *skipped) {
    bp_fnorm_body(a, blockIdx.x, gridDim.x, zf, skipped);
}

__device__ __forceinline__ void bp_moments_add(unsigned long long *M, int slot, long long x) {
    if (slot >= 0 && x != 0) (void)__hip_atomic_fetch_add(M + slot, (unsigned long long)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The Bethe moments, one lane per table entry: q = rint(((x(a) / Z_f) * feat_f(a)) * 2^32) into M[weight slot of f].  A
// wave holds 64 consecutive entries a trip; consecutive entries belong to one factor and hence one slot, so the lanes
// form runs of equal slot.  A segmented prefix sum leaves every run's total in its last lane, which issues the run's one
// atomic -- but for the run that ends the wave: it is carried in a register (wave-uniform) into the next trip and joins
// that trip's first run when the slots agree, as k_moments_piece carries its pieces.  What a block's waves carry at the
// end meets in LDS and equal slots leave as one atomic.  Integers: no order changes a bit.
// (Every lane comes to the barrier: a wave without an entry of its own carries nothing, slot -1.)
__device__ __forceinline__ void bp_moments_body(const BpArgs &a, unsigned int bid, unsigned int nblk, const double *zf, unsigned long long *M) {
    __shared__ long long lds_run[NSK_BLOCK / 64];
    __shared__ int lds_slot[NSK_BLOCK / 64];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    int cslot = -1;                 // the slot of the carried sum (-1: none)
    long long carry = 0;
    for (long long base = (long long)bid * NSK_BLOCK + wave * 64; base < a.ntable; base += (long long)nblk * NSK_BLOCK) {
        const long long idx = base + lane;
        int slot = -1;
        long long acc = 0;
        if (idx < a.ntable) {
            const long long f = bp_factor_of(a, idx);
            const long long t0 = a.tab_off[f];
            const int T = (int)(a.tab_off[f + 1] - t0);
            const int e0 = a.edge_off[f];
            slot = (int)a.f_rec[f].z;
            const double Z = zf[f];
            if (Z > 0.0 && Z < __longlong_as_double(0x7ff0000000000000LL)) {
                const double b = bp_entry_x(a, t0, T, e0, a.edge_off[f + 1] - e0, (int)(idx - t0)) / Z;
                const double p = b * a.feat[idx];
                acc = __double2ll_rn(p * NSK_GRAD_SCALE);
            }
        }
        const int prev = __shfl_up(slot, 1, 64), next = __shfl_down(slot, 1, 64);
        const bool head = lane == 0 || prev != slot, tail = lane == 63 || next != slot;
        const unsigned long long heads = __ballot(head);
        const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));      // the first lane of this lane's run
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const long long o = __shfl_up(acc, off, 64);
            if (lane - off >= start) acc += o;
        }
        const int first = __shfl(slot, 0, 64);
        if (first != cslot) {
            if (lane == 0) bp_moments_add(M, cslot, carry);
            carry = 0;
        }
        if (start == 0) acc += carry;               // (the carry belongs to the first run now, or is 0)
        if (tail && lane != 63) bp_moments_add(M, slot, acc);
        cslot = __shfl(slot, 63, 64);
        carry = __shfl(acc, 63, 64);
    }
    if (lane == 0) { lds_slot[wave] = cslot; lds_run[wave] = carry; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NSK_BLOCK / 64; k++) {
            const int s = lds_slot[k];
            if (s < 0) continue;
            long long x = lds_run[k];
            for (int j = k + 1; j < NSK_BLOCK / 64; j++)
                if (lds_slot[j] == s) { x += lds_run[j]; lds_slot[j] = -1; }
            bp_moments_add(M, s, x);
        }
    }
}
static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_moments(const BpArgs a, const double *zf, unsigned long long *M) {
    bp_moments_body(a, blockIdx.x, gridDim.x, zf, M);
}

// ---- two set-ups in the same launches (nsk_bp_latent_steps) ----
// blockIdx.y names the set-up (0: evidence clamped, 1: free), gridDim.x is what the larger of the two needs; the bodies
// are those of the single kernels above, so a set-up computes here what it computes alone, bit for bit.  A block whose
// set-up has fewer items than the grid covers loops no time and still reaches every barrier; each early exit reads its
// own set-up's row of residuals and is uniform over the block.
struct BpPair {
    BpArgs a[2];
    unsigned long long *res[2];     // the step's row of residuals
    double *zf[2];                  // [nfactor] each
    unsigned long long *M[2];       // [nweight] each: the clamped set-up's sums are k_pcd_update's Mc
    unsigned long long *skipped[2];
    int nvbin[2];                   // NskBp::nvbin: v_list holds the binary variables first
};

static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_refresh2(const BpPair p) { bp_refresh_body(p.a[blockIdx.y], blockIdx.x, gridDim.x); }
static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_psi2(const BpPair p) { bp_psi_body(p.a[blockIdx.y], blockIdx.x, gridDim.x); }
static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_reset2(const BpPair p) { bp_reset_body(p.a[blockIdx.y], blockIdx.x, gridDim.x); }
static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_factor2(const BpPair p, int t, double tol, double lam, double oml) {
    bp_factor_body(p.a[blockIdx.y], blockIdx.x, gridDim.x, t, tol, lam, oml, p.res[blockIdx.y]);
}
template <bool BIN>
__global__ __launch_bounds__(NSK_BP_VAR_BLOCK) void k_bp_var2(const BpPair p, int t, double tol) {
    const BpArgs &a = p.a[blockIdx.y];
    const int nbin = p.nvbin[blockIdx.y];
    bp_var_body<BIN>(a, blockIdx.x, gridDim.x, BIN ? 0 : nbin, BIN ? nbin : a.nvlist, t, tol, p.res[blockIdx.y]);
}
static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_fnorm2(const BpPair p) {
    bp_fnorm_body(p.a[blockIdx.y], blockIdx.x, gridDim.x, p.zf[blockIdx.y], p.skipped[blockIdx.y]);
}
static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_moments2(const BpPair p) {
    bp_moments_body(p.a[blockIdx.y], blockIdx.x, gridDim.x, p.zf[blockIdx.y], p.M[blockIdx.y]);
}

}  // namespace nsk
