// nsk_kernels_bpres.h -- sum-product belief propagation under a residual schedule (nsk_bp_residual_run, nsk_bp_residual.hip;
// the rule is stated in include/numbskull_amd.h and restated in numpy by numbskull_amd.diagnostics.rbp_iterate, bit for
// bit).  The per-item arithmetic is that of nsk_kernels_bp.h -- bp_edge_sum, bp_store's damping, the variable walks --
// but the lanes run over WORKLISTS instead of index ranges, so a round costs what moved, not what exists:
//
//   k_bpres_cand    one lane per entry of the dirty-edge queue D_t: the candidate message (the factor phase without damping)
//                   into cand, the change a commit would make into r[e]
//   k_bpres_max     dense scan of r, 8 bytes an edge: residual[t], an integer maximum of bit patterns
//   k_bpres_commit  dense scan of r: the edges at or above frac * residual[t] store their damped candidate into f2v and
//                   enter their variable into the touched queue V_t (binary variables and the rest have one each)
//   k_bpres_var     one lane per entry of V_t: the variable phase of k_bp_var (the same three homes of a vector, the same
//                   register walk) with the hook that tells which v2f vectors changed in any bit; for each of those the
//                   factor's other edges enter D_{t+1}
//   k_bpres_vpos    once per set-up: the position in v_list of every edge's variable
//
// Queues.  A queue is an int32 array as long as the index range it draws from and a counter PER ROUND (nD[t], nV[2t + b]),
// zeroed once per call: no launch resets anything.  An item enters at most once a round: the first lane to turn its flag
// byte from 0 to 1 pushes it (bpres_claim), the consumer turns it back.  Pushes are aggregated per wave (bpres_push): a
// ballot of the pushing lanes, ONE atomic add of their number by the lowest of them, slots by the population count of
// the lanes below -- so every loop that pushes is written in wave-uniform steps (`for (..; __ballot(lane has a step);
// ..)`) and all 64 lanes reach every ballot.  The order of a queue is therefore arbitrary; no result depends on it,
// because an item reads nothing that another item of the same launch writes (a candidate reads psi, v2f and its own
// f2v slot and writes its own cand and r; a variable reads the f2v slots of its own edges and writes their v2f slots
// and its belief), and what the items share -- counters, the maximum -- are integers.
// D_t is consumed by k_bpres_cand before k_bpres_var writes D_{t+1}: one buffer per queue.
// Every kernel of round t >= 1 returns at once when residual[t - 1] <= tol, as the kernels of nsk_bp_run do.
#pragma once

#include "nsk_kernels_bp.h"

namespace nsk {

// what the kernels read of a set-up's residual state (nsk_internal.h NskBp rs_*) and of the call
struct ResArgs {
    BpArgs b;
    double *cand;                   // [nmsg] the candidate message of every edge, msg_off's layout
    double *r;                      // [E] the largest entry of the change a commit of the edge would make
    double *pre;                    // [nmsg] the prefix products of the walks through memory (null: no variable takes one)
    uint8_t *chg;                   // [E] the walks' note "this edge's v2f changed" (null with pre)
    uint8_t *dflag, *vflag;         // [E], [nvlist], each rounded up to a multiple of 4: the item is in its queue
    int32_t *dq, *vq;               // [E] dirty edges; [nvlist] touched v_list positions, the binary ones in [0, nvbin)
    int32_t *e_vpos;                // [E] the v_list position of an edge's variable
    unsigned long long *res, *upd;  // [S] the call's rows: residual bit patterns, edges selected
    unsigned long long *nD, *nV;    // [S + 1] entries of D_t; [2 S] entries of V_t, binary then rest
    int32_t nvbin;
};

__device__ __forceinline__ bool bpres_done(const ResArgs &q, int t, double tol) {
    return t > 0 && __longlong_as_double((long long)q.res[t - 1]) <= tol;
}

// the flag byte's exchange with 1, as an atomic OR on the word that holds it: true for the one lane that found it 0
__device__ __forceinline__ bool bpres_claim(uint8_t *flags, int i) {
    const unsigned int bit = 1u << ((i & 3) * 8);
    return (atomicOr((unsigned int *)flags + (i >> 2), bit) & bit) == 0u;
}

// Every lane of the wave comes here; the lanes with p take consecutive slots of q behind one atomic of the lowest of them.
// (An item enters a queue once a round, so a round's count stays within cap: the bound is a guard only.)
__device__ __forceinline__ void bpres_push(int32_t *q, unsigned long long *cnt, bool p, int item, int cap) {
    const unsigned long long m = __ballot(p);
    if (m == 0ull) return;          // wave-uniform
    const int lane = (int)(threadIdx.x & 63), lead = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == lead) base = __hip_atomic_fetch_add(cnt, (unsigned long long)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, lead, 64);
    const unsigned long long slot = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
    if (p && slot < (unsigned long long)cap) q[slot] = item;
}

// Every lane of the wave comes here; a lane with `want` enters the other edges of e's factor into the next dirty queue,
// one edge a wave-uniform step.
__device__ __forceinline__ void bpres_push_others(const ResArgs &q, bool want, int e, unsigned long long *cnt) {
    int e0 = 0, A = 0;
    if (want) {
        const int f = q.b.e_fac[e];
        e0 = q.b.edge_off[f];
        A = q.b.edge_off[f + 1] - e0;
    }
    for (int i = 0; __ballot(i < A) != 0ull; i++) {
        const int ei = e0 + i;
        const bool p = i < A && ei != e && bpres_claim(q.dflag, ei);
        bpres_push(q.dq, cnt, p, ei, q.b.nedge);
    }
}

static __global__ __launch_bounds__(NSK_BLOCK) void k_bpres_vpos(const ResArgs q) {
    const BpArgs &a = q.b;
    for (int pos = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); pos < a.nvlist; pos += (int)(gridDim.x * NSK_BLOCK))
        for (int x = a.v_eoff[pos]; x < a.v_eoff[pos + 1]; x++) q.e_vpos[a.v_edges[x]] = pos;
}

// |what a commit would store - what is stored|, bp_store's arithmetic without the store
__device__ __forceinline__ double bpres_delta(double old, double c, double lam, double oml) {
    if (lam > 0.0) c = oml * c + lam * old;
    const double d = fabs(c - old);
    return d == d ? d : __longlong_as_double(0x7ff0000000000000LL);
}

// the candidate of edge e: bp_factor_body's sums, Z and divisions, stored undamped; returns r[e]
__device__ __forceinline__ double bpres_cand_edge(const ResArgs &q, int e, double lam, double oml) {
    const BpArgs &a = q.b;
    const int f = a.e_fac[e];
    const int e0 = a.edge_off[f], A = a.edge_off[f + 1] - e0, j = e - e0;
    const long long t0 = a.tab_off[f];
    const int T = (int)(a.tab_off[f + 1] - t0);
    const long long mo = a.msg_off[e];
    const int cj = (int)(a.msg_off[e + 1] - mo);
    int sj = 1;
    for (int i = A - 1; i > j; i--) sj *= (int)(a.msg_off[e0 + i + 1] - a.msg_off[e0 + i]);
    double res = 0.0;
    if (cj == 2) {
        const double m0 = bp_edge_sum(a, t0, T, e0, A, j, 2, sj, 0), m1 = bp_edge_sum(a, t0, T, e0, A, j, 2, sj, 1);
        const double Z = m0 + m1;
        const double c0 = m0 / Z, c1 = m1 / Z;
        q.cand[mo] = c0; q.cand[mo + 1] = c1;
        res = fmax(res, bpres_delta(a.f2v[mo], c0, lam, oml));
        res = fmax(res, bpres_delta(a.f2v[mo + 1], c1, lam, oml));
    } else if (cj <= NSK_ZLOCAL) {
        double m[NSK_ZLOCAL];
        double Z = 0.0;
        for (int k = 0; k < cj; k++) {
            m[k] = bp_edge_sum(a, t0, T, e0, A, j, cj, sj, k);
            Z = k == 0 ? m[0] : Z + m[k];
        }
        for (int k = 0; k < cj; k++) {
            const double c = m[k] / Z;
            q.cand[mo + k] = c;
            res = fmax(res, bpres_delta(a.f2v[mo + k], c, lam, oml));
        }
    } else {            // large domains: two passes, the second recomputes the identical sums
        double Z = 0.0;
        for (int k = 0; k < cj; k++) {
            const double mk = bp_edge_sum(a, t0, T, e0, A, j, cj, sj, k);
            Z = k == 0 ? mk : Z + mk;
        }
        for (int k = 0; k < cj; k++) {
            const double c = bp_edge_sum(a, t0, T, e0, A, j, cj, sj, k) / Z;
            q.cand[mo + k] = c;
            res = fmax(res, bpres_delta(a.f2v[mo + k], c, lam, oml));
        }
    }
    return res;
}

// round t, candidate phase over D_t (all: every edge, round 0 of a call)
static __global__ __launch_bounds__(NSK_BLOCK) void k_bpres_cand(const ResArgs q, int t, int all, double tol, double lam, double oml) {
    if (bpres_done(q, t, tol)) return;
    const int ne = q.b.nedge;
    const unsigned long long have = all ? (unsigned long long)ne : q.nD[t];
    const int n = have < (unsigned long long)ne ? (int)have : ne;
    for (int idx = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); idx < n; idx += (int)(gridDim.x * NSK_BLOCK)) {
        int e = all ? idx : q.dq[idx];
        if (e < 0 || e >= ne) continue;             // (a guard only: the queue holds edges)
        q.dflag[e] = 0;
        q.r[e] = bpres_cand_edge(q, e, lam, oml);
    }
}

// round t, the maximum of r over all edges (the tail is bp_factor_body's)
static __global__ __launch_bounds__(NSK_BLOCK) void k_bpres_max(const ResArgs q, int t, double tol) {
    __shared__ double lds[NSK_BLOCK / 64];
    if (bpres_done(q, t, tol)) return;              // block-uniform, before the barrier
    double res = 0.0;
    for (int e = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); e < q.b.nedge; e += (int)(gridDim.x * NSK_BLOCK)) res = fmax(res, q.r[e]);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) res = fmax(res, __shfl_xor(res, off, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = res;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < NSK_BLOCK / 64; k++) res = fmax(res, lds[k]);
        if (res > 0.0) atomicMax(q.res + t, (unsigned long long)__double_as_longlong(res));
    }
}

// round t, select and commit over all edges, 64 consecutive edges a wave and trip.  push == 0 (round 0 of a cold call:
// every variable is walked anyway) leaves the touched queues alone.
static __global__ __launch_bounds__(NSK_BLOCK) void k_bpres_commit(const ResArgs q, int t, double tol, double frac, double lam, double oml, int push) {
    if (bpres_done(q, t, tol)) return;
    const BpArgs &a = q.b;
    const double tau = frac > 0.0 ? frac * __longlong_as_double((long long)q.res[t]) : 0.0;
    const int lane = (int)(threadIdx.x & 63), nrest = a.nvlist - q.nvbin;
    for (int base = (int)(blockIdx.x * NSK_BLOCK + (threadIdx.x & ~63u)); base < a.nedge; base += (int)(gridDim.x * NSK_BLOCK)) {
        const int e = base + lane;
        bool sel = false;
        int pos = 0;
        if (e < a.nedge) {
            const double re = q.r[e];
            sel = re > 0.0 && re >= tau;
        }
        if (sel) {
            const long long m0 = a.msg_off[e], m1 = a.msg_off[e + 1];
            double rn = 0.0;
            for (long long i = m0; i < m1; i++) {
                const double old = a.f2v[i], c = q.cand[i];
                const double nw = lam > 0.0 ? oml * c + lam * old : c;
                a.f2v[i] = nw;
                rn = fmax(rn, bpres_delta(nw, c, lam, oml));
            }
            q.r[e] = rn;
            pos = q.e_vpos[e];
        }
        const unsigned long long m = __ballot(sel);
        if (lane == 0 && m != 0ull)
            (void)__hip_atomic_fetch_add(q.upd + t, (unsigned long long)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (push && m != 0ull) {
            const bool mine = sel && bpres_claim(q.vflag, pos), bin = pos < q.nvbin;
            bpres_push(q.vq, q.nV + 2 * t, mine && bin, pos, q.nvbin);
            bpres_push(q.vq + q.nvbin, q.nV + 2 * t + 1, mine && !bin, pos, nrest);
        }
    }
}

// Round t, variable phase over V_t (all: every entry of the kernel's part of v_list).  The binary variables have a queue
// and a launch of their own, for k_bp_var's reason: the lane-private vectors of the middle cardinalities would cost the
// binary lanes their occupancy.  64 consecutive queue entries a wave and trip; the walk is lane-private and divergent, the
// pushes behind it run in wave-uniform steps, one of the variable's edges a step.
template <bool BIN>
__global__ __launch_bounds__(NSK_BP_VAR_BLOCK) void k_bpres_var(const ResArgs q, int t, int all, double tol) {
    if (bpres_done(q, t, tol)) return;
    const BpArgs &a = q.b;
    const int lo = BIN ? 0 : q.nvbin, part = BIN ? q.nvbin : a.nvlist - q.nvbin;
    const unsigned long long have = all ? (unsigned long long)part : q.nV[2 * t + (BIN ? 0 : 1)];
    const int n = have < (unsigned long long)part ? (int)have : part;
    const int lane = (int)(threadIdx.x & 63);
    unsigned long long *cnt = q.nD + t + 1;
    for (int base = (int)(blockIdx.x * NSK_BP_VAR_BLOCK + (threadIdx.x & ~63u)); base < n; base += (int)(gridDim.x * NSK_BP_VAR_BLOCK)) {
        const int idx = base + lane;
        int e0 = 0, d = 0;
        unsigned int cm = 0;        // the register walk's changed edges, a bit each
        bool reg = false;
        int pos = idx < n ? (all ? lo + idx : q.vq[lo + idx]) : -1;
        if (pos < lo || pos >= lo + part) pos = -1; // (a guard only: the queue holds positions of this part)
        if (pos >= 0) {
            q.vflag[pos] = 0;
            const int id = a.v_list[pos];
            e0 = a.v_eoff[pos];
            d = a.v_eoff[pos + 1] - e0;
            const long long b0 = a.b_off[id];
            const int nv = (int)(a.b_off[id + 1] - b0);
            if (BIN && d <= NSK_BP_VAR_REG) { cm = bp_var_lane_reg<true>(a, a.v_edges + e0, d, a.belief + b0); reg = true; }
            else if (BIN) bp_var_lane<2, true>(a, 2, a.v_edges + e0, d, a.belief + b0, nullptr, q.pre, q.chg);
            else if (nv <= NSK_ZLOCAL) bp_var_lane<NSK_ZLOCAL, true>(a, nv, a.v_edges + e0, d, a.belief + b0, nullptr, q.pre, q.chg);
            else bp_var_lane<0, true>(a, nv, a.v_edges + e0, d, a.belief + b0, a.wk + b0, q.pre, q.chg);
        }
        for (int s = 0; __ballot(s < d) != 0ull; s++) {
            bool want = false;
            int e = 0;
            if (s < d) {
                e = a.v_edges[e0 + s];
                want = reg ? ((cm >> s) & 1u) != 0u : q.chg[e] != 0;
            }
            bpres_push_others(q, want, e, cnt);
        }
    }
}

}  // namespace nsk
