// nsk_kernels_sw.h -- Swendsen-Wang cluster updates of pairwise binary graphs, every chain in the same launches
// (nsk_sw_setup / nsk_sw_sweeps, nsk_sw.hip; the rule is stated in include/numbskull_amd.h and restated in numpy by
// numbskull_amd.diagnostics.sw_tables / sw_step -- device and numpy agree bit for bit and integer for integer).
//
//   k_sw_factor   one lane per factor: a bond's J and signed q and the g of its two ends, a field's g, from theta
//   k_sw_field    one lane per ordinal: h = the sum of its g entries in ascending factor id, H = h in Q31.32
//   k_sw_tile     one block per (tile, chain): values and parents of the tile in LDS, the lanes draw the tile's bonds and
//                 unite the ends of the active ones by a lock-free union-find on LDS atomics; then every local root is
//                 found and parent[ordinal] = tile base + local root goes to global memory, the accumulators zeroed
//   k_sw_cross    one lane per bond of the cross list: drawn again, both roots found in the global parent array, the
//                 larger hooked under the smaller by a compare-and-swap
//   k_sw_flatten  one lane per ordinal: pointer-jump to the root, store it as the label, add +-H and 1 into the root's
//                 two int64 accumulators -- the lanes of a wave that share a root leave as one atomic each
//   k_sw_decide   one lane per ordinal that is its own label: the heat-bath decision, clusters and largest
//   k_sw_flip     one lane per ordinal: a member of a flipping cluster writes 1 - x; flipped
//
// Union-find.  parent[x] <= x always, with equality exactly at a root, and a parent entry changes only once: by the
// compare-and-swap that finds it a root and hooks it under a SMALLER root.  So every chain of parents descends strictly
// and ends, a read that is out of date still names an ancestor, and a failed hook means another lane lowered that root.
// No lane waits for another: every loop below ends by its own progress or by somebody else's.  A bond is drawn where it
// is needed (one Philox block, counter = the bond ordinal) and never stored.  The order of the hooks is arbitrary; the
// result is not: the components of a graph do not depend on the order their edges are united in, the label is the
// smallest ordinal, and the sums are integers.
#pragma once

#include "nsk_kernels_bp.h"
#include "nsk_sw_plan.h"           // NSK_SW_TILE

namespace nsk {

#define NSK_SW_MAX_BLOCKS 2048      // the lanes of a larger launch loop (8 blocks per CU)
#define NSK_SW_AGG_ROUNDS 4         // distinct roots of a wave that leave aggregated; the lanes behind them add alone

// what the table kernels read of a set-up (nsk_internal.h NskSw)
struct SwTabArgs {
    const double *theta;
    const long long *tab_off;       // [F + 1]
    const int32_t *edge_off;        // [F + 1] directed edges, factor-major: a bond has two, a field one
    const int32_t *f_bond;          // [F] bond ordinal or -1
    const int32_t *ve_off, *ve_edge;   // [nvars + 1] by ordinal: the variable's directed edges, ascending
    double *g;                      // [E] a directed edge's share of its variable's field
    double *J, *qs;                 // [nbonds] the coupling; q = exp(-2 |J|) with the sign bit of J
    double *h;                      // [nvars]
    long long *H;                   // [nvars]
    long long nfactor;
    int32_t nvars;
};

static __global__ __launch_bounds__(NSK_BLOCK) void k_sw_factor(const SwTabArgs a) {
    for (long long f = (long long)blockIdx.x * NSK_BLOCK + threadIdx.x; f < a.nfactor; f += (long long)gridDim.x * NSK_BLOCK) {
        const int e0 = a.edge_off[f], A = a.edge_off[f + 1] - e0;
        const double *th = a.theta + a.tab_off[f];
        if (A == 1) a.g[e0] = th[1] - th[0];
        if (A != 2) continue;
        const double t00 = th[0], t01 = th[1], t10 = th[2], t11 = th[3];
        const double J = ((t00 + t11) - (t01 + t10)) * 0.25;
        a.g[e0] = ((t10 + t11) - (t00 + t01)) * 0.5;
        a.g[e0 + 1] = ((t01 + t11) - (t00 + t10)) * 0.5;
        const double q = nsk_exp(-2.0 * fabs(J));
        const int b = a.f_bond[f];
        a.J[b] = J;
        a.qs[b] = J < 0.0 ? -q : q;
    }
}

static __global__ __launch_bounds__(NSK_BLOCK) void k_sw_field(const SwTabArgs a) {
    for (int o = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); o < a.nvars; o += (int)(gridDim.x * NSK_BLOCK)) {
        double h = 0.0;
        for (int k = a.ve_off[o]; k < a.ve_off[o + 1]; k++) h = h + a.g[a.ve_edge[k]];
        a.h[o] = h;
        a.H[o] = __double2ll_rn(h * NSK_GRAD_SCALE);
    }
}

// what the kernels of an update read; blockIdx.y names the chain
struct SwArgs {
    char *val;                      // chain 0's values
    long long chain_stride;         // bytes between chains
    const int32_t *ord_id;          // [nvars] ordinal -> internal id
    const int32_t *tile_off, *tb_off;  // [ntiles + 1]
    const int2 *tb_rec;             // {local u | local v << 16, bond ordinal}
    const int4 *cross;              // {ordinal u, ordinal v, bond ordinal, 0}
    const double *qs;               // [nbonds]
    const long long *H;             // [nvars]
    int32_t *parent;                // [chains][nvars]: parents, then (k_sw_flatten) labels
    long long *acc;                 // [chains][nvars][2]: Delta and size, at the root
    uint8_t *flip;                  // [chains][nvars]: the decision, at the root
    unsigned long long *out;        // [chains][3] of this step: clusters, largest, flipped
    int32_t nvars, ntiles, ncross;
    uint32_t k0, k1, s_lo, s_hi;    // the key of chain 0 (chain r: k1 ^ r), the update's sweep index (high word ^ tag)
};

// the project's 53-bit draw from words x and y of the block (c, stream, sweep)
__device__ __forceinline__ double sw_draw(const SwArgs &a, uint32_t chain, uint32_t c, uint32_t stream) {
    const u32x4 r = philox4x32(a.k0, a.k1 ^ chain, c, stream, a.s_lo, a.s_hi);
    return u53(r.x, r.y);
}

// a bond is active iff J != 0 (q = 1 otherwise, which no draw reaches), its ends agree (equal values for J > 0, unequal
// for J < 0) and u(b, 4) >= q; the block is computed only where the ends agree
__device__ __forceinline__ bool sw_active(const SwArgs &a, uint32_t chain, int b, int xu, int xv) {
    const double qs = a.qs[b];
    const bool neg = __double_as_longlong(qs) < 0;
    if ((xu == xv) == neg) return false;
    return sw_draw(a, chain, (uint32_t)b, 4u) >= fabs(qs);
}

__device__ __forceinline__ int sw_load_parent(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_sw_tile(const SwArgs a) {
    __shared__ int par[NSK_SW_TILE];
    __shared__ uint8_t x[NSK_SW_TILE];
    const volatile int *vpar = par;                 // (the union loop reads what other lanes' atomics wrote)
    const uint32_t chain = blockIdx.y;
    const VT *val = (const VT *)(a.val + (long long)chain * a.chain_stride);
    int32_t *parent = a.parent + (long long)chain * a.nvars;
    long long *acc = a.acc + 2ll * chain * a.nvars;
    for (int t = (int)blockIdx.x; t < a.ntiles; t += (int)gridDim.x) {      // block-uniform: every lane meets every barrier
        const int base = a.tile_off[t], n = a.tile_off[t + 1] - base;
        for (int l = (int)threadIdx.x; l < n; l += NSK_BLOCK) {
            x[l] = (uint8_t)val[a.ord_id[base + l]];
            par[l] = l;
        }
        __syncthreads();
        for (int i = a.tb_off[t] + (int)threadIdx.x; i < a.tb_off[t + 1]; i += NSK_BLOCK) {
            const int2 rec = a.tb_rec[i];
            int u = rec.x & 0xffff, v = (int)((unsigned int)rec.x >> 16);
            if (!sw_active(a, chain, rec.y, x[u], x[v])) continue;
            for (;;) {              // ends: a failed hook returns the smaller parent another lane gave that root; roots only fall
                for (int p; (p = vpar[u]) != u;) u = p;     // ends: par[u] < u below a root
                for (int p; (p = vpar[v]) != v;) v = p;     // ends: par[v] < v below a root
                if (u == v) break;
                const int hi = u > v ? u : v, lo = u > v ? v : u;
                const int old = atomicCAS(&par[hi], hi, lo);
                if (old == hi) break;
                u = old; v = lo;
            }
        }
        __syncthreads();
        for (int l = (int)threadIdx.x; l < n; l += NSK_BLOCK) {
            int r = l;
            while (par[r] != r) r = par[r];         // ends: par[r] < r below a root; nothing is written here
            parent[base + l] = base + r;
            acc[2 * (long long)(base + l)] = 0;
            acc[2 * (long long)(base + l) + 1] = 0;
        }
        __syncthreads();
    }
}

// the root of o in the global array as it stands (or stood: an entry read late names an ancestor all the same)
__device__ __forceinline__ int sw_find(const int32_t *parent, int o) {
    for (;;) {                      // ends: parent[o] < o below a root
        const int p = sw_load_parent(parent + o);
        if (p == o) return o;
        o = p;
    }
}

template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_sw_cross(const SwArgs a) {
    const uint32_t chain = blockIdx.y;
    const VT *val = (const VT *)(a.val + (long long)chain * a.chain_stride);
    int32_t *parent = a.parent + (long long)chain * a.nvars;
    for (int i = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); i < a.ncross; i += (int)(gridDim.x * NSK_BLOCK)) {
        const int4 rec = a.cross[i];
        if (!sw_active(a, chain, rec.z, (int)val[a.ord_id[rec.x]], (int)val[a.ord_id[rec.y]])) continue;
        int u = rec.x, v = rec.y;
        for (;;) {                  // ends: a failed hook returns the smaller parent another lane gave that root; roots only fall
            u = sw_find(parent, u);
            v = sw_find(parent, v);
            if (u == v) break;
            const int hi = u > v ? u : v, lo = u > v ? v : u;
            const int old = atomicCAS(parent + hi, hi, lo);
            if (old == hi) break;
            u = old; v = lo;
        }
    }
}

template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_sw_flatten(const SwArgs a) {
    const uint32_t chain = blockIdx.y;
    const VT *val = (const VT *)(a.val + (long long)chain * a.chain_stride);
    int32_t *parent = a.parent + (long long)chain * a.nvars;
    unsigned long long *acc = (unsigned long long *)a.acc + 2ll * chain * a.nvars;
    const int lane = (int)(threadIdx.x & 63);
    // 64 consecutive ordinals a wave and trip: all 64 lanes reach every ballot and shuffle
    for (int base = (int)(blockIdx.x * NSK_BLOCK + (threadIdx.x & ~63u)); base < a.nvars; base += (int)(gridDim.x * NSK_BLOCK)) {
        const int o = base + lane;
        bool todo = o < a.nvars;
        int r = -1;
        long long d = 0;
        if (todo) {
            r = sw_find(parent, o);
            // the label: a root keeps itself, anything else jumps to its root (a lane that walks through o meanwhile reads
            // the old parent or the root, an ancestor either way)
            __hip_atomic_store(parent + o, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const long long Hv = a.H[o];
            d = val[a.ord_id[o]] == 0 ? Hv : -Hv;
        }
        for (int round = 0; round < NSK_SW_AGG_ROUNDS; round++) {
            const unsigned long long m = __ballot(todo);
            if (m == 0ull) break;   // wave-uniform
            const int lead = __ffsll((long long)m) - 1;
            const int rl = __shfl(r, lead, 64);
            const bool mine = todo && r == rl;
            long long s = mine ? d : 0;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
            const int cnt = __popcll(__ballot(mine));
            if (lane == lead) {
                (void)__hip_atomic_fetch_add(acc + 2ll * rl, (unsigned long long)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_add(acc + 2ll * rl + 1, (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            todo = todo && !mine;
        }
        if (todo) {                 // many small clusters: nobody contends
            (void)__hip_atomic_fetch_add(acc + 2ll * r, (unsigned long long)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(acc + 2ll * r + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// D = Delta 2^-32, e = exp(-D); the cluster flips iff u(label, 5) (1 + e) < 1 (a NaN does not flip)
static __global__ __launch_bounds__(NSK_BLOCK) void k_sw_decide(const SwArgs a) {
    const uint32_t chain = blockIdx.y;
    const int32_t *label = a.parent + (long long)chain * a.nvars;
    const long long *acc = a.acc + 2ll * chain * a.nvars;
    uint8_t *flip = a.flip + (long long)chain * a.nvars;
    const int lane = (int)(threadIdx.x & 63);
    unsigned long long nroots = 0, largest = 0;
    for (int base = (int)(blockIdx.x * NSK_BLOCK + (threadIdx.x & ~63u)); base < a.nvars; base += (int)(gridDim.x * NSK_BLOCK)) {
        const int o = base + lane;
        const bool root = o < a.nvars && label[o] == o;
        if (root) {
            const double D = (double)acc[2ll * o] * (1.0 / NSK_GRAD_SCALE);
            const double e = nsk_exp(-D);
            flip[o] = sw_draw(a, chain, (uint32_t)o, 5u) * (1.0 + e) < 1.0 ? 1 : 0;
            const unsigned long long size = (unsigned long long)acc[2ll * o + 1];
            largest = size > largest ? size : largest;
        }
        nroots += (unsigned long long)__popcll(__ballot(root));
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long other = __shfl_xor(largest, off, 64);
        largest = other > largest ? other : largest;
    }
    if (lane == 0 && nroots) {
        (void)__hip_atomic_fetch_add(a.out + 3 * chain, nroots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)atomicMax(a.out + 3 * chain + 1, largest);
    }
}

template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_sw_flip(const SwArgs a) {
    const uint32_t chain = blockIdx.y;
    VT *val = (VT *)(a.val + (long long)chain * a.chain_stride);
    const int32_t *label = a.parent + (long long)chain * a.nvars;
    const uint8_t *flip = a.flip + (long long)chain * a.nvars;
    const int lane = (int)(threadIdx.x & 63);
    unsigned long long n = 0;
    for (int base = (int)(blockIdx.x * NSK_BLOCK + (threadIdx.x & ~63u)); base < a.nvars; base += (int)(gridDim.x * NSK_BLOCK)) {
        const int o = base + lane;
        const bool f = o < a.nvars && flip[label[o]] != 0;
        if (f) {
            const int id = a.ord_id[o];
            val[id] = (VT)(1 - (int)val[id]);
        }
        n += (unsigned long long)__popcll(__ballot(f));
    }
    if (lane == 0 && n) (void)__hip_atomic_fetch_add(a.out + 3 * chain + 2, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace nsk
