// nsk_kernels_bpwide.h -- the factor phase of sum-product belief propagation for WIDE logical factors (nsk_bp_wide_plan.h;
// nsk_bp_wide.hip launches these; the rule is stated in include/numbskull_amd.h and restated in numpy by
// numbskull_amd.diagnostics.bp_wide_factor).  A wide factor has no table.  With nu_l = (nu_l(0), nu_l(1)) the incoming
// message at member position l -- the indicator of its value for a clamped member -- the boolean functions are a
// constant plus a correction on one or two patterns, psi = cb + d [pattern], cb and cb + d the nsk_exp(theta - max theta)
// of the function's two values, so the message to position j is
//     m_j(x) = cb * prod_{l != j} (nu_l(0) + nu_l(1))  +  d * (the pattern's product over l != j, where x fits it)
// and LINEAR is a product over the body given the head h, prod_l c_l(h) with c_l(h) = ge nu_l(h) + gd nu_l(1 - h), where
// (ge, gd) = (1, q) for w >= 0 and (q, 1) below, q = nsk_exp(-|w|): every factor is at most 1.  All of it is leave-one-out
// products of three streams a position, formed WITHOUT a division as prefix x suffix, so the exact zeros of clamped members
// do no harm.  Messages are normalised, so every product of the pattern functions is at most about 1 and an underflow to 0
// is the correct answer to every bit that matters: no rescaling is needed there.  LINEAR keeps exponents (bpw_linear).
//
//   k_bp_wide           one wave per wide factor (grid stride over the factors), lanes take the positions 64 at a time.
//                       Forward: the position's pair, its three stream values, an inclusive product scan across the wave
//                       (six shuffle steps a stream, fixed association) times the carry of the chunks before; the
//                       exclusive prefixes go to LDS, the carry comes from lane 63.  Backward: the same with a suffix
//                       carry; leave-one-out = prefix x suffix, the function's formula, Z = m[0] + m[1], damping and
//                       residual as k_bp_factor's.  The head of LINEAR, LOGICAL and IMPLY_MLN (the last position) is
//                       read first and stays out of the streams; its message comes from the body's totals.
//                       A lane reads from LDS only what it wrote itself: no barrier inside a factor.
//   k_bp_wide_terms     the same walk, one double per wide factor: sum_a b_f (theta_f - ln b_f) in its closed form
//                       ln Z' + max theta - sum_l sum_x b_l(x) ln nu_l(x), Z' = sum_x nu_j(x) m_j(x) at the last position j,
//                       b_l(x) = nu_l(x) m_l(x) / Z', 0 ln 0 = 0
//   k_bp_factor_narrow  k_bp_factor's edges of the table route, from a list: in a set-up with wide factors the directed
//                       edges of both routes interleave, and k_bp_factor would walk all of them
//   k_bp_wide_clamp     set-up: -1 - internal id of a clamped position becomes -1 - value
//
// Dynamic LDS: 3 x 8 bytes a position of the largest wide factor (rounded up to 64 positions) a wave, at most 48 KB; four
// waves a block while a wave stays within 16 KB, one beyond (nsk_bp_wide_plan.h).
#pragma once

#include "nsk_kernels_bp.h"

namespace nsk {

struct BpWideArgs {
    const int4 *rec;                // [nwide] {factor, function, weight slot, first position}
    const int32_t *pos_off;         // [nwide + 1]
    const int32_t *pos;             // directed edge, or -1 - value of a clamped member
    const int32_t *narrow;          // [nnarrow] the directed edges of the table route
    const long long *msg_off;       // what the wide kernels read of BpArgs (a kernel that took all of it would spill)
    const double *w, *v2f;
    double *f2v;
    int32_t nwide, nnarrow, wave_lds;       // wave_lds: doubles of LDS a wave
};

enum { BPW_ALL1 = 0, BPW_ALL0 = 1, BPW_EQ = 2, BPW_LOGICAL = 3, BPW_MLN = 4, BPW_LINEAR = 5 };   // from BPW_LOGICAL on: a head

struct BpwConst {
    int kind;
    double cb, d, ge, gd, mx;
};

// nb: the body's positions (LINEAR's largest value)
__device__ __forceinline__ BpwConst bpw_const(int fn, double w, int nb) {
    BpwConst c = {};
    c.ge = 1.0; c.gd = 1.0;
    if (fn == F_LINEAR) {
        const double q = nsk_exp(-fabs(w));
        c.kind = BPW_LINEAR;
        if (w >= 0.0) { c.gd = q; c.mx = w * (double)nb; } else { c.ge = q; c.mx = 0.0; }
        return c;
    }
    const bool sym = fn == F_AND || fn == F_ISTRUE || fn == F_OR || fn == F_EQUAL;     // values -1 and 1; the others 0 and 1
    const double lo = sym ? -w : 0.0;
    c.mx = fmax(lo, w);
    const double clo = nsk_exp(lo - c.mx), chi = nsk_exp(w - c.mx);
    const bool base_hi = fn == F_OR || fn == F_LOGICAL || fn == F_IMPLY_MLN;            // the pattern takes the LOW value
    c.cb = base_hi ? chi : clo;
    c.d = (base_hi ? clo : chi) - c.cb;
    c.kind = fn == F_OR ? BPW_ALL0 : fn == F_EQUAL ? BPW_EQ : fn == F_LOGICAL ? BPW_LOGICAL : fn == F_IMPLY_MLN ? BPW_MLN : BPW_ALL1;
    return c;
}

struct __attribute__((aligned(8))) BpwPair { double x, y; };

// the incoming pair at a position record and where its outgoing message lies (-1: clamped)
__device__ __forceinline__ void bpw_pair(const BpWideArgs &a, int r, long long &mo, double &n0, double &n1) {
    if (r >= 0) {
        mo = a.msg_off[r];
        const BpwPair v = *(const BpwPair *)(a.v2f + mo);
        n0 = v.x; n1 = v.y;
    } else {
        mo = -1;
        n0 = r == -1 ? 1.0 : 0.0; n1 = r == -2 ? 1.0 : 0.0;
    }
}

// the three stream values of a body position of a pattern function: nu(0), nu(1) and their sum
__device__ __forceinline__ void bpw_streams(const BpwConst &, double n0, double n1, double &x0, double &x1, double &x2) {
    x0 = n0; x1 = n1; x2 = n0 + n1;
}

// inclusive products of the lanes up to and including this one / from this one on
__device__ __forceinline__ double bpw_scan_up(double x, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(x, off, 64);
        if (lane >= off) x = o * x;
    }
    return x;
}
__device__ __forceinline__ double bpw_scan_down(double x, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_down(x, off, 64);
        if (lane + off < 64) x = x * o;
    }
    return x;
}

// the unnormalised message to a body position from the leave-one-out products (L0, L1, L2) of the streams; (h0, h1): the head's pair
__device__ __forceinline__ void bpw_body_msg(const BpwConst &c, double L0, double L1, double L2, double h0, double h1, double &m0, double &m1) {
    const bool head = c.kind >= BPW_LOGICAL;
    const double base = head ? (c.cb * L2) * (h0 + h1) : c.cb * L2;
    const double a0 = c.kind == BPW_LOGICAL ? h1 * L0 : L0, a1 = head ? h0 * L1 : L1;
    const double y0 = base + c.d * a0, y1 = base + c.d * a1;
    m0 = (c.kind == BPW_ALL0 || c.kind == BPW_EQ || c.kind == BPW_LOGICAL) ? y0 : base;
    m1 = c.kind != BPW_ALL0 ? y1 : base;
}

// ... and to the head from the body's totals
__device__ __forceinline__ void bpw_head_msg(const BpwConst &c, double T0, double T1, double T2, double &m0, double &m1) {
    const double base = c.cb * T2;
    m0 = base + c.d * T1;
    m1 = c.kind == BPW_LOGICAL ? base + c.d * T0 : base;
}

__device__ __forceinline__ double bpw_xlogn(double nu, double m, double Z) {
    const double b = (nu * m) / Z;
    return b > 0.0 ? b * log(nu) : 0.0;
}

// ---- LINEAR.  Its two streams c_l(0), c_l(1) are both below 1, and nothing near 1 stands beside them as the pattern
// functions' nu(0) + nu(1) does: over 2048 positions both products leave the range of a double (from about |w| x positions
// = 700 on) although their ratio, which is all a normalised message keeps, is ordinary.  So a LINEAR product is a
// mantissa in [0.5, 1) (or 0) and an int exponent, renormalised by frexp after every multiplication -- powers of two,
// exact -- and the two leave-one-out products meet at their larger exponent before the formula.
struct BpwX { double m; int e; };
__device__ __forceinline__ BpwX bpw_x(double v) { BpwX x; x.m = frexp(v, &x.e); return x; }
__device__ __forceinline__ BpwX bpw_xmul(BpwX a, BpwX b) {
    int e;
    BpwX r;
    r.m = frexp(a.m * b.m, &e);
    r.e = a.e + b.e + e;
    return r;
}
__device__ __forceinline__ BpwX bpw_xshfl(BpwX x, int src) { BpwX r; r.m = __shfl(x.m, src, 64); r.e = __shfl(x.e, src, 64); return r; }
__device__ __forceinline__ BpwX bpw_xscan(BpwX x, int lane, bool up) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int src = up ? lane - off : lane + off;
        const BpwX o = bpw_xshfl(x, src & 63);
        if (src >= 0 && src < 64) x = up ? bpw_xmul(o, x) : bpw_xmul(x, o);
    }
    return x;
}
// (a x 2^ea, b x 2^eb) at the larger exponent of the two that are not 0; returns that exponent
__device__ __forceinline__ int bpw_xjoin(BpwX a, BpwX b, double &va, double &vb) {
    const int E = a.m == 0.0 ? b.e : (b.m == 0.0 ? a.e : (a.e > b.e ? a.e : b.e));
    const int da = a.e - E, db = b.e - E;
    va = ldexp(a.m, da < -1200 ? -1200 : da); vb = ldexp(b.m, db < -1200 ? -1200 : db);
    return E;
}

template <bool TERMS>
__device__ __forceinline__ double bpw_linear(const BpWideArgs &q, const int32_t *pos, int n, const BpwConst &c, double *pre, double lam, double oml) {
    const int lane = (int)(threadIdx.x & 63), stride = q.wave_lds / 3, nb = n - 1;
    int2 *pre_e = (int2 *)(pre + 2 * stride);       // the exponents of the two prefixes, in the third stream's place
    const BpwX one = bpw_x(1.0);
    long long hmo;
    double h0, h1;
    bpw_pair(q, pos[n - 1], hmo, h0, h1);
    BpwX c0 = one, c1 = one;
    for (int base = 0; base < nb; base += 64) {
        const int p = base + lane;
        BpwX x0 = one, x1 = one;
        if (p < nb) {
            long long mo;
            double n0, n1;
            bpw_pair(q, pos[p], mo, n0, n1);
            x0 = bpw_x(c.ge * n0 + c.gd * n1); x1 = bpw_x(c.gd * n0 + c.ge * n1);
        }
        const BpwX i0 = bpw_xscan(x0, lane, true), i1 = bpw_xscan(x1, lane, true);
        BpwX e0 = bpw_xshfl(i0, (lane + 63) & 63), e1 = bpw_xshfl(i1, (lane + 63) & 63);
        if (lane == 0) { e0 = one; e1 = one; }
        if (p < nb) {
            const BpwX p0 = bpw_xmul(c0, e0), p1 = bpw_xmul(c1, e1);
            pre[p] = p0.m; pre[stride + p] = p1.m; pre_e[p] = make_int2(p0.e, p1.e);
        }
        c0 = bpw_xmul(c0, bpw_xshfl(i0, 63)); c1 = bpw_xmul(c1, bpw_xshfl(i1, 63));
    }
    double res = 0.0, acc = 0.0, lnZ = 0.0;
    {   // the head, from the body's totals
        double m0, m1;
        if (TERMS) {    // nu_h(x) m_h(x): the head's pair is multiplied in BEFORE the two totals meet at one exponent, so
            BpwX z0 = c0, z1 = c1;      // that a head clamped against the larger total keeps the smaller one
            z0.m = h0 * z0.m; z1.m = h1 * z1.m;
            const int E = bpw_xjoin(z0, z1, m0, m1);
            const double Z = m0 + m1;
            lnZ = log(Z) + (double)E * 0.6931471805599453;
            const double b0 = m0 / Z, b1 = m1 / Z;
            if (lane == 0) acc = (b0 > 0.0 ? b0 * log(h0) : 0.0) + (b1 > 0.0 ? b1 * log(h1) : 0.0);
        } else if (lane == 0 && hmo >= 0) {
            (void)bpw_xjoin(c0, c1, m0, m1);
            const double Z = m0 + m1;
            res = fmax(res, bp_store(q.f2v + hmo, m0 / Z, lam, oml));
            res = fmax(res, bp_store(q.f2v + hmo + 1, m1 / Z, lam, oml));
        }
    }
    BpwX s0 = one, s1 = one;
    for (int base = nb > 0 ? (nb - 1) / 64 * 64 : -64; base >= 0; base -= 64) {
        const int p = base + lane;
        long long mo = -1;
        double n0 = 0.0, n1 = 0.0;
        BpwX x0 = one, x1 = one;
        if (p < nb) {
            bpw_pair(q, pos[p], mo, n0, n1);
            x0 = bpw_x(c.ge * n0 + c.gd * n1); x1 = bpw_x(c.gd * n0 + c.ge * n1);
        }
        const BpwX i0 = bpw_xscan(x0, lane, false), i1 = bpw_xscan(x1, lane, false);
        BpwX e0 = bpw_xshfl(i0, (lane + 1) & 63), e1 = bpw_xshfl(i1, (lane + 1) & 63);
        if (lane == 63) { e0 = one; e1 = one; }
        if (p < nb) {
            const int2 pe = pre_e[p];
            BpwX L0, L1;
            L0.m = pre[p]; L0.e = pe.x; L1.m = pre[stride + p]; L1.e = pe.y;
            L0 = bpw_xmul(L0, bpw_xmul(e0, s0)); L1 = bpw_xmul(L1, bpw_xmul(e1, s1));
            L0.m = h0 * L0.m; L1.m = h1 * L1.m;     // u_x = nu_h(x) * L(c(x))_j
            double u0, u1;
            (void)bpw_xjoin(L0, L1, u0, u1);
            const double m0 = u0 * c.ge + u1 * c.gd, m1 = u0 * c.gd + u1 * c.ge;
            if (TERMS) {
                const double Z = n0 * m0 + n1 * m1;         // (the position's own normaliser: Z' at this position's scale)
                acc = acc + (bpw_xlogn(n0, m0, Z) + bpw_xlogn(n1, m1, Z));
            } else if (mo >= 0) {
                const double Z = m0 + m1;
                res = fmax(res, bp_store(q.f2v + mo, m0 / Z, lam, oml));
                res = fmax(res, bp_store(q.f2v + mo + 1, m1 / Z, lam, oml));
            }
        }
        s0 = bpw_xmul(bpw_xshfl(i0, 0), s0); s1 = bpw_xmul(bpw_xshfl(i1, 0), s1);
    }
    if (!TERMS) return res;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) acc = acc + __shfl_xor(acc, off, 64);
    return (lnZ + c.mx) - acc;
}

// Wide factor k by one wave; pre: the wave's 3 x stride doubles of LDS.  TERMS: returns the factor's Bethe term (the same
// double in every lane) and stores nothing; otherwise stores f2v and returns the lane's largest residual.
template <bool TERMS>
__device__ __forceinline__ double bpw_factor(const BpWideArgs &q, int k, double *pre, double lam, double oml) {
    const int lane = (int)(threadIdx.x & 63), stride = q.wave_lds / 3;
    const int4 rec = q.rec[k];
    const int n = q.pos_off[k + 1] - rec.w;
    const int32_t *pos = q.pos + rec.w;
    const bool has_head = rec.y == F_LINEAR || rec.y == F_LOGICAL || rec.y == F_IMPLY_MLN;
    const int nb = has_head ? n - 1 : n;
    const BpwConst c = bpw_const(rec.y, q.w[rec.z], nb);
    if (rec.y == F_LINEAR) return bpw_linear<TERMS>(q, pos, n, c, pre, lam, oml);       // (wave-uniform)
    long long hmo = -1;
    double h0 = 1.0, h1 = 1.0;
    if (has_head) bpw_pair(q, pos[n - 1], hmo, h0, h1);        // (every lane reads the one address)
    // ---- forward: exclusive prefixes to LDS, the totals in the carries
    double c0 = 1.0, c1 = 1.0, c2 = 1.0;
    for (int base = 0; base < nb; base += 64) {
        const int p = base + lane;
        double x0 = 1.0, x1 = 1.0, x2 = 1.0;
        if (p < nb) {
            long long mo;
            double n0, n1;
            bpw_pair(q, pos[p], mo, n0, n1);
            bpw_streams(c, n0, n1, x0, x1, x2);
        }
        const double i0 = bpw_scan_up(x0, lane), i1 = bpw_scan_up(x1, lane), i2 = bpw_scan_up(x2, lane);
        double e0 = __shfl_up(i0, 1, 64), e1 = __shfl_up(i1, 1, 64), e2 = __shfl_up(i2, 1, 64);
        if (lane == 0) { e0 = 1.0; e1 = 1.0; e2 = 1.0; }
        if (p < nb) { pre[p] = c0 * e0; pre[stride + p] = c1 * e1; pre[2 * stride + p] = c2 * e2; }
        c0 = c0 * __shfl(i0, 63, 64); c1 = c1 * __shfl(i1, 63, 64); c2 = c2 * __shfl(i2, 63, 64);
    }
    double res = 0.0, acc = 0.0, Zp = 0.0;
    if (has_head) {
        double m0, m1;
        bpw_head_msg(c, c0, c1, c2, m0, m1);
        if (TERMS) {
            Zp = h0 * m0 + h1 * m1;
            if (lane == 0) acc = bpw_xlogn(h0, m0, Zp) + bpw_xlogn(h1, m1, Zp);
        } else if (lane == 0 && hmo >= 0) {
            const double Z = m0 + m1;
            res = fmax(res, bp_store(q.f2v + hmo, m0 / Z, lam, oml));
            res = fmax(res, bp_store(q.f2v + hmo + 1, m1 / Z, lam, oml));
        }
    }
    // ---- backward: the suffix carries, leave-one-out = prefix x suffix
    double s0 = 1.0, s1 = 1.0, s2 = 1.0;
    for (int base = nb > 0 ? (nb - 1) / 64 * 64 : -64; base >= 0; base -= 64) {
        const int p = base + lane;
        long long mo = -1;
        double n0 = 0.0, n1 = 0.0, x0 = 1.0, x1 = 1.0, x2 = 1.0;
        if (p < nb) {
            bpw_pair(q, pos[p], mo, n0, n1);
            bpw_streams(c, n0, n1, x0, x1, x2);
        }
        const double i0 = bpw_scan_down(x0, lane), i1 = bpw_scan_down(x1, lane), i2 = bpw_scan_down(x2, lane);
        double e0 = __shfl_down(i0, 1, 64), e1 = __shfl_down(i1, 1, 64), e2 = __shfl_down(i2, 1, 64);
        if (lane == 63) { e0 = 1.0; e1 = 1.0; e2 = 1.0; }
        double m0 = 0.0, m1 = 0.0;
        if (p < nb) bpw_body_msg(c, pre[p] * (e0 * s0), pre[stride + p] * (e1 * s1), pre[2 * stride + p] * (e2 * s2), h0, h1, m0, m1);
        if (TERMS) {
            if (!has_head && base + 64 >= nb) Zp = __shfl(n0 * m0 + n1 * m1, (nb - 1) & 63, 64);     // the first trip: the last position
            if (p < nb) acc = acc + (bpw_xlogn(n0, m0, Zp) + bpw_xlogn(n1, m1, Zp));
        } else if (mo >= 0) {
            const double Z = m0 + m1;
            res = fmax(res, bp_store(q.f2v + mo, m0 / Z, lam, oml));
            res = fmax(res, bp_store(q.f2v + mo + 1, m1 / Z, lam, oml));
        }
        s0 = __shfl(i0, 0, 64) * s0; s1 = __shfl(i1, 0, 64) * s1; s2 = __shfl(i2, 0, 64) * s2;
    }
    if (!TERMS) return res;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) acc = acc + __shfl_xor(acc, off, 64);
    return (log(Zp) + c.mx) - acc;
}

// the block's largest residual into residual[t]'s word, as k_bp_factor leaves it (every lane of the block comes here)
__device__ __forceinline__ void bpw_commit(double res, unsigned long long *slot) {
    __shared__ double lds[NSK_BLOCK / 64];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) res = fmax(res, __shfl_xor(res, off, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = res;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (unsigned int k = 1; k < (blockDim.x >> 6); k++) res = fmax(res, lds[k]);
        if (res > 0.0) atomicMax(slot, (unsigned long long)__double_as_longlong(res));
    }
}

extern __shared__ double bpw_lds[];

static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_wide(const BpWideArgs q, int t, double tol, double lam, double oml,
                                                             unsigned long long *residual) {
    if (t > 0 && __longlong_as_double((long long)residual[t - 1]) <= tol) return;      // block-uniform, before the barrier
    const int wave = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    double res = 0.0;
    for (int k = (int)blockIdx.x * wpb + wave; k < q.nwide; k += (int)gridDim.x * wpb)
        res = fmax(res, bpw_factor<false>(q, k, bpw_lds + wave * q.wave_lds, lam, oml));
    bpw_commit(res, residual + t);
}

static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_wide_terms(const BpWideArgs q, double *terms) {
    const int wave = (int)(threadIdx.x >> 6), wpb = (int)(blockDim.x >> 6);
    for (int k = (int)blockIdx.x * wpb + wave; k < q.nwide; k += (int)gridDim.x * wpb) {
        const double v = bpw_factor<true>(q, k, bpw_lds + wave * q.wave_lds, 0.0, 1.0);
        if ((threadIdx.x & 63) == 0) terms[k] = v;
    }
}

// The message of the directed edge e of a table factor, damped and stored; `res` joined by the edge's residual.  This is
// the loop body of bp_factor_body (nsk_kernels_bp.h), operation by operation: it is written out here because taking it
// out of that function changed k_bp_factor's register allocation, and that kernel's code is held to its disassembly.
__device__ __forceinline__ double bp_factor_edge(const BpArgs &a, int e, double lam, double oml, double res) {
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
        return fmax(res, bp_store(a.f2v + mo + 1, m1 / Z, lam, oml));
    }
    double Z = 0.0;             // (k_bp_factor keeps the sums of the middle cardinalities in registers: the same sums, formed twice here)
    for (int k = 0; k < cj; k++) {
        const double mk = bp_edge_sum(a, t0, T, e0, A, j, cj, sj, k);
        Z = k == 0 ? mk : Z + mk;
    }
    for (int k = 0; k < cj; k++) res = fmax(res, bp_store(a.f2v + mo + k, bp_edge_sum(a, t0, T, e0, A, j, cj, sj, k) / Z, lam, oml));
    return res;
}

static __global__ __launch_bounds__(NSK_BLOCK) void k_bp_factor_narrow(const BpArgs a, const BpWideArgs q, int t, double tol, double lam, double oml,
                                                                      unsigned long long *residual) {
    if (t > 0 && __longlong_as_double((long long)residual[t - 1]) <= tol) return;
    double res = 0.0;
    for (int i = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); i < q.nnarrow; i += (int)(gridDim.x * NSK_BLOCK))
        res = bp_factor_edge(a, q.narrow[i], lam, oml, res);
    bpw_commit(res, residual + t);
}

template <typename VT>
__global__ __launch_bounds__(NSK_BLOCK) void k_bp_wide_clamp(int32_t *pos, int npos, const VT *val) {
    for (int i = (int)(blockIdx.x * NSK_BLOCK + threadIdx.x); i < npos; i += (int)(gridDim.x * NSK_BLOCK)) {
        const int r = pos[i];
        if (r < 0) pos[i] = (int)val[-1 - r] != 0 ? -2 : -1;
    }
}

}  // namespace nsk
