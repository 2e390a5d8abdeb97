// nsk_pcd.hip -- the chain-summed per-weight moments and persistent contrastive divergence (nsk_kernels_pcd.h): the entry
// points nsk_weight_moments and nsk_pcd_steps.  They read the records of the factor walk and the by-weight list of the
// statistics (nsk_wstats.hip nsk_wstats_ensure); the work list, the int64 sums, the target, the factor counts and the
// per-step outputs live for the call only.  nsk_pcd_steps enqueues (the burn-in sweeps of nsk_gibbs_sweeps, zero the sums,
// the moment launches, k_pcd_update) per step on the handle's stream without a host wait and synchronises once.
// nsk_pcd_latent_steps does the same for two populations of the handle's chains, clamped and free, each swept through a
// ChainRange view (nsk_internal.h), each with its own sums, and k_pcd_latent_update takes its target from the clamped ones.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "nsk_internal.h"
#include "nsk_kernels_pcd.h"

using namespace nsk;

namespace {

// the per-function bound of a factor's value, as nsk_pl_gradient's range rule has it
double moments_vmax(uint32_t head) {
    const int fn = NSK_FHEAD_FUNC(head);
    const double ar = (double)std::max(NSK_FHEAD_ARITY(head), 1);
    return fn == F_LINEAR ? ar : fn == F_RATIO ? std::log(ar + 1.0) : fn == F_UFO ? 1e6 : 1.0;
}

// The range of the int64 sums, from the graph alone: B_w = the sum of vmax(f) over the factors of weight w.  Every term is
// at most vmax * 2^32 in magnitude, so B_w * nchains < 2^30 keeps a weight's sum over all chains below 2^62.
int moments_range(const nsk_graph *g, int64_t nchains, const std::string &what) {
    const Compiled &c = g->c;
    const double limit = 1073741824.0 / (double)nchains;
    const size_t nf = (size_t)c.nfactor;
    // every B_w is at most the sum over ALL factors: most calls are decided by that one number (host threads; with a
    // factor of two to spare, so that the order of their partial sums cannot matter)
    std::vector<double> part((size_t)nsk::compile_threads(), 0.0);
    nsk::parallel_for((int64_t)nf, [&](int64_t b0, int64_t b1, int t) {
        double s = 0.0;
        for (int64_t f = b0; f < b1; f++) s += moments_vmax(c.f_rec[4 * (size_t)f]);
        part[(size_t)t] = s;
    });
    double total = 0.0;
    for (double x : part) total += x;
    if (total < 0.5 * limit) return NSK_OK;
    std::vector<double> B((size_t)c.nweight, 0.0);
    for (size_t f = 0; f < nf; f++) {
        const uint32_t slot = c.f_rec[4 * f + 2];
        if (slot < (uint32_t)c.nweight) B[slot] += moments_vmax(c.f_rec[4 * f]);
    }
    for (int64_t s = 0; s < c.nweight; s++)
        if (B[(size_t)s] >= limit) {
            const int64_t wid = c.wuser.empty() ? s : (int64_t)c.wuser[(size_t)s];
            return fail(NSK_E_RANGE, what + ": the moment sum of weight " + std::to_string((long long)wid) + " over " +
                                     std::to_string((long long)nchains) + " chain(s) may reach 2^62 (its bound B = " + std::to_string(B[(size_t)s]) +
                                     "; B x chains must stay below 2^30)");
        }
    return NSK_OK;
}

// the buffers of one call: entered in the ledger, gone when the call returns
struct PcdBufs {
    nsk_graph *g;
    uint2 *shorts = nullptr;
    uint4 *pieces = nullptr;
    unsigned long long *M = nullptr, *gmax = nullptr;
    double *target = nullptr, *nfac = nullptr;
    long long *rows = nullptr;
    unsigned long long *Mf = nullptr;      // nsk_pcd_latent_steps: the free chains' sums (M holds the clamped chains')
    int2 *pairs = nullptr;                 // ... and the clamp's {internal id, value} list
    explicit PcdBufs(nsk_graph *g_) : g(g_) {}
    ~PcdBufs() {
        dev_free(g, pairs); dev_free(g, Mf);
        dev_free(g, rows); dev_free(g, nfac); dev_free(g, target); dev_free(g, gmax); dev_free(g, M); dev_free(g, pieces); dev_free(g, shorts);
    }
};

template <typename T>
int pcd_alloc(nsk_graph *g, T **ptr, size_t n, const std::string &who, const char *what) {
    const int rc = dev_alloc(g, ptr, n);
    if (rc != NSK_E_NOMEM) return rc;
    return fail(NSK_E_NOMEM, who + ": " + what + " (" + std::to_string((long long)((n ? n : 1) * sizeof(T))) + " bytes) do not fit on the device");
}

// The work list of ALL weights by slot (nsk_kernels_pcd.h), cut where the statistics cut, and the accumulator.  The
// uploads read host vectors that `keep` holds until the call has synchronised.
struct PcdHost { std::vector<uint2> shorts; std::vector<uint4> pieces; };

int moments_plan(nsk_graph *g, PcdBufs &b, MomentsArgs &a, PcdHost &keep, int nchains, const std::string &what) {
    const NskWstats &ws = g->wstats;
    const size_t nw = (size_t)g->c.nweight;
    std::vector<std::vector<uint64_t>> bylen(NSK_WSTATS_SHORT);       // first factor << 32 | slot, per length
    for (size_t s = 0; s < nw; s++) {
        const uint32_t off = ws.wf_off[s], len = ws.wf_off[s + 1] - off;
        if (len == 0) continue;                     // (reads 0: the accumulator is zeroed)
        if (len <= NSK_WSTATS_SHORT) { bylen[len - 1].push_back((uint64_t)(uint32_t)ws.wf_first[s] << 32 | (uint64_t)s); continue; }
        for (uint32_t k = 0; k < len; k += NSK_WSTATS_PIECE)
            keep.pieces.push_back(make_uint4(off + k, std::min<uint32_t>(NSK_WSTATS_PIECE, len - k), (uint32_t)s, 0u));
    }
    a = MomentsArgs();
    for (int k = 0; k < NSK_WSTATS_SHORT; k++) {
        std::sort(bylen[(size_t)k].begin(), bylen[(size_t)k].end());
        for (uint64_t key : bylen[(size_t)k]) { const uint32_t s = (uint32_t)(key & 0xffffffffu); keep.shorts.push_back(make_uint2(ws.wf_off[s], s)); }
        a.len_end[k] = (unsigned int)keep.shorts.size();
        std::vector<uint64_t>().swap(bylen[(size_t)k]);
    }
    int rc = pcd_alloc(g, &b.M, nw, what, "the int64 sums, 8 bytes a weight");
    if (!rc && !keep.shorts.empty()) rc = dev_upload(g, &b.shorts, keep.shorts);
    if (!rc && !keep.pieces.empty()) rc = dev_upload(g, &b.pieces, keep.pieces);
    if (rc == NSK_E_NOMEM)
        return fail(NSK_E_NOMEM, what + ": the work list of the weights (" + std::to_string((long long)(keep.shorts.size() * 8 + keep.pieces.size() * 16)) +
                                 " bytes) does not fit on the device");
    if (rc) return rc;
    a.e = energy_args(g);
    a.wf_idx = ws.wf_idx;
    a.shorts = b.shorts; a.pieces = b.pieces;
    a.nshort = (long long)keep.shorts.size(); a.npiece = (long long)keep.pieces.size();
    a.nchains = nchains;
    return NSK_OK;
}

template <typename VT>
void moments_launch(nsk_graph *g, const MomentsArgs &a, const void *val, unsigned long long *M, int cap) {
    const dim3 block(NSK_BLOCK);
    if (a.nshort > 0) {
        const unsigned int nb = nsk_moments_blocks(a.nshort, NSK_BLOCK, cap);
        k_moments_short<VT><<<dim3(nb, nsk_moments_chain_groups(nb, a.nchains)), block, 0, g->stream>>>(a, (const VT *)val, M);
    }
    if (a.npiece > 0) {
        const unsigned int nb = nsk_moments_blocks(a.npiece, NSK_BLOCK / 64, cap);
        k_moments_piece<VT><<<dim3(nb, nsk_moments_chain_groups(nb, a.nchains)), block, 0, g->stream>>>(a, (const VT *)val, M);
    }
}

// zero the sums, then up to two launches; not counted by the profiling bracket (sweep kernels only)
hipError_t moments_enqueue(nsk_graph *g, const MomentsArgs &a, const void *val, unsigned long long *M, int cap) {
    const hipError_t e = hipMemsetAsync(M, 0, (size_t)std::max<int64_t>(1, g->c.nweight) * sizeof(unsigned long long), g->stream);
    if (e != hipSuccess) return e;
    if (g->c.vbytes == 4) moments_launch<int32_t>(g, a, val, M, cap);
    else moments_launch<int8_t>(g, a, val, M, cap);
    return hipGetLastError();
}

// (diagnostic, NSK_DIAG=1 NSK_MOMENTS_GRID_CAP=blocks, read at each call: small grids, later trips)
int moments_cap() {
    const char *env = nsk::diag_env("NSK_MOMENTS_GRID_CAP");
    return env ? std::max(1, std::min(1 << 20, atoi(env))) : 0;
}

}  // namespace

int nsk_moments_range(const nsk_graph *g, int64_t nchains, const char *what) { return moments_range(g, nchains, what); }

extern "C" {

int nsk_weight_moments(nsk_graph *g, int which, int64_t first_chain, int64_t nchains, int64_t *moments) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!moments) return fail(NSK_E_INVALID, "null argument");
    if (which != NSK_BUF_VALUE && which != NSK_BUF_VALUE_EVID) return fail(NSK_E_INVALID, "nsk_weight_moments: which must be NSK_BUF_VALUE or NSK_BUF_VALUE_EVID");
    const int64_t R = which == NSK_BUF_VALUE ? g->nchains : 1;
    if (first_chain < 0 || nchains < 1 || first_chain >= R || nchains > R - first_chain)
        return fail(NSK_E_INVALID, "nsk_weight_moments: chains outside those the handle has (the evidence chain exists once)");
    int rc = energy_whole_graph(g, "nsk_weight_moments");
    if (rc) return rc;
    const Compiled &c = g->c;
    if (c.nweight == 0) return NSK_OK;
    if ((rc = moments_range(g, nchains, "nsk_weight_moments"))) return rc;
    HIPCHECK(hipSetDevice(g->device));
    if ((rc = energy_ensure(g, 0, "nsk_weight_moments"))) return rc;
    if ((rc = nsk_wstats_ensure(g, false, "nsk_weight_moments"))) return rc;
    // a tally kept in bits 1-7 of the value bytes goes back to its array first: the walk sees plain values
    if ((rc = nsk_unpack_tally(g))) return rc;
    PcdBufs b(g);
    MomentsArgs a;
    PcdHost keep;
    if ((rc = moments_plan(g, b, a, keep, (int)nchains, "nsk_weight_moments"))) { (void)hipStreamSynchronize(g->stream); return rc; }
    const size_t nw = (size_t)c.nweight;
    const char *val = which == NSK_BUF_VALUE ? (const char *)g->val + (size_t)first_chain * g->chain_stride : (const char *)g->val_evid;
    std::vector<long long> host(nw);
    hipError_t e = moments_enqueue(g, a, val, b.M, moments_cap());
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), b.M, nw * sizeof(long long), hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);      // (also: the uploads read the work list's vectors)
    HIPCHECK(e);
    HIPCHECK(e2);
    // slots -> the caller's weight ids, as nsk_state_download maps the weights
    const int32_t *wmap = c.wmap.empty() ? nullptr : c.wmap.data();
    for (size_t i = 0; i < nw; i++) moments[i] = (int64_t)host[wmap ? (size_t)wmap[i] : i];
    return NSK_OK;
}

int nsk_pcd_steps(nsk_graph *g, const double *target, int64_t nsteps, int64_t sweeps_per_step, int sample_evidence,
                  double step, double decay, double reg_param, int normalize, double *gmax, int64_t *moments) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!target) return fail(NSK_E_INVALID, "null argument");
    if (nsteps < 1 || nsteps > 65536) return fail(NSK_E_INVALID, "nsk_pcd_steps: nsteps must lie in [1, 65536]");
    if (sweeps_per_step < 1 || sweeps_per_step > INT32_MAX / nsteps)
        return fail(NSK_E_INVALID, "nsk_pcd_steps: sweeps_per_step must be at least 1 and nsteps x sweeps_per_step at most 2^31 - 1");
    if (!std::isfinite(step) || !std::isfinite(decay) || !std::isfinite(reg_param) || reg_param < 0.0)
        return fail(NSK_E_INVALID, "nsk_pcd_steps: step, decay and reg_param must be finite, reg_param not negative");
    if (normalize != 0 && normalize != 1) return fail(NSK_E_INVALID, "nsk_pcd_steps: normalize must be 0 or 1");
    if (g->scan != NSK_SCAN_CHROMATIC) return fail(NSK_E_INVALID, "nsk_pcd_steps: the sequential scan is not served");
    int rc = energy_whole_graph(g, "nsk_pcd_steps");
    if (rc) return rc;
    const Compiled &c = g->c;
    const size_t nw = (size_t)c.nweight, T = (size_t)nsteps;
    for (size_t i = 0; i < nw; i++)
        if (!std::isfinite(target[i])) return fail(NSK_E_INVALID, "nsk_pcd_steps: the target of weight " + std::to_string((long long)i) + " is not finite");
    if (nw == 0) return NSK_OK;
    const int R = g->nchains;
    if ((rc = moments_range(g, R, "nsk_pcd_steps"))) return rc;
    HIPCHECK(hipSetDevice(g->device));
    if ((rc = energy_ensure(g, 0, "nsk_pcd_steps"))) return rc;
    if ((rc = nsk_wstats_ensure(g, false, "nsk_pcd_steps"))) return rc;
    // a tally kept in bits 1-7 of the value bytes goes back to its array first, as in nsk_tempered_sweeps
    if ((rc = nsk_unpack_tally(g))) return rc;

    PcdBufs b(g);
    MomentsArgs a;
    PcdHost keep;
    // the target and the factor counts by slot (w_fixed is by slot too: a renumbered weight is a direct one, never fixed)
    const NskWstats &ws = g->wstats;
    const int32_t *wmap = c.wmap.empty() ? nullptr : c.wmap.data();
    std::vector<double> tgt(nw), nfac(nw);
    for (size_t i = 0; i < nw; i++) tgt[wmap ? (size_t)wmap[i] : i] = target[i];
    for (size_t s = 0; s < nw; s++) { const uint32_t n = ws.wf_off[s + 1] - ws.wf_off[s]; nfac[s] = n ? (double)n : 1.0; }
    rc = moments_plan(g, b, a, keep, R, "nsk_pcd_steps");
    if (!rc) rc = pcd_alloc(g, &b.target, nw, "nsk_pcd_steps", "the target, 8 bytes a weight");
    if (!rc) rc = pcd_alloc(g, &b.nfac, nw, "nsk_pcd_steps", "the factor counts, 8 bytes a weight");
    if (!rc) rc = pcd_alloc(g, &b.gmax, T, "nsk_pcd_steps", "the largest gradients, 8 bytes a step");
    if (!rc && moments) rc = pcd_alloc(g, &b.rows, T * nw, "nsk_pcd_steps", "the kept moments, nsteps x nweight int64");
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(b.target, tgt.data(), nw * sizeof(double), hipMemcpyHostToDevice, g->stream);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(b.nfac, nfac.data(), nw * sizeof(double), hipMemcpyHostToDevice, g->stream);
    if (!rc && e == hipSuccess) e = hipMemsetAsync(b.gmax, 0, T * sizeof(unsigned long long), g->stream);
    if (rc || e != hipSuccess) { (void)hipStreamSynchronize(g->stream); if (rc) return rc; HIPCHECK(e); }

    const int cap = moments_cap();
    const unsigned wblocks = (unsigned)((nw + NSK_BLOCK - 1) / NSK_BLOCK);
    double st = step;           // step_0 = step, step_{t+1} = step_t * decay: the products are formed here, in t order
    for (size_t t = 0; t < T && !rc && e == hipSuccess; t++) {
        // 1. sweep: what a burn-in call enqueues (nothing tallied, no trace row); it refreshes what derives from the weights
        if ((rc = nsk_gibbs_sweeps(g, sweeps_per_step, sample_evidence, 1))) break;
        // 2. the moments of all chains
        if ((e = moments_enqueue(g, a, g->val, b.M, cap)) != hipSuccess) break;
        // 3. the update
        k_pcd_update<<<dim3(wblocks), dim3(NSK_BLOCK), 0, g->stream>>>((const long long *)b.M, b.target, b.nfac, (double)R, (int)nw, g->w, g->w_fixed,
                                                                      normalize, st, reg_param, b.gmax + t, b.rows ? b.rows + t * nw : nullptr);
        e = hipGetLastError();
        g->weights_dirty = true;            // the next sweep call rebuilds what derives from the weights
        st = st * decay;
    }
    std::vector<unsigned long long> hmax(T);
    std::vector<long long> hrows(b.rows ? T * nw : 0);
    const bool ok = !rc && e == hipSuccess;
    if (ok) e = hipMemcpyAsync(hmax.data(), b.gmax, T * sizeof(unsigned long long), hipMemcpyDeviceToHost, g->stream);
    if (ok && b.rows && e == hipSuccess) e = hipMemcpyAsync(hrows.data(), b.rows, T * nw * sizeof(long long), hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);      // (also: the uploads read the host vectors)
    if (rc) return rc;
    HIPCHECK(e);
    HIPCHECK(e2);
    if (gmax) std::memcpy(gmax, hmax.data(), T * sizeof(double));
    if (moments)
        for (size_t t = 0; t < T; t++)
            for (size_t i = 0; i < nw; i++) moments[t * nw + i] = (int64_t)hrows[t * nw + (wmap ? (size_t)wmap[i] : i)];
    return NSK_OK;
}

int nsk_pcd_latent_steps(nsk_graph *g, int64_t nclamped, int clamp, int64_t nsteps, int64_t sweeps_per_step, int free_sample_evidence,
                         double step, double decay, double reg_param, int normalize, double *gmax, int64_t *moments) {
    const char *who = "nsk_pcd_latent_steps";
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (nsteps < 1 || nsteps > 65536) return fail(NSK_E_INVALID, "nsk_pcd_latent_steps: nsteps must lie in [1, 65536]");
    if (sweeps_per_step < 1 || sweeps_per_step > INT32_MAX / (2 * nsteps))
        return fail(NSK_E_INVALID, "nsk_pcd_latent_steps: sweeps_per_step must be at least 1 and 2 x nsteps x sweeps_per_step at most 2^31 - 1");
    if (!std::isfinite(step) || !std::isfinite(decay) || !std::isfinite(reg_param) || reg_param < 0.0)
        return fail(NSK_E_INVALID, "nsk_pcd_latent_steps: step, decay and reg_param must be finite, reg_param not negative");
    if (normalize != 0 && normalize != 1) return fail(NSK_E_INVALID, "nsk_pcd_latent_steps: normalize must be 0 or 1");
    if (clamp != 0 && clamp != 1) return fail(NSK_E_INVALID, "nsk_pcd_latent_steps: clamp must be 0 or 1");
    if (g->scan != NSK_SCAN_CHROMATIC) return fail(NSK_E_INVALID, "nsk_pcd_latent_steps: the sequential scan is not served");
    int rc = energy_whole_graph(g, who);
    if (rc) return rc;
    const int R = g->nchains;
    if (nclamped < 1 || nclamped > R - 1)
        return fail(NSK_E_INVALID, "nsk_pcd_latent_steps: nclamped must lie in [1, chains - 1]: a clamped and a free population, each of at least one "
                                   "chain (nsk_set_chains)");
    const Compiled &c = g->c;
    const size_t nw = (size_t)c.nweight, T = (size_t)nsteps;
    if (nw == 0) return NSK_OK;
    const int K = (int)nclamped, F = R - K;
    if ((rc = moments_range(g, std::max(K, F), who))) return rc;
    HIPCHECK(hipSetDevice(g->device));
    if ((rc = energy_ensure(g, 0, who))) return rc;
    if ((rc = nsk_wstats_ensure(g, false, who))) return rc;
    // a tally kept in bits 1-7 of the value bytes goes back to its array first, as in nsk_pcd_steps
    if ((rc = nsk_unpack_tally(g))) return rc;

    PcdBufs b(g);
    MomentsArgs a;
    PcdHost keep;
    const NskWstats &ws = g->wstats;
    const int32_t *wmap = c.wmap.empty() ? nullptr : c.wmap.data();
    std::vector<double> nfac(nw);
    for (size_t s = 0; s < nw; s++) { const uint32_t n = ws.wf_off[s + 1] - ws.wf_off[s]; nfac[s] = n ? (double)n : 1.0; }
    // the clamp's list: every variable with isEvidence 1, 2 or 3 has a position (only isEvidence 4 has none), whose word
    // names it; its internal id is where its value lies in a chain
    std::vector<int2> pairs;
    bool clamp_regular = true;
    if (clamp)
        for (size_t p = 0; p < (size_t)c.npos; p++) {
            const int64_t v = c.p_vid[p];
            const uint32_t ev = v >= 0 ? (c.p_info[p] & 0xFFu) : 0u;
            if (ev < 1u || ev > 3u) continue;
            const int32_t x = c.v_init[(size_t)v];
            pairs.push_back(make_int2(c.iid[(size_t)v], x));
            if (x < 0 || x >= c.v_card[(size_t)v]) clamp_regular = false;
        }
    rc = moments_plan(g, b, a, keep, K, who);
    if (!rc) rc = pcd_alloc(g, &b.Mf, nw, who, "the free chains' int64 sums, 8 bytes a weight");
    if (!rc) rc = pcd_alloc(g, &b.nfac, nw, who, "the factor counts, 8 bytes a weight");
    if (!rc) rc = pcd_alloc(g, &b.gmax, T, who, "the largest gradients, 8 bytes a step");
    if (!rc && moments) rc = pcd_alloc(g, &b.rows, T * 2 * nw, who, "the kept moments, nsteps x 2 x nweight int64");
    if (!rc && !pairs.empty()) rc = pcd_alloc(g, &b.pairs, pairs.size(), who, "the clamp's list, 8 bytes an evidence variable");
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(b.nfac, nfac.data(), nw * sizeof(double), hipMemcpyHostToDevice, g->stream);
    if (!rc && e == hipSuccess) e = hipMemsetAsync(b.gmax, 0, T * sizeof(unsigned long long), g->stream);
    if (!rc && e == hipSuccess && b.pairs) e = hipMemcpyAsync(b.pairs, pairs.data(), pairs.size() * sizeof(int2), hipMemcpyHostToDevice, g->stream);
    if (rc || e != hipSuccess) { (void)hipStreamSynchronize(g->stream); if (rc) return rc; HIPCHECK(e); }

    // the clamp: one launch over the clamped chains; their values lie in their domains afterwards where they did before
    // and every initial value written does
    if (b.pairs) {
        const long long np = (long long)pairs.size();
        const unsigned nb = (unsigned)std::min<long long>(NSK_MOMENTS_MAX_BLOCKS, (np + NSK_BLOCK - 1) / NSK_BLOCK);
        const dim3 grid(nb, nsk_moments_chain_groups(nb, K));
        if (c.vbytes == 4) k_pcd_clamp<int32_t><<<grid, dim3(NSK_BLOCK), 0, g->stream>>>((int32_t *)g->val, (long long)g->chain_stride, K, b.pairs, np);
        else k_pcd_clamp<int8_t><<<grid, dim3(NSK_BLOCK), 0, g->stream>>>((int8_t *)g->val, (long long)g->chain_stride, K, b.pairs, np);
        e = hipGetLastError();
        if (!clamp_regular) {
            g->chain_regular[0] = false;
            if (K > 1) g->chains_regular = false;
            g->values_regular = false;
        }
    }

    MomentsArgs af = a;             // the same work list over the free chains
    af.nchains = F;
    const char *val_free = (const char *)g->val + (size_t)K * g->chain_stride;
    const int cap = moments_cap();
    const unsigned wblocks = (unsigned)((nw + NSK_BLOCK - 1) / NSK_BLOCK);
    double st = step;           // step_0 = step, step_{t+1} = step_t * decay: the products are formed here, in t order
    for (size_t t = 0; t < T && !rc && e == hipSuccess; t++) {
        // 1. the clamped phase: a burn-in call through the view [0, K); it refreshes what derives from the weights
        { ChainRange view(g, 0, K); rc = nsk_gibbs_sweeps(g, sweeps_per_step, 0, 1); }
        if (rc) break;
        // 2. the free phase, through the view [K, R), at the sweep indices that follow
        { ChainRange view(g, K, F); rc = nsk_gibbs_sweeps(g, sweeps_per_step, free_sample_evidence ? 1 : 0, 1); }
        if (rc) break;
        // 3. the moments of each population
        if ((e = moments_enqueue(g, a, g->val, b.M, cap)) != hipSuccess) break;
        if ((e = moments_enqueue(g, af, val_free, b.Mf, cap)) != hipSuccess) break;
        // 4. the update
        k_pcd_latent_update<<<dim3(wblocks), dim3(NSK_BLOCK), 0, g->stream>>>((const long long *)b.M, (const long long *)b.Mf, b.nfac, (double)K, (double)F,
                                                                             (int)nw, g->w, g->w_fixed, normalize, st, reg_param, b.gmax + t,
                                                                             b.rows ? b.rows + t * 2 * nw : nullptr);
        e = hipGetLastError();
        g->weights_dirty = true;            // the next sweep call rebuilds what derives from the weights
        st = st * decay;
    }
    std::vector<unsigned long long> hmax(T);
    std::vector<long long> hrows(b.rows ? T * 2 * nw : 0);
    const bool ok = !rc && e == hipSuccess;
    if (ok) e = hipMemcpyAsync(hmax.data(), b.gmax, T * sizeof(unsigned long long), hipMemcpyDeviceToHost, g->stream);
    if (ok && b.rows && e == hipSuccess) e = hipMemcpyAsync(hrows.data(), b.rows, T * 2 * nw * sizeof(long long), hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);      // (also: the uploads read the host vectors)
    if (rc) return rc;
    HIPCHECK(e);
    HIPCHECK(e2);
    if (gmax) std::memcpy(gmax, hmax.data(), T * sizeof(double));
    if (moments)
        for (size_t t = 0; t < 2 * T; t++)
            for (size_t i = 0; i < nw; i++) moments[t * nw + i] = (int64_t)hrows[t * nw + (wmap ? (size_t)wmap[i] : i)];
    return NSK_OK;
}

}  // extern "C"
