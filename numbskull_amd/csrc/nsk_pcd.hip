// nsk_pcd.hip -- the chain-summed per-weight moments and persistent contrastive divergence (nsk_kernels_pcd.h): the entry
// points nsk_weight_moments and nsk_pcd_steps.  They read the records of the factor walk and the by-weight list of the
// statistics (nsk_wstats.hip nsk_wstats_ensure); the work list, the int64 sums, the target, the factor counts and the
// per-step outputs live for the call only.  nsk_pcd_steps and nsk_pcd_latent_steps check their own arguments and run
// through pcd_run: per step (the burn-in sweeps of nsk_gibbs_sweeps, zero the sums, the moment launches, k_pcd_update)
// on the handle's stream without a host wait, one synchronisation at the end.  nsk_pcd_steps has one population, the
// handle's chains, and a fixed target; nsk_pcd_latent_steps two, clamped and free, each swept through a ChainRange view
// (nsk_internal.h), each with its own sums, and the update takes its target from the clamped ones.
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
    unsigned long long *M = nullptr;
    double *target = nullptr, *nfac = nullptr;
    unsigned long long *Mf = nullptr;      // nsk_pcd_latent_steps: the free chains' sums (M holds the clamped chains')
    int2 *pairs = nullptr;                 // ... and the clamp's {internal id, value} list
    explicit PcdBufs(nsk_graph *g_) : g(g_) {}
    ~PcdBufs() { dev_free(g, pairs); dev_free(g, Mf); dev_free(g, nfac); dev_free(g, target); dev_free(g, M); dev_free(g, pieces); dev_free(g, shorts); }
};

// The work list of ALL weights by slot (nsk_kernels_pcd.h) from the statistics' cut (nsk_steps.h weight_cut: the list of
// every slot, so a tag is a slot; a weight without a factor reads 0, the accumulator is zeroed), and the accumulator.
// The uploads read host vectors that `keep` holds until the call has synchronised.
struct PcdHost { std::vector<WeightCutShort> shorts; std::vector<WeightItem> pieces; };
static_assert(sizeof(WeightCutShort) == sizeof(uint2) && sizeof(WeightItem) == sizeof(uint4), "the items are uploaded as they are");

int moments_plan(nsk_graph *g, PcdBufs &b, MomentsArgs &a, PcdHost &keep, int nchains, const std::string &what) {
    const NskWstats &ws = g->wstats;
    const size_t nw = (size_t)g->c.nweight;
    std::vector<int32_t> slots(nw);
    for (size_t s = 0; s < nw; s++) slots[s] = (int32_t)s;
    WeightCut cut = weight_cut(ws.wf_off, ws.wf_first, slots.data(), nw, NSK_WSTATS_SHORT);
    keep.pieces = moments_items(cut, NSK_WSTATS_PIECE);
    keep.shorts.swap(cut.shorts);
    a = MomentsArgs();
    std::copy(cut.len_end.begin(), cut.len_end.end(), a.len_end);
    int rc = call_alloc(g, &b.M, nw, what, "the int64 sums, 8 bytes a weight");
    if (!rc && !keep.shorts.empty()) rc = dev_upload(g, (WeightCutShort **)&b.shorts, keep.shorts);
    if (!rc && !keep.pieces.empty()) rc = dev_upload(g, (WeightItem **)&b.pieces, keep.pieces);
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

// What nsk_pcd_steps and nsk_pcd_latent_steps ask of pcd_run, their own arguments checked.  One population, the whole
// handle, moves the weights towards `target` (by the caller's weight id); of two, each swept through a ChainRange view,
// the first is the clamped one, whose mean is the target, and with `clamp` gets its evidence written first.
struct PcdPop { int first, count, sample_evidence; };
struct PcdCall {
    const char *who;
    int npop;
    PcdPop pop[2];
    const double *target;
    bool clamp;
};

int pcd_run(nsk_graph *g, const PcdCall &call, int64_t nsteps, int64_t sweeps_per_step, double step, double decay, double reg_param, int normalize,
            double *gmax, int64_t *moments) {
    const char *who = call.who;
    const Compiled &c = g->c;
    const size_t nw = (size_t)c.nweight, T = (size_t)nsteps;
    if (nw == 0) return NSK_OK;
    const bool latent = call.npop == 2;
    const PcdPop &model = call.pop[call.npop - 1];          // the chains whose mean the update subtracts
    int rc = moments_range(g, std::max(call.pop[0].count, model.count), who);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(g->device));
    if ((rc = energy_ensure(g, 0, who))) return rc;
    if ((rc = nsk_wstats_ensure(g, false, who))) return rc;
    // a tally kept in bits 1-7 of the value bytes goes back to its array first, as in nsk_tempered_sweeps
    if ((rc = nsk_unpack_tally(g))) return rc;

    PcdBufs b(g);
    StepOutputs out(g, T, (size_t)call.npop);
    MomentsArgs a;
    PcdHost keep;
    // the target and the factor counts by slot
    std::vector<double> tgt(call.target ? nw : 0);
    if (call.target) SlotMap(c).to_slots(call.target, tgt.data());
    const std::vector<double> nfac = factors_per_slot(c);
    // the clamp's list: every variable with isEvidence 1, 2 or 3 has a position (only isEvidence 4 has none), whose word
    // names it; its internal id is where its value lies in a chain
    std::vector<int2> pairs;
    bool clamp_regular = true;
    if (call.clamp)
        for (size_t p = 0; p < (size_t)c.npos; p++) {
            const int64_t v = c.p_vid[p];
            const uint32_t ev = v >= 0 ? (c.p_info[p] & 0xFFu) : 0u;
            if (ev < 1u || ev > 3u) continue;
            const int32_t x = c.v_init[(size_t)v];
            pairs.push_back(make_int2(c.iid[(size_t)v], x));
            if (x < 0 || x >= c.v_card[(size_t)v]) clamp_regular = false;
        }
    rc = moments_plan(g, b, a, keep, call.pop[0].count, who);
    if (!rc && latent) rc = call_alloc(g, &b.Mf, nw, who, "the free chains' int64 sums, 8 bytes a weight");
    if (!rc && call.target) rc = call_alloc(g, &b.target, nw, who, "the target, 8 bytes a weight");
    if (!rc) rc = call_alloc(g, &b.nfac, nw, who, "the factor counts, 8 bytes a weight");
    if (!rc) rc = out.alloc_gmax(who);
    if (!rc && moments) rc = out.alloc_rows(who);
    if (!rc && !pairs.empty()) rc = call_alloc(g, &b.pairs, pairs.size(), who, "the clamp's list, 8 bytes an evidence variable");
    hipError_t e = hipSuccess;
    if (!rc && b.target) e = hipMemcpyAsync(b.target, tgt.data(), nw * sizeof(double), hipMemcpyHostToDevice, g->stream);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(b.nfac, nfac.data(), nw * sizeof(double), hipMemcpyHostToDevice, g->stream);
    if (!rc && e == hipSuccess) e = out.zero();
    if (!rc && e == hipSuccess && b.pairs) e = hipMemcpyAsync(b.pairs, pairs.data(), pairs.size() * sizeof(int2), hipMemcpyHostToDevice, g->stream);
    if (rc || e != hipSuccess) { (void)hipStreamSynchronize(g->stream); if (rc) return rc; HIPCHECK(e); }

    // the clamp: one launch over the clamped chains (the handle's first); their values lie in their domains afterwards
    // where they did before and every initial value written does
    if (b.pairs) {
        const int K = call.pop[0].count;
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

    MomentsArgs am = a;             // the same work list over the model's chains
    am.nchains = model.count;
    const char *val_model = (const char *)g->val + (size_t)model.first * g->chain_stride;
    unsigned long long *Mm = latent ? b.Mf : b.M;
    const int cap = moments_cap();
    const unsigned wblocks = (unsigned)((nw + NSK_BLOCK - 1) / NSK_BLOCK);
    double st = step;           // step_0 = step, step_{t+1} = step_t * decay: the products are formed here, in t order
    for (size_t t = 0; t < T && !rc && e == hipSuccess; t++) {
        // 1. sweep: what a burn-in call enqueues (nothing tallied, no trace row); it refreshes what derives from the
        //    weights.  Two populations: the clamped phase through its view, then the free one at the sweep indices that follow
        for (int p = 0; p < call.npop && !rc; p++) {
            const PcdPop &pop = call.pop[p];
            if (latent) { ChainRange view(g, pop.first, pop.count); rc = nsk_gibbs_sweeps(g, sweeps_per_step, pop.sample_evidence, 1); }
            else rc = nsk_gibbs_sweeps(g, sweeps_per_step, pop.sample_evidence, 1);
        }
        if (rc) break;
        // 2. the moments of each population
        if (latent && (e = moments_enqueue(g, a, g->val, b.M, cap)) != hipSuccess) break;
        if ((e = moments_enqueue(g, am, val_model, Mm, cap)) != hipSuccess) break;
        // 3. the update
        k_pcd_update<<<dim3(wblocks), dim3(NSK_BLOCK), 0, g->stream>>>((const long long *)Mm, (double)model.count, latent ? (const long long *)b.M : nullptr,
                                                                      (double)call.pop[0].count, b.target, b.nfac, (int)nw, g->w, g->w_fixed, normalize,
                                                                      st, reg_param, out.gmax + t, out.row(t));
        e = hipGetLastError();
        g->weights_dirty = true;            // the next sweep call rebuilds what derives from the weights
        st = st * decay;
    }
    const bool ok = !rc && e == hipSuccess;
    if (ok) e = out.download();
    const hipError_t e2 = hipStreamSynchronize(g->stream);      // (also: the uploads read the host vectors)
    if (rc) return rc;
    HIPCHECK(e);
    HIPCHECK(e2);
    out.deliver(gmax, moments);
    return NSK_OK;
}

}  // namespace

int nsk_moments_range(const nsk_graph *g, int64_t nchains, const char *what) { return moments_range(g, nchains, what); }

extern "C" {

int nsk_weight_moments(nsk_graph *g, int which, int64_t first_chain, int64_t nchains, int64_t *moments) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!moments) return fail(NSK_E_INVALID, "null argument");
    int rc = chain_select(g, which, first_chain, nchains, "nsk_weight_moments");
    if (!rc) rc = energy_whole_graph(g, "nsk_weight_moments");
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
    std::vector<long long> host(nw);
    hipError_t e = moments_enqueue(g, a, chain_val(g, which, first_chain), b.M, moments_cap());
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), b.M, nw * sizeof(long long), hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);      // (also: the uploads read the work list's vectors)
    HIPCHECK(e);
    HIPCHECK(e2);
    // slots -> the caller's weight ids, as nsk_state_download maps the weights
    SlotMap(c).from_slots(host.data(), moments);
    return NSK_OK;
}

int nsk_pcd_steps(nsk_graph *g, const double *target, int64_t nsteps, int64_t sweeps_per_step, int sample_evidence,
                  double step, double decay, double reg_param, int normalize, double *gmax, int64_t *moments) {
    const char *who = "nsk_pcd_steps";
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!target) return fail(NSK_E_INVALID, "null argument");
    int rc = refuse(check_nsteps(who, nsteps, 65536));
    if (rc) return rc;
    if (sweeps_per_step < 1 || sweeps_per_step > INT32_MAX / nsteps)
        return fail(NSK_E_INVALID, "nsk_pcd_steps: sweeps_per_step must be at least 1 and nsteps x sweeps_per_step at most 2^31 - 1");
    if ((rc = refuse(check_rates(who, step, decay, reg_param)))) return rc;
    if ((rc = refuse(check_normalize(who, normalize)))) return rc;
    if (g->scan != NSK_SCAN_CHROMATIC) return fail(NSK_E_INVALID, "nsk_pcd_steps: the sequential scan is not served");
    if ((rc = energy_whole_graph(g, who))) return rc;
    if ((rc = refuse(check_target(who, target, (size_t)g->c.nweight)))) return rc;
    const PcdCall call = {who, 1, {{0, g->nchains, sample_evidence}, {}}, target, false};
    return pcd_run(g, call, nsteps, sweeps_per_step, step, decay, reg_param, normalize, gmax, moments);
}

int nsk_pcd_latent_steps(nsk_graph *g, int64_t nclamped, int clamp, int64_t nsteps, int64_t sweeps_per_step, int free_sample_evidence,
                         double step, double decay, double reg_param, int normalize, double *gmax, int64_t *moments) {
    const char *who = "nsk_pcd_latent_steps";
    if (!g) return fail(NSK_E_INVALID, "null graph");
    int rc = refuse(check_nsteps(who, nsteps, 65536));
    if (rc) return rc;
    if (sweeps_per_step < 1 || sweeps_per_step > INT32_MAX / (2 * nsteps))
        return fail(NSK_E_INVALID, "nsk_pcd_latent_steps: sweeps_per_step must be at least 1 and 2 x nsteps x sweeps_per_step at most 2^31 - 1");
    if ((rc = refuse(check_rates(who, step, decay, reg_param)))) return rc;
    if ((rc = refuse(check_normalize(who, normalize)))) return rc;
    if (clamp != 0 && clamp != 1) return fail(NSK_E_INVALID, "nsk_pcd_latent_steps: clamp must be 0 or 1");
    if (g->scan != NSK_SCAN_CHROMATIC) return fail(NSK_E_INVALID, "nsk_pcd_latent_steps: the sequential scan is not served");
    if ((rc = energy_whole_graph(g, who))) return rc;
    const int R = g->nchains;
    if (nclamped < 1 || nclamped > R - 1)
        return fail(NSK_E_INVALID, "nsk_pcd_latent_steps: nclamped must lie in [1, chains - 1]: a clamped and a free population, each of at least one "
                                   "chain (nsk_set_chains)");
    const int K = (int)nclamped;
    const PcdCall call = {who, 2, {{0, K, 0}, {K, R - K, free_sample_evidence ? 1 : 0}}, nullptr, clamp != 0};
    return pcd_run(g, call, nsteps, sweeps_per_step, step, decay, reg_param, normalize, gmax, moments);
}

}  // extern "C"
