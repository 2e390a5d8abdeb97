// nsk_bp.hip -- loopy belief propagation (nsk_internal.h NskBp, nsk_kernels_bp.h): nsk_bp_setup takes the structure of one
// state from nsk_bp_plan.h (which variables are clamped, every factor's distinct members, table axes, directed edges, the
// per-variable edge lists: pure host arithmetic over the compiled records), uploads it and fills the tables; nsk_bp_run
// enqueues every iteration on the handle's stream without a synchronisation between them -- once the residual is at or
// below the tolerance the later launches end on the device -- and copies the residuals back once.  The launches are not
// counted by the profiling bracket.
// Learning by BP on the resident set-up: nsk_bp_refresh rewrites theta and psi from the device weights through the feature
// table the set-up keeps, nsk_bp_moments reduces the expected per-weight statistics under the factor beliefs in int64 fixed
// point, and nsk_bp_learn_steps enqueues (refresh, iterations, moments, nsk_pcd.hip's update with one chain) per step
// without a host wait, as nsk_pcd_steps does; the sums, the target and the per-step outputs live for the call only.
// A handle holds two set-ups (nsk_bp_select swaps the selected one in; everything above acts on it alone), and
// nsk_bp_latent_steps learns from their difference, evidence clamped and free: the same steps with both set-ups in the
// same launches (the pair kernels of nsk_kernels_bp.h) and nsk_pcd_latent_steps' update with one chain a side.  Both
// learners are bp_steps_run, with n = 1 or 2 set-ups.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "nsk_bp_plan.h"
#include "nsk_internal.h"
#include "nsk_kernels_bp.h"
#include "nsk_kernels_pcd.h"     // k_pcd_update

using namespace nsk;

// (diagnostic, NSK_DIAG=1 NSK_BP_GRID_CAP=blocks, read at each call: small grids, later trips)
static unsigned int bp_blocks(long long items, int block = NSK_BLOCK) {
    long long limit = NSK_BP_MAX_BLOCKS;
    if (const char *env = nsk::diag_env("NSK_BP_GRID_CAP")) {
        const long long cap = atoll(env);
        if (cap > 0 && cap < limit) limit = cap;
    }
    const long long need = (items + block - 1) / block;
    return (unsigned int)std::max<long long>(1, std::min(need, limit));
}

static void bp_free(nsk_graph *g) {
    NskBp &b = g->bp;
    for (void *p : b.owned) dev_free(g, p);
    b = NskBp();
}

static BpArgs bp_args(const nsk_graph *g, const NskBp &b) {
    BpArgs a = {};
    a.f_rec = (const uint4 *)g->f_rec; a.mrec = (const int2 *)b.mrec; a.pm_off = b.pm_off;
    a.slot_off = b.slot_off; a.slot_rec = (const int2 *)b.slot_rec;
    a.tab_off = b.tab_off; a.edge_off = b.edge_off; a.e_fac = b.e_fac; a.msg_off = b.msg_off;
    a.v_list = b.v_list; a.v_eoff = b.v_eoff; a.v_edges = b.v_edges;
    a.b_off = b.d_b_off; a.v_state = b.v_state; a.v_card = g->v_card;
    a.w = g->w; a.logtab = g->logtab;
    a.theta = b.theta; a.psi = b.psi; a.f2v = b.f2v; a.v2f = b.v2f; a.belief = b.belief; a.wk = b.wk; a.feat = b.feat;
    a.nfactor = (long long)g->c.nfactor; a.ntable = (long long)b.info.ntable; a.nid = (long long)g->c.nid;
    a.nedge = (int32_t)b.info.nedges; a.nvlist = b.nvlist;
    return a;
}
static BpArgs bp_args(const nsk_graph *g) { return bp_args(g, g->bp); }       // the selected set-up's

// the set-up of a slot, whichever is selected
static NskBp &bp_slot(nsk_graph *g, int slot) { return slot == g->bp_slot ? g->bp : g->bp_other; }

template <typename T>
static int bp_upload(nsk_graph *g, T **ptr, const std::vector<T> &h) {
    int rc = dev_upload(g, ptr, h);
    if (!rc) g->bp.owned.push_back(*ptr);
    return rc;
}
template <typename T>
static int bp_alloc(nsk_graph *g, T **ptr, size_t n) {
    int rc = dev_alloc(g, ptr, n);
    if (!rc) g->bp.owned.push_back(*ptr);
    return rc;
}

static int bp_common(nsk_graph *g, const char *what, bool need_setup) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    int rc = energy_whole_graph(g, what);
    if (rc) return rc;
    if (need_setup && !g->bp.ready) return fail(NSK_E_INVALID, std::string(what) + ": no belief propagation is set up (nsk_bp_setup)");
    return NSK_OK;
}

// theta and psi from the device weight table as it stands; messages and beliefs stay
static void bp_refresh_enqueue(nsk_graph *g, const BpArgs &a) {
    if (a.nfactor == 0) return;
    k_bp_refresh<<<dim3(bp_blocks(a.ntable)), dim3(NSK_BLOCK), 0, g->stream>>>(a);
    k_bp_psi<<<dim3(bp_blocks(a.nfactor)), dim3(NSK_BLOCK), 0, g->stream>>>(a);
}

// max_iters iterations as nsk_bp_run enqueues them, the residuals at res[0 .. max_iters)
static hipError_t bp_iterations_enqueue(nsk_graph *g, const BpArgs &a, size_t max_iters, double damping, double tol, unsigned long long *res) {
    const double oml = 1.0 - damping;
    const int nbin = g->bp.nvbin, nall = a.nvlist;
    const dim3 block(NSK_BLOCK), gf(bp_blocks(a.nedge)), vblock(NSK_BP_VAR_BLOCK),
               gb(bp_blocks(nbin, NSK_BP_VAR_BLOCK)), gr(bp_blocks(nall - nbin, NSK_BP_VAR_BLOCK));
    hipError_t e = hipSuccess;
    if (a.nedge > 0)
        for (size_t t = 0; t < max_iters && e == hipSuccess; t++) {
            k_bp_factor<<<gf, block, 0, g->stream>>>(a, (int)t, tol, damping, oml, res);
            if (nbin > 0) k_bp_var<true><<<gb, vblock, 0, g->stream>>>(a, 0, nbin, (int)t, tol, res);
            if (nall > nbin) k_bp_var<false><<<gr, vblock, 0, g->stream>>>(a, nbin, nall, (int)t, tol, res);
            e = hipGetLastError();
        }
    return e;
}

// zero the sums and the skip counter, then Z_f of every factor and the moment launch
static hipError_t bp_moments_enqueue(nsk_graph *g, const BpArgs &a, double *zf, unsigned long long *M, unsigned long long *skipped) {
    hipError_t e = hipMemsetAsync(M, 0, (size_t)std::max<int64_t>(1, g->c.nweight) * sizeof(unsigned long long), g->stream);
    if (e == hipSuccess) e = hipMemsetAsync(skipped, 0, sizeof(unsigned long long), g->stream);
    if (e != hipSuccess || a.nfactor == 0) return e;
    k_bp_fnorm<<<dim3(bp_blocks(a.nfactor)), dim3(NSK_BLOCK), 0, g->stream>>>(a, zf, skipped);
    k_bp_moments<<<dim3(bp_blocks(a.ntable)), dim3(NSK_BLOCK), 0, g->stream>>>(a, zf, M);
    return hipGetLastError();
}

// ---- both set-ups in the same launches (nsk_bp_latent_steps): what the three routines above enqueue for one set-up, one
// launch for the pair where they have one; gridDim.x is what the larger set-up needs, so NSK_BP_GRID_CAP holds here too
static void bp_refresh_enqueue(nsk_graph *g, const BpPair &p) {
    if (p.a[0].nfactor == 0) return;                // (the factors are the graph's: both set-ups have them or neither)
    const dim3 block(NSK_BLOCK);
    k_bp_refresh2<<<dim3(bp_blocks(std::max(p.a[0].ntable, p.a[1].ntable)), 2), block, 0, g->stream>>>(p);
    k_bp_psi2<<<dim3(bp_blocks(p.a[0].nfactor), 2), block, 0, g->stream>>>(p);
}

// p.res: the step's two rows.  A set-up without an edge stays out of every loop; its row stays 0, as alone.
static hipError_t bp_iterations_enqueue(nsk_graph *g, const BpPair &p, size_t max_iters, double damping, double tol) {
    const double oml = 1.0 - damping;
    const int nedge = std::max(p.a[0].nedge, p.a[1].nedge), nbin = std::max(p.nvbin[0], p.nvbin[1]),
              nrest = std::max(p.a[0].nvlist - p.nvbin[0], p.a[1].nvlist - p.nvbin[1]);
    const dim3 block(NSK_BLOCK), gf(bp_blocks(nedge), 2), vblock(NSK_BP_VAR_BLOCK), gb(bp_blocks(nbin, NSK_BP_VAR_BLOCK), 2),
               gr(bp_blocks(nrest, NSK_BP_VAR_BLOCK), 2);
    hipError_t e = hipSuccess;
    if (nedge > 0)
        for (size_t t = 0; t < max_iters && e == hipSuccess; t++) {
            k_bp_factor2<<<gf, block, 0, g->stream>>>(p, (int)t, tol, damping, oml);
            if (nbin > 0) k_bp_var2<true><<<gb, vblock, 0, g->stream>>>(p, (int)t, tol);
            if (nrest > 0) k_bp_var2<false><<<gr, vblock, 0, g->stream>>>(p, (int)t, tol);
            e = hipGetLastError();
        }
    return e;
}

// p.M[0] and p.M[1] are the halves of one array, p.skipped[0] and [1] neighbours: one memset each
static hipError_t bp_moments_enqueue(nsk_graph *g, const BpPair &p) {
    hipError_t e = hipMemsetAsync(p.M[0], 0, 2 * (size_t)std::max<int64_t>(1, g->c.nweight) * sizeof(unsigned long long), g->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p.skipped[0], 0, 2 * sizeof(unsigned long long), g->stream);
    if (e != hipSuccess || p.a[0].nfactor == 0) return e;
    k_bp_fnorm2<<<dim3(bp_blocks(p.a[0].nfactor), 2), dim3(NSK_BLOCK), 0, g->stream>>>(p);
    k_bp_moments2<<<dim3(bp_blocks(std::max(p.a[0].ntable, p.a[1].ntable)), 2), dim3(NSK_BLOCK), 0, g->stream>>>(p);
    return hipGetLastError();
}

// the device buffers of one call beside its StepOutputs: entered in the ledger, gone when the call returns
struct BpLearnBufs {
    nsk_graph *g;
    unsigned long long *M = nullptr, *skipped = nullptr, *res = nullptr;
    double *zf = nullptr, *target = nullptr, *nfac = nullptr;
    explicit BpLearnBufs(nsk_graph *g_) : g(g_) {}
    ~BpLearnBufs() { dev_free(g, nfac); dev_free(g, target); dev_free(g, zf); dev_free(g, res); dev_free(g, skipped); dev_free(g, M); }
};

// the step parameters both learners take, in the order they are refused
static int bp_steps_check(const std::string &who, int64_t nsteps, int64_t iters_per_step, double damping, double tol, int warm, double step,
                          double decay, double reg_param, int normalize) {
    if (int rc = refuse(check_nsteps(who, nsteps, 4096))) return rc;
    if (iters_per_step < 1 || iters_per_step > 4096) return fail(NSK_E_INVALID, who + ": iters_per_step must lie in [1, 4096]");
    if (nsteps * iters_per_step > 65536) return fail(NSK_E_INVALID, who + ": nsteps x iters_per_step must be at most 65536");
    if (!(damping >= 0.0 && damping < 1.0)) return fail(NSK_E_INVALID, who + ": damping must lie in [0, 1)");
    if (!(tol >= 0.0)) return fail(NSK_E_INVALID, who + ": tol must be at least 0");
    if ((warm != 0 && warm != 1) || (normalize != 0 && normalize != 1)) return fail(NSK_E_INVALID, who + ": warm and normalize must be 0 or 1");
    return refuse(check_rates(who, step, decay, reg_param));
}

// What nsk_bp_learn_steps (n = 1: the selected set-up against `target`, by the caller's weight ids) and nsk_bp_latent_steps
// (n = 2: slot 0 against slot 1, target null) enqueue, their own arguments checked; per step refresh, (reset), iterations,
// moments and k_pcd_update, one synchronisation a call.  Every per-set-up buffer is n x the single one, row (step, set-up).
static int bp_steps_run(nsk_graph *g, const char *who, int n, const double *target, int64_t nsteps, int64_t iters_per_step, double damping,
                        double tol, int warm, double step, double decay, double reg_param, int normalize, double *gmax, int64_t *iters,
                        double *residual, int64_t *moments, int64_t *skipped) {
    const Compiled &c = g->c;
    const size_t N = (size_t)n, nw = (size_t)c.nweight, T = (size_t)nsteps, I = (size_t)iters_per_step, F = (size_t)c.nfactor;
    if (nw == 0) return NSK_OK;
    int rc = nsk_moments_range(g, 1, who);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(g->device));

    // the target and the factor counts by slot
    std::vector<double> tgt(target ? nw : 0);
    if (target) SlotMap(c).to_slots(target, tgt.data());
    const std::vector<double> nfac = factors_per_slot(c);
    BpLearnBufs b(g);
    StepOutputs out(g, T, N);
    rc = call_alloc(g, &b.M, N * nw, who, n == 1 ? "the int64 sums, 8 bytes a weight" : "the int64 sums of both set-ups, 16 bytes a weight");
    if (!rc) rc = call_alloc(g, &b.skipped, N * T, who, n == 1 ? "the skip counters, 8 bytes a step" : "the skip counters, 16 bytes a step");
    if (!rc) rc = call_alloc(g, &b.zf, N * F, who, n == 1 ? "the factors' normalisers, 8 bytes a factor" : "the factors' normalisers of both set-ups, 16 bytes a factor");
    if (!rc && target) rc = call_alloc(g, &b.target, nw, who, "the target, 8 bytes a weight");
    if (!rc) rc = call_alloc(g, &b.nfac, nw, who, "the factor counts, 8 bytes a weight");
    if (!rc) rc = out.alloc_gmax(who);
    if (!rc) rc = call_alloc(g, &b.res, N * T * I, who, n == 1 ? "the residuals, nsteps x iters_per_step doubles" : "the residuals, nsteps x 2 x iters_per_step doubles");
    if (!rc && moments) rc = out.alloc_rows(who);
    if (rc) return rc;
    hipError_t e = target ? hipMemcpyAsync(b.target, tgt.data(), nw * sizeof(double), hipMemcpyHostToDevice, g->stream) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(b.nfac, nfac.data(), nw * sizeof(double), hipMemcpyHostToDevice, g->stream);
    if (e == hipSuccess) e = out.zero();
    if (e == hipSuccess) e = hipMemsetAsync(b.res, 0, N * T * I * sizeof(unsigned long long), g->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(g->stream); HIPCHECK(e); }

    // n = 1 launches the single kernels on the selected set-up (a; p lends it its first pointers), n = 2 the pair kernels
    // on p: index 0 of every pair is the clamped set-up (slot 0), index 1 the free one (slot 1)
    const BpArgs a = bp_args(g);
    BpPair p = {};
    for (int s = 0; s < n; s++) {
        if (n == 2) { p.a[s] = bp_args(g, bp_slot(g, s)); p.nvbin[s] = bp_slot(g, s).nvbin; }
        p.zf[s] = b.zf + (size_t)s * F; p.M[s] = b.M + (size_t)s * nw;
    }
    const int nedge = n == 1 ? a.nedge : std::max(p.a[0].nedge, p.a[1].nedge);
    auto refresh = [&] { if (n == 1) bp_refresh_enqueue(g, a); else bp_refresh_enqueue(g, p); };
    const unsigned wblocks = (unsigned)((nw + NSK_BLOCK - 1) / NSK_BLOCK);
    // the update: nsk_pcd_steps' against the target, or nsk_pcd_latent_steps' (M = {Mc, M}), with one chain a side
    const long long *Mfree = (const long long *)p.M[n - 1], *Mc = n == 1 ? nullptr : (const long long *)p.M[0];
    double st = step;           // step_0 = step, step_{t+1} = step_t * decay: the products are formed here, in t order
    for (size_t t = 0; t < T && e == hipSuccess; t++) {
        for (size_t s = 0; s < N; s++) { p.res[s] = b.res + (N * t + s) * I; p.skipped[s] = b.skipped + N * t + s; }
        // 1. the tables under the weights as they stand; a cold start resets the messages
        refresh();
        if (!warm && nedge > 0) {
            if (n == 1) k_bp_reset<<<dim3(bp_blocks(nedge)), dim3(NSK_BLOCK), 0, g->stream>>>(a);
            else k_bp_reset2<<<dim3(bp_blocks(nedge), 2), dim3(NSK_BLOCK), 0, g->stream>>>(p);
        }
        if ((e = hipGetLastError()) != hipSuccess) break;
        // 2. the iterations, each set-up's early exit inside the step's own row of residuals
        if ((e = n == 1 ? bp_iterations_enqueue(g, a, I, damping, tol, p.res[0]) : bp_iterations_enqueue(g, p, I, damping, tol)) != hipSuccess) break;
        // 3. the Bethe moments
        if ((e = n == 1 ? bp_moments_enqueue(g, a, p.zf[0], p.M[0], p.skipped[0]) : bp_moments_enqueue(g, p)) != hipSuccess) break;
        // 4. the update
        k_pcd_update<<<dim3(wblocks), dim3(NSK_BLOCK), 0, g->stream>>>(Mfree, 1.0, Mc, n == 1 ? 0.0 : 1.0, b.target, b.nfac, (int)nw, g->w, g->w_fixed,
                                                                      normalize, st, reg_param, out.gmax + t, out.row(t));
        e = hipGetLastError();
        g->weights_dirty = true;            // the next sweep call rebuilds what derives from the weights
        st = st * decay;
    }
    // the resident tables agree with the learned weights: a following nsk_bp_run continues under them
    if (e == hipSuccess) { refresh(); e = hipGetLastError(); }
    std::vector<unsigned long long> hskip(N * T);
    std::vector<double> hres(N * T * I);
    if (e == hipSuccess) e = out.download();
    if (e == hipSuccess) e = hipMemcpyAsync(hskip.data(), b.skipped, N * T * 8, hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hres.data(), b.res, N * T * I * 8, hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);      // (also: the uploads read the host vectors)
    HIPCHECK(e);
    HIPCHECK(e2);
    out.deliver(gmax, moments);
    for (size_t r = 0; r < N * T; r++) {            // row r = (step, set-up)
        int64_t ran = -iters_per_step;
        for (size_t i = 0; i < I; i++) {
            if (residual) residual[r * I + i] = hres[r * I + i];
            if (ran < 0 && hres[r * I + i] <= tol) ran = (int64_t)i + 1;
        }
        if (iters) iters[r] = ran;
        if (skipped) skipped[r] = (int64_t)hskip[r];
    }
    return NSK_OK;
}

extern "C" {

int nsk_bp_setup(nsk_graph *g, int which, int64_t chain, int sample_evidence, nsk_bp_info *info_out) {
    int rc = bp_common(g, "nsk_bp_setup", false);
    if (rc) return rc;
    if ((rc = chain_select(g, which, chain, 1, "nsk_bp_setup", true))) return rc;
    // ---- the structure: every refusal names the lowest offending factor and precedes any allocation
    const Compiled &c = g->c;
    BpPlan pl;
    const std::string why = bp_plan(c, sample_evidence, NSK_BP_MAX_MEMBERS, NSK_BP_MAX_TABLE, NSK_ZLOCAL, pl);
    if (!why.empty()) return fail(NSK_E_INVALID, why);
    const nsk_bp_info &info = pl.info;
    const int64_t F = c.nfactor, nid = c.nid, E = info.nedges;
    // ---- the handle's side: plain values, the records and weights on the device
    HIPCHECK(hipSetDevice(g->device));
    if ((rc = energy_ensure(g, 0, "nsk_bp_setup"))) return rc;
    if ((rc = nsk_unpack_tally(g))) return rc;
    HIPCHECK(hipStreamSynchronize(g->stream));
    bp_free(g);
    NskBp &b = g->bp;
    b.big = pl.big; b.b_off.swap(pl.b_off); b.info = info; b.nvlist = (int32_t)pl.v_list.size(); b.nvbin = pl.nvbin;
    const int64_t before = g->mem.total;
    const double bytes = 24.0 * (double)info.ntable + 16.0 * (double)info.nmsg + 20.0 * (double)E + 8.0 * (double)(pl.mrec.size() / 2) +
                         8.0 * (double)(pl.slot_rec.size() / 2) + 24.0 * (double)F + 17.0 * (double)nid + (b.big ? 16.0 : 8.0) * (double)info.nbelief;
    rc = bp_upload(g, &b.pm_off, pl.pm_off);
    if (!rc) rc = bp_upload(g, &b.tab_off, pl.tab_off);
    if (!rc) rc = bp_upload(g, &b.msg_off, pl.msg_off);
    if (!rc) rc = bp_upload(g, &b.d_b_off, b.b_off);
    if (!rc) rc = bp_upload(g, &b.slot_off, pl.slot_off);
    if (!rc) rc = bp_upload(g, &b.edge_off, pl.edge_off);
    if (!rc) rc = bp_upload(g, &b.e_fac, pl.e_fac);
    if (!rc) rc = bp_upload(g, &b.e_var, pl.e_var);
    if (!rc) rc = bp_upload(g, &b.v_list, pl.v_list);
    if (!rc) rc = bp_upload(g, &b.v_eoff, pl.v_eoff);
    if (!rc) rc = bp_upload(g, &b.v_edges, pl.v_edges);
    if (!rc) rc = bp_upload(g, &b.mrec, pl.mrec);
    if (!rc) rc = bp_upload(g, &b.slot_rec, pl.slot_rec);
    if (!rc) rc = bp_upload(g, &b.v_state, pl.state);
    if (!rc) rc = bp_alloc(g, &b.theta, (size_t)info.ntable);
    if (!rc) rc = bp_alloc(g, &b.psi, (size_t)info.ntable);
    if (!rc) rc = bp_alloc(g, &b.feat, (size_t)info.ntable);
    if (!rc) rc = bp_alloc(g, &b.f2v, (size_t)info.nmsg);
    if (!rc) rc = bp_alloc(g, &b.v2f, (size_t)info.nmsg);
    if (!rc) rc = bp_alloc(g, &b.belief, (size_t)info.nbelief);
    if (!rc && b.big) rc = bp_alloc(g, &b.wk, (size_t)info.nbelief);
    if (rc) {
        (void)hipStreamSynchronize(g->stream);
        bp_free(g);
        if (rc != NSK_E_NOMEM) return rc;
        return fail(NSK_E_NOMEM, "nsk_bp_setup: structure, tables, messages and beliefs (" + std::to_string((long long)bytes) +
                                 " bytes) do not fit on the device");
    }
    b.info.device_bytes = g->mem.total - before;
    const BpArgs a = bp_args(g);
    const char *val = chain_val(g, which, chain);
    const dim3 block(NSK_BLOCK);
    if (F > 0) {
        if (c.vbytes == 4) k_bp_tables<int32_t><<<dim3(bp_blocks(a.ntable)), block, 0, g->stream>>>(a, (const int32_t *)val);
        else k_bp_tables<int8_t><<<dim3(bp_blocks(a.ntable)), block, 0, g->stream>>>(a, (const int8_t *)val);
        k_bp_psi<<<dim3(bp_blocks(F)), block, 0, g->stream>>>(a);
    }
    if (E > 0) k_bp_reset<<<dim3(bp_blocks(E)), block, 0, g->stream>>>(a);
    if (nid > 0) {
        if (c.vbytes == 4) k_bp_belief0<int32_t><<<dim3(bp_blocks(nid)), block, 0, g->stream>>>(a, (const int32_t *)val);
        else k_bp_belief0<int8_t><<<dim3(bp_blocks(nid)), block, 0, g->stream>>>(a, (const int8_t *)val);
    }
    hipError_t e = hipGetLastError();
    const hipError_t e2 = hipStreamSynchronize(g->stream);      // (the uploads read the vectors of this scope)
    if (e != hipSuccess || e2 != hipSuccess) {
        bp_free(g);
        HIPCHECK(e);
        HIPCHECK(e2);
    }
    b.ready = true;
    if (info_out) *info_out = b.info;
    return NSK_OK;
}

int nsk_bp_layout(nsk_graph *g, int64_t *table_off, int64_t *edge_off, int64_t *edge_var, int64_t *msg_off) {
    int rc = bp_common(g, "nsk_bp_layout", true);
    if (rc) return rc;
    const NskBp &b = g->bp;
    const size_t F = (size_t)b.info.nfactor, E = (size_t)b.info.nedges;
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets cross as they are");
    if (table_off) HIPCHECK(hipMemcpy(table_off, b.tab_off, (F + 1) * 8, hipMemcpyDeviceToHost));
    if (msg_off) HIPCHECK(hipMemcpy(msg_off, b.msg_off, (E + 1) * 8, hipMemcpyDeviceToHost));
    std::vector<int32_t> tmp;
    if (edge_off) {
        tmp.resize(F + 1);
        HIPCHECK(hipMemcpy(tmp.data(), b.edge_off, (F + 1) * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i <= F; i++) edge_off[i] = tmp[i];
    }
    if (edge_var && E) {
        tmp.resize(E);
        HIPCHECK(hipMemcpy(tmp.data(), b.e_var, E * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < E; i++) edge_var[i] = g->c.p_vid[(size_t)tmp[i]];       // (a free variable has a position)
    }
    return NSK_OK;
}

int nsk_bp_run(nsk_graph *g, int64_t max_iters, double damping, double tol, int64_t *iters, double *residual) {
    int rc = bp_common(g, "nsk_bp_run", true);
    if (rc) return rc;
    if (!iters) return fail(NSK_E_INVALID, "null argument");
    if (max_iters < 1 || max_iters > 4096) return fail(NSK_E_INVALID, "nsk_bp_run: max_iters must lie in [1, 4096]");
    if (!(damping >= 0.0 && damping < 1.0)) return fail(NSK_E_INVALID, "nsk_bp_run: damping must lie in [0, 1)");
    if (!(tol >= 0.0)) return fail(NSK_E_INVALID, "nsk_bp_run: tol must be at least 0");
    HIPCHECK(hipSetDevice(g->device));
    const size_t S = (size_t)max_iters;
    unsigned long long *res = nullptr;          // [max_iters] bit patterns, for this call only
    if ((rc = dev_alloc(g, &res, S))) {
        if (rc != NSK_E_NOMEM) return rc;
        return fail(NSK_E_NOMEM, "nsk_bp_run: the residuals (" + std::to_string((long long)(S * 8)) + " bytes) do not fit on the device");
    }
    hipError_t e = hipMemsetAsync(res, 0, S * 8, g->stream);
    if (e == hipSuccess) e = bp_iterations_enqueue(g, bp_args(g), S, damping, tol, res);
    std::vector<double> host(S);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), res, S * 8, hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);
    dev_free(g, res);
    HIPCHECK(e);
    HIPCHECK(e2);
    int64_t ran = -max_iters;
    for (size_t t = 0; t < S; t++) {
        if (residual) residual[t] = host[t];
        if (ran < 0 && host[t] <= tol) ran = (int64_t)t + 1;
    }
    *iters = ran;
    return NSK_OK;
}

int nsk_bp_beliefs(nsk_graph *g, const int64_t *vids, int64_t nvids, double *out) {
    int rc = bp_common(g, "nsk_bp_beliefs", true);
    if (rc) return rc;
    const Compiled &c = g->c;
    if (nvids < 0 || (!vids && nvids != 0)) return fail(NSK_E_INVALID, "nsk_bp_beliefs: a null selection with a count, or a negative count");
    if (vids && nvids == 0) return NSK_OK;
    const int64_t n = vids ? nvids : c.nvar;
    for (int64_t i = 0; vids && i < n; i++)
        if (vids[i] < 0 || vids[i] >= c.nvar) return fail(NSK_E_INDEX, "nsk_bp_beliefs: variable id out of range");
    const NskBp &b = g->bp;
    if (b.info.nbelief == 0) return NSK_OK;
    if (!out) return fail(NSK_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    std::vector<double> all((size_t)b.info.nbelief);
    HIPCHECK(hipMemcpy(all.data(), b.belief, all.size() * 8, hipMemcpyDeviceToHost));
    size_t o = 0;
    for (int64_t i = 0; i < n; i++) {
        const size_t id = (size_t)c.iid[(size_t)(vids ? vids[i] : i)];
        for (long long k = b.b_off[id]; k < b.b_off[id + 1]; k++) out[o++] = all[(size_t)k];
    }
    return NSK_OK;
}

int nsk_bp_download(nsk_graph *g, int what, double *out) {
    int rc = bp_common(g, "nsk_bp_download", true);
    if (rc) return rc;
    if (what < NSK_BP_THETA || what > NSK_BP_V2F) return fail(NSK_E_INVALID, "nsk_bp_download: what must be NSK_BP_THETA .. NSK_BP_V2F");
    const NskBp &b = g->bp;
    const size_t n = (size_t)(what <= NSK_BP_FACTOR_BELIEFS ? b.info.ntable : b.info.nmsg);
    if (n == 0) return NSK_OK;
    if (!out) return fail(NSK_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(g->device));
    if (what != NSK_BP_FACTOR_BELIEFS) {
        HIPCHECK(hipStreamSynchronize(g->stream));
        HIPCHECK(hipMemcpy(out, what == NSK_BP_THETA ? b.theta : (what == NSK_BP_F2V ? b.f2v : b.v2f), n * 8, hipMemcpyDeviceToHost));
        return NSK_OK;
    }
    double *fb = nullptr;                       // for this call only
    if ((rc = dev_alloc(g, &fb, n))) {
        if (rc != NSK_E_NOMEM) return rc;
        return fail(NSK_E_NOMEM, "nsk_bp_download: the factor beliefs (" + std::to_string((long long)(n * 8)) + " bytes) do not fit on the device");
    }
    k_bp_fbelief<<<dim3(bp_blocks((long long)b.info.nfactor)), dim3(NSK_BLOCK), 0, g->stream>>>(bp_args(g), fb);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, fb, n * 8, hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);
    dev_free(g, fb);
    HIPCHECK(e);
    HIPCHECK(e2);
    return NSK_OK;
}

int nsk_bp_refresh(nsk_graph *g) {
    int rc = bp_common(g, "nsk_bp_refresh", true);
    if (rc) return rc;
    HIPCHECK(hipSetDevice(g->device));
    bp_refresh_enqueue(g, bp_args(g));
    HIPCHECK(hipGetLastError());
    return NSK_OK;
}

int nsk_bp_moments(nsk_graph *g, int64_t *moments, int64_t *skipped) {
    const char *who = "nsk_bp_moments";
    int rc = bp_common(g, who, true);
    if (rc) return rc;
    const Compiled &c = g->c;
    const size_t nw = (size_t)c.nweight;
    if (nw == 0) return NSK_OK;
    if (!moments) return fail(NSK_E_INVALID, "null argument");
    if ((rc = nsk_moments_range(g, 1, who))) return rc;
    HIPCHECK(hipSetDevice(g->device));
    BpLearnBufs b(g);
    rc = call_alloc(g, &b.M, nw, who, "the int64 sums, 8 bytes a weight");
    if (!rc) rc = call_alloc(g, &b.skipped, 1, who, "the skip counter");
    if (!rc) rc = call_alloc(g, &b.zf, (size_t)g->bp.info.nfactor, who, "the factors' normalisers, 8 bytes a factor");
    if (rc) return rc;
    std::vector<long long> host(nw);
    unsigned long long hskip = 0;
    hipError_t e = bp_moments_enqueue(g, bp_args(g), b.zf, b.M, b.skipped);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), b.M, nw * sizeof(long long), hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&hskip, b.skipped, sizeof(hskip), hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);
    HIPCHECK(e);
    HIPCHECK(e2);
    SlotMap(c).from_slots(host.data(), moments);
    if (skipped) *skipped = (int64_t)hskip;
    return NSK_OK;
}

int nsk_bp_learn_steps(nsk_graph *g, const double *target, int64_t nsteps, int64_t iters_per_step, double damping, double tol, int warm,
                       double step, double decay, double reg_param, int normalize, double *gmax, int64_t *iters, double *residual,
                       int64_t *moments, int64_t *skipped) {
    const char *who = "nsk_bp_learn_steps";
    int rc = bp_common(g, who, true);
    if (rc) return rc;
    if (!target) return fail(NSK_E_INVALID, "null argument");
    if ((rc = bp_steps_check(who, nsteps, iters_per_step, damping, tol, warm, step, decay, reg_param, normalize))) return rc;
    if ((rc = refuse(check_target(who, target, (size_t)g->c.nweight)))) return rc;
    return bp_steps_run(g, who, 1, target, nsteps, iters_per_step, damping, tol, warm, step, decay, reg_param, normalize, gmax, iters, residual,
                        moments, skipped);
}

int nsk_bp_latent_steps(nsk_graph *g, int64_t nsteps, int64_t iters_per_step, double damping, double tol, int warm, double step,
                        double decay, double reg_param, int normalize, double *gmax, int64_t *iters, double *residual, int64_t *moments,
                        int64_t *skipped) {
    const char *who = "nsk_bp_latent_steps";
    int rc = bp_common(g, who, false);
    if (rc) return rc;
    if (!bp_slot(g, 0).ready || !bp_slot(g, 1).ready)
        return fail(NSK_E_INVALID, std::string(who) + ": slot " + (bp_slot(g, 0).ready ? "1 (the free phase)" : "0 (the clamped phase)") +
                                   " has no belief propagation set up (nsk_bp_select, nsk_bp_setup)");
    if ((rc = bp_steps_check(who, nsteps, iters_per_step, damping, tol, warm, step, decay, reg_param, normalize))) return rc;
    return bp_steps_run(g, who, 2, nullptr, nsteps, iters_per_step, damping, tol, warm, step, decay, reg_param, normalize, gmax, iters, residual,
                        moments, skipped);
}

int nsk_bp_select(nsk_graph *g, int slot) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (slot != 0 && slot != 1) return fail(NSK_E_INVALID, "nsk_bp_select: slot must be 0 or 1");
    if (slot != g->bp_slot) {                       // host records only: what is enqueued keeps its arrays
        std::swap(g->bp, g->bp_other);
        g->bp_slot = slot;
    }
    return NSK_OK;
}

int nsk_bp_selected(nsk_graph *g) { return g ? g->bp_slot : fail(NSK_E_INVALID, "null graph"); }

int nsk_bp_clear(nsk_graph *g) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!g->bp.ready) return NSK_OK;
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    bp_free(g);
    return NSK_OK;
}

}  // extern "C"
