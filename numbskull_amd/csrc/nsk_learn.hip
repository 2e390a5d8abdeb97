// nsk_learn.hip -- learning sweep driver: replaces the epoch loop around run_pool(learnthread) at
// numbskull/factorgraph.py:194-206; kernels in nsk_kernels_learn.h.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "nsk_class_plan.h"
#include "nsk_internal.h"
#include "nsk_kernels_learn.h"
#include "nsk_kernels_misc.h"

using namespace nsk;

static_assert(PLAN_BLOCK == NSK_BLOCK && PLAN_LEARN_FAST_BLOCKS == NSK_LEARN_FAST_BLOCKS && PLAN_LEARN_LIST_BLOCKS == NSK_LEARN_LIST_BLOCKS &&
              PLAN_LEARN_GEN_BLOCKS == NSK_LEARN_GEN_BLOCKS && PLAN_LEARN_HEAVY_BLOCKS == NSK_LEARN_HEAVY_BLOCKS &&
              PLAN_LEARN_GENERAL_BLOCKS == NSK_LEARN_GENERAL_BLOCKS, "nsk_class_plan.h copies the kernels' block size and grid caps");

#ifndef NSK_LEARN_TPW
#define NSK_LEARN_TPW 2          // tiles per trip of the learning table kernel (1: 41.6 us, 2: 41.6 us, 4: 46.7 us
                                 // per 10M-grid class before the kernel was pipelined)
#endif

// the fast-path refresh after a weight update of the large-table path, for one weight set on one stream
static void refresh_after_update(nsk_graph *g, int set, hipStream_t st) {
    const int n = (int)g->c.tile_hdr.size();
    // (n <= 8: the closing pad alone -- a graph of general tiles and entry-parallel groups has no slot programs, and
    // the launch would be 4.7 us per class of nothing: 4 % of a 5M LR graph's learning sweep)
    if (n > 8 && g->c.nfast > 0 && g->c.nweight > 0) {
        k_refresh_prog_weights<<<dim3((n + NSK_BLOCK - 1) / NSK_BLOCK), dim3(NSK_BLOCK), 0, st>>>(
            g->tile_hdr, set ? g->w1 : g->w, set ? g->prog_w1 : g->prog_w, n);
        nsk_refresh_ztab(g, set, st);
    }
}

static_assert(SEG_LEARN_TPW == NSK_LEARN_TPW && SEG_LEARN_SEG_BLOCKS == NSK_LEARN_SEG_BLOCKS && SEG_SERVICE_BLOCKS == NSK_SERVICE_BLOCKS,
              "nsk_seg_plan.h copies the trip width and grid constants of the learning segment kernels");

// The segment launches of learning (Compiled::learn_seg; nsk_seg_plan.h plan_learn_segment), planned once per handle and
// set of options -- walking a launch's quad descriptors on the host for every launch of every sweep cost more than the
// launch itself from a few million variables on.  The switches are read here, once per call.
static const std::vector<LearnSegPlan> &learn_seg_plans(nsk_graph *g, bool smallw) {
    SegPlanOpts o;
    o.use_tab = g->values_regular;
    o.byte_values = g->c.vbytes == 1;
    o.no_tabw_rest = nsk::diag_env("NSK_NO_TABW_REST") != nullptr;
    o.nweight = (int)g->c.nweight;
    o.smallw = smallw;
    const char *min_env = nsk::diag_env("NSK_WIDE_LEARN_MIN");                 // (the small-grid tests use 0)
    if (min_env) o.wide_learn_min_quads = atoi(min_env);
    o.no_wide_learn = nsk::diag_env("NSK_NO_WIDE_LEARN") != nullptr;
    o.learn_grid_cap = seg_cap_blocks(nsk::diag_env("NSK_LEARN_GRID_CAP"));
    o.learn_tabw_grid_cap = seg_cap_rounds(nsk::diag_env("NSK_LEARN_TABW_GRID_CAP"));
    if (g->learn_seg_plans.size() != g->c.learn_seg.size() || !(o == g->learn_seg_opts)) {
        g->learn_seg_plans.clear();
        for (const Compiled::SegLaunch &sl : g->c.learn_seg) g->learn_seg_plans.push_back(plan_learn_segment(g->c, sl, o));
        g->learn_seg_opts = o;
    }
    return g->learn_seg_plans;
}

// The chromatic learning sweep is instantiated four times (value type x accumulator flavour) and every
// instantiation carries a dozen kernels: the Makefile compiles this file once per instantiation
// (-DNSK_LEARN_PART=0..3, in parallel; part 0 also holds the entry point) -- one translation unit with all four
// (NSK_LEARN_PART undefined: the ablation builds) takes six minutes.
#ifndef NSK_LEARN_PART
#define NSK_LEARN_PART -1
#endif
#define NSK_LEARN_HAS(P) (NSK_LEARN_PART == -1 || NSK_LEARN_PART == (P))
#define NSK_LEARN_SIG nsk_graph *g, int64_t nsweeps, double step, double decay, int regularization, \
                      double reg_param, int64_t truncation, int learn_non_evidence
template <typename VT, bool SMALLW>
int nsk_learn_chromatic(NSK_LEARN_SIG);
#if NSK_LEARN_PART != -1        // the instantiations of the other parts are theirs
#if !NSK_LEARN_HAS(0)
extern template int nsk_learn_chromatic<int8_t, false>(NSK_LEARN_SIG);
#endif
#if !NSK_LEARN_HAS(1)
extern template int nsk_learn_chromatic<int8_t, true>(NSK_LEARN_SIG);
#endif
#if !NSK_LEARN_HAS(2)
extern template int nsk_learn_chromatic<int32_t, false>(NSK_LEARN_SIG);
#endif
#if !NSK_LEARN_HAS(3)
extern template int nsk_learn_chromatic<int32_t, true>(NSK_LEARN_SIG);
#endif
#endif

template <typename VT, bool SMALLW>
int nsk_learn_chromatic(nsk_graph *g, int64_t nsweeps, double step, double decay, int regularization,
                        double reg_param, int64_t truncation, int learn_non_evidence) {
    const size_t nphase = g->c.phase_start.size() - 1;
    const int nw = (int)g->c.nweight;
    const size_t shmem = SMALLW ? (size_t)nw * 16 : 0;
    LearnParams lp;
    lp.regularization = regularization;
    lp.learn_non_evidence = learn_non_evidence;
    lp.inv_trunc = 1.0 / (double)truncation;
    lp.k0 = (uint32_t)g->seed; lp.k1 = (uint32_t)(g->seed >> 32);
    lp.kstat = 0;
    g->adj_wt_skip = true;          // the learning kernels gather weights themselves
    nsk_refresh_prog_weights(g);
    // One-class lag (nsk_set_learn_lag): class c of this call samples from weight set c & 1 -- the weights
    // as of the end of class c - 2 -- and adds into accumulator set c & 1; its update U(c) reads the weights
    // of set (c + 1) & 1 (end of class c - 1) and writes set c & 1, and is enqueued BEHIND class c + 1,
    // which does not read it: fused into that class's table launch when there is one (block 0 of
    // k_learn_seg_tab, beside the sampling), else as a launch of its own after the class.  Both sets start
    // from the call's weights.  (A second stream with events around every class cost more than the update:
    // 34 against 28.5 us per 10M-grid class.)
    // (only handles that accumulate in LDS -- at most NSK_SMALLW weights: the grids -- run lagged: there the
    // update rides in the next class's launch; with a large weight table it is a launch of its own either
    // way, and the in-kernel updates of single-factor weights below want one weight set)
    const bool lag = g->learn_lag && nw > 0 && SMALLW;
    DevGraph<VT> dv[2];
    dv[0] = view<VT>(g);
    dv[1] = dv[0];
    if (lag) {
        int rc = nsk_ensure_lag_sets(g);
        if (rc) return rc;
        dv[1].w = g->w1; dv[1].prog_w = g->prog_w1; dv[1].ztab = g->ztab1;
        dv[1].G = g->G1; dv[1].K = g->K1; dv[1].T = g->T1;
        dv[1].part_G = g->part_G1; dv[1].part_K = g->part_K1; dv[1].part_T = g->part_T1;
        HIPCHECK(hipMemcpyAsync(g->w1, g->w, (size_t)nw * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
        if (!g->c.tile_hdr.empty())
            HIPCHECK(hipMemcpyAsync(g->prog_w1, g->prog_w, 2 * g->c.tile_hdr.size() * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
        if (g->c.nztab)
            HIPCHECK(hipMemcpyAsync(g->ztab1, g->ztab, (size_t)g->c.nztab * sizeof(uint4), hipMemcpyDeviceToDevice, g->stream));
    }
    int64_t cls = 0;                // classes launched in this call
    struct Pending {                // the update of the previous class, not yet enqueued
        bool valid = false;
        int set = 0;
        bool tabs_here = false, kstat = false;
        size_t ph = 0;
        double step = 0.0;
        ApplyArgs aa;
    } pend;
    auto launch_update = [&](const Pending &u) {      // as launches of their own on the main stream
        const DevGraph<VT> &du = dv[u.set];
        if (SMALLW) {
            k_apply_bins<<<dim3(1), dim3(NSK_BLOCK), 0, g->stream>>>(u.aa);
            if (g->c.nfast > 0 && !u.tabs_here) nsk_refresh_ztab(g, u.set, g->stream);   // big tables: own launch
        } else {
            // (with direct weights only the others are walked -- none at all when every weight has one factor)
            const bool direct = g->c.ndirect > 0;
            const int nwalk = direct ? (int)g->c.multi_wids.size() : nw;
            if (nwalk > 0) {
                k_apply_weights<<<dim3((nwalk + NSK_BLOCK - 1) / NSK_BLOCK), dim3(NSK_BLOCK), 0, g->stream>>>(
                    du.w, u.aa.w_in, du.G, du.K, du.T, nw, u.step, regularization, reg_param, (double)truncation,
                    (!SMALLW && g->c.packed_grad) ? 1 : 0, g->learn_cap, g->clip_count, g->acc_copies, du.grad_inv,
                    u.kstat ? du.ep_kstat + (size_t)(2 * u.ph) * (size_t)nw : nullptr,
                    (u.kstat && learn_non_evidence) ? du.ep_kstat + (size_t)(2 * u.ph + 1) * (size_t)nw : nullptr,
                    direct ? g->multi_wids : nullptr, nwalk);
                refresh_after_update(g, u.set, g->stream);
            }
        }
    };
    ApplyArgs no_update;
    memset(&no_update, 0, sizeof(no_update));
    // every class's plan (nsk_class_plan.h) and its segment launches, once per call: nothing a sweep changes enters them
    struct LearnSeg { const Compiled::SegLaunch *sl; const LearnSegPlan *pl; };
    struct LearnClass { ClassShape s; LearnClassPlan p; std::vector<LearnSeg> segs; };
    const std::vector<LearnSegPlan> &seg_plans = learn_seg_plans(g, SMALLW);
    std::vector<LearnClass> classes(nphase);
    PlanOpts opts;
    opts.overlap = !g->no_overlap;
    opts.smallw = SMALLW; opts.nweight = nw; opts.has_kstat = dv[0].ep_kstat != nullptr; opts.regularization = regularization;
    opts.grid_cap = plan_grid_cap(nsk::diag_env("NSK_CLASS_GRID_CAP"));     // (diagnostic: small persistent grids, later trips)
    for (size_t ph = 0; ph < nphase; ph++) {
        LearnClass &c = classes[ph];
        c.s = class_shape(g->c, ph);
        opts.seg_tiles = 0;
        for (size_t i = 0; i < g->c.learn_seg.size(); i++) {
            const Compiled::SegLaunch &sl = g->c.learn_seg[i];
            if (sl.phase == (int)ph) { c.segs.push_back(LearnSeg{&sl, &seg_plans[i]}); opts.seg_tiles += sl.tile_start[sl.n]; }
        }
        if (c.s.ep && c.s.e > c.s.fb) opts.ep_per_cu = plan_per_cu(nsk::diag_env("NSK_EP_PER_CU"));    // (diagnostic: workgroups per CU)
        c.p = plan_learn_class(c.s, opts);
    }
    for (int64_t s = 0; s < nsweeps; s++) {
        lp.s0 = (uint32_t)g->sweep; lp.s1 = nsk_sweep_hi(g);
        for (size_t ph = 0; ph < nphase; ph++) {
            const ClassShape &cl = classes[ph].s;
            const LearnClassPlan &p = classes[ph].p;
            if (p.skip) continue;
            const int set = lag ? (int)(cls & 1) : 0;
            DevGraph<VT> d = dv[set];
            // the parameters of this class's update, for the weights the kernels update in place (w_direct)
            d.upd_step = step; d.upd_regularization = regularization; d.upd_reg_param = reg_param;
            d.upd_truncation = (double)truncation; d.upd_cap = g->learn_cap;
            d.upd_a1 = 1.0 / (1.0 + reg_param * step);
            lp.hub0 = cl.hub0;
            ColourStreams cs(g, !g->no_overlap);
            // the weight update of the class (SMALLW): arguments of k_apply_bins
            const bool tabs_here = g->c.nfast > 0 && g->c.nztab <= 2048;
            ApplyArgs aa;
            memset(&aa, 0, sizeof(aa));
            aa.w = d.w; aa.w_in = lag ? dv[set ^ 1].w : d.w;
            aa.part_G = d.part_G; aa.part_K = d.part_K; aa.part_T = d.part_T;
            aa.nweight = nw; aa.step = step; aa.regularization = regularization; aa.reg_param = reg_param;
            aa.truncation = (double)truncation; aa.prog = g->tile_hdr; aa.prog_w = const_cast<double *>(d.prog_w);
            aa.nprog = g->c.nfast > 0 ? (int)g->c.tile_hdr.size() : 0; aa.zp = g->zprogs;
            aa.nzp = tabs_here ? (int)g->c.zprogs.size() : 0; aa.nztab = tabs_here ? (int)g->c.nztab : 0;
            aa.ztab = const_cast<uint4 *>(d.ztab); aa.cap = g->learn_cap; aa.clipped = g->clip_count; aa.grad_inv = d.grad_inv;
            if (p.generic.on) {         // variables outside the fast path: generic kernel, range mode
                k_learn_phase<VT, SMALLW, true><<<dim3(p.generic.grid), dim3(NSK_BLOCK), shmem, cs.of(p.generic.stream)>>>(
                    d, cl.he, cl.e, nullptr, p.generic.n, lp);
                g->launches++;
            }
            if (p.heavy.on) {           // hubs no general launch carries: one wave per variable
                k_learn_heavy<VT, SMALLW><<<dim3(p.heavy.grid), dim3(NSK_BLOCK), shmem, cs.of(p.heavy.stream)>>>(d, cl.fe, cl.he, lp);
                g->launches++;
            }
            lp.kstat = p.kstat ? 1 : 0;
            if (p.general.on) {         // hubs, general tiles (as entry-parallel groups: L.ep) and the class's rest tiles
                const GeneralLaunch &L = p.general;
                const uint32_t *lrest = g->learn_rest_tiles + cl.lrest0;
                hipStream_t st = cs.of(L.stream);
#define NSK_LEP(KERNEL, MAXC) KERNEL<VT, SMALLW, MAXC><<<dim3(L.grid), dim3(NSK_BLOCK), shmem, st>>>( \
                    d, cl.fb, cl.fe, cl.wb_base, L.tile0, L.ntiles, cl.ngroups, cl.group0, L.gblocks, \
                    cl.fe, cl.he, L.hblocks, cl.nbh, cl.bh0, lrest, L.nrest, lp)
#define NSK_LGEN(MAXC) k_learn_general<VT, SMALLW, MAXC><<<dim3(L.grid), dim3(NSK_BLOCK), shmem, st>>>( \
                    d, cl.fb, cl.fe, cl.wb_base, L.tile0, L.ntiles, cl.fe, cl.he, L.hblocks, lrest, L.nrest, lp)
                // (a colour's all-binary groups -- its tail: categorical lanes come first -- in a launch of their own with the
                // two-candidate kernel, 114 vector registers and four waves per SIMD instead of 152 and three: 50M LR graph
                // 5.57 -> 5.73e9 updates/s, 5M 5.13 -> 4.17e9 with the split forced (two tails per class); inference, 86 / 5
                // against 102 / 4: 1.540 / 1.540e10 -- tools/sessions/r5_s24.sh; not kept)
                if (L.ep) { if (L.capped) NSK_LEP(k_learn_ep_w4, 8); else NSK_LEP(k_learn_ep, 2); }
                else if (L.maxc == 8) NSK_LGEN(8);
                else NSK_LGEN(2);
#undef NSK_LGEN
#undef NSK_LEP
                g->launches++;
            }
            for (const LearnSeg &ls : classes[ph].segs) {       // homogeneous segments, from their plans
                const Compiled::SegLaunch &sl = *ls.sl;
                const LearnSegPlan &pl = *ls.pl;
                const bool use_tab = sl.tab && g->values_regular;
                const SegTable &tab = pl.tab;
                const int grid = pl.grid;
                // the previous class's update rides in a table launch (block 0 of the service blocks in front)
                const bool fuse = use_tab && SMALLW && pend.valid && pend.tabs_here;
                const ApplyArgs &prev = fuse ? pend.aa : no_update;
                const int service = SMALLW ? NSK_SERVICE_BLOCKS : 0;
#define NSK_LSEG(KIND, NCH) k_learn_seg<VT, SMALLW, KIND, NCH><<<dim3(grid), dim3(NSK_BLOCK), shmem, g->stream>>>(d, tab, lp)
#define NSK_LTAB(NCH) k_learn_seg_tab<VT, SMALLW, NCH, NSK_LEARN_TPW><<<dim3(grid + service), dim3(NSK_BLOCK), shmem, g->stream>>>(d, tab, lp, prev)
#define NSK_LTABW(NCH) k_learn_seg_tabw<SMALLW, NCH><<<dim3(grid + service), dim3(NSK_BLOCK), shmem, g->stream>>>(d, tab, lp, prev, rest)
                if (pl.wide) {
                    if constexpr (sizeof(VT) == 1) {        // (only a plan over byte values is wide)
                        TabwRest rest;
                        rest.n = pl.nrest;
                        memcpy(rest.q, pl.rest, sizeof(rest.q));
                        if (sl.nch == 1) NSK_LTABW(1); else NSK_LTABW(2);
                    }
                } else {
                    if (use_tab) { if (sl.nch == 1) NSK_LTAB(1); else NSK_LTAB(2); }
                    else if (sl.tab) { if (sl.nch == 1) NSK_LSEG(0, 1); else NSK_LSEG(0, 2); }   // tables unusable: the
                                                                           // generic slot algebra serves every function
                    else if (sl.kind == 4) { if (sl.nch == 1) NSK_LSEG(4, 1); else NSK_LSEG(4, 2); }
                    else if (sl.kind == 2) { if (sl.nch == 1) NSK_LSEG(2, 1); else NSK_LSEG(2, 2); }
                    else if (sl.kind == 0) { if (sl.nch == 1) NSK_LSEG(0, 1); else NSK_LSEG(0, 2); }
                    else { if (sl.nch == 1) NSK_LSEG(3, 1); else NSK_LSEG(3, 2); }
                }
#undef NSK_LTABW
#undef NSK_LTAB
#undef NSK_LSEG
                if (fuse) pend.valid = false;
                g->launches++;
            }
            if (p.fast.on) {            // the other uniform and shape tiles: descriptor-driven kernel
                k_learn_fast<VT, SMALLW><<<dim3(p.fast.grid), dim3(NSK_BLOCK), shmem, g->stream>>>(
                    d, cl.fb, cl.fe, cl.wb_base, g->learn_rest_tiles + cl.lrest0, cl.nlrest, lp);
                g->launches++;
            }
            if (p.dyn.on) {             // tiles with per-lane headers: generic kernel, list mode
                k_learn_phase<VT, SMALLW, false><<<dim3(p.dyn.grid), dim3(NSK_BLOCK), shmem, g->stream>>>(
                    d, cl.fb, cl.fe, g->dyn_tiles + cl.dyn0, cl.ndyn, lp);
                g->launches++;
            }
            cs.join();
            if (p.update) {
                if (pend.valid) { launch_update(pend); pend.valid = false; }     // the previous class's, not fused above
                Pending u;
                u.valid = true; u.set = set; u.tabs_here = tabs_here; u.kstat = p.kstat; u.ph = ph; u.step = step; u.aa = aa;
                if (lag) pend = u;              // behind the next class
                else launch_update(u);
            }
            cls++;
        }
        g->sweep++;
        step *= decay;                                   // factorgraph.py:206
    }
    if (pend.valid) { launch_update(pend); pend.valid = false; }
    if (lag && cls > 0 && ((cls - 1) & 1))          // the call leaves the weights, every update applied, in set 0
        HIPCHECK(hipMemcpyAsync(g->w, g->w1, (size_t)nw * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
    g->adj_wt_skip = false;
    g->weights_dirty = true;        // the next inference call rebuilds prog_w and the weight rows
    HIPCHECK(hipGetLastError());
    return NSK_OK;
}

#if NSK_LEARN_PART != -1
#if NSK_LEARN_HAS(0)
template int nsk_learn_chromatic<int8_t, false>(NSK_LEARN_SIG);
#endif
#if NSK_LEARN_HAS(1)
template int nsk_learn_chromatic<int8_t, true>(NSK_LEARN_SIG);
#endif
#if NSK_LEARN_HAS(2)
template int nsk_learn_chromatic<int32_t, false>(NSK_LEARN_SIG);
#endif
#if NSK_LEARN_HAS(3)
template int nsk_learn_chromatic<int32_t, true>(NSK_LEARN_SIG);
#endif
#endif

#if NSK_LEARN_PART <= 0         // the sequential validation scan and the entry point
template <typename VT>
static int learn_impl(nsk_graph *g, int64_t nsweeps, double step, double decay, int regularization,
                      double reg_param, int64_t truncation, int learn_non_evidence) {
    if (g->scan == NSK_SCAN_SEQUENTIAL) {
        DevGraph<VT> d = view<VT>(g);
        k_seq_learn<VT><<<dim3(1), dim3(64), 0, g->stream>>>(d, g->v_pos, g->mt_np, g->mt_py, (int)nsweeps,
                                                            step, decay, regularization, reg_param,
                                                            (double)truncation, learn_non_evidence);
        HIPCHECK(hipGetLastError());
        g->launches++;
        g->sweep += (uint64_t)nsweeps;
    } else {
        int rc = g->smallw ? nsk_learn_chromatic<VT, true>(g, nsweeps, step, decay, regularization, reg_param,
                                                           truncation, learn_non_evidence)
                           : nsk_learn_chromatic<VT, false>(g, nsweeps, step, decay, regularization, reg_param,
                                                            truncation, learn_non_evidence);
        if (rc) return rc;
    }
    g->sweeps_done += nsweeps;
    return NSK_OK;
}

extern "C" int nsk_learn_sweeps(nsk_graph *g, int64_t nsweeps, double step, double decay, int regularization,
                     double reg_param, int64_t truncation, int learn_non_evidence) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    NSK_ONE_CHAIN(g, "nsk_learn_sweeps");
    NSK_NO_TRACE(g, "nsk_learn_sweeps");
    if (nsweeps < 0 || nsweeps > INT32_MAX) return fail(NSK_E_INVALID, "bad sweep count");
    if (regularization == 1 && truncation == 0) return fail(NSK_E_INVALID, "truncation must be non-zero (ZeroDivisionError in the reference)");
    if (nsweeps == 0) return NSK_OK;
    // chromatic learning sums a class's gradients as fixed point (order-free, deterministic): Q31.32, or
    // Q(31+s).(32-s) when the bound on one weight's sum reaches 2^30 (nsk_compile.cpp grad_shift)
    if (g->scan == NSK_SCAN_CHROMATIC && g->c.grad_bound >= 1073741824.0 * 4294967296.0)
        return fail(NSK_E_RANGE, "the gradient sum of one weight in one colour class can exceed a 63-bit integer "
                                 "accumulator (|featureValue| x visits >= 2^62); rescale featureValue or "
                                 "use the sequential scan");
    HIPCHECK(hipSetDevice(g->device));
    { int frc = nsk_p2p_flush(g); if (frc) return frc; }
    return NSK_BY_VT(g, learn_impl, g, nsweeps, step, decay, regularization, reg_param, truncation, learn_non_evidence);
}
#endif
