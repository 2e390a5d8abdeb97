// nsk_gibbs.hip -- inference sweep driver: replaces run_pool(gibbsthread) at
// numbskull/factorgraph.py:141 (burn-in) and :163 (inference); kernels in nsk_kernels_gibbs.h.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nsk_class_plan.h"
#include "nsk_internal.h"
#include "nsk_kernels_misc.h"

using namespace nsk;

// The arrays the wide-quad kernels address as 256-byte units from `val` (nsk_kernels_gibbs.h NSK_TABW_HOT): does p lie
// whole units from it that fit 32 bits -- `shift` units further down for the last chain of a batched launch?  (Device
// allocations are 256-byte aligned.)
static inline long long val_units(const nsk_graph *g, const void *p) { return ((const char *)p - (const char *)g->val) / 256; }
static bool val_offset_fits(const nsk_graph *g, const void *p, long long shift = 0) {
    const long long u = val_units(g, p) - shift;
    return ((const char *)p - (const char *)g->val) % 256 == 0 && u > -(1ll << 31) && u < (1ll << 31);
}
#define NSK_TABW_HOT_ARGS(G, T, NB, NF, SB) (signed char *)(G)->val, (int)val_units(G, (G)->cnt_pos), (int)val_units(G, (G)->seg_wide),            \
        (int)val_units(G, (G)->ztab), (T).e[1].tile_start, (T).e[0].ntiles_lead, (T).e[0].pos0, (T).e[0].wide_off, (T).e[0].zoff,                \
        (uint32_t)(T).ntiles | ((uint32_t)((T).n - 1) << 28),                                                                                    \
        ((T).e[0].zmask_ev & 0xFFu) | ((uint32_t)(((NB) >> 3) * (NSK_BLOCK / 64)) << 8) | ((uint32_t)(NF) << 24),                                \
        (const unsigned long long *)(SB)

// The segment launches of every colour (nsk_seg_plan.h plan_segments), planned once and kept in the handle (a small
// graph's sweep is two 4 us kernels: rebuilding the tables per sweep made the host the bottleneck).  The switches and the
// addresses are read here, once per call; the plans are rebuilt when the options differ from the ones they were made for
// -- and then the captured sweep sequences go, so that no replay carries a table or a grid of other options.
static void ensure_seg_plans(nsk_graph *g, int sample_evidence) {
    SegPlanOpts o;
    o.sample_evidence = sample_evidence != 0;
    o.use_tab = g->values_regular;
    o.byte_values = g->c.vbytes == 1;
    o.offsets_fit = val_offset_fits(g, g->cnt_pos) && val_offset_fits(g, g->seg_wide) && val_offset_fits(g, g->ztab);
    o.fused = g->p2p.fused;
    o.border_tiles = &g->p2p.border_tiles;
    o.no_wide_kernel = nsk::diag_env("NSK_NO_WIDE_KERNEL") != nullptr;
    o.no_tabw_rest = nsk::diag_env("NSK_NO_TABW_REST") != nullptr;
    o.tab_grid_cap = seg_cap_rounds(nsk::diag_env("NSK_TAB_GRID_CAP"));
    o.tabw_grid_cap = seg_cap_rounds(nsk::diag_env("NSK_TABW_GRID_CAP"));
    if (g->seg_plans_valid && o == g->seg_opts) return;
    SegPlans r = plan_segments(g->c, o);
    g->seg_plans.swap(r.by_class);
    g->seg_opts = o;
    g->seg_plans_valid = true;
    g->p2p.first_phase = r.first_phase;
    g->p2p.border_total = r.border_total;
    g->p2p.border_all = r.border_all;
    g->seg_plans_all_tab = r.all_tab;
    g->seg_plans_all_wide = r.all_wide;
    nsk_drop_sweep_graph(g);
}

// Where a table launch gets its counters.  An eager launch carries the Philox key, the sweep index and the exchange tag
// in its arguments; a captured one (hipGraph) reads them from d_counters and adds the offsets of its sweep in the sequence.
struct CounterSrc {
    uint32_t K0, K1, S0, S1;
    const unsigned long long *sweep_base;
    uint32_t sweep_off;
    unsigned int tag;
    static CounterSrc eager(const nsk_graph *g) {
        return {(uint32_t)g->seed, (uint32_t)(g->seed >> 32), (uint32_t)g->sweep, nsk_sweep_hi(g), nullptr, 0u, g->p2p.tag};
    }
    static CounterSrc captured(const nsk_graph *g, int i) { return {0u, 0u, 0u, 0u, g->d_counters, (uint32_t)i, (unsigned int)(i + 1)}; }
};

// L(NCH, ...) with the chunk count of the plan `pl` as a constant
#define NSK_BY_NCH(L, ...) do { if (pl.nch == 1) { L(1, __VA_ARGS__); } else { L(2, __VA_ARGS__); } } while (0)

// The wide-quad launch of a plan (four positions to a lane) -- chains: for every chain of the handle, over as many copies
// of the one-chain grid
static void launch_tabw(nsk_graph *g, const SegLaunchPlan &pl, int burnin, const CounterSrc &src, bool chains) {
    TabwCold cold{src.K0, src.K1, src.S0, src.S1, src.sweep_off, 0u, view<signed char>(g), pl.tab, pl.nrest, {}};
    memcpy(cold.rest, pl.rest, sizeof(cold.rest));
    const int nbw = pl.wide_grid, nf = pl.front;
    const dim3 grid((chains ? (unsigned)g->nchains : 1u) * (unsigned)(nf + nbw));     // (the kernel derives nf + nbw from its hot arguments)
#define NSK_TABW(NCH, K, MODE) K<NCH, MODE><<<grid, dim3(NSK_BLOCK), 0, g->stream>>>(NSK_TABW_HOT_ARGS(g, pl.tab, nbw, nf, src.sweep_base), cold)
    if (chains) { if (burnin) NSK_BY_NCH(NSK_TABW, k_gibbs_seg_tabw_chains, 1); else NSK_BY_NCH(NSK_TABW, k_gibbs_seg_tabw_chains, 0); }
    else if (burnin) NSK_BY_NCH(NSK_TABW, k_gibbs_seg_tabw, 1);
    else if (g->pack_now) NSK_BY_NCH(NSK_TABW, k_gibbs_seg_tabw, 2);      // the tally inside the value bytes
    else NSK_BY_NCH(NSK_TABW, k_gibbs_seg_tabw, 0);
#undef NSK_TABW
}

// One table launch (a plan of kind 8) of class `ph`, eager or captured: the one place that picks its kernel.  Every chain
// of a handle with several in one launch (chains_batched; R copies of the one-chain grid), else the boundary exchange
// inside the launch, else (mostly) wide quads, else a wave per tile pair.
template <typename VT>
static void launch_table(nsk_graph *g, const SegLaunchPlan &pl, int ph, int burnin, const CounterSrc &src) {
    // (under a ChainSwap the one-chain launches sample the one chain.  The capture needs no such test, and this one is the
    // same there: only nsk_gibbs_run captures, and chains_run sweeps a swapped handle through gibbs_eager alone.)
    const bool chains = g->nchains > 1 && !g->chain_swapped;
    const bool wide = sizeof(VT) == 1 && pl.tab.wide;
    // a wave per tile pair while that fits the resident grid, else its waves loop over quads
    const unsigned nbp = (unsigned)pl.grid;
#define NSK_TAB_ARGS view<VT>(g), pl.tab, burnin, src.K0, src.K1, src.S0, src.S1, src.sweep_base, src.sweep_off
#define NSK_TAB(NCH, K, NB, ...) K<VT, NCH><<<dim3(NB), dim3(NSK_BLOCK), 0, g->stream>>>(__VA_ARGS__)
    if (chains) {
        const TabChains ch{nbp, 0u, (long long)g->chain_stride};
        if (wide) launch_tabw(g, pl, burnin, src, true);
        else NSK_BY_NCH(NSK_TAB, k_gibbs_seg_tab_chains, (unsigned)g->nchains * nbp, NSK_TAB_ARGS, ch);
    }
    else if (g->p2p.fused_now) {        // (the border waves of the sweep's first class with border tiles wait for the peers)
        TabP2P px;
        nsk_p2p_fill(g, px, src.sweep_base, src.tag, ph == g->p2p.first_phase);
        NSK_BY_NCH(NSK_TAB, k_gibbs_seg_tab_p2p, nbp, NSK_TAB_ARGS, px);
    }
    else if (wide) launch_tabw(g, pl, burnin, src, false);
    else NSK_BY_NCH(NSK_TAB, k_gibbs_seg_tab, nbp, NSK_TAB_ARGS);
#undef NSK_TAB
#undef NSK_TAB_ARGS
}
// batched chain launches: a handle with several chains whose sweep is table launches only, its values in their domains,
// and the kernels' 32-bit offsets valid for the last chain
static bool chains_batched(nsk_graph *g, int sample_evidence) {
    if (g->nchains < 2 || g->chain_swapped || g->scan != NSK_SCAN_CHROMATIC || !g->values_regular || !nsk_tables_only(g) ||
        nsk::diag_env("NSK_NO_CHAIN_BATCH"))
        return false;
    ensure_seg_plans(g, sample_evidence);
    if (!g->seg_plans_all_tab) return false;
    const long long shift = (long long)(g->nchains - 1) * (long long)(g->chain_stride / 256);
    if (g->c.vbytes == 1 && !(val_offset_fits(g, g->seg_wide, shift) && val_offset_fits(g, g->ztab, shift)))
        for (const auto &v : g->seg_plans)
            for (const SegLaunchPlan &pl : v)
                if (pl.tab.wide) return false;
    return true;
}

// ---- the launches of a class plan (nsk_class_plan.h), one routine per kernel family ----
static_assert(PLAN_BLOCK == NSK_BLOCK, "nsk_class_plan.h copies the kernels' block size");

// what the launches of one eager sweep share
template <typename VT>
struct EagerSweep { nsk_graph *g; DevGraph<VT> d; int sample_evidence, burnin; CounterSrc src; };
#define NSK_SWEEP_TAIL(W) (W).sample_evidence, (W).burnin, (W).src.K0, (W).src.K1, (W).src.S0, (W).src.S1

// hubs (one wave per variable) + general tiles + the class's rest tiles
template <typename VT, int MAXC>
static void launch_general(const EagerSweep<VT> &w, const ClassShape &s, const GeneralLaunch &L, hipStream_t st) {
    k_gibbs_general<VT, MAXC><<<dim3(L.grid), dim3(NSK_BLOCK), 0, st>>>(
        w.d, s.fb, s.fe, s.wb_base, L.tile0, L.ntiles, L.nblocks, s.fe, s.he, L.hblocks, s.hub0,
        w.g->rest_tiles + s.rest0, L.nrest, NSK_SWEEP_TAIL(w));
}
// entry-parallel groups: hubs, the class's general tiles and its rest tiles
template <typename VT>
static void launch_ep(const EagerSweep<VT> &w, const ClassShape &s, const GeneralLaunch &L, hipStream_t st) {
#define NSK_EP(K, MAXC) K<VT, MAXC><<<dim3(L.grid), dim3(NSK_BLOCK), 0, st>>>(                                                       \
        w.d, s.fb, s.fe, s.wb_base, L.tile0, L.ntiles, s.ngroups, s.group0, L.gblocks, s.fe, s.he, L.hblocks, s.hub0, s.nbh, s.bh0, \
        w.g->rest_tiles + s.rest0, L.nrest, NSK_SWEEP_TAIL(w))
    if (L.capped) NSK_EP(k_gibbs_ep_w5, 8); else if (L.maxc == 8) NSK_EP(k_gibbs_ep, 8); else NSK_EP(k_gibbs_ep, 2);
#undef NSK_EP
}
// generic CSR kernel, one lane per variable
template <typename VT>
static void launch_generic(const EagerSweep<VT> &w, const ClassShape &s, const SimpleLaunch &L, hipStream_t st) {
    k_gibbs_phase<VT><<<dim3(L.grid), dim3(NSK_BLOCK), 0, st>>>(w.d, s.he, s.e, NSK_SWEEP_TAIL(w));
}
// a prepared segment launch without a draw table: the inlined-adjacency kernel of its kind
template <typename VT>
static void launch_seg(const EagerSweep<VT> &w, const SegLaunchPlan &pl) {
    const int nb = (pl.tab.ntiles + 3) / 4;         // a wave per tile
    const dim3 grid(pl.grid);
#define NSK_SEG(NCH, KIND) k_gibbs_seg<VT, KIND, NCH><<<grid, dim3(NSK_BLOCK), 0, w.g->stream>>>(w.d, pl.tab, nb, w.burnin, w.src.K0, w.src.K1, w.src.S0, w.src.S1)
    if (pl.kind == 4) NSK_BY_NCH(NSK_SEG, 4);
    else if (pl.kind == 2) NSK_BY_NCH(NSK_SEG, 2);
    else if (pl.kind == 0) NSK_BY_NCH(NSK_SEG, 0);
    else NSK_BY_NCH(NSK_SEG, 3);
#undef NSK_SEG
}
// the rest tiles no general launch took: descriptor-driven kernel
template <typename VT>
static void launch_fast(const EagerSweep<VT> &w, const ClassShape &s, const SimpleLaunch &L) {
    k_gibbs_fast<VT><<<dim3(L.grid), dim3(NSK_BLOCK), 0, w.g->stream>>>(
        w.d, s.fb, s.fe, s.wb_base, plan_quarter(L.n), w.g->rest_tiles + s.rest0, L.n, NSK_SWEEP_TAIL(w));
}

template <typename VT>
static int gibbs_impl(nsk_graph *g, int64_t nsweeps, int sample_evidence, int burnin) {
    DevGraph<VT> d = view<VT>(g);
    if (g->scan == NSK_SCAN_SEQUENTIAL) {
        k_seq_gibbs<VT><<<dim3(1), dim3(64), 0, g->stream>>>(d, g->v_pos, g->mt_np, (int)nsweeps,
                                                            sample_evidence, burnin);
        HIPCHECK(hipGetLastError());
        g->launches++;
        g->sweep += (uint64_t)nsweeps;
    } else {
        const size_t nphase = g->c.phase_start.size() - 1;
        nsk_refresh_prog_weights(g);
        ensure_seg_plans(g, sample_evidence);
        // every class's plan, once per call: cheap, and nothing a sweep changes enters it
        std::vector<ClassShape> shapes(nphase);
        std::vector<GibbsClassPlan> plans(nphase);
        PlanOpts opts;
        opts.overlap = !g->no_overlap;
        opts.value_bytes = (size_t)g->c.nid * (size_t)g->c.vbytes;
        opts.grid_cap = plan_grid_cap(nsk::diag_env("NSK_CLASS_GRID_CAP"));     // (diagnostic: a small group grid, later trips)
        for (size_t ph = 0; ph < nphase; ph++) {
            shapes[ph] = class_shape(g->c, ph);
            if (shapes[ph].ep && shapes[ph].fe > shapes[ph].fb)
                opts.ep_per_cu = plan_per_cu(nsk::diag_env("NSK_EP_PER_CU"));        // (diagnostic: workgroups per CU)
            plans[ph] = plan_gibbs_class(shapes[ph], opts);
        }
        for (int64_t s = 0; s < nsweeps; s++) {
            // uint8 tally: folded BEFORE the sweep that would take a byte past 255, whatever left the residue -- sweeps of
            // this loop or, from an earlier call, replays that stopped at 255 exactly (nsk_gibbs_run folds the same way)
            if (!burnin && g->pos_tally_sweeps >= 255) nsk_fold_position_tally(g);
            if (g->pack_now && !burnin && g->packed_sweeps >= 127) (void)nsk_unpack_tally(g);       // 7 tally bits per value byte
            if (g->p2p.fused_now) ++g->p2p.tag;            // the exchange rides in this sweep's table launches
            const EagerSweep<VT> w{g, d, sample_evidence, burnin, CounterSrc::eager(g)};
            for (size_t ph = 0; ph < nphase; ph++) {
                const ClassShape &cl = shapes[ph];
                const GibbsClassPlan &p = plans[ph];
                ColourStreams cs(g, !g->no_overlap);
                const GeneralLaunch &L = p.general;
                // (the all-binary launch, and only it, goes behind the generic kernel's fork: L.behind_generic)
                if (L.on && !L.behind_generic) {
                    if (L.ep) launch_ep<VT>(w, cl, L, cs.of(L.stream));
                    else launch_general<VT, 8>(w, cl, L, cs.of(L.stream));
                    g->launches++;
                }
                if (p.generic.on) { launch_generic<VT>(w, cl, p.generic, cs.of(p.generic.stream)); g->launches++; }
                if (L.on && L.behind_generic) { launch_general<VT, 2>(w, cl, L, g->stream); g->launches++; }
                if (p.segments)         // the launches prepared before the sweep loop
                    for (const SegLaunchPlan &pl : g->seg_plans[ph]) {
                        if (pl.kind >= 8) launch_table<VT>(g, pl, (int)ph, burnin, w.src);
                        else launch_seg<VT>(w, pl);
                        g->launches++;
                    }
                if (p.fast.on) { launch_fast<VT>(w, cl, p.fast); g->launches++; }
                cs.join();
            }
            g->sweep++;
            if (!burnin && g->pack_now) g->packed_sweeps++;
            if (!burnin) g->pos_tally_sweeps++;
        }
        HIPCHECK(hipGetLastError());
    }
    if (!burnin) g->cnt_dirty = true;
    g->sweeps_done += nsweeps;
    return NSK_OK;
}


#ifdef NSK_ABL_TIMING       // (instrumented build: the per-wave time stamps of the last wide-quad launch, tools/timing_tabw.py)
extern "C" int nsk_debug_dump(unsigned long long *out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(nsk::nsk_dbg), sizeof(unsigned long long) * (size_t)n);
}
#endif

static int gibbs_eager(nsk_graph *g, int64_t nsweeps, int sample_evidence, int burnin) {
    return NSK_BY_VT(g, gibbs_impl, g, nsweeps, sample_evidence, burnin);
}

// ---- captured sweep sequences (hipGraph) -------------------------------------------------------------
// A handle whose inference sweep consists of table launches only (grids and their shards: two ~4 us
// kernels per sweep, plus two exchange kernels in an N-rank run) is bound by launches, not by kernels.
// Does every sampled variable of the handle live in a table segment (the grids and their shards)?
bool nsk_tables_only(const nsk_graph *g) {
    const nsk::Compiled &c = g->c;
    const size_t nphase = c.phase_start.size() - 1;
    if (g->scan != NSK_SCAN_CHROMATIC || nphase == 0) return false;
    for (size_t ph = 0; ph < nphase; ph++) {
        const ClassShape s = class_shape(c, ph);
        if (s.e > s.fe) return false;                    // generic-path variables / hubs
        if (s.ntiles > s.gt0) return false;              // general tiles
        if (s.nrest > 0) return false;                   // tiles outside segments
    }
    for (const nsk::Compiled::Segment &sg : c.segments) if (sg.ztab < 0) return false;
    return true;
}

// the captured sweep sequences bake array addresses and exchange pointers: dropped when those change
void nsk_drop_sweep_graph(nsk_graph *g) {
    for (SweepGraph &sg : g->sweep_graphs) {
        if (sg.exec) { (void)hipGraphExecDestroy(sg.exec); sg.exec = nullptr; }
        sg.key = -1;
    }
}

// NSK_GRAPH_SWEEPS sweeps -- class launches, peer-to-peer push and wait/unpack -- are captured once into
// a hipGraph whose kernels read the sweep index (and the exchange tag) from device memory + a per-node
// offset, so the same executable graph serves every replay; a one-thread kernel at its end advances the
// counters.  The uint8 position tally is folded between replays when it would overflow.
static bool graph_eligible(const nsk_graph *g, bool p2p) {
    if (g->scan != NSK_SCAN_CHROMATIC || !g->values_regular || nsk::diag_env("NSK_NO_GRAPH")) return false;
    const nsk::Compiled &c = g->c;
    // launches set the pace only while the class kernels are short: beyond a few million variables per
    // handle (10M grid: 12 us per class) a replay saves nothing and its launch latency shows in short runs.
    // A handle that exchanges peer to peer adds two tiny kernels per sweep: its sequences are captured up
    // to twice the size (the two shards of the 10M grid)
    // (a handle with several chains: the work of one launch is every chain's)
    if (c.nsampled * (int64_t)std::max(1, g->nchains) > (p2p ? 6000000 : 3000000)) return false;
    return nsk_tables_only(g);
}

template <typename VT>
static int graph_build(nsk_graph *g, int burnin, bool p2p, int key, SweepGraph &sg) {
    hipGraphExec_t &exec = sg.exec;
    const int nsw = sg.nsweeps;
    if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
    sg.key = -1;
    hipGraph_t graph = nullptr;
    // (the legacy default stream cannot be captured: a caller that pointed the library at it -- torch's
    // current stream in a process without its own streams -- keeps the eager loop)
    if (g->stream == nullptr) return nsk::fail(NSK_E_DEVICE, "the default stream cannot be captured");
    HIPCHECK(hipStreamBeginCapture(g->stream, hipStreamCaptureModeThreadLocal));
    int launches = 0;
    for (int i = 0; i < nsw; i++) {
        for (size_t ph = 0; ph < g->seg_plans.size(); ph++)
            for (const SegLaunchPlan &pl : g->seg_plans[ph]) {
                launch_table<VT>(g, pl, (int)ph, burnin, CounterSrc::captured(g, i));     // (the exchange tag of sweep i: counter + i + 1)
                launches++;
            }
        if (p2p && !g->p2p.fused_now) {
            int rc = nsk_p2p_enqueue(g, g->d_counters, (unsigned int)(i + 1));
            if (rc) { (void)hipStreamEndCapture(g->stream, &graph); if (graph) (void)hipGraphDestroy(graph); return rc; }
        }
    }
    k_graph_counters<<<dim3(1), dim3(1), 0, g->stream>>>(g->d_counters, (unsigned long long)nsw, p2p ? (unsigned long long)nsw : 0ull, 0, 0ull, 0ull);
    hipError_t e = hipStreamEndCapture(g->stream, &graph);
    if (e != hipSuccess || !graph) return nsk::fail(NSK_E_DEVICE, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) { exec = nullptr; return nsk::fail(NSK_E_DEVICE, std::string("hipGraphInstantiate: ") + hipGetErrorString(e)); }
    sg.key = key;
    sg.launches = launches;
    return NSK_OK;
}

// keep_packed: a run of a traced call that another run of the same call follows (traced_sweeps) -- a packed tally stays in
// the value bytes when the run ends; the next run decides pack_now from the same handle state and carries packed_sweeps on
int nsk_gibbs_run(nsk_graph *g, int64_t nsweeps, int sample_evidence, int burnin, bool p2p, bool keep_packed) {
    int64_t left = nsweeps;
    // A shard whose sweep is table launches only exchanges its boundary INSIDE them (nsk_internal.h p2p_fused): the
    // ghosts the first sweep reads are packed into the receive block here, the wait for the peers' last flags and
    // the unpack into the value array are enqueued lazily (nsk_p2p_flush)
    bool fuse = false;
    if (p2p && g->p2p.fused && g->scan == NSK_SCAN_CHROMATIC && g->values_regular && nsweeps > 0) {
        ensure_seg_plans(g, sample_evidence);
        fuse = g->p2p.border_all && g->seg_plans_all_tab;
        // (a fused call right behind a fused call continues it: the receive block already holds what the first
        // sweep reads -- nothing to unpack into the value array and pack back)
        if (fuse && !g->p2p.close_pending) {
            int rc = nsk_p2p_ghost_pack(g);
            if (rc) return rc;
        }
    }
    if (!fuse) { int frc = nsk_p2p_flush(g); if (frc) return frc; }
    g->p2p.close_pending = false;
    g->p2p.fused_now = fuse;
    // Packed tally (nsk_internal.h): a whole-graph handle whose every launch of this call is the wide-quad kernel's keeps
    // the tally inside the value bytes while the call runs; it is unpacked before the call returns
    g->pack_now = false;
    if (!p2p && !burnin && g->nchains == 1 && g->scan == NSK_SCAN_CHROMATIC && g->values_regular && g->c.vbytes == 1 && nsweeps > 0 &&
        nsk_tables_only(g) && !nsk::diag_env("NSK_NO_PACK_TALLY")) {
        ensure_seg_plans(g, sample_evidence);
        g->pack_now = g->seg_plans_all_wide;
    }
    struct Done { nsk_graph *g; bool fuse, keep; ~Done() { g->p2p.fused_now = false; if (fuse) g->p2p.close_pending = true;
                                                            if (!keep) (void)nsk_unpack_tally(g);
                                                            g->pack_now = false; } } done{g, fuse, keep_packed};
    // (under a ChainRange the sequences stay as they are: they hold the whole handle's pointers and chain count)
    if (left >= NSK_GRAPH_SWEEPS && !g->chain_view && graph_eligible(g, p2p)) {
        // the plans of this (sample_evidence, tables) combination and the tables of the current weights (what an eager
        // sweep does in front of its launches; an eager sweep in front of the replays cost a 400-sweep call of the 1M grid
        // 16 sweeps outside them -- this one and the 15 that 399 leaves over)
        int rc = NSK_OK;
        nsk_refresh_prog_weights(g);
        ensure_seg_plans(g, sample_evidence);
        // (what a sequence was captured for, beside the plans: planning again drops every sequence)
        const int key = (burnin ? 8 : 0) | (p2p ? 16 : 0) | (fuse ? 32 : 0) | (g->pack_now ? 64 : 0);
        if (g->seg_plans_all_tab && left >= NSK_GRAPH_SWEEPS) {
            // two sizes: NSK_GRAPH_SWEEPS_BIG sweeps per replay while the call is long enough, NSK_GRAPH_SWEEPS for what is left
            for (int big = (left >= NSK_GRAPH_SWEEPS_BIG && !nsk::diag_env("NSK_NO_BIG_GRAPH")) ? 1 : 0; big >= 0; big--) {
                SweepGraph &sg = g->sweep_graphs[big];
                const int nsw = sg.nsweeps;
                if (left < nsw || g->sweep_graph_off) continue;
                if (sg.key != key) {
                    rc = NSK_BY_VT(g, graph_build, g, burnin, p2p, key, sg);
                    if (rc) {               // capture is an optimisation: without it the eager loop runs
                        g->sweep_graph_off = true;
                        (void)hipGetLastError();
                        continue;
                    }
                }
                k_graph_counters<<<dim3(1), dim3(1), 0, g->stream>>>(g->d_counters, g->sweep, g->p2p.tag, 1, g->seed, g->rng_tag);
                while (left >= nsw && sg.key == key) {
                    if (!burnin && g->pos_tally_sweeps + nsw > 255) nsk_fold_position_tally(g);   // uint8 tally
                    if (g->pack_now && g->packed_sweeps + nsw > 127) (void)nsk_unpack_tally(g);   // 7 bits in a value byte
                    HIPCHECK(hipGraphLaunch(sg.exec, g->stream));
                    g->sweep += (uint64_t)nsw;
                    if (p2p) g->p2p.tag += (unsigned int)nsw;
                    if (!burnin) { g->pos_tally_sweeps += nsw; g->cnt_dirty = true; if (g->pack_now) g->packed_sweeps += nsw; }
                    g->sweeps_done += nsw;
                    g->launches += sg.launches;
                    left -= nsw;
                }
            }
            HIPCHECK(hipGetLastError());
        }
    }
    for (; left > 0; left--) {              // the rest eagerly (one sweep at a time when exchanging with kernels of their own)
        int rc = gibbs_eager(g, (p2p && !fuse) ? 1 : left, sample_evidence, burnin);
        if (rc) return rc;
        if (!p2p || fuse) break;
        if ((rc = nsk_p2p_enqueue(g, nullptr, 0))) return rc;
    }
    return NSK_OK;
}

// A handle with several chains (nsk_set_chains): the table launches of a sweep serve every chain at once (chains_batched:
// eager or captured, through nsk_gibbs_run); any other handle samples chain after chain, each through a ChainSwap view
// of the handle (its values and tallies, key word 1 XOR r) by the one-chain launches, from the same sweep index on.
static int chains_run(nsk_graph *g, int64_t nsweeps, int sample_evidence, int burnin) {
    if (g->scan != NSK_SCAN_CHROMATIC) return fail(NSK_E_INVALID, "several chains: the sequential scan samples one chain");
    if (chains_batched(g, sample_evidence)) return nsk_gibbs_run(g, nsweeps, sample_evidence, burnin, false);
    const uint64_t sweep0 = g->sweep;
    const int pts0 = g->pos_tally_sweeps;
    const int64_t done0 = g->sweeps_done;
    for (int r = 0; r < g->nchains; r++) {
        ChainSwap cs(g, r);
        g->sweep = sweep0; g->pos_tally_sweeps = pts0; g->sweeps_done = done0;
        const int rc = gibbs_eager(g, nsweeps, sample_evidence, burnin);
        if (rc) return rc;
    }
    return NSK_OK;
}

// Chain r of the handle alone (nsk_pt.hip: a replica under its own weight table): what chains_run's loop does for one
// chain -- the one-chain launches through a ChainSwap view, eagerly, from the handle's sweep index on.  The caller sets
// the sweep index and sweeps_done back between replicas; with burnin == 0 the sweeps are tallied into chain r's arrays and
// pos_tally_sweeps counts them.
int nsk_gibbs_chain(nsk_graph *g, int r, int64_t nsweeps, int sample_evidence, int burnin) {
    if (g->scan != NSK_SCAN_CHROMATIC) return fail(NSK_E_INVALID, "one chain of several: the sequential scan is not served");
    ChainSwap cs(g, r);
    return gibbs_eager(g, nsweeps, sample_evidence, burnin);
}

// (keep_packed: nsk_gibbs_run; only a one-chain handle keeps its tally in the value bytes)
static int sweeps_run(nsk_graph *g, int64_t nsweeps, int sample_evidence, int burnin, bool keep_packed = false) {
    if (g->nchains > 1) return chains_run(g, nsweeps, sample_evidence, burnin);
    return nsk_gibbs_run(g, nsweeps, sample_evidence, burnin, false, keep_packed);
}

// Tallied sweeps of a handle that records a sample trace (nsk_trace_setup): the call is split into runs that end where a
// row is due, every run goes through the path an untraced call takes (captured sequences and batched chain launches
// included; chains that are not batched go chain after chain through the RUN), and one record launch follows it on
// the stream.  A sweep's samples depend on the seed, the layout and the sweep index only, so the split call leaves the
// values and tallies of the unsplit one.  A handle that keeps its tally in the value bytes (pack_now) stays packed
// between the runs of one call: bit 0 is the value either way, and the record kernels read nothing else of a packed row.
// Everything that can refuse does so before the first sweep is enqueued.
static int traced_sweeps(nsk_graph *g, int64_t nsweeps, int sample_evidence) {
    NskTrace &t = g->trace;
    if (t.chains != g->nchains) return fail(NSK_E_INVALID, "nsk_gibbs_sweeps: the chain count changed under the sample trace");
    if (t.packed && !g->values_regular)
        return fail(NSK_E_RANGE, "nsk_gibbs_sweeps: a value lies outside its domain and the sample trace keeps one bit per binary variable");
    if (t.rows + (t.phase + nsweeps) / t.every > t.capacity)
        return fail(NSK_E_RANGE, "nsk_gibbs_sweeps: the call needs more rows than the sample trace has left");
    for (int64_t left = nsweeps; left > 0;) {
        const int64_t run = std::min(left, t.every - t.phase);
        int rc = sweeps_run(g, run, sample_evidence, 0, t.packed && left > run);     // (the call's last run unpacks)
        if (!rc) {
            left -= run;
            t.phase += run;
            if (t.phase == t.every) { rc = nsk_trace_record(g); t.phase = 0; }
        }
        if (rc) { (void)nsk_unpack_tally(g); return rc; }
    }
    return NSK_OK;
}

extern "C" int nsk_gibbs_sweeps(nsk_graph *g, int64_t nsweeps, int sample_evidence, int burnin) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (nsweeps < 0 || nsweeps > INT32_MAX) return fail(NSK_E_INVALID, "bad sweep count");
    if (nsweeps == 0) return NSK_OK;
    HIPCHECK(hipSetDevice(g->device));
    if (g->trace.capacity > 0 && g->scan != NSK_SCAN_CHROMATIC)
        return fail(NSK_E_INVALID, "nsk_gibbs_sweeps: the handle records a sample trace (nsk_trace_setup), which the sequential scan "
                                   "does not serve; tear it down first (capacity = 0)");
    if (g->trace.capacity > 0 && !burnin) return traced_sweeps(g, nsweeps, sample_evidence);
    return sweeps_run(g, nsweeps, sample_evidence, burnin);
}
