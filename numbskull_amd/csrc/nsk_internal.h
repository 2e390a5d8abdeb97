// nsk_internal.h -- host-side state of a compiled graph handle, shared by the translation units of
// the library (nsk_api.hip: C-ABI, state sync; nsk_exchange.hip: the multi-GPU boundary exchange; nsk_gibbs.hip /
// nsk_learn.hip: the sweep drivers of numbskull/factorgraph.py:141,163,202; nsk_trace.hip, nsk_energy.hip, nsk_wstats.hip,
// nsk_cond.hip: the diagnostics; nsk_icm.hip: the greedy MAP search; nsk_temper.hip: tempered sweep schedules;
// nsk_smc.hip: population annealing on top of them; nsk_pt.hip: parallel tempering; nsk_plgrad.hip: the pseudo-likelihood
// gradient and MPLE learning; nsk_pcd.hip: the chain-summed moments and persistent contrastive divergence, fully observed
// and with latent variables; nsk_bp.hip: loopy belief propagation).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/numbskull_amd.h"
#include "nsk_alloc.h"
#include "nsk_compile.h"
#include "nsk_device.h"
#include "nsk_kernels_gibbs.h"
#include "nsk_seg_plan.h"
#include "nsk_steps.h"

namespace nsk {
int fail(int code, const std::string &msg);       // records nsk_last_error, returns code
}

#define HIPCHECK(expr)                                                                          \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return nsk::fail(NSK_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));  \
    } while (0)

// Per-weight statistics (nsk_weight_stats / the trace's stats column; nsk_kernels_wstats.h).  A PLAN is the device work
// list of a selection of weights: one lane per short weight, one wave per piece of a longer one, a second launch for
// the weights of several pieces, each item with the output column it serves (nsk_wstats.hip wstats_plan_build).
#define NSK_WSTATS_SHORT 16         // a weight of at most this many factors is one lane's
#define NSK_WSTATS_PIECE 2048       // entries of one wave's piece (32 a lane)
#define NSK_WSTATS_MAX_BLOCKS 2048  // the lanes and waves of a larger plan loop (8 blocks per CU)
struct NskWstatsPlan {
    uint2 *shorts = nullptr;
    uint4 *pieces = nullptr, *multi = nullptr;
    double *partial = nullptr;         // partial_chains x npartial piece sums of the weights of several pieces
    unsigned int len_end[NSK_WSTATS_SHORT] = {};    // shorts below len_end[k] have at most k + 1 entries
    int64_t nshort = 0, npiece = 0, nmulti = 0, npartial = 0, ncols = 0;
    int partial_chains = 0;
};
// The by-weight index list (built on the host and uploaded at the first use), the plan of ALL weights and a query's
// result buffer.  wf_off stays on the host: the plans carry the offsets.  A handle that never asks holds none of this.
struct NskWstats {
    bool ready = false;
    std::vector<uint32_t> wf_off;      // [nweight + 1] by weight SLOT (f_rec.z): its entries in wf_idx
    std::vector<int32_t> wf_first;     // [nweight] the first of them (what the plans sort the short weights by)
    int32_t *wf_idx = nullptr;         // [nfactor] device: factor ids, ascending inside a weight
    bool all_ready = false;
    NskWstatsPlan all;                 // every weight, output column = the caller's id
    double *result = nullptr;          // result_chains x nweight
    int result_chains = 0;
};

// A selection of variables for the conditionals (nsk_conditionals / nsk_trace_conditionals; nsk_cond.hip): the caller's
// columns in the caller's order ("full" layout: column j owns card[j] doubles at off[j]) and the device's -- the
// positions of the selected variables that have one, ascending, without repeats; device column i owns the doubles
// [doff[i], doff[i + 1]) of a chain's device output.  col[j] = the device column of caller column j, -1: the variable
// has no position (it reads NaN).
struct NskCondSel {
    std::vector<int64_t> off, col;     // [ncols + 1], [ncols]
    std::vector<int32_t> sel;          // [ndev] positions
    std::vector<long long> doff;       // [ndev + 1]
    int32_t *d_sel = nullptr;          // device copies of sel and doff (nsk_cond_sel_upload)
    long long *d_off = nullptr;
    int64_t ncols() const { return (int64_t)col.size(); }
    int64_t total() const { return off.empty() ? 0 : off.back(); }
    int64_t ndev() const { return (int64_t)sel.size(); }
    int64_t dtotal() const { return doff.empty() ? 0 : (int64_t)doff.back(); }
};

// Sample trace (nsk_trace_setup): thinned joint samples recorded on the device.  After every `every`-th tallied sweep
// one k_trace_record_* launch appends a row: for every chain the values of the traced variables, in DEVICE column order
// (sorted by internal id; every internal id when cols == nullptr, "all variables") -- bit-packed, ceil(ndev / 64) words a
// chain, when every traced variable is binary, one element of vbytes a column otherwise.  pos[] undoes the order on download.
struct NskTrace {
    void *buf = nullptr;               // capacity x chains x row_bytes
    int32_t *cols = nullptr;           // device column -> internal id (nullptr: the identity over [0, nid))
    int64_t ncols = 0, ndev = 0;       // the caller's columns; the device's
    int64_t every = 0, capacity = 0;   // capacity == 0: no trace set up
    int64_t rows = 0, phase = 0;       // rows recorded; tallied sweeps since the last row (or set-up / clear)
    bool packed = false;
    int chains = 1;                    // the handle's chain count at set-up (nsk_set_chains refuses another while it lives)
    size_t row_bytes = 0;              // one chain's share of a row
    std::vector<int64_t> pos;          // the caller's column j is device column pos[j]
    std::vector<int32_t> card;         // ... and its variable's cardinality (the domain nsk_trace_value_* hold a value to)
    std::vector<int64_t> sweep_index;  // per recorded row: the handle's sweep index it was taken after
    double *lp = nullptr;              // the lp column (nsk_trace_log_potential): capacity x chains log-potentials, or off
    double *ws = nullptr;              // the stats column (nsk_trace_weight_stats): capacity x chains x ws_plan.ncols sums, or off
    NskWstatsPlan ws_plan;             // ... the work list of its selection
    bool ws_scaled = false;
    double *cond = nullptr;            // the accumulators (nsk_trace_conditionals): chains x cond_sel.dtotal() sums of probabilities, or off
    NskCondSel cond_sel;               // ... their selection
    int64_t cond_rows = 0;             // ... and the rows added to them since the selection was set or cleared
};

// Log-potential (nsk_log_potential / nsk_factor_values / the trace's lp column): the factor walk of nsk_kernels_energy.h
// reads f_rec, m_rec, v_card (and iid_of_vid on a graph with literal heads) -- the arrays nsk_ensure_generic uploads, taken
// from it when it ran, uploaded at the first use otherwise (nsk_energy.hip energy_ensure) -- and leaves one partial sum per
// block and chain.  A handle that never asks holds none of this.
struct NskEnergy {
    bool ready = false;                // every factor was checked and the arrays are on the device
    int chains = 0;                    // chains the buffers below serve
    double *partial = nullptr;         // chains x nsk_energy_blocks(nfactor) block partials
    double *result = nullptr;          // chains sums (a query's; a trace writes into its lp column)
};

// Belief propagation (nsk_bp_setup .. nsk_bp_clear; nsk_bp.hip, nsk_kernels_bp.h): the structure of one state's clamped
// and free variables, the tables, both message arrays and the beliefs, resident from set-up to clear.  Every device
// array is on the ledger and listed in `owned`; the host keeps the sizes and the beliefs' offsets by internal id.
// A handle holds two of them, slots 0 and 1 (nsk_graph::bp is the selected one); they share nothing.
struct NskBp {
    bool ready = false;
    nsk_bp_info info = {};
    bool big = false;                  // a free variable of cardinality above NSK_ZLOCAL has an edge: wk exists
    std::vector<long long> b_off;      // [nid + 1]
    std::vector<void *> owned;
    long long *pm_off = nullptr, *tab_off = nullptr, *msg_off = nullptr, *d_b_off = nullptr;
    int32_t *slot_off = nullptr, *edge_off = nullptr, *e_fac = nullptr, *e_var = nullptr;
    int32_t *v_list = nullptr, *v_eoff = nullptr, *v_edges = nullptr;
    int32_t *mrec = nullptr, *slot_rec = nullptr;
    uint8_t *v_state = nullptr;
    double *theta = nullptr, *psi = nullptr, *f2v = nullptr, *v2f = nullptr, *belief = nullptr, *wk = nullptr;
    double *feat = nullptr;            // the tables without the weight, filled with theta (nsk_bp_refresh, nsk_bp_moments)
    int32_t nvlist = 0, nvbin = 0;     // free variables with an edge; the binary ones among them, first in v_list
};

// Boundary exchange, the collective path (nsk_exchange.hip: nsk_exchange_setup, nsk_comm_init, nsk_*_sweeps_exchange):
// every rank packs the values its peers read into `send`, an all-gather -- the caller's, or RCCL's through `comm` --
// fills `recv` with every rank's slot, and the unpack scatters them to the ghost ids.  The handle owns the seven
// arrays (the ledger frees them; a repeated set-up replaces all seven) and the communicator (nsk_exchange_release).
struct NskGather {
    int world = 0;                     // 0: not set up
    int64_t slot = 0, nsend = 0, nrecv = 0;
    int32_t *send_vids = nullptr, *recv_vids = nullptr, *recv_slot = nullptr;      // internal ids; position in recv (-1: skipped)
    void *send = nullptr, *recv = nullptr, *send_evid = nullptr, *recv_evid = nullptr;   // slot and slot x world values, per chain
    void *comm = nullptr;              // ncclComm_t (nsk_comm_init); survives a repeated set-up
    void reset() { void *keep = comm; *this = NskGather(); comm = keep; }          // back to "not set up" (the arrays are the caller's to free first)
};

// Boundary exchange, the peer-to-peer path (nsk_exchange.hip: nsk_pf_setup, nsk_p2p_*): pairwise boundary lists, ONE
// fine-grained allocation per rank (flags | received values of both chains, two parities | weight deltas;
// nsk_kernels_misc.h), the peers' mappings of theirs, the exchange counter.  The handle owns the device arrays (ledger;
// a repeated nsk_p2p_setup replaces send_iid / recv_iid, nsk_p2p_export a block that became too small, the fuse plan
// its push map) and the hipIpc mappings of the peers' blocks (closed at the next import and by nsk_exchange_release).
struct NskP2PSetup {                   // what one nsk_p2p_setup .. import establishes
    int world = 0, rank = 0;           // world 0: not set up
    int64_t nsend = 0, nrecv = 0;
    std::vector<int64_t> soff, roff, dbase, dtotal;
    int32_t *send_iid = nullptr, *recv_iid = nullptr;
    std::vector<int32_t> send_host, recv_host;      // the send / receive lists (internal ids), host copies
    unsigned int peer_mask = 0, tag = 0;
    bool ready = false;                // set up, exported and the peers' blocks imported
    // Fused boundary exchange of the table launches (p2p_fuse_plan, nsk_kernels_gibbs.h TabP2P): the inference sweeps
    // of a handle that lives in table segments read their ghosts from the receive block and push their boundary values
    // from inside the class launches -- no exchange kernels per sweep
    bool fused = false;                // the handle qualifies (decided when the peers' buffers are imported)
    bool fused_now = false;            // ... and the running nsk_gibbs_sweeps_p2p call sweeps that way
    bool close_pending = false;        // the closing wait + unpack of the last fused sweep is not enqueued yet
    std::vector<int32_t> border_tiles; // sorted: tiles (position >> 6) that own a value a peer reads or read a ghost;
                                       //   a tile's rank here is its row in the push map
    uint32_t ghost_lo = 0, border_total = 0;   // first ghost id; border tiles one sweep of the current plans samples
    int first_phase = -1;              // the sweep's first class with table launches: its border tiles wait for the flags
    bool border_all = true;            // ... and that is every border tile (else the call takes the exchange kernels)
};
struct NskP2P : NskP2PSetup {          // ... and what outlives it: the block, the push map, the error / ticket words, the peers' mappings
    void *base = nullptr;
    size_t bytes = 0;
    uint32_t *push_map = nullptr;      // [rows][64] reader << 28 | index in the reader's receive block; NSK_NO_STREAM
    unsigned int *err = nullptr;       // [0] error mark, [1] [2] the kernels' tickets, [3] the fused launches' counter
    void *peer_base[16] = {nullptr};
    bool peer_ipc[16] = {false};       // mapped with hipIpcOpenMemHandle
    unsigned long long timeout_ticks = 3000000000ull;      // 30 s of the 100 MHz wall clock (NSK_P2P_TIMEOUT_S)
    // partial-factor aggregates this rank computes for its readers (nsk_pf_setup): value slots [nid, nid + npf)
    int64_t npf = 0;
    uint8_t *pf_op = nullptr;
    int32_t *pf_off = nullptr, *pf_mem = nullptr;
    void reset() { (NskP2PSetup &)*this = NskP2PSetup(); }     // back to "not set up" (send_iid / recv_iid are the caller's to free first)
};

// blocks of the factor walk, a function of nfactor ALONE (the sum must not depend on anything else): one lane per factor
// up to 8 blocks per CU, grid-stride beyond; whole rounds of XCDs
#define NSK_ENERGY_MAX_BLOCKS 2048
static inline unsigned int nsk_energy_blocks(long long nfactor) {
    const long long need = (nfactor + 255) / 256;
    return (unsigned int)(need < 8 ? 8 : (need >= NSK_ENERGY_MAX_BLOCKS ? NSK_ENERGY_MAX_BLOCKS : (need + 7) / 8 * 8));
}

// one captured sweep sequence (nsk_gibbs.hip graph_build): the executable graph, what it was captured for (-1: nothing),
// the kernel launches of one replay and its sweeps
#define NSK_GRAPH_SWEEPS 16
#define NSK_GRAPH_SWEEPS_BIG 64
struct SweepGraph { hipGraphExec_t exec; int key, launches, nsweeps; };

// F<VT>(...) with the value type of the handle G
#define NSK_BY_VT(G, F, ...) ((G)->c.vbytes == 1 ? F<int8_t>(__VA_ARGS__) : F<int32_t>(__VA_ARGS__))

struct nsk_graph {
    nsk::Compiled c;
    NskTrace trace;
    NskEnergy energy;
    NskWstats wstats;
    NskBp bp;                          // the SELECTED set-up: every nsk_bp_* call acts on it (nsk_bp_select)
    NskBp bp_other;                    // ... and the one that is not: nsk_bp_select swaps the two
    int bp_slot = 0;                   // which of the two slots `bp` is (nsk_bp_latent_steps: 0 clamped, 1 free)
    // The segment launches (nsk_seg_plan.h), kept across calls (the N-rank loops sweep one epoch per call) together with
    // the options they were planned for; a call whose options differ plans again.  Learning: per Compiled::learn_seg entry.
    std::vector<nsk::LearnSegPlan> learn_seg_plans;
    nsk::SegPlanOpts learn_seg_opts;
    // Inference: per colour.  seg_plans_valid is also cleared where something the options only point at changes (the
    // border tiles, the arrays' addresses); planning again drops the captured sweep sequences.
    std::vector<std::vector<nsk::SegLaunchPlan>> seg_plans;
    nsk::SegPlanOpts seg_opts;
    bool seg_plans_valid = false;
    bool seg_plans_all_tab = false, seg_plans_all_wide = false;   // every plan is a table launch (kind 8); ... a wide one
    // captured sweep sequences (hipGraph): [0] NSK_GRAPH_SWEEPS inference sweeps of a handle whose sweep is
    // table launches only (+ the peer-to-peer exchange), replayed with the sweep index in device memory;
    // [1] NSK_GRAPH_SWEEPS_BIG of them for long calls (the one-thread kernel that advances the counters and the
    // replay's own latency are ~5 us per replay: 4 % of a 16-sweep replay of the 1M grid)
    SweepGraph sweep_graphs[2] = {{nullptr, -1, 0, NSK_GRAPH_SWEEPS}, {nullptr, -1, 0, NSK_GRAPH_SWEEPS_BIG}};
    bool sweep_graph_off = false;                  // capture failed once (e.g. the legacy default stream): eager from then on
    unsigned long long *d_counters = nullptr;      // [0] sweep index, [1] exchange tag, [2] Philox key, [3] shard tag
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // the kernels of one colour class are independent: hubs and generic-path variables run on side
    // streams next to the tile kernels (fork/join with events around every colour)
    hipStream_t side[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    bool no_overlap = nsk::diag_env("NSK_NO_OVERLAP") != nullptr;     // diagnostic: one stream
    NskLedger mem;                     // every device array below and what it counts for (nsk_alloc.h; nsk_graph_info.device_bytes)
    // device arrays
    int32_t *p_vid = nullptr, *p_slot = nullptr, *p_cnt = nullptr, *slot_off = nullptr, *fidx = nullptr;
    uint32_t *p_info = nullptr, *f_rec = nullptr;
    void *p_init = nullptr;
    int32_t *iid_of_vid = nullptr;
    int32_t *m_rec = nullptr, *v_card = nullptr,
            *v_pos = nullptr;
    double *f_feat = nullptr, *w = nullptr, *logtab = nullptr;
    uint8_t *w_fixed = nullptr;
    uint32_t *w_direct = nullptr;      // bit per weight: updated in place by the learning kernels (nsk_compile.h)
    int32_t *multi_wids = nullptr;     // the other weights: what k_apply_weights walks then
    void *val = nullptr, *val_evid = nullptr;
    int32_t *cnt = nullptr;
    uint8_t *cnt_pos = nullptr;
    int pos_tally_sweeps = 0;      // sweeps accumulated in the uint8 position tally
    // Packed tally (k_gibbs_seg_tabw): while a nsk_gibbs_sweeps call runs on a handle whose every launch is the wide-quad
    // kernel's, the tally of its sweeps lives in the value bytes (bit 0 value, bits 1-7 count): one store per trip
    // instead of two.  packed_sweeps = tallied sweeps since the last k_unpack_tally (at most 127; 0 whenever the
    // library returns to the caller: every other reader of values sees plain 0 / 1).
    int packed_sweeps = 0;
    bool pack_now = false;         // the running call sweeps in packed mode
    uint32_t *adj = nullptr, *tiles = nullptr, *tile_hdr = nullptr, *gstream = nullptr, *gs_off = nullptr;
    double *prog_w = nullptr, *adj_wt = nullptr;
    uint32_t *tile_wrow = nullptr;
    uint4 *ztab = nullptr;              // draw tables (k_refresh_ztab)
    uint32_t *seg_aff = nullptr;        // implicit adjacency of table segments
    uint32_t *seg_wide = nullptr, *wide_exc = nullptr;   // wide quads of table segments (nsk_compile.h)
    uint8_t *sink = nullptr;            // scratch line for padding lanes' stores
    uint32_t *hub_desc = nullptr, *hub_adj = nullptr;   // entry-parallel hub streams
    uint32_t *ep_desc = nullptr, *ep_adj = nullptr;     // entry-parallel groups of general tiles
    uint32_t *bighub_pos = nullptr, *ep_wrow = nullptr, *ep_kstat = nullptr, *ep_win = nullptr, *ep_win_off = nullptr;
    double *ep_wt = nullptr;
    nsk::ZProgDev *zprogs = nullptr;
    bool values_regular = true;         // every value on the device lies in [0, cardinality): the
                                        // table kernels index with the neighbours' low bits
    bool chain_regular[2] = {true, true};   // ... per chain (var_value, var_value_evid)
    double compile_seconds = 0;
    nsk::RouteCounts route_counts = {0, 0, 0, 0, 0, 0, 0};   // nsk_graph_info's tile / group counters, counted once (nsk_graph_get_info)
    bool have_route_counts = false;
    uint32_t *dyn_tiles = nullptr, *rest_tiles = nullptr, *learn_rest_tiles = nullptr;
    int acc_copies = 1;                // copies of the global learning accumulators (one per XCD, or 1)
    int bins_xcd = 0;                  // SMALLW bins private to XCDs (close_sink)
    bool generic_uploaded = false;     // CSR-style arrays of the generic kernels are on the device
    double learn_cap = 0.5;            // per-class cap on visits * step of one weight (nsk_set_learn_cap)
    unsigned int *clip_count = nullptr;   // weight updates whose step was clipped (device counter)
    long long *part_G = nullptr;       // SMALLW: NSK_LEARN_BINS bins of partial sums per weight
    uint32_t *part_K = nullptr, *part_T = nullptr;
    bool smallw = false;
    // One-class-lagged learning (nsk_set_learn_lag, default on): class c samples with the weights as of
    // the end of class c - 2 while the update of class c - 1 runs beside it (block 0 of the class's table
    // launch) or behind it; weights, slot-program terms, draw tables and accumulators exist twice (set 0 =
    // the arrays above) and the classes alternate between them.
    bool learn_lag = true;
    double *w1 = nullptr, *prog_w1 = nullptr;
    uint4 *ztab1 = nullptr;
    long long *G1 = nullptr, *part_G1 = nullptr;
    uint32_t *K1 = nullptr, *T1 = nullptr, *part_K1 = nullptr, *part_T1 = nullptr;
    // state transfer (nsk_state_upload / nsk_state_download): values cross PCIe narrowed (1 or 4 bytes) in the
    // caller's order through pinned staging buffers; the permutation to layout order runs on the device
    void *xfer_host[2] = {nullptr, nullptr};       // pinned, nvar * vbytes each (one per chain)
    void *xfer_dev = nullptr;                      // nvar * vbytes
    int32_t *xfer_iid = nullptr;                   // internal id of every variable
    void *cnt_host = nullptr;                      // pinned, ncount * 4: the tally crosses PCIe as int32 when it fits
    int32_t *cnt_dev32 = nullptr;
    unsigned int *cnt_wide = nullptr;
    bool weights_dirty = true;      // prog_w must be rebuilt before the next fast-path launch
    bool weights_exposed = false;
    std::vector<double> w_stage;        // host staging of weight transfers when the table is in slot order (wmap)
    bool adj_wt_skip = false;       // learning reads weights directly: skip the shape-tile rows until the next inference   // the weight buffer was handed out: assume it changes between calls
    // boundary exchange (multi-GPU): the collective path, the peer-to-peer path, and what the weight merge of both keeps
    NskGather gather;
    NskP2P p2p;
    double *w_start = nullptr, *w_delta = nullptr;     // the weights an epoch started from; this rank's share of the change (nsk_ensure_w_start)
    long long *cnt_total = nullptr, *G = nullptr;
    uint32_t *K = nullptr, *T = nullptr;
    nsk::MTState *mt_np = nullptr, *mt_py = nullptr;
    // run state
    uint64_t seed = 0, sweep = 0;
    // Generator ids are positions in THIS handle's layout, so two shards of one graph would draw
    // the same uniforms at equal positions: Philox counter word 3 is the sweep index's high half
    // XOR this tag -- the first variable id the handle owns (disjoint shards => distinct tags;
    // 0 for a handle that owns the whole graph).
    uint32_t rng_tag = 0;
    int scan = NSK_SCAN_CHROMATIC;
    bool cnt_dirty = false;
    int64_t sweeps_done = 0;
    // Several chains (nsk_set_chains): R value arrays, position tallies, delta tallies and masters over ONE compiled
    // layout and weight table.  Once a handle's chain count was set, chain r's values lie at val + r chain_stride and its
    // uint8 position tally at cnt_pos + r chain_stride (one slab: values in the first half of each chain's stride, the
    // tally in the second, so cnt_pos - val is the same for every chain -- k_gibbs_seg_tabw_chains); its int32 and int64
    // tallies at cnt / cnt_total + r ncount.  The handle's pointers are chain 0's except while ChainSwap points them at
    // another chain (launches of the kernel families that sample one chain per launch).
    int nchains = 1;
    size_t chain_stride = 0;
    bool chains_regular = true;    // the values of chains 1 .. R - 1 lie in their domains (see values_regular)
    bool chain_swapped = false;    // a ChainSwap is active: the pointers are one chain's, the sweep samples that chain only
    bool chain_view = false;       // a ChainRange is active: the pointers and nchains are a range's; no captured sequence runs
    // profiling bracket
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int64_t launches = 0, launches_at_begin = 0;
};

// The allocation helpers of every translation unit: a device array is entered in the handle's ledger with the
// (n ? n : 1) * sizeof(T) bytes it counts for (fine: a fine-grained allocation, the peer-to-peer block) ...
template <typename T>
static int dev_alloc(nsk_graph *g, T **ptr, size_t n, bool fine = false) {
    size_t bytes = (n ? n : 1) * sizeof(T);
    void *p = nullptr;
    // (diagnostic, NSK_DIAG=1 NSK_ALLOC_ALIGN=1: arrays of a megabyte or more start on a 2 MB boundary whatever the
    // allocator does -- where the arrays of the table kernels lie moves their launch time by 3 %)
    static const bool align2m = nsk::diag_env("NSK_ALLOC_ALIGN") != nullptr;
    const size_t big = (size_t)1 << 20, two = (size_t)2 << 20;
    const bool al = align2m && bytes >= big && !fine;
    hipError_t e = fine ? hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained) : hipMalloc(&p, al ? bytes + two : bytes);
    if (e != hipSuccess) return nsk::fail(fine ? NSK_E_DEVICE : NSK_E_NOMEM, std::string(fine ? "hipExtMallocWithFlags: " : "hipMalloc: ") + hipGetErrorString(e));
    void *raw = p;
    if (al) p = (void *)(((uintptr_t)p + two - 1) / two * two);
    g->mem.add(p, raw, bytes);
    *ptr = (T *)p;
    return NSK_OK;
}
// ... and dev_free takes it off again (null is a no-op)
static inline void nsk_free_raw(void *raw) { (void)hipFree(raw); }
static inline void dev_free(nsk_graph *g, void *p) { if (void *raw = g->mem.remove(p)) nsk_free_raw(raw); }
template <typename T>
static int dev_upload(nsk_graph *g, T **ptr, const std::vector<T> &h) {
    int rc = dev_alloc(g, ptr, h.size());
    if (rc) return rc;
    if (!h.empty()) HIPCHECK(hipMemcpyAsync(*ptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, g->stream));
    return NSK_OK;
}
// a buffer that lives for one call of `who`: dev_alloc, with the refusal that names it
template <typename T>
static int call_alloc(nsk_graph *g, T **ptr, size_t n, const std::string &who, const char *what) {
    const int rc = dev_alloc(g, ptr, n);
    if (rc != NSK_E_NOMEM) return rc;
    return nsk::fail(NSK_E_NOMEM, who + ": " + what + " (" + std::to_string((long long)((n ? n : 1) * sizeof(T))) + " bytes) do not fit on the device");
}
// a check of nsk_steps.h as a return code
static inline int refuse(const std::string &why) { return why.empty() ? NSK_OK : nsk::fail(NSK_E_INVALID, why); }

// The per-step outputs of a learner's call (nsk_pcd_steps, nsk_pcd_latent_steps, nsk_bp_learn_steps): gmax[T], the bit
// patterns of the steps' largest gradients, and -- where the caller keeps the moments -- rows[T x k x nweight] int64 by
// slot.  On the ledger from alloc_* to the end of the call.
struct StepOutputs {
    nsk_graph *g;
    size_t T, k, nw;
    unsigned long long *gmax = nullptr;
    long long *rows = nullptr;
    std::vector<unsigned long long> hmax;
    std::vector<long long> hrows;
    StepOutputs(nsk_graph *g_, size_t T_, size_t k_) : g(g_), T(T_), k(k_), nw((size_t)g_->c.nweight) {}
    ~StepOutputs() { dev_free(g, rows); dev_free(g, gmax); }
    int alloc_gmax(const std::string &who) { return call_alloc(g, &gmax, T, who, "the largest gradients, 8 bytes a step"); }
    int alloc_rows(const std::string &who) {
        return call_alloc(g, &rows, T * k * nw, who, k == 1 ? "the kept moments, nsteps x nweight int64" : "the kept moments, nsteps x 2 x nweight int64");
    }
    hipError_t zero() { return hipMemsetAsync(gmax, 0, T * sizeof(unsigned long long), g->stream); }
    long long *row(size_t t) const { return rows ? rows + t * k * nw : nullptr; }       // step t's, or null
    // enqueue the copies to the host (the caller synchronises the stream) ...
    hipError_t download() {
        hmax.resize(T);
        hrows.resize(rows ? T * k * nw : 0);
        hipError_t e = hipMemcpyAsync(hmax.data(), gmax, T * sizeof(unsigned long long), hipMemcpyDeviceToHost, g->stream);
        if (rows && e == hipSuccess) e = hipMemcpyAsync(hrows.data(), rows, hrows.size() * sizeof(long long), hipMemcpyDeviceToHost, g->stream);
        return e;
    }
    // ... and hand them over: the rows by the caller's weight ids (either may be null)
    void deliver(double *gmax_out, int64_t *moments) const {
        if (gmax_out) std::memcpy(gmax_out, hmax.data(), T * sizeof(double));
        if (moments) nsk::SlotMap(g->c).from_slots(hrows.data(), moments, T * k);
    }
};

// The chains an entry point names: `which` is NSK_BUF_VALUE (chains [first_chain, first_chain + nchains) of the handle's)
// or NSK_BUF_VALUE_EVID (the evidence chain, which exists once).  one: the entry point takes a single chain.
static inline int chain_select(const nsk_graph *g, int which, int64_t first_chain, int64_t nchains, const std::string &who, bool one = false) {
    if (which != NSK_BUF_VALUE && which != NSK_BUF_VALUE_EVID) return nsk::fail(NSK_E_INVALID, who + ": which must be NSK_BUF_VALUE or NSK_BUF_VALUE_EVID");
    const int64_t R = which == NSK_BUF_VALUE ? g->nchains : 1;
    if (first_chain < 0 || nchains < 1 || first_chain >= R || nchains > R - first_chain)
        return nsk::fail(NSK_E_INVALID, who + (one ? ": chain" : ": chains") + " outside those the handle has (the evidence chain exists once)");
    return NSK_OK;
}
// ... and where the first of them lies (const char * to a reader, char * to nsk_icm, which writes)
static inline char *chain_val(const nsk_graph *g, int which, int64_t first_chain) {
    return which == NSK_BUF_VALUE ? (char *)g->val + (size_t)first_chain * g->chain_stride : (char *)g->val_evid;
}

#define NSK_MAX_CHAINS 1024
// entry points that serve one chain only: refused on a handle with several (nsk_set_chains)
#define NSK_ONE_CHAIN(G, WHAT)                                                                                         \
    do {                                                                                                               \
        if ((G)->nchains > 1)                                                                                          \
            return nsk::fail(NSK_E_INVALID, std::string(WHAT) + ": the handle has several chains (nsk_set_chains); "   \
                                            "only chromatic inference sweeps (nsk_gibbs_sweeps) serve them");          \
    } while (0)
// entry points a handle with a sample trace refuses (nsk_trace_setup): rows are taken behind the inference sweeps of
// nsk_gibbs_sweeps only
#define NSK_NO_TRACE(G, WHAT)                                                                                          \
    do {                                                                                                               \
        if ((G)->trace.capacity > 0)                                                                                   \
            return nsk::fail(NSK_E_INVALID, std::string(WHAT) + ": the handle records a sample trace "                 \
                                            "(nsk_trace_setup); tear it down first (capacity = 0)");                   \
    } while (0)
// Points the handle's per-chain state at chain r while it lives: values, tallies, and the key (word 1 XOR r -- chain r
// draws what a one-chain handle seeded seed ^ (r << 32) draws)
struct ChainSwap {
    nsk_graph *g;
    void *val; uint8_t *cnt_pos; int32_t *cnt; long long *cnt_total; uint64_t seed;
    ChainSwap(nsk_graph *g_, int r) : g(g_), val(g_->val), cnt_pos(g_->cnt_pos), cnt(g_->cnt), cnt_total(g_->cnt_total), seed(g_->seed) {
        g->chain_swapped = true;
        const size_t off = (size_t)r * g->chain_stride, nc = (size_t)r * (size_t)g->c.ncount;
        g->val = (char *)val + off; g->cnt_pos = cnt_pos + off; g->cnt = cnt + nc; g->cnt_total = cnt_total + nc;
        g->seed = seed ^ ((uint64_t)(uint32_t)r << 32);
    }
    ~ChainSwap() { g->val = val; g->cnt_pos = cnt_pos; g->cnt = cnt; g->cnt_total = cnt_total; g->seed = seed; g->chain_swapped = false; }
};
// Points the handle at its chains [r0, r0 + n) while it lives: values and tallies are chain r0's and nchains == n, so
// what nsk_gibbs_sweeps(.., burnin = 1) enqueues serves those n chains and no other -- the batched chain launches, the
// ChainSwap loop (which nests: it offsets from the view's pointers) or, with n == 1, the one-chain launches.  The key
// stays the handle's: local chain i (global chain r0 + i) draws what a one-chain handle seeded seed ^ (i << 32) draws,
// which is what the kernels make of the launch-local chain index -- no kernel and no kernel argument knows of the view.
// Captured sweep sequences bake the whole handle's pointers and chain count, so nsk_gibbs_run takes the eager path
// under a view (chain_view) and leaves the sequences alone: they stay valid for the whole handle unless the plans are
// made again, which drops them.  values_regular stays the conjunction over ALL chains of the handle.
struct ChainRange {
    nsk_graph *g;
    void *val; uint8_t *cnt_pos; int32_t *cnt; long long *cnt_total; int nchains;
    ChainRange(nsk_graph *g_, int r0, int n) : g(g_), val(g_->val), cnt_pos(g_->cnt_pos), cnt(g_->cnt), cnt_total(g_->cnt_total), nchains(g_->nchains) {
        const size_t off = (size_t)r0 * g->chain_stride, nc = (size_t)r0 * (size_t)g->c.ncount;
        g->val = (char *)val + off; g->cnt_pos = cnt_pos + off; g->cnt = cnt + nc; g->cnt_total = cnt_total + nc;
        g->nchains = n;
        g->chain_view = true;
    }
    ~ChainRange() { g->val = val; g->cnt_pos = cnt_pos; g->cnt = cnt; g->cnt_total = cnt_total; g->nchains = nchains; g->chain_view = false; }
};

// Philox counter word 3 of every sweep kernel (see rng_tag)
static inline uint32_t nsk_sweep_hi(const nsk_graph *g) { return (uint32_t)(g->sweep >> 32) ^ g->rng_tag; }

template <typename VT>
static nsk::DevGraph<VT> view(nsk_graph *g) {
    nsk::DevGraph<VT> d;
    d.p_vid = g->p_vid; d.p_info = g->p_info; d.p_slot = g->p_slot; d.p_cnt = g->p_cnt;
    d.p_init = (const VT *)g->p_init;
    d.slot_off = g->slot_off; d.fidx = g->fidx;
    d.gstream = (const uint2 *)g->gstream; d.gs_off = g->gs_off;
    d.f_rec = (const uint4 *)g->f_rec; d.f_feat = g->f_feat;
    d.m_rec = (const int2 *)g->m_rec; d.v_card = g->v_card; d.iid_of_vid = g->iid_of_vid;
    d.w = g->w; d.w_fixed = g->w_fixed; d.logtab = g->logtab;
    d.val = (VT *)g->val; d.val_evid = (VT *)g->val_evid; d.cnt = g->cnt;
    d.G = g->G; d.K = g->K; d.T = g->T;
    d.adj = (const uint4 *)g->adj; d.tiles = (const uint4 *)g->tiles; d.tile_hdr = g->tile_hdr;
    d.prog_w = g->prog_w; d.adj_wt = g->adj_wt; d.tile_wrow = g->tile_wrow;
    d.part_G = g->part_G; d.part_K = g->part_K; d.part_T = g->part_T;
    d.nweight = (int32_t)g->c.nweight;
    d.packed_grad = g->c.packed_grad ? 1 : 0;
    d.grad_mul = 1ll << (32 - g->c.grad_shift);
    d.grad_inv = 1.0 / (double)d.grad_mul;
    d.acc_copies = g->acc_copies;
    d.bins_xcd = g->bins_xcd;
    d.cnt_pos = g->cnt_pos;
    d.ztab = g->ztab;
    d.sink = g->sink;
    d.hub_desc = (const uint4 *)g->hub_desc; d.hub_adj = g->hub_adj;
    d.ep_desc = (const uint4 *)g->ep_desc; d.ep_adj = g->ep_adj; d.bighub_pos = g->bighub_pos;
    d.ep_wrow = g->ep_wrow; d.ep_wt = g->ep_wt;
    d.ep_win = g->c.ep_win.empty() ? nullptr : g->ep_win; d.ep_win_off = g->ep_win_off;
    d.ep_kstat = g->c.ep_kstat.empty() ? nullptr : g->ep_kstat;
    d.seg_aff = (const uint4 *)g->seg_aff;
    d.seg_wide = g->seg_wide; d.wide_exc = (const uint2 *)g->wide_exc;
    d.w_direct = g->c.ndirect > 0 ? g->w_direct : nullptr;
    d.upd_step = 0.0; d.upd_reg_param = 0.0; d.upd_truncation = 1.0; d.upd_cap = 0.0; d.upd_regularization = 0; d.upd_a1 = 1.0;
    d.upd_clipped = g->clip_count;
    d.nvar = (int32_t)g->c.nvar;
    d.head_by_vid = (g->c.flags & NSK_FLAG_HEAD_BY_VID) ? 1 : 0;
    return d;
}

// Streams for the kernels of one colour: the tile kernels stay on the main stream; when there are
// tile kernels to overlap with, hubs go to side stream 0, the generic kernel to side stream 1 and
// the categorical general tiles to side stream 2.
struct ColourStreams {
    nsk_graph *g;
    bool forked[3] = {false, false, false};
    bool overlap;
    bool recorded = false;
    ColourStreams(nsk_graph *g_, bool overlap_) : g(g_), overlap(overlap_) {}
    // side streams must be requested before anything of the colour is put on the main stream
    hipStream_t side(int i) {
        if (!overlap) return g->stream;
        if (!recorded) { (void)hipEventRecord(g->ev_fork, g->stream); recorded = true; }
        if (!forked[i]) { (void)hipStreamWaitEvent(g->side[i], g->ev_fork, 0); forked[i] = true; }
        return g->side[i];
    }
    hipStream_t of(int i) { return i < 0 ? g->stream : side(i); }      // a class plan's stream (nsk_class_plan.h PlanStream)
    void join() {
        for (int i = 0; i < 3; i++)
            if (forked[i]) {
                (void)hipEventRecord(g->ev_join[i], g->side[i]);
                (void)hipStreamWaitEvent(g->stream, g->ev_join[i], 0);
                forked[i] = false;
            }
    }
};

// the fast path reads weights through prog_w (and the draw tables): rebuilt whenever weights may
// have changed (nsk_api.hip)
extern "C" int nsk_ensure_generic(nsk_graph *g);       // internal (not in the public header)
// one chain's device values at `src` -> the caller's ids, int64, through staging buffer k; synchronises (nsk_api.hip)
extern "C" int nsk_download_values(nsk_graph *g, const void *src, int64_t *dst, int k);
int nsk_ensure_lag_sets(nsk_graph *g);                 // second set of weights / tables / accumulators (nsk_api.hip)
// one peer-to-peer exchange on the library's stream; tag_base != null: a captured launch whose tag is
// the device counter + tag_off; learn: both chains + the weight deltas; part 0 = all of it, 1 = the
// pushes only, 2 = wait + unpack (+ the owner's half of the weight merge), 3 = the closing half of the
// weight merge (nsk_exchange.hip)
int nsk_p2p_enqueue(nsk_graph *g, const unsigned long long *tag_base, unsigned int tag_off, bool learn = false, int part = 0);
bool nsk_tables_only(const nsk_graph *g);           // every sampled variable lives in a table segment (nsk_gibbs.hip)
int nsk_p2p_ghost_pack(nsk_graph *g);
void nsk_exchange_release(nsk_graph *g);           // nsk_graph_destroy: the peers' hipIpc mappings and the RCCL communicator (nsk_exchange.hip)
int nsk_p2p_flush(nsk_graph *g);                   // enqueue the pending closing wait + unpack of a fused sweep sequence, if any
void nsk_p2p_fill(nsk_graph *g, nsk::TabP2P &px, const unsigned long long *tag_base, unsigned int tag, bool wait);   // kernel argument of a fused launch
void nsk_drop_sweep_graph(nsk_graph *g);            // the captured sweep sequence bakes exchange pointers: drop it when they change
int nsk_gibbs_run(nsk_graph *g, int64_t nsweeps, int sample_evidence, int burnin, bool p2p, bool keep_packed = false);   // nsk_gibbs.hip
int nsk_gibbs_chain(nsk_graph *g, int r, int64_t nsweeps, int sample_evidence, int burnin);   // chain r alone, eagerly (nsk_gibbs.hip)
void nsk_refresh_prog_weights(nsk_graph *g, bool force = false);
void nsk_refresh_ztab(nsk_graph *g, int set = 0, hipStream_t st = nullptr);
int nsk_fold_position_tally(nsk_graph *g);
int nsk_unpack_tally(nsk_graph *g);
int nsk_trace_record(nsk_graph *g);                 // one row of the sample trace behind what the stream holds (nsk_trace.hip)
void wstats_plan_free(nsk_graph *g, NskWstatsPlan &plan);      // nsk_wstats.hip (the trace's stats column goes with the trace)
int nsk_wstats_ensure(nsk_graph *g, bool scaled, const char *what);    // ... the by-weight list at the first use (after energy_ensure)
// the range rule of the int64 moment sums over `nchains` chains: NSK_E_RANGE naming the weight (nsk_pcd.hip; nsk_bp.hip asks with 1)
int nsk_moments_range(const nsk_graph *g, int64_t nchains, const char *what);
// the handles the diagnostics serve (whole graph, no exchange); the arrays of the factor walk at the first use (nsk_energy.hip)
int energy_whole_graph(const nsk_graph *g, const char *what);
int energy_ensure(nsk_graph *g, int chains, const char *what);
// ... its part that the conditionals share: f_rec, m_rec, v_card and, with `literal`, iid_of_vid, where the handle lacks them
int nsk_records_ensure(nsk_graph *g, bool literal, const char *what);
// the arrays potential() reads, each where the handle lacks it (nsk_cond.hip; nsk_icm walks the same lists)
int cond_ensure(nsk_graph *g, const char *what);
// the accumulators of a sample trace: sums[r * sel.dtotal() + ..] += the conditionals of chain r at `val`, one launch (nsk_cond.hip)
int nsk_cond_accumulate(nsk_graph *g, const NskCondSel &sel, const void *val, int nchains, bool packed_bytes, double *sums);
void nsk_cond_sel_free(nsk_graph *g, NskCondSel &sel);      // the device copies of a selection (the trace's goes with the trace)
namespace nsk { struct EnergyArgs; }
nsk::EnergyArgs energy_args(const nsk_graph *g);
// the log-potential of `nchains` chains from `val` on / every factor's value, enqueued on the handle's stream (nsk_energy.hip)
int nsk_energy_enqueue(nsk_graph *g, const void *val, int nchains, bool packed_bytes, double *out);
int nsk_factor_values_enqueue(nsk_graph *g, const void *val, double *out);
// the per-weight statistics of `nchains` chains from `val` on, as `plan` lists them: chain r's sums at out + r * out_stride
// (nsk_wstats.hip; the columns of weights without a factor are not written)
int nsk_wstats_enqueue(nsk_graph *g, const NskWstatsPlan &plan, const void *val, int nchains, bool packed_bytes, bool scaled,
                       double *out, int64_t out_stride);
