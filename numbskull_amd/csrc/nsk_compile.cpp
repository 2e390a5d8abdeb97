// nsk_compile.cpp -- validate + colour + lay out a factor graph for the device: the pipeline (compile_graph), the
// descriptor checks, the narrow records, the switches of a call (read_knobs) and the hash of a whole layout.
//
// Input: the arrays a reference FactorGraph is built from (factorgraph.py:30-37) in their packed
// numpy layouts.  Output: the SoA device layout of DESIGN.md.  Nothing here runs per sweep.
// Fills here: the sizes, vbytes, flags, own_begin / own_end, v_card, v_init, cstart, ncount, values_regular, w_init,
// w_fixed, f_rec, f_feat, m_rec; everything else in the stage files (nsk_compile_ctx.h lists them in order).
#include "nsk_compile_ctx.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace nsk {

// The switches of one call.  The only function of the compiler that reads the environment.
// Wide quads pay from a few hundred thousand variables per handle on (one MI355X, us per sweep, tile-by-tile kernel /
// wide-quad kernel, tools/sessions/r6_s25.sh: 256 x 256 grid 6.63 / 6.60, 512 x 512 6.82 / 7.10, 500 x 1000 7.30 / 6.33, 1M grid
// 9.00 / 6.64, 4M 13.8 / 10.2-11.9, 10M 23.9 / 15.4) -- since the launch's few quads that are NOT wide are sampled by workgroups
// of their own (TabwCold.rest); while the waves whose turn they were sampled them in line, the bound was 3M (1M grid 9.1
// against 10.9).  NSK_DIAG=1 NSK_WIDE_MIN=n moves the bound (the small-grid tests use 0): wide_min.
static CompileKnobs read_knobs() {
    CompileKnobs k;
    auto on = [](const char *name) { return diag_env(name) != nullptr; };
    k.no_direct = on("NSK_NO_DIRECT"); k.no_worder = on("NSK_NO_WORDER"); k.no_packed = on("NSK_NO_PACKED");
    k.no_recolour = on("NSK_NO_RECOLOUR"); k.no_balance = on("NSK_NO_BALANCE");
    if (const char *e = diag_env("NSK_RECOLOUR_PASSES")) k.recolour_passes = atoi(e);
    k.no_fast = on("NSK_NO_FAST"); k.no_general = on("NSK_NO_GENERAL"); k.no_word_cache = on("NSK_NO_WORD_CACHE");
    if (const char *e = diag_env("NSK_GEN_MAX_ENTRIES")) k.gen_max_entries = std::max(1, std::min(24, atoi(e)));
    if (const char *e = diag_env("NSK_GEN_BLOCK")) k.gen_block = std::max<int64_t>(64, atoll(e));
    if (const char *e = diag_env("NSK_EP_BLOCK")) k.ep_block = std::max<int64_t>(64, atoll(e));
    k.no_pad_shape = on("NSK_NO_PAD_SHAPE"); k.no_shape = on("NSK_NO_SHAPE"); k.no_heavy = on("NSK_NO_HEAVY");
    k.no_ep = on("NSK_NO_EP"); k.no_run_pad = on("NSK_NO_RUN_PAD");
    if (const char *e = diag_env("NSK_SHAPE_PARTS")) k.shape_parts = std::max<int64_t>(1, atoll(e));
    if (const char *e = diag_env("NSK_SHAPE_MAX_WORDS")) k.shape_words = k.shape_words_ep = std::max<int64_t>(4, std::min<int64_t>(32, atoll(e)));
    k.no_ztab = on("NSK_NO_ZTAB");
    k.no_affine = on("NSK_NO_AFFINE"); k.no_wide = on("NSK_NO_WIDE"); k.no_learn_seg = on("NSK_NO_LEARN_SEG");
    if (const char *e = diag_env("NSK_WIDE_MIN")) k.wide_min = atoll(e);
    k.debug_var = diag_env("NSK_DEBUG_VAR");
    k.no_kstat = on("NSK_NO_KSTAT"); k.no_ep_win = on("NSK_NO_EP_WIN"); k.no_hub_ep = on("NSK_NO_HUB_EP");
    k.verbose = getenv("NSK_VERBOSE") != nullptr;
    k.debug_wide = getenv("NSK_DEBUG_WIDE") != nullptr;
    k.debug_tiles = getenv("NSK_DEBUG_TILES") != nullptr;
    return k;
}

void CompileCtx::lap(const char *what) {
    if (!knobs.verbose) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[nsk] compile %-28s %8.3f s\n", what, std::chrono::duration<double>(now - t_last).count());
    t_last = now;
}

// Descriptor checks: sizes, arrays, the owned range; the flags of the handle.
int CompileCtx::check_descriptor() {
    const int64_t nvar = d->nvar, nfac = d->nfactor, nedge = d->nedge, nw = d->nweight;
    const int64_t nvtf = d->nvtf, nfi = d->nfactor_index;
    const int64_t LIM = (int64_t)1 << 31;
    if (nvar < 0 || nfac < 0 || nedge < 0 || nw < 0 || nvtf < 0 || nfi < 0) {
        err = "negative size in graph descriptor";
        return NSK_E_INVALID;
    }
    if (nvar >= LIM - 1 || nfac >= LIM - 1 || nedge >= LIM - 1 || nw >= LIM - 1 || nfi >= LIM - 1 ||
        nvtf >= LIM - 1) {
        err = "graph too large for 32-bit device indices";
        return NSK_E_RANGE;
    }
    if ((nvar && !d->variable) || (nfac && !d->factor) || (nedge && !d->fmap) || (nw && !d->weight) ||
        (nvtf && !d->vmap) || (nfi && !d->factor_index)) {
        err = "null array in graph descriptor";
        return NSK_E_INVALID;
    }
    c.nvar = nvar; c.nfactor = nfac; c.nedge = nedge; c.nweight = nw; c.flags = d->flags;
    // NSK_FLAG_PARTITION: the owned range is taken literally -- (0, 0) is an EMPTY shard (what the
    // reference's shard formula yields for rank 0 when nvar < ranks).  Without the flag the handle
    // samples the whole graph; a non-zero range given without the flag is honoured too (round-1 ABI).
    int64_t ob = d->own_begin, oe = d->own_end;
    if (!(d->flags & NSK_FLAG_PARTITION) && ob == 0 && oe == 0) oe = nvar;
    if (ob < 0 || oe > nvar || ob > oe) {
        err = "owned range outside [0, nvar]";
        return NSK_E_INVALID;
    }
    c.own_begin = ob; c.own_end = oe;
    head_by_vid = (d->flags & NSK_FLAG_HEAD_BY_VID) != 0;
    // (general-tile member words keep the id in 27 bits: positions include padding, so stay well below)
    no_general = knobs.no_general || nvar >= (int64_t)100000000;
    return NSK_OK;
}

// Narrow copies of the caller's records: variables (with their checks), weights, factors and edges (validated lazily,
// for the factors that are reachable: validate_reachable).
int CompileCtx::build_records() {
    const int64_t nvar = d->nvar, nfac = d->nfactor, nedge = d->nedge, nw = d->nweight, nvtf = d->nvtf;
    const int64_t LIM = (int64_t)1 << 31;
    // ---- variables ---------------------------------------------------------------------------
    c.v_card.resize(nvar); c.v_init.resize(nvar); c.cstart.resize(nvar + 1);
    int64_t maxcard = 1, minval = 0, maxval = 0, cs = 0;
    for (int64_t v = 0; v < nvar; v++) {
        const nsk_variable &var = d->variable[v];
        if (var.cardinality < 1 || var.cardinality >= ((int64_t)1 << 22)) {
            err = fmt("variable %lld: cardinality %lld not in [1, 2^22)", v, var.cardinality);
            return NSK_E_RANGE;
        }
        int64_t nslots = var.dataType == 0 ? 1 : var.cardinality;
        if (var.vtf_offset < 0 || var.vtf_offset + nslots > nvtf) {
            err = fmt("variable %lld: vtf_offset %lld outside vmap", v, var.vtf_offset);
            return NSK_E_INDEX;
        }
        if (var.initialValue < INT32_MIN || var.initialValue > INT32_MAX) {
            err = fmt("variable %lld: initialValue does not fit int32", v);
            return NSK_E_RANGE;
        }
        // an evidence value is used as a value-slot / member index by the learning kernels
        // (learning.py:61-62 with get_factor_id_range's vmap[vtf_offset + value]): the reference
        // reads a neighbouring variable's lists or faults; here it is an error
        if (var.dataType != 0 && var.isEvidence == 1 &&
            (var.initialValue < 0 || var.initialValue >= var.cardinality)) {
            err = fmt("variable %lld: evidence value %lld outside its domain [0, %lld)", v, var.initialValue,
                      var.cardinality);
            return NSK_E_INDEX;
        }
        if (var.initialValue < 0 || var.initialValue >= var.cardinality) c.values_regular = false;
        c.v_card[v] = (int32_t)var.cardinality;
        c.v_init[v] = (int32_t)var.initialValue;
        maxcard = std::max(maxcard, var.cardinality);
        minval = std::min(minval, var.initialValue);
        maxval = std::max(maxval, var.initialValue);
        c.cstart[v] = cs;
        cs += var.cardinality == 2 ? 1 : var.cardinality;      // factorgraph.py:41-45
    }
    c.cstart[nvar] = cs;
    if (cs >= LIM - 1) {
        err = "tally array too large for 32-bit device indices";
        return NSK_E_RANGE;
    }
    c.ncount = cs;
    c.vbytes = (maxcard <= 127 && minval >= -128 && maxval <= 127) ? 1 : 4;

    // ---- weights -----------------------------------------------------------------------------
    c.w_init.resize(nw); c.w_fixed.resize(nw);
    for (int64_t i = 0; i < nw; i++) {
        c.w_init[i] = d->weight[i].initialValue;
        c.w_fixed[i] = d->weight[i].isFixed ? 1 : 0;
    }

    // ---- factors and edges: narrow copies; validated lazily for factors that are reachable ----
    c.f_rec.assign((size_t)nfac * 4 + 4, 0); c.f_feat.resize(nfac);
    for (int64_t f = 0; f < nfac; f++)
        if (d->factor[f].arity >= ((int64_t)1 << 24)) {
            err = fmt("factor %lld: arity %lld too large", f, d->factor[f].arity);
            return NSK_E_RANGE;
        }
    parallel_for(nfac, [&](int64_t fb0, int64_t fb1, int) {
    for (int64_t f = fb0; f < fb1; f++) {
        const nsk_factor &fa = d->factor[f];
        int64_t ar = fa.arity;
        if (ar < 0) ar = 0;
        c.f_rec[4 * f] = ((uint32_t)ar << 8) | (uint32_t)((fa.factorFunction + 1) & 0xff);
        c.f_rec[4 * f + 1] = (uint32_t)(int32_t)std::max<int64_t>(std::min<int64_t>(fa.ftv_offset, LIM - 2), -1);
        c.f_rec[4 * f + 2] = (uint32_t)(int32_t)std::max<int64_t>(std::min<int64_t>(fa.weightId, LIM - 2), -1);
        c.f_feat[f] = fa.featureValue;
    }
    });
    c.m_rec.assign((size_t)nedge * 2 + 2, 0);
    parallel_for(nedge, [&](int64_t lb0, int64_t lb1, int) {
    for (int64_t l = lb0; l < lb1; l++) {
        int64_t vid = d->fmap[l].vid, deo = d->fmap[l].dense_equal_to;
        c.m_rec[2 * l] = (vid < 0 || vid >= nvar) ? -1 : (int32_t)vid;
        c.m_rec[2 * l + 1] = (int32_t)std::max<int64_t>(std::min<int64_t>(deo, INT32_MAX), INT32_MIN);
    }
    });

    return NSK_OK;
}

// 64-bit hash of the compiled layout (nsk_graph_info.layout_hash): FNV-1a over 8-byte words per array, the arrays and
// scalars folded in the declaration order of struct Compiled -- every data member, none left out.  Doubles go in by
// their bit pattern; Segment and SegLaunch field by field (their raw bytes hold padding), in declaration order.
namespace {
struct LayoutHasher {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    static uint64_t bytes(const void *data, size_t n) {
        const unsigned char *p = (const unsigned char *)data;
        uint64_t x = 0xcbf29ce484222325ull ^ (uint64_t)n;
        size_t i = 0;
        for (; i + 8 <= n; i += 8) { uint64_t w; memcpy(&w, p + i, 8); x = (x ^ w) * 0x100000001b3ull; x ^= x >> 29; }
        for (; i < n; i++) x = (x ^ p[i]) * 0x100000001b3ull;
        return x;
    }
    void fold(uint64_t x) { h = (h ^ x) * 0x100000001b3ull; h ^= h >> 31; }
    void num(int64_t x) { fold((uint64_t)x); }
    void real(double x) { uint64_t w; memcpy(&w, &x, 8); fold(w); }
    template <typename T> void array(const std::vector<T> &v) { fold(bytes(v.data(), v.size() * sizeof(T))); }   // (T without padding)
    template <typename T, size_t N> void fixed(const T (&a)[N]) { fold(bytes(a, sizeof(a))); }
};
}  // namespace

int64_t layout_hash(const Compiled &c) {
    LayoutHasher H;
    H.num(c.nvar); H.num(c.nweight); H.num(c.nfactor); H.num(c.nedge); H.num(c.ncount);
    H.num(c.npos); H.num(c.nslot); H.num(c.nsampled); H.num(c.vbytes); H.num(c.flags);
    H.num(c.own_begin); H.num(c.own_end);
    H.array(c.color); H.array(c.phase_start); H.array(c.phase_end); H.array(c.phase_fast_end);
    H.array(c.phase_heavy_end); H.array(c.phase_wb_base); H.array(c.tiles); H.array(c.tile_wrow); H.num(c.nwrows);
    H.array(c.adj); H.array(c.hub_desc); H.array(c.hub_adj); H.array(c.phase_hub_base); H.array(c.bighub_pos);
    H.array(c.phase_bighub_base); H.num(c.nhub_ep); H.array(c.tile_hdr); H.array(c.dyn_tiles); H.array(c.phase_dyn_base);
    H.num((int64_t)c.segments.size());
    for (const Compiled::Segment &s : c.segments) {
        H.num(s.phase); H.num(s.pos0); H.num(s.ntiles); H.num(s.adj_off); H.num(s.prog); H.num(s.nslots); H.num(s.kind);
        H.num(s.ev); H.num(s.ztab); H.num(s.aff); H.num(s.wide);
    }
    H.array(c.seg_aff); H.array(c.seg_wide); H.array(c.wide_exc); H.num(c.ntab_quads); H.num(c.nwide_quads);
    H.array(c.zprogs);                                       // (four uint32, `pad` hashed as data)
    H.num(c.nztab); H.num(c.values_regular); H.num(c.has_ufo); H.real(c.grad_bound); H.num(c.grad_shift);
    H.array(c.rest_tiles);
    H.num((int64_t)c.learn_seg.size());
    for (const Compiled::SegLaunch &s : c.learn_seg) {
        H.num(s.phase); H.num(s.kind); H.num(s.nch); H.num(s.n); H.num(s.tab);
        H.fixed(s.tile_start); H.fixed(s.pos0); H.fixed(s.adj_off); H.fixed(s.prog); H.fixed(s.zoff); H.fixed(s.zmask);
        H.fixed(s.aff); H.fixed(s.ev); H.fixed(s.wide);
    }
    H.array(c.learn_rest_tiles); H.array(c.phase_learn_rest_base); H.array(c.phase_rest_base); H.array(c.phase_gen_tile);
    H.num(c.packed_grad); H.array(c.phase_gen_bin_tile);
    H.array(c.ep_desc); H.array(c.ep_adj); H.array(c.ep_wrow); H.array(c.ep_win); H.array(c.ep_win_off); H.array(c.ep_kstat);
    H.array(c.phase_ep_base); H.array(c.phase_ep); H.array(c.phase_ep_emax); H.num(c.nfast);
    H.array(c.p_vid); H.array(c.p_slot); H.array(c.p_cnt); H.array(c.p_info); H.array(c.p_init);
    H.array(c.slot_off); H.array(c.fidx); H.array(c.gstream); H.array(c.gs_off);
    H.array(c.f_rec); H.array(c.f_feat); H.array(c.m_rec); H.array(c.v_card); H.array(c.v_pos);
    H.array(c.iid); H.array(c.v_card_i); H.num(c.nid); H.num(c.zero_id); H.num(c.literal_heads); H.array(c.cstart);
    H.array(c.w_init); H.array(c.w_fixed); H.array(c.w_direct); H.array(c.repeated_factors); H.array(c.multi_wids);
    H.num(c.ndirect); H.array(c.wmap); H.array(c.wuser); H.array(c.logtab); H.array(c.ghost_needs); H.array(c.v_init);
    H.real(c.alg_bytes_inference); H.real(c.alg_bytes_learning);
    H.real(c.layout_bytes_inference); H.real(c.layout_bytes_learning);
    return (int64_t)(H.h >> 1);             // non-negative
}

int compile_graph(const nsk_graph_desc *d, Compiled &c, std::string &err) {
    CompileCtx x(d, c, err, read_knobs());
    int rc;
    if ((rc = x.check_descriptor())) return rc;
    if ((rc = x.build_records())) return rc;
    x.lap("records");
    if ((rc = x.validate_reachable())) return rc;
    x.lap("validate");
    // ---- colouring: no two variables of a colour may read each other ---------------------------
    x.build_read_lists();
    x.lap("read lists");
    x.colour_sampled();
    x.lap("balancing");
    x.find_ghosts();
    x.lap("ghosts");
    // ---- which kernel family takes a variable: fast path, general tile or the generic path
    x.mark_fast();
    x.lap("fast eligibility");
    x.mark_general();
    x.lap("general eligibility");
    // ---- positions (colour-major, classes inside a colour) and the internal ids that follow from them
    if ((rc = x.place_variables())) return rc;
    if ((rc = x.assign_internal_ids())) return rc;
    x.lap("positions");
    // ---- tiles: shapes, the weights updated in place, segments, then the stream
    if ((rc = x.shape_tiles())) return rc;
    x.lap("tile shapes (pass 1)");
    x.find_direct_weights();
    if (x.number_direct_weights()) x.lap("weight numbering");
    x.plan_segments();
    x.lap("segments");
    x.fill_tiles();
    x.lap("tile fill (pass 2)");
    // ---- what rides on tiles and segments
    if ((rc = x.build_ep_groups())) return rc;
    x.lap("entry-parallel groups");
    if ((rc = x.build_segment_adjacency())) return rc;
    if ((rc = x.build_segment_wide())) return rc;
    x.build_hub_streams();
    x.lap("compact streams");
    x.plan_learning_launches();
    return x.build_index_and_census();
}

}  // namespace nsk
