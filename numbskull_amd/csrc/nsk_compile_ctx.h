// nsk_compile_ctx.h -- internal to the graph compiler (nsk_compile*.cpp; nothing else includes it): the constants the
// stages share, the diagnostic switches of one compile_graph call (CompileKnobs) and the state the stages hand on
// (CompileCtx).  The stages are CompileCtx's member functions, one file per group of stages; compile_graph
// (nsk_compile.cpp) calls them in order.
#pragma once

#include <chrono>
#include <cstdio>
#include <string>
#include <vector>

#include "nsk_compile.h"

namespace nsk {

// a variable whose factor lists hold at least this many entries in total is sampled by a whole wave
static const int64_t NSK_HEAVY_LIST = 32;
// ... and so is every generic-path variable of a colour class that has at most this many of them
static const int64_t NSK_FEW_GENERIC = 32768;
// stream words per lane of a shape tile at most (role program in TileShape::key, 32 words).  A lane walks its
// words chunk by chunk, every chunk a load and then its gathers: longer lists belong to the entry-parallel
// groups.  Measured on the 4M-variable weighted boolean graph (tools/sessions/history/r4_s24.sh, r4_s25.sh; learning /
// inference, updates/s): 16 words 3.68e9 / 1.28e10, 20 words 2.93e9 / 1.18e10, 24 words 1.72e9 / 1.11e10,
// 32 words 2.2e8 / 5.3e9.
static const int64_t NSK_SHAPE_WORDS = 16;
// ... and the same limit for variables the entry-parallel groups can take.  Once the single-factor weights had
// slots in layout order (nsk_compile.h wmap) the groups overtook the shape tiles at every list length; same
// graph, every rest tile with a wave of its own (tools/sessions/history/r4_s31.sh .. r4_s33.sh), learning / inference:
// 20 words 4.20e9 / 1.20e10, 16 words 4.78e9 / 1.30e10, 12 words 5.25e9 / 1.56e10, 10 words 5.61e9 / 1.60e10,
// 8 words 6.13e9 / 1.60e10, 6 words 6.35e9 / 1.59e10, 4 words 6.56e9 / 1.60e10.
static const int64_t NSK_SHAPE_WORDS_EP = 4;
// a member slot of a shape tile that a lane does not have (its entry has fewer members than the tile's layout)
static const uint32_t NSK_SHAPE_NULL = 0xFFFFFFFFu;

static inline bool is_cat_function(int fn) { return fn == 12 || (fn >= 14 && fn <= 17); }
static inline bool literal_head_function(int fn) { return fn == 13 || fn == 16 || fn == 17; }

static inline std::string fmt(const char *f, long long a = 0, long long b = 0, long long c = 0) {
    char buf[256];
    snprintf(buf, sizeof(buf), f, a, b, c);
    return std::string(buf);
}

// Every environment switch the compiler looks at, read once at the start of every compile_graph call (read_knobs,
// nsk_compile.cpp -- the only place of the compiler that reads the environment; never cached: tests and tools set
// switches between calls of one process).  The layout switches count only with NSK_DIAG=1 (diag_env, nsk_compile.h);
// the three reporting switches are plain.  Defaults and clamps as the stages always had them.
struct CompileKnobs {
    // weights and gradients (nsk_compile_tiles.cpp)
    bool no_direct = false, no_worder = false, no_packed = false;
    // colouring (nsk_compile_colour.cpp)
    bool no_recolour = false, no_balance = false;
    int recolour_passes = 6;
    // eligibility and word lists (nsk_compile_words.cpp)
    bool no_fast = false, no_general = false, no_word_cache = false;
    int64_t gen_max_entries = 16;                   // [1, 24]
    // positions (nsk_compile_place.cpp)
    int64_t gen_block = 262144, ep_block = 1024;    // >= 64
    bool no_pad_shape = false, no_shape = false, no_heavy = false, no_ep = false, no_run_pad = false;
    int64_t shape_parts = 0;                        // >= 1; 0: not set, one part per 2^18 variables (at most 64)
    int64_t shape_words = NSK_SHAPE_WORDS, shape_words_ep = NSK_SHAPE_WORDS_EP;    // NSK_SHAPE_MAX_WORDS, [4, 32], sets both
    // tiles (nsk_compile_tiles.cpp: no_shape too)
    bool no_ztab = false;
    // segments (nsk_compile_segments.cpp; no_wide and wide_min also decide the run padding of the positions)
    bool no_affine = false, no_wide = false, no_learn_seg = false;
    int64_t wide_min = 400000;                      // variables per handle from which wide quads pay (read_knobs)
    const char *debug_var = nullptr;                // NSK_DEBUG_VAR: comma-separated variable ids to report
    // groups (nsk_compile_groups.cpp)
    bool no_kstat = false, no_ep_win = false, no_hub_ep = false;
    // reporting (plain getenv)
    bool verbose = false, debug_wide = false, debug_tiles = false;
};

struct CompileCtx {
    const nsk_graph_desc *d;
    Compiled &c;
    std::string &err;
    const CompileKnobs knobs;
    CompileCtx(const nsk_graph_desc *d_, Compiled &c_, std::string &err_, const CompileKnobs &k)
        : d(d_), c(c_), err(err_), knobs(k), t_last(std::chrono::steady_clock::now()) {}

    bool head_by_vid = false;           // NSK_FLAG_HEAD_BY_VID
    bool no_general = false;            // no general tiles: the switch, or ids that would not fit their 27-bit member field
    int32_t ncolors = 0;
    std::vector<uint8_t> sampled;       // [nvar] this handle samples the variable
    std::vector<uint8_t> fast;          // [nvar] 1 fast path, 2 general tile, 0 generic
    // compact read lists (build_read_lists); use_rd = false: too long, walk the records
    std::vector<int64_t> rd_off;
    std::vector<int32_t> rd_len, rd;
    bool use_rd = true;
    // word cache of the general-tile variables (mark_general; nsk_compile_words.cpp)
    std::vector<std::vector<uint32_t>> gw_chunk;           // the words, id order inside a chunk
    std::vector<int64_t> gw_v0;                            // first variable of every chunk (ascending)
    std::vector<uint32_t> gw_at;                           // [nvar] start inside the variable's chunk
    std::vector<uint8_t> gw_len;                           // [nvar] words (a lane's list is at most 120); 0: not kept
    // [shape_at[k], shape_end[k]): the positions of colour k's shape classes (place_variables -> shape_tiles)
    std::vector<int64_t> shape_at, shape_end;
    // tiles (shape_tiles -> fill_tiles, find_direct_weights): their number, colour of each, stream size in 16-byte units
    int64_t nwb = 0;
    std::vector<int32_t> tile_colour;
    uint64_t total4 = 0;
    std::chrono::steady_clock::time_point t_last;

    void lap(const char *what);         // closes a timed stage (reported with NSK_VERBOSE)

    // reads(v) = members of every factor in v's lists (+ the literal head index variable)
    template <typename Fn>
    void for_each_read_slow(int64_t v, Fn &&fn_) const {
        const nsk_variable &var = d->variable[v];
        const int64_t nslots = var.dataType == 0 ? 1 : var.cardinality;
        for (int64_t k = 0; k < nslots; k++) {
            const nsk_vtf &vt = d->vmap[var.vtf_offset + k];
            for (int64_t j = 0; j < vt.factor_index_length; j++) {
                const int64_t f = d->factor_index[vt.factor_index_offset + j];
                const nsk_factor &fa = d->factor[f];
                const int fnid = fa.factorFunction;
                if (fnid == -1) continue;
                int64_t need = (fnid == 21 || fnid == 22 || fnid == 25 || fnid == 26) ? 2
                             : (fnid == 23 || fnid == 24) ? 3 : (fnid >= 18 && fnid <= 20) ? 1 : 0;
                int64_t s = fa.ftv_offset, e = std::max(s + fa.arity, s + need);
                if (fnid == 30) e = std::max(e, s + d->variable[d->fmap[s].vid].cardinality - 1);
                for (int64_t l = s; l < e; l++) fn_(d->fmap[l].vid);
                if (literal_head_function(fnid) && !head_by_vid) fn_(s + fa.arity - 1);
            }
        }
    }
    // ... from the read lists once they exist: fn_(b) for every variable b != v that v reads, ascending
    template <typename Fn>
    void for_each_read(int64_t v, Fn &&fn_) const {
        if (!use_rd) { for_each_read_slow(v, fn_); return; }
        const int32_t *p = rd.data() + rd_off[v];
        for (int32_t j = 0, n = rd_len[v]; j < n; j++) fn_((int64_t)p[j]);
    }
    // the weight's slot in the device table (nsk_compile.h wmap; the caller's id until the numbering exists:
    // eligibility and the shapes of pass 1 never look at a direct weight's id)
    uint32_t slot_of_weight(int64_t wid) const {
        return (c.wmap.empty() || wid < 0 || wid >= c.nweight) ? (uint32_t)wid : (uint32_t)c.wmap[(size_t)wid];
    }

    // the stages, in the order compile_graph runs them
    int check_descriptor();             // nsk_compile.cpp
    int build_records();
    int validate_reachable();           // nsk_compile_colour.cpp
    void build_read_lists();
    void colour_sampled();
    void find_ghosts();
    void mark_fast();                   // nsk_compile_words.cpp
    void mark_general();
    int place_variables();              // nsk_compile_place.cpp
    int assign_internal_ids();
    int shape_tiles();                  // nsk_compile_tiles.cpp
    void find_direct_weights();
    bool number_direct_weights();
    void plan_segments();               // nsk_compile_segments.cpp
    void fill_tiles();                  // nsk_compile_tiles.cpp
    int build_ep_groups();              // nsk_compile_groups.cpp
    int build_segment_adjacency();      // nsk_compile_segments.cpp
    int build_segment_wide();
    void build_hub_streams();           // nsk_compile_groups.cpp
    void plan_learning_launches();      // nsk_compile_segments.cpp
    int build_index_and_census();       // nsk_compile_index.cpp

    // what the stages call (nsk_compile_words.cpp, _tiles.cpp)
    bool general_words_walk(int64_t v, std::vector<uint32_t> *out, bool hub, size_t hub_cap) const;
    bool general_words(int64_t v, std::vector<uint32_t> *out, bool hub = false, size_t hub_cap = 0) const;
    void lane_words(int64_t v, std::vector<uint32_t> &out) const;
    void choose_gradient_format();
};

}  // namespace nsk
