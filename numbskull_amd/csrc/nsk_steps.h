// nsk_steps.h -- what the host side of the full-batch learners shares (nsk_pcd.hip, nsk_bp.hip, nsk_plgrad.hip) and the
// cut of the by-weight list (nsk_wstats.hip, nsk_pcd.hip).  Like nsk_seg_plan.h, host only and pure: no HIP type, nothing
// of the handle (tests/test_steps_cpu.py pins it down without a GPU).  What needs the handle -- the per-call allocation,
// the owner of the per-step outputs -- lies beside dev_alloc in nsk_internal.h.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "nsk_compile.h"

namespace nsk {

// ---- the step parameters: each check returns the refusal's text, empty where the argument passes ----
static inline std::string check_nsteps(const std::string &who, int64_t nsteps, int64_t max) {
    if (nsteps >= 1 && nsteps <= max) return "";
    return who + ": nsteps must lie in [1, " + std::to_string((long long)max) + "]";
}
static inline std::string check_rates(const std::string &who, double step, double decay, double reg_param) {
    if (std::isfinite(step) && std::isfinite(decay) && std::isfinite(reg_param) && reg_param >= 0.0) return "";
    return who + ": step, decay and reg_param must be finite, reg_param not negative";
}
static inline std::string check_normalize(const std::string &who, int normalize) {
    return normalize == 0 || normalize == 1 ? "" : who + ": normalize must be 0 or 1";
}
static inline std::string check_target(const std::string &who, const double *target, size_t nweight) {
    for (size_t i = 0; i < nweight; i++)
        if (!std::isfinite(target[i])) return who + ": the target of weight " + std::to_string((long long)i) + " is not finite";
    return "";
}

// ---- weight slots: the device's weight table is in slot order where the compiler renumbered the weights (Compiled::wmap:
// slot of the caller's id; empty: the identity).  w_fixed is by slot too: a renumbered weight is a direct one, never fixed.
struct SlotMap {
    const int32_t *wmap;
    size_t nw;
    explicit SlotMap(const Compiled &c) : wmap(c.wmap.empty() ? nullptr : c.wmap.data()), nw((size_t)c.nweight) {}
    size_t slot(size_t id) const { return wmap ? (size_t)wmap[id] : id; }
    // by the caller's id -> by slot
    template <typename S, typename D>
    void to_slots(const S *src, D *dst) const { for (size_t i = 0; i < nw; i++) dst[slot(i)] = (D)src[i]; }
    // nrows rows by slot -> by the caller's id
    template <typename S, typename D>
    void from_slots(const S *src, D *dst, size_t nrows = 1) const {
        for (size_t r = 0; r < nrows; r++)
            for (size_t i = 0; i < nw; i++) dst[r * nw + i] = (D)src[r * nw + slot(i)];
    }
};

// the factors of every weight slot as the learners divide by them: a weight without a factor counts 1
static inline std::vector<double> factors_per_slot(const Compiled &c) {
    std::vector<double> n((size_t)c.nweight, 0.0);
    for (size_t f = 0; f < (size_t)c.nfactor; f++) {
        const uint32_t slot = c.f_rec[4 * f + 2];
        if (slot < (uint32_t)c.nweight) n[slot] += 1.0;
    }
    for (double &x : n) if (x == 0.0) x = 1.0;
    return n;
}

// ---- the cut of the by-weight list (wf_off[slot] .. wf_off[slot + 1]: a weight's entries; wf_first[slot]: its first
// factor) for the weights slot[0 .. n): entry j's TAG is j, what the caller's kernels get -- an output column, or with
// the list of all slots the slot itself; a slot named twice is cut twice.  A weight of no factor is left out.  One of at
// most `short_max` is a SHORT: {first entry, tag}, sorted by length, then by first factor, then by tag; len_end[k] = the
// shorts of at most k + 1 entries.  A longer one is a LONG, in the order of the list: the callers' kernels take it in
// pieces of their own kind (moments_items, wstats_items).
struct WeightCutShort { uint32_t off, tag; };
struct WeightCutLong { uint32_t off, len, tag; };
struct WeightCut {
    std::vector<WeightCutShort> shorts;
    std::vector<unsigned int> len_end;         // [short_max]
    std::vector<WeightCutLong> longs;
};
static inline WeightCut weight_cut(const std::vector<uint32_t> &wf_off, const std::vector<int32_t> &wf_first, const int32_t *slot, size_t n,
                                   uint32_t short_max) {
    WeightCut cut;
    std::vector<std::vector<uint64_t>> bylen(short_max);       // first factor << 32 | tag, per length
    for (size_t j = 0; j < n; j++) {
        const size_t s = (size_t)slot[j];
        const uint32_t off = wf_off[s], len = wf_off[s + 1] - off;
        if (len == 0) continue;
        if (len <= short_max) bylen[len - 1].push_back((uint64_t)(uint32_t)wf_first[s] << 32 | (uint64_t)j);
        else cut.longs.push_back({off, len, (uint32_t)j});
    }
    for (std::vector<uint64_t> &keys : bylen) {
        std::sort(keys.begin(), keys.end());
        for (uint64_t key : keys) { const uint32_t j = (uint32_t)(key & 0xffffffffu); cut.shorts.push_back({wf_off[(size_t)slot[j]], j}); }
        cut.len_end.push_back((unsigned int)cut.shorts.size());
    }
    return cut;
}
// A work item of the long weights as the kernels read it (a uint4; a short is a uint2): {first entry, entries, z, w}.
struct WeightItem { uint32_t x, y, z, w; };
// The moments' items (nsk_kernels_pcd.h): pieces of at most `piece` entries, z = the tag, ascending by entry in a weight.
static inline std::vector<WeightItem> moments_items(const WeightCut &cut, uint32_t piece) {
    std::vector<WeightItem> pieces;
    for (const WeightCutLong &l : cut.longs)
        for (uint32_t k = 0; k < l.len; k += piece) pieces.push_back({l.off + k, std::min(piece, l.len - k), l.tag, 0u});
    return pieces;
}
// The statistics' items (nsk_kernels_wstats.h): a weight of one piece is {.., z = the tag, w = 0}, which writes its column;
// one of several leaves partial sums -- pieces {.., z = the partial's index, w = 1} -- that a multi item {first partial,
// partials, tag, 0} adds in a second launch.
struct WstatsItems {
    std::vector<WeightItem> pieces, multi;
    int64_t npartial = 0;
};
static inline WstatsItems wstats_items(const WeightCut &cut, uint32_t piece) {
    WstatsItems it;
    for (const WeightCutLong &l : cut.longs) {
        const uint32_t npc = (l.len + piece - 1) / piece;
        if (npc == 1) { it.pieces.push_back({l.off, l.len, l.tag, 0u}); continue; }
        it.multi.push_back({(uint32_t)it.npartial, npc, l.tag, 0u});
        for (uint32_t k = 0; k < npc; k++) it.pieces.push_back({l.off + k * piece, std::min(piece, l.len - k * piece), (uint32_t)(it.npartial + k), 1u});
        it.npartial += npc;
    }
    return it;
}

}  // namespace nsk
