// nsk_bp_trw_plan.h -- which kernel serves which factor in the factor phase of tree-reweighted belief propagation
// (nsk_bp_trw.hip, nsk_kernels_bptrw.h), the LDS a wave of the wave route needs, and the check of the caller's rho.  Like
// nsk_bp_map_plan.h, host only and pure: no HIP type, nothing of the handle.
// A factor with at least one directed edge has T table entries over A axes whose cardinalities sum to C; it goes
//   the LANE route  where T <= lane_max and C <= lane_cards: one lane walks the table once, ascending, its C running
//                   sums in a lane-private array (a 2 x 2 table: in registers);
//   the WAVE route  otherwise: one wave stages the table and the incoming vectors in LDS and every lane sums the output
//                   entries it owns out of LDS.
// By default lane_max = NSK_TRW_LANE_TABLE (a table below 64 entries does not fill one trip of a wave) and lane_cards =
// the device's NSK_ZLOCAL (what a lane keeps private).  The knob NSK_TRW_LANE_MAX = n (diagnostic: read with NSK_DIAG=1
// when a set-up is built) makes lane_max = n and drops the bound on C -- the lane route then sums a factor of more than
// NSK_ZLOCAL values entry by entry, as the wave route's lanes do -- so that 0 sends every factor down the wave route and
// NSK_BP_MAX_TABLE every factor down the lane route.  Both defaults come from reasoning.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "nsk_bp_plan.h"

namespace nsk {

#define NSK_TRW_LANE_TABLE 63
#define NSK_TRW_WAVES 4             // factors (waves) a block of the wave route at most
#define NSK_TRW_LDS_BYTES 163840    // LDS of a gfx950 compute unit, all of which one block may take

struct BpTrwRoutes {
    std::vector<int32_t> lane, wave;        // factor ids, ascending; in `lane` the 2 x 2 tables come first, npair of them
    int64_t npair = 0;
    int64_t counts[2] = {0, 0};             // factors per route: lane, wave
    int64_t wave_lds = 0;                   // doubles of LDS a wave needs: the largest T + 2 C on the wave route
};

// the knob's value: -1 where it is unset or no number
static inline long long trw_lane_max(const char *env) {
    if (!env || !*env) return -1;
    char *end = nullptr;
    const long long v = strtoll(env, &end, 10);
    return (end == env || v < 0) ? -1 : v;
}

// from the set-up's table, edge and message offsets; zlocal is the device's NSK_ZLOCAL, lane_max the knob (-1: unset)
static inline void bp_trw_routes(const BpPlan &p, int zlocal, long long lane_max, BpTrwRoutes &r) {
    r = BpTrwRoutes();
    const size_t F = p.edge_off.empty() ? 0 : p.edge_off.size() - 1;
    const long long tmax = lane_max < 0 ? NSK_TRW_LANE_TABLE : lane_max;
    std::vector<int32_t> rest;              // the lane route's factors that are no 2 x 2 table
    for (size_t f = 0; f < F; f++) {
        const int32_t e0 = p.edge_off[f], e1 = p.edge_off[f + 1];
        if (e1 == e0) continue;
        const long long T = p.tab_off[f + 1] - p.tab_off[f], C = p.msg_off[(size_t)e1] - p.msg_off[(size_t)e0];
        if (T <= tmax && (lane_max >= 0 || C <= zlocal)) {
            if (T == 4 && e1 - e0 == 2 && p.msg_off[(size_t)e0 + 1] - p.msg_off[(size_t)e0] == 2) r.lane.push_back((int32_t)f);
            else rest.push_back((int32_t)f);
            r.counts[0]++;
        } else {
            r.wave.push_back((int32_t)f);
            r.counts[1]++;
            r.wave_lds = std::max<int64_t>(r.wave_lds, T + 2 * C);
        }
    }
    r.npair = (int64_t)r.lane.size();
    r.lane.insert(r.lane.end(), rest.begin(), rest.end());
}

// waves a block of the wave route: as many as the LDS of a compute unit holds, NSK_TRW_WAVES at most, one at least (the
// largest factor nsk_bp_setup accepts needs 4096 + 2 x 4112 doubles, 98560 bytes: it fits)
static inline int trw_block_waves(int64_t wave_lds) {
    const int64_t fit = (NSK_TRW_LDS_BYTES - 256) / (8 * std::max<int64_t>(wave_lds, 1));
    return (int)std::max<int64_t>(1, std::min<int64_t>(NSK_TRW_WAVES, fit));
}

// the refusal of a rho (empty: none): every entry finite and > 0
static inline std::string trw_check_rho(const double *rho, int64_t nfactor) {
    for (int64_t f = 0; f < nfactor; f++)
        if (!(rho[f] > 0.0) || std::isinf(rho[f]))
            return "nsk_bp_trw_run: rho[" + std::to_string((long long)f) + "] must be finite and greater than 0";
    return "";
}

}  // namespace nsk
