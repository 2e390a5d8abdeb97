// nsk_bp_dual_plan.h -- the schedule of max-sum diffusion on a belief propagation set-up (nsk_bp_dual.hip,
// nsk_kernels_bpdual.h): per colour class of the compiled layout the free variables with an edge, which route serves each,
// and the LDS a wave of the wave route needs.  Like nsk_bp_trw_plan.h, host only and pure: no HIP type, nothing of the
// handle.  An item is a variable's index in BpPlan::v_list (so that v_eoff names its edges); within a class and route the
// items ascend by internal id.  A variable of cardinality n with d edges goes
//   the LANE route  where n <= lane_cards, every incident table has at most lane_max entries and d <= lane_edges: one lane
//                   walks each incident table once, its n running maxima and the n totals in lane-private arrays;
//   the WAVE route  otherwise: one wave a variable, the co-members' vectors of the factor under way, the n maxima and the n
//                   totals in LDS (2 n + the largest sum C of a factor's cardinalities, in doubles).
// By default lane_max = NSK_DUAL_LANE_TABLE (a table below 64 entries does not fill one trip of a wave), lane_edges =
// NSK_DUAL_LANE_EDGES (a lane walks its edges one after the other; beyond, the wave's lanes take one edge each) and
// lane_cards = the device's NSK_ZLOCAL.  The knob NSK_DUAL_LANE_MAX = n (diagnostic: read with NSK_DIAG=1 when a set-up
// is first planned) makes lane_max = n and drops the bound on d, so that 0 sends every variable down the wave route and
// NSK_BP_MAX_TABLE every variable of cardinality <= lane_cards down the lane route.
// The colour classes are the compiled layout's: a free variable's internal id is its position, class k owns the positions
// [phase_start[k], phase_end[k]).  Two variables of a class must share no factor -- one launch updates the whole class --
// and the plan checks that on the set-up's own edges; it does not trust the colouring.  (A factor's edges are its DISTINCT
// free members, nsk_bp_plan.h: a variable that fills two slots of a factor is one edge and no conflict with itself.)
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "nsk_bp_plan.h"
#include "nsk_bp_trw_plan.h"        // trw_lane_max: a knob's value; NSK_TRW_LDS_BYTES

namespace nsk {

#define NSK_DUAL_LANE_TABLE 63
#define NSK_DUAL_LANE_EDGES 32
#define NSK_DUAL_WAVES 4            // variables (waves) a block of the wave route at most

struct BpDualPlan {
    std::vector<int32_t> cls;               // [nid] the class of a free variable with an edge, -1 otherwise
    std::vector<int32_t> lane, wave;        // items, class-major
    std::vector<int32_t> lane_off, wave_off;    // [nclass + 1] a class's items in `lane` / `wave`
    int64_t counts[2] = {0, 0};             // variables per route: lane, wave
    int64_t wave_lds = 0;                   // doubles of LDS a wave needs: the largest 2 n + max C on the wave route
};

// from the set-up's plan and the compiled classes; returns the refusal's text, empty where there is none
static inline std::string bp_dual_plan(const Compiled &c, const BpPlan &p, int zlocal, long long lane_max, BpDualPlan &r) {
    r = BpDualPlan();
    const size_t nid = p.state.size(), ncls = c.phase_end.size(), nv = p.v_list.size();
    const size_t F = p.edge_off.empty() ? 0 : p.edge_off.size() - 1;
    r.cls.assign(nid, -1);
    for (size_t i = 0; i < nv; i++) {
        const int64_t id = p.v_list[i];
        size_t k = 0;
        while (k < ncls && !(c.phase_start[k] <= id && id < c.phase_end[k])) k++;
        if (k == ncls) return "nsk_bp_dual_run: a free variable with an edge lies in no colour class of the compiled layout";
        r.cls[(size_t)id] = (int32_t)k;
    }
    for (size_t f = 0; f < F; f++)
        for (int32_t e = p.edge_off[f]; e < p.edge_off[f + 1]; e++)
            for (int32_t h = p.edge_off[f]; h < e; h++)
                if (r.cls[(size_t)p.e_var[(size_t)e]] == r.cls[(size_t)p.e_var[(size_t)h]])
                    return "nsk_bp_dual_run: factor " + std::to_string((long long)f) + " has two free members of colour class " +
                           std::to_string((long long)r.cls[(size_t)p.e_var[(size_t)e]]) + ": a class step would update both at once";
    const long long tmax = lane_max < 0 ? NSK_DUAL_LANE_TABLE : lane_max;
    std::vector<std::vector<std::pair<int32_t, int32_t>>> by_lane(ncls), by_wave(ncls);     // {internal id, item}
    for (size_t i = 0; i < nv; i++) {
        const int32_t id = p.v_list[i];
        const long long n = c.v_card_i[(size_t)id];
        const int32_t d = p.v_eoff[i + 1] - p.v_eoff[i];
        long long Tmax = 0, Cmax = 0;
        for (int32_t q = p.v_eoff[i]; q < p.v_eoff[i + 1]; q++) {
            const size_t f = (size_t)p.e_fac[(size_t)p.v_edges[(size_t)q]];
            Tmax = std::max(Tmax, p.tab_off[f + 1] - p.tab_off[f]);
            Cmax = std::max(Cmax, p.msg_off[(size_t)p.edge_off[f + 1]] - p.msg_off[(size_t)p.edge_off[f]]);
        }
        const size_t k = (size_t)r.cls[(size_t)id];
        if (n <= zlocal && Tmax <= tmax && (lane_max >= 0 || d <= NSK_DUAL_LANE_EDGES)) {
            by_lane[k].push_back({id, (int32_t)i});
            r.counts[0]++;
        } else {
            by_wave[k].push_back({id, (int32_t)i});
            r.counts[1]++;
            r.wave_lds = std::max<int64_t>(r.wave_lds, 2 * n + Cmax);
        }
    }
    r.lane_off.assign(1, 0); r.wave_off.assign(1, 0);
    for (size_t k = 0; k < ncls; k++) {
        std::sort(by_lane[k].begin(), by_lane[k].end());
        std::sort(by_wave[k].begin(), by_wave[k].end());
        for (const auto &it : by_lane[k]) r.lane.push_back(it.second);
        for (const auto &it : by_wave[k]) r.wave.push_back(it.second);
        r.lane_off.push_back((int32_t)r.lane.size());
        r.wave_off.push_back((int32_t)r.wave.size());
    }
    return "";
}

// waves a block of the wave route: as many as the LDS of a compute unit holds, NSK_DUAL_WAVES at most, one at least (the
// largest variable nsk_bp_setup accepts needs 2 x 4096 + 4111 doubles, 98424 bytes: it fits)
static inline int dual_block_waves(int64_t wave_lds) {
    const int64_t fit = (NSK_TRW_LDS_BYTES - 256) / (8 * std::max<int64_t>(wave_lds, 1));
    return (int)std::max<int64_t>(1, std::min<int64_t>(NSK_DUAL_WAVES, fit));
}

}  // namespace nsk
