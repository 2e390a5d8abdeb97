// nsk_bp_map_plan.h -- which kernel serves which factor in the factor phase of max-product belief propagation
// (nsk_bp_map.hip, nsk_kernels_bpmap.h).  Like nsk_bp_plan.h, host only and pure: no HIP type, nothing of the handle.
// A factor with at least one directed edge has T table entries over A axes whose cardinalities sum to C; it goes
//   the LANE route  where T < NSK_MS_LANE_TABLE and C <= NSK_ZLOCAL: one lane walks the table once, its C running maxima
//                   in a lane-private array;
//   the WAVE route  otherwise where C <= NSK_MS_LDS: one wave, the C incoming values and the C accumulators in LDS;
//   the EDGE route  otherwise (an axis of several hundred values): one lane per directed edge.
// Both thresholds come from reasoning and are unmeasured: a table below 64 entries does not fill one trip of
// a wave, and 512 doubles twice over are 8 KB a wave, 32 KB a block of four.
#pragma once

#include <cstdint>
#include <vector>

#include "nsk_bp_plan.h"

namespace nsk {

#define NSK_MS_LANE_TABLE 64
#define NSK_MS_LDS 512

struct BpMapRoutes {
    std::vector<int32_t> lane, wave;        // factor ids, ascending
    std::vector<int32_t> edge;              // the directed edges of the edge route's factors, ascending
    int64_t counts[3] = {0, 0, 0};          // FACTORS per route: lane, wave, edge
};

// from the set-up's table, edge and message offsets; zlocal is the device's NSK_ZLOCAL
static inline void bp_map_routes(const BpPlan &p, int zlocal, BpMapRoutes &r) {
    r = BpMapRoutes();
    const size_t F = p.edge_off.empty() ? 0 : p.edge_off.size() - 1;
    for (size_t f = 0; f < F; f++) {
        const int32_t e0 = p.edge_off[f], e1 = p.edge_off[f + 1];
        if (e1 == e0) continue;
        const long long T = p.tab_off[f + 1] - p.tab_off[f], C = p.msg_off[(size_t)e1] - p.msg_off[(size_t)e0];
        if (T < NSK_MS_LANE_TABLE && C <= zlocal) { r.lane.push_back((int32_t)f); r.counts[0]++; }
        else if (C <= NSK_MS_LDS) { r.wave.push_back((int32_t)f); r.counts[1]++; }
        else {
            for (int32_t e = e0; e < e1; e++) r.edge.push_back(e);
            r.counts[2]++;
        }
    }
}

}  // namespace nsk
