// nsk_routes.cpp -- which kernel family samples every variable of a compiled layout, read back from the layout itself
// (tiles, streams, group descriptors, segments, phase ranges): the route words of nsk_graph_plan_routes /
// nsk_graph_get_routes and the tile / group counters of nsk_graph_info (include/numbskull_amd.h "Routes").  Host only;
// decides nothing and keeps no state of its own -- what it reports is what the kernels will be launched over.
#include "nsk_compile.h"

namespace nsk {

void compiled_routes(const Compiled &c, int32_t *route, RouteCounts *counts) {
    RouteCounts n = {0, 0, 0, 0, 0, 0, 0};
    const int32_t ncolors = (int32_t)c.phase_start.size() - 1;
    std::vector<int32_t> of((size_t)std::max<int64_t>(c.npos, 1), 0);       // per position
    std::vector<uint8_t> table((size_t)std::max<int64_t>(c.npos, 1), 0);    // inside a segment with a draw table
    for (const Compiled::Segment &sg : c.segments)
        if (sg.ztab >= 0)
            for (int64_t p = sg.pos0; p < sg.pos0 + 64 * (int64_t)sg.ntiles && p < c.npos; p++) table[(size_t)p] = 1;
    for (int32_t k = 0; k < ncolors; k++) {
        const int64_t nt = c.phase_wb_base[k + 1] - c.phase_wb_base[k];
        for (int64_t b = 0; b < nt; b++) {
            const uint32_t *td = &c.tiles[4 * (size_t)(c.phase_wb_base[k] + b)];
            const int64_t p0 = c.phase_start[k] + 64 * b, p1 = std::min(p0 + 64, c.phase_fast_end[k]);
            const uint32_t kind = (td[3] >> 8) & 7u;
            const uint64_t base = (uint64_t)td[0] * 4;
            auto word = [&](int64_t p, uint32_t j) { return c.adj[base + 256 * (uint64_t)(j / 4) + 4 * (uint64_t)(p - p0) + (j % 4)]; };
            bool any = false, tile_null = false;
            for (int64_t p = p0; p < p1; p++) {
                if (c.p_vid[(size_t)p] < 0) continue;
                any = true;
                int32_t r;
                if (td[2] == 0xFFFFFFFFu) r = NSK_ROUTE_LANE;
                else if (kind < 6u) r = table[(size_t)p] ? NSK_ROUTE_TABLE : NSK_ROUTE_UNIFORM;
                else if (kind == 7u) {
                    r = NSK_ROUTE_SHAPE;
                    for (uint32_t j = 0; j < td[1]; j++)
                        if ((c.tile_hdr[td[2] + j] & 0x80000010u) == 0x80000010u && word(p, j) == 0xFFFFFFFFu) { r |= 1 << 21; tile_null = true; break; }
                } else if (c.phase_ep[k]) r = NSK_ROUTE_GROUP;                   // (filled in from the group rows, below)
                else {
                    const uint32_t M = (td[3] >> 16) & 7u, E = (td[3] & 0xFFu) / (2 + M);
                    uint32_t ne = 0, mo = 0;
                    for (uint32_t e = 0; e < E; e++) {
                        const uint32_t d1 = word(p, e * (2 + M) + 1);
                        if (((d1 >> 14) & 15u) == 14u) continue;                 // an entry no candidate value owns
                        ne++;
                        mo = std::max(mo, (d1 >> 4) & 7u);
                    }
                    r = NSK_ROUTE_GENERAL | (int32_t)(ne << 4) | (int32_t)(mo << 9) | (int32_t)(E << 12) | (int32_t)(M << 17);
                }
                of[(size_t)p] = r;
            }
            if (!any) continue;
            if (td[2] == 0xFFFFFFFFu) n.tiles_lane++;
            else if (kind == 7u) { n.tiles_shape++; n.tiles_shape_padded += tile_null; }
            else if (kind == 6u && !c.phase_ep[k]) { n.tiles_general++; n.tiles_general_roles += ((td[3] >> 16) & 7u) >= 4u; }
        }
        // the groups of an entry-parallel colour: own entries and widest entry of a variable from the rows that name its position
        for (int64_t gi = c.phase_ep_base.empty() ? 0 : c.phase_ep_base[k]; !c.phase_ep_base.empty() && gi < c.phase_ep_base[k + 1]; gi++) {
            const uint32_t *gd = &c.ep_desc[(size_t)gi * 4];
            const int64_t p0 = c.phase_start[k] + 64 * (c.phase_gen_tile[k] + 4 * (gi - c.phase_ep_base[k]));
            const int64_t p1 = std::min(p0 + 256, c.phase_fast_end[k]);
            const bool two = gd[3] != 0;
            n.ep_groups++;
            n.ep_groups_two_pass += two;
            uint32_t ne[256], mo[256];
            for (int i = 0; i < 256; i++) { ne[i] = 0; mo[i] = 0; }
            uint64_t sr = gd[0];
            for (uint32_t cl = 0; cl < 8; cl++) {
                const uint32_t m = cl & 3u, rows = (gd[cl < 4 ? 1 : 3] >> (8 * m)) & 255u;
                for (uint64_t r = 0; r < rows; r++)
                    for (uint32_t e = 0; e < 64; e++) {
                        const uint32_t d1 = c.ep_adj[(sr + r * (2 + m)) * 64 + 2 * e + 1];
                        if (((d1 >> 14) & 15u) == 14u) continue;
                        const uint32_t at = (d1 >> 23) & 255u;
                        ne[at]++;
                        mo[at] = std::max(mo[at], m);
                    }
                sr += (uint64_t)rows * (2 + m);
            }
            for (int64_t p = p0; p < p1; p++)
                if (c.p_vid[(size_t)p] >= 0)
                    of[(size_t)p] = NSK_ROUTE_GROUP | (int32_t)(ne[p - p0] << 4) | (int32_t)(mo[p - p0] << 9) |
                                    (int32_t)((gd[2] & 255u) << 12) | (two ? 1 << 20 : 0);
        }
        for (int64_t p = c.phase_fast_end[k]; p < c.phase_heavy_end[k]; p++) {
            if (c.p_vid[(size_t)p] < 0) continue;
            const uint32_t *hd = &c.hub_desc[(size_t)(c.phase_hub_base[k] + (p - c.phase_fast_end[k])) * 4];
            of[(size_t)p] = NSK_ROUTE_HUB | (hd[1] ? 1 << 22 : 0) | (hd[3] ? 1 << 23 : 0);
        }
        for (int64_t p = c.phase_heavy_end[k]; p < c.phase_end[k]; p++)
            if (c.p_vid[(size_t)p] >= 0) of[(size_t)p] = NSK_ROUTE_GENERIC;
    }
    if (route)
        for (int64_t v = 0; v < c.nvar; v++) route[v] = c.v_pos[(size_t)v] >= 0 ? of[(size_t)c.v_pos[(size_t)v]] : NSK_ROUTE_NONE;
    if (counts) *counts = n;
}

}  // namespace nsk
