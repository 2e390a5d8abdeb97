// nsk_sw_plan.h -- the structure of one Swendsen-Wang set-up (nsk_sw.hip nsk_sw_setup uploads it as it stands; the kernels
// of nsk_kernels_sw.h trust every index in it without a check).  Like nsk_bp_plan.h, host only and pure: no HIP type,
// nothing of the handle.  It takes the clamped / free classification, the distinct members and the table axes from
// bp_plan, sorts the factors into bonds (two free members), fields (one) and the rest, and orders the free variables
// that have a factor into TILES of at most `tile` ordinals, grown breadth-first over the bond graph, so that most bonds
// have both ends in one tile: those go to the tile's own list (local ends), the others to one cross list.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "nsk_bp_plan.h"

namespace nsk {

#define NSK_SW_TILE 1024            // ordinals of a tile at most: its values and parents live in LDS, a local end is 10 bits
#define NSK_SW_MAX_ITEMS 0x7ffffff0ll       // ordinals or bonds a set-up holds at most

struct SwPlan {
    BpPlan bp;                                      // what k_bp_tables reads: member records, slots, table and edge offsets
    std::vector<int32_t> ord_id;                    // [nvars] SW ordinal -> internal id
    std::vector<int32_t> tile_off;                  // [ntiles + 1] a tile's ordinals
    std::vector<int32_t> tb_off;                    // [ntiles + 1] a tile's bonds in tb_rec
    std::vector<int32_t> tb_rec;                    // pairs {local u | local v << 16, bond ordinal}
    std::vector<int32_t> cross;                     // quadruples {ordinal u, ordinal v, bond ordinal, 0}
    std::vector<int32_t> bond_fac;                  // [nbonds] the factor of a bond, ascending
    std::vector<int32_t> bond_ends;                 // [2 nbonds] the ordinals of its axes u, v
    std::vector<int32_t> f_bond;                    // [F] a factor's bond ordinal, -1: a field or ignored
    std::vector<int32_t> ve_off, ve_edge;           // [nvars + 1] by ordinal: the variable's directed edges, ascending
    nsk_sw_info info = {};                          // the counts (device_bytes is the set-up's to fill)
};

// Fills `p` for the state whose evidence is clamped (sample_evidence == 0) or free; `tile` in [32, NSK_SW_TILE].  Returns
// the refusal's text, empty where there is none; a refusal names the lowest offending factor.  A factor bp_plan refuses
// is refused in its words.
static inline std::string sw_plan(const Compiled &c, int sample_evidence, int max_members, long long max_table, int zlocal, int tile, SwPlan &p) {
    p = SwPlan();
    BpPlan &bp = p.bp;
    std::string why = bp_plan(c, sample_evidence, max_members, max_table, zlocal, bp);
    const int64_t F = c.nfactor;
    // bp_plan fills a factor's offsets when it has accepted it, and every factor has a table entry: the factors in front
    // of the one it refused are those whose table offset moved
    int64_t seen = 0;
    while (seen < F && (int64_t)bp.tab_off.size() == F + 1 && bp.tab_off[(size_t)seen + 1] > 0) seen++;
    for (int64_t f = 0; f < seen; f++) {
        const int32_t e0 = bp.edge_off[(size_t)f], A = bp.edge_off[(size_t)f + 1] - e0;
        for (int32_t j = 0; j < A; j++) {
            const long long card = bp.msg_off[(size_t)(e0 + j) + 1] - bp.msg_off[(size_t)(e0 + j)];
            if (card != 2)
                return "nsk_sw_setup: factor " + std::to_string((long long)f) + " has a free member of cardinality " + std::to_string(card) +
                       ": the cluster update serves binary free variables";
        }
        if (A > 2)
            return "nsk_sw_setup: factor " + std::to_string((long long)f) + " has " + std::to_string(A) +
                   " distinct free members: the cluster update serves at most two";
    }
    if (!why.empty()) {
        const size_t at = why.find("nsk_bp_setup");
        if (at != std::string::npos) why.replace(at, 12, "nsk_sw_setup");
        return why;
    }
    // ---- bonds and fields; the variables with a factor are bp's v_list (all binary: ascending internal id)
    const int64_t nv = (int64_t)bp.v_list.size();
    if (nv > NSK_SW_MAX_ITEMS) return "nsk_sw_setup: more than 2^31 - 16 free variables with a factor";
    std::vector<int32_t> slot_of((size_t)c.nid, -1);
    for (int64_t i = 0; i < nv; i++) slot_of[(size_t)bp.v_list[(size_t)i]] = (int32_t)i;
    p.f_bond.assign((size_t)F, -1);
    std::vector<int32_t> deg((size_t)nv + 1, 0);    // bonds of a variable, by v_list slot
    for (int64_t f = 0; f < F; f++) {
        const int32_t e0 = bp.edge_off[(size_t)f], A = bp.edge_off[(size_t)f + 1] - e0;
        if (A == 1) p.info.nfields++;
        if (A != 2) continue;
        p.f_bond[(size_t)f] = (int32_t)p.bond_fac.size();
        p.bond_fac.push_back((int32_t)f);
        deg[(size_t)slot_of[(size_t)bp.e_var[(size_t)e0]]]++;
        deg[(size_t)slot_of[(size_t)bp.e_var[(size_t)e0 + 1]]]++;
    }
    const int64_t nb = (int64_t)p.bond_fac.size();
    if (nb > NSK_SW_MAX_ITEMS) return "nsk_sw_setup: more than 2^31 - 16 bonds";
    std::vector<long long> adj_off((size_t)nv + 1, 0);
    for (int64_t i = 0; i < nv; i++) adj_off[(size_t)i + 1] = adj_off[(size_t)i] + deg[(size_t)i];
    std::vector<int32_t> adj((size_t)(2 * nb));     // per variable its bonds, ascending (filled in bond order)
    {
        std::vector<long long> cur(adj_off.begin(), adj_off.end() - 1);
        for (int64_t b = 0; b < nb; b++) {
            const int32_t e0 = bp.edge_off[(size_t)p.bond_fac[(size_t)b]];
            for (int k = 0; k < 2; k++) adj[(size_t)cur[(size_t)slot_of[(size_t)bp.e_var[(size_t)e0 + k]]]++] = (int32_t)b;
        }
    }
    // ---- tiles: breadth-first from the lowest caller id not yet placed, neighbours in ascending bond ordinal; a tile closes
    // at `tile` ordinals or with an empty frontier
    std::vector<int32_t> ord_of((size_t)nv, -1);    // v_list slot -> ordinal
    p.ord_id.reserve((size_t)nv);
    p.tile_off.assign(1, 0);
    for (int64_t v = 0; v < c.nvar; v++) {
        const int32_t s0 = slot_of[(size_t)c.iid[(size_t)v]];
        if (s0 < 0 || ord_of[(size_t)s0] >= 0) continue;
        const size_t first = p.ord_id.size();
        ord_of[(size_t)s0] = (int32_t)first;
        p.ord_id.push_back(bp.v_list[(size_t)s0]);
        for (size_t head = first; head < p.ord_id.size() && p.ord_id.size() - first < (size_t)tile; head++) {
            const int32_t s = slot_of[(size_t)p.ord_id[head]];
            for (long long k = adj_off[(size_t)s]; k < adj_off[(size_t)s + 1] && p.ord_id.size() - first < (size_t)tile; k++) {
                const int32_t e0 = bp.edge_off[(size_t)p.bond_fac[(size_t)adj[(size_t)k]]];
                const int32_t a = slot_of[(size_t)bp.e_var[(size_t)e0]], b = slot_of[(size_t)bp.e_var[(size_t)e0 + 1]];
                const int32_t o = a == s ? b : a;
                if (ord_of[(size_t)o] >= 0) continue;
                ord_of[(size_t)o] = (int32_t)p.ord_id.size();
                p.ord_id.push_back(bp.v_list[(size_t)o]);
            }
        }
        p.tile_off.push_back((int32_t)p.ord_id.size());
    }
    const int64_t nt = (int64_t)p.tile_off.size() - 1;
    // ---- the bonds by tile, or across
    std::vector<int32_t> tile_of((size_t)nv);
    for (int64_t t = 0; t < nt; t++)
        for (int32_t o = p.tile_off[(size_t)t]; o < p.tile_off[(size_t)t + 1]; o++) tile_of[(size_t)o] = (int32_t)t;
    p.bond_ends.resize((size_t)(2 * nb));
    p.tb_off.assign((size_t)nt + 1, 0);
    for (int64_t b = 0; b < nb; b++) {
        const int32_t e0 = bp.edge_off[(size_t)p.bond_fac[(size_t)b]];
        const int32_t u = ord_of[(size_t)slot_of[(size_t)bp.e_var[(size_t)e0]]], w = ord_of[(size_t)slot_of[(size_t)bp.e_var[(size_t)e0 + 1]]];
        p.bond_ends[2 * (size_t)b] = u;
        p.bond_ends[2 * (size_t)b + 1] = w;
        if (tile_of[(size_t)u] == tile_of[(size_t)w]) p.tb_off[(size_t)tile_of[(size_t)u] + 1]++;
        else { p.cross.push_back(u); p.cross.push_back(w); p.cross.push_back((int32_t)b); p.cross.push_back(0); }
    }
    for (int64_t t = 0; t < nt; t++) p.tb_off[(size_t)t + 1] += p.tb_off[(size_t)t];
    p.tb_rec.resize(2 * (size_t)p.tb_off[(size_t)nt]);
    {
        std::vector<int32_t> cur(p.tb_off.begin(), p.tb_off.end() - 1);
        for (int64_t b = 0; b < nb; b++) {
            const int32_t u = p.bond_ends[2 * (size_t)b], w = p.bond_ends[2 * (size_t)b + 1], t = tile_of[(size_t)u];
            if (t != tile_of[(size_t)w]) continue;
            const int32_t base = p.tile_off[(size_t)t], at = cur[(size_t)t]++;
            p.tb_rec[2 * (size_t)at] = (u - base) | ((w - base) << 16);
            p.tb_rec[2 * (size_t)at + 1] = (int32_t)b;
        }
    }
    // ---- a variable's directed edges by ordinal (bp numbers them factor-major, so ascending edge = ascending factor)
    p.ve_off.assign((size_t)nv + 1, 0);
    for (int64_t o = 0; o < nv; o++) {
        const int32_t s = slot_of[(size_t)p.ord_id[(size_t)o]];
        p.ve_off[(size_t)o + 1] = p.ve_off[(size_t)o] + (bp.v_eoff[(size_t)s + 1] - bp.v_eoff[(size_t)s]);
        p.ve_edge.insert(p.ve_edge.end(), bp.v_edges.begin() + bp.v_eoff[(size_t)s], bp.v_edges.begin() + bp.v_eoff[(size_t)s + 1]);
    }
    p.info.nvars = nv; p.info.nbonds = nb; p.info.ncross = (int64_t)p.cross.size() / 4; p.info.ntiles = nt;
    return "";
}

}  // namespace nsk
