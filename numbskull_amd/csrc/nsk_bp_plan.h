// nsk_bp_plan.h -- the structure of one belief propagation set-up (nsk_bp.hip nsk_bp_setup uploads it as it stands; the
// kernels of nsk_kernels_bp.h trust every index in it without a check).  Like nsk_seg_plan.h, host only and pure: no HIP
// type, nothing of the handle (tests/test_bp_plan_cpu.py pins it down without a GPU).
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "nsk_compile.h"

namespace nsk {

struct BpPlan {
    std::vector<uint8_t> state;                     // [nid] 0: no variable, 1: clamped, 2: free -- by internal id
    std::vector<long long> pm_off, tab_off;         // [F + 1] a factor's member records in mrec; its table entries
    std::vector<long long> msg_off;                 // [E + 1] doubles of a directed edge in f2v / v2f
    std::vector<long long> b_off;                   // [nid + 1] doubles of a variable in belief
    std::vector<int32_t> slot_off, edge_off;        // [F + 1] a factor's distinct members in slot_rec; its directed edges
    std::vector<int32_t> slot_rec;                  // pairs {internal id, free ? 1 : 0}, in order of first occurrence
    std::vector<int32_t> mrec;                      // pairs {local slot, dense_equal_to} per member position
    std::vector<int32_t> e_fac, e_var;              // [E] the factor and the variable of a directed edge, factor-major
    std::vector<int32_t> v_list, v_eoff, v_edges;   // free variables with an edge: id, CSR into v_edges (edges ascending)
    int32_t nvbin = 0;                              // the binary variables come first in v_list: how many
    bool big = false;                               // a free variable of cardinality above zlocal has an edge
    nsk_bp_info info = {};                          // the counts (device_bytes is the set-up's to fill)
};

// member positions a function reads whatever its arity says (nsk_energy.hip energy_check_factors)
static inline int64_t bp_need(int fn) {
    switch (fn) {
    case 3: case 18: case 19: case 20: case 30: return 1;
    case 21: case 22: case 25: case 26: return 2;
    case 23: case 24: return 3;
    default: return 0;
    }
}

// Fills `p` for the state whose evidence is clamped (sample_evidence == 0) or free.  max_members, max_table and zlocal
// are NSK_BP_MAX_MEMBERS, NSK_BP_MAX_TABLE and the device's NSK_ZLOCAL.  Returns the refusal's text, empty where there is
// none; a refusal names the lowest offending factor.
static inline std::string bp_plan(const Compiled &c, int sample_evidence, int max_members, long long max_table, int zlocal, BpPlan &p) {
    const int64_t F = c.nfactor, nedge = c.nedge, nid = c.nid, npos = std::min<int64_t>(c.npos, (int64_t)c.p_info.size());
    const bool head_by_vid = (c.flags & NSK_FLAG_HEAD_BY_VID) != 0;
    p = BpPlan();
    p.state.assign((size_t)nid, 0);
    p.info.nfactor = F;
    for (int64_t v = 0; v < c.nvar; v++) {
        const int64_t id = c.iid[(size_t)v];
        if (id < 0 || id >= nid) return "nsk_bp_setup: a variable without an internal id";
        const bool clamped = id >= npos || ((c.p_info[(size_t)id] & 0xffu) != 0 && !sample_evidence);
        p.state[(size_t)id] = clamped ? 1 : 2;
    }
    // ---- factor by factor
    p.pm_off.assign((size_t)F + 1, 0); p.tab_off.assign((size_t)F + 1, 0); p.msg_off.assign(1, 0);
    p.slot_off.assign((size_t)F + 1, 0); p.edge_off.assign((size_t)F + 1, 0);
    std::vector<int32_t> deg((size_t)nid, 0), ids((size_t)std::max(max_members, 1));
    auto refuse = [](int64_t f, const std::string &why) { return "nsk_bp_setup: factor " + std::to_string((long long)f) + " " + why; };
    for (int64_t f = 0; f < F; f++) {
        const uint32_t head = c.f_rec[4 * (size_t)f];
        const int fn = (int)(head & 0xffu) - 1;
        const int64_t ar = (int64_t)(head >> 8), s = (int32_t)c.f_rec[4 * (size_t)f + 1], wz = (int32_t)c.f_rec[4 * (size_t)f + 2];
        if (!known_function(fn) || wz < 0 || wz >= c.nweight) return refuse(f, "has an unknown function or a weight outside the table");
        if (fn == 30) return refuse(f, "is UFO, which reads its members by value: belief propagation has no table for it");
        if ((fn == 13 || fn == 16 || fn == 17) && !head_by_vid)
            return refuse(f, "reads its head at the literal edge index (function 13, 16 or 17 without NSK_FLAG_HEAD_BY_VID): it has no single energy");
        if (fn == 8 && ar >= (int64_t)c.logtab.size()) return refuse(f, "(RATIO) has more members than the logarithm table");
        const int64_t np = fn == -1 ? 0 : std::max(ar, bp_need(fn));
        if (s < 0 || s + np > nedge) return refuse(f, "has member positions outside the edge array");
        int ns = 0;
        long long T = 1;
        for (int64_t l = s; l < s + np; l++) {
            const int32_t id = c.m_rec[2 * (size_t)l];
            if (id < 0 || id >= nid || !p.state[(size_t)id]) return refuse(f, "has a member outside the variables");
            int k = 0;
            while (k < ns && ids[(size_t)k] != id) k++;
            if (k == ns) {
                if (ns == max_members)
                    return refuse(f, "has more than NSK_BP_MAX_MEMBERS = " + std::to_string(max_members) + " distinct members");
                ids[(size_t)ns++] = id;
            }
            p.mrec.push_back(k);
            p.mrec.push_back(c.m_rec[2 * (size_t)l + 1]);
        }
        for (int k = 0; k < ns; k++) {
            if (p.state[(size_t)ids[(size_t)k]] != 2) continue;
            const long long card = c.v_card_i[(size_t)ids[(size_t)k]];
            if (card < 1) return refuse(f, "has a free member of cardinality below 1");
            T *= card;
            if (T > max_table)
                return refuse(f, "has a table of more than NSK_BP_MAX_TABLE = " + std::to_string(max_table) + " entries over its free members");
        }
        for (int k = 0; k < ns; k++) {
            const int32_t id = ids[(size_t)k];
            const bool free = p.state[(size_t)id] == 2;
            p.slot_rec.push_back(id);
            p.slot_rec.push_back(free ? 1 : 0);
            if (free) {
                p.e_fac.push_back((int32_t)f);
                p.e_var.push_back(id);
                p.msg_off.push_back(p.msg_off.back() + c.v_card_i[(size_t)id]);
                deg[(size_t)id]++;
            }
        }
        if ((int64_t)p.e_fac.size() > (int64_t)0x7ffffff0) return refuse(f, "and those before it have more than 2^31 directed edges");
        p.pm_off[(size_t)f + 1] = p.pm_off[(size_t)f] + np;
        p.slot_off[(size_t)f + 1] = p.slot_off[(size_t)f] + ns;
        p.edge_off[(size_t)f + 1] = (int32_t)p.e_fac.size();
        p.tab_off[(size_t)f + 1] = p.tab_off[(size_t)f] + T;
        p.info.max_table = std::max<int64_t>(p.info.max_table, T);
    }
    const int64_t E = (int64_t)p.e_fac.size();
    // ---- per variable: the beliefs' offsets, the free variables with an edge and their edges, ascending
    p.b_off.assign((size_t)nid + 1, 0); p.v_eoff.assign(1, 0); p.v_edges.assign((size_t)E, 0);
    std::vector<int32_t> slot_of((size_t)nid, -1);
    for (int64_t id = 0; id < nid; id++) {
        const long long card = p.state[(size_t)id] ? std::max<long long>(c.v_card_i[(size_t)id], 0) : 0;
        p.b_off[(size_t)id + 1] = p.b_off[(size_t)id] + card;
        if (p.state[(size_t)id] == 1) p.info.nclamped++;
        if (p.state[(size_t)id] != 2) continue;
        p.info.nfree++;
        if (!deg[(size_t)id]) p.info.nisolated++;
        else if (card > zlocal) p.big = true;
    }
    for (int pass = 0; pass < 2; pass++) {          // the binary variables first (k_bp_var), ascending in each part
        for (int64_t id = 0; id < nid; id++) {
            if (p.state[(size_t)id] != 2 || !deg[(size_t)id] || (c.v_card_i[(size_t)id] == 2) != (pass == 0)) continue;
            slot_of[(size_t)id] = (int32_t)p.v_list.size();
            p.v_list.push_back((int32_t)id);
            p.v_eoff.push_back(p.v_eoff.back() + deg[(size_t)id]);
        }
        if (pass == 0) p.nvbin = (int32_t)p.v_list.size();
    }
    std::vector<int32_t> cur(p.v_eoff.begin(), p.v_eoff.end() - 1);
    for (int64_t e = 0; e < E; e++) p.v_edges[(size_t)cur[(size_t)slot_of[(size_t)p.e_var[(size_t)e]]]++] = (int32_t)e;
    p.info.nedges = E; p.info.ntable = p.tab_off[(size_t)F]; p.info.nmsg = p.msg_off[(size_t)E]; p.info.nbelief = p.b_off[(size_t)nid];
    return "";
}

}  // namespace nsk
