// nsk_bp_wide_plan.h -- the set-up of nsk_bp_plan.h with the WIDE route on: a logical factor beyond the two caps of the
// table route has no table; its messages are closed forms in leave-one-out products of the incoming ones
// (nsk_kernels_bpwide.h), so all the plan keeps of it is the list of its member positions.  Host only and pure, like
// nsk_bp_plan.h, whose parts it shares (tests/test_bp_wide_cpu.py pins it down without a GPU).
#pragma once

#include "nsk_bp_plan.h"

namespace nsk {

// The wide factors of a set-up, ascending.  rec: {factor, function, weight slot, first position in pos} per wide factor;
// pos_off: [nwide + 1]; pos: per member position the directed edge of a free member, or -1 - internal id of a clamped one
// (the set-up puts -1 - value there: the plan knows no state).
struct BpWidePlan {
    std::vector<int32_t> rec, pos_off, pos;
    std::vector<int32_t> narrow;                    // the directed edges of the table route, ascending (all of them without a wide factor)
    int64_t nwide = 0, max_positions = 0;
};

// the functions with a closed form (nsk_kernels_bpwide.h): IMPLY_NATURAL, OR, AND, EQUAL, ISTRUE, LINEAR, LOGICAL, IMPLY_MLN
static inline bool bp_wide_function(int fn) { return fn == 0 || fn == 1 || fn == 2 || fn == 3 || fn == 4 || fn == 7 || fn == 9 || fn == 13; }

// bp_plan with every factor of at least wide_min distinct members, or beyond max_members / max_table, routed WIDE where
// it is eligible: a function above, every member binary, no free variable at two positions, at most max_wide positions.
// A factor that is not eligible takes the table route and bp_plan's refusals -- but an eligible function beyond the caps
// that names a free member twice or has too many positions is refused in words of its own.
static inline std::string bp_plan_wide(const Compiled &c, int sample_evidence, int max_members, long long max_table, int zlocal, int wide_min,
                                       int max_wide, BpPlan &p, BpWidePlan &wp) {
    BpPlanWork k;
    wp = BpWidePlan();
    wp.pos_off.assign(1, 0);
    std::string why = bp_plan_begin(c, sample_evidence, max_members, p, k);
    std::vector<int64_t> seen((size_t)c.nid, -1);   // the factor that last named a variable
    wide_min = std::max(wide_min, 1);
    for (int64_t f = 0; f < c.nfactor && why.empty(); f++) {
        int fn;
        int64_t s, np;
        if (!(why = bp_plan_record(c, k, f, fn, s, np)).empty()) break;
        // ---- the route: what the table route would need, and whether the closed form serves
        int64_t ns = 0;
        long long T = 1;
        bool valid = true, binary = true, twice = false;
        for (int64_t l = s; l < s + np && valid; l++) {
            const int32_t id = c.m_rec[2 * (size_t)l];
            if (id < 0 || id >= c.nid || !p.state[(size_t)id]) { valid = false; break; }
            const bool again = seen[(size_t)id] == f, free = p.state[(size_t)id] == 2;
            seen[(size_t)id] = f;
            binary = binary && c.v_card_i[(size_t)id] == 2;
            if (again) { twice = twice || free; continue; }
            ns++;
            if (free && T <= max_table) T *= std::max<long long>(c.v_card_i[(size_t)id], 1);
        }
        const bool fits = ns <= max_members && T <= max_table;
        const bool wide = valid && np >= 1 && (!fits || ns >= wide_min) && bp_wide_function(fn) && binary;
        if (!wide || (fits && (twice || np > max_wide))) {
            why = bp_plan_factor(c, max_members, max_table, f, s, np, p, k);
            if (why.empty())
                for (int32_t e = p.edge_off[(size_t)f]; e < p.edge_off[(size_t)f + 1]; e++) wp.narrow.push_back(e);
            continue;
        }
        if (twice) { why = bp_refuse(f, "names a free member twice on the wide route"); break; }
        if (np > max_wide) {
            why = bp_refuse(f, "has more than NSK_BP_WIDE_MAX_MEMBERS = " + std::to_string(max_wide) + " member positions on the wide route");
            break;
        }
        // ---- WIDE: no member record, no distinct-member slot, no table entry; an edge per free position
        wp.rec.push_back((int32_t)f); wp.rec.push_back(fn);
        wp.rec.push_back((int32_t)c.f_rec[4 * (size_t)f + 2]); wp.rec.push_back(wp.pos_off.back());
        for (int64_t l = s; l < s + np; l++) {
            const int32_t id = c.m_rec[2 * (size_t)l];
            if (p.state[(size_t)id] != 2) { wp.pos.push_back(-1 - id); continue; }
            wp.pos.push_back((int32_t)p.e_fac.size());
            p.e_fac.push_back((int32_t)f);
            p.e_var.push_back(id);
            p.msg_off.push_back(p.msg_off.back() + 2);
            k.deg[(size_t)id]++;
        }
        wp.pos_off.push_back((int32_t)wp.pos.size());
        wp.nwide++;
        wp.max_positions = std::max(wp.max_positions, np);
        why = bp_plan_close(p, f, 0, 0, 0);
    }
    if (why.empty()) bp_plan_finish(c, zlocal, p, k);
    return why;
}

// doubles of LDS a wave of k_bp_wide takes (three exclusive prefixes a position) and the waves of a block: four where a
// wave stays within a quarter of 64 KB, one beyond
static inline int64_t bp_wide_wave_lds(int64_t max_positions) { return 3 * ((max_positions + 63) / 64 * 64); }
static inline int bp_wide_block_waves(int64_t max_positions) { return bp_wide_wave_lds(max_positions) * 8 <= 16384 ? 4 : 1; }

}  // namespace nsk
