// nsk_class_records.cpp -- the launches of every colour class as plain numbers: the records of nsk_graph_plan_classes
// (include/numbskull_amd.h "Class plans").  Host only; decides nothing of its own -- class_shape, plan_gibbs_class and
// plan_learn_class (nsk_class_plan.h) under the options the caller hands in, which are the ones the sweep drivers fill
// (per class: seg_tiles, and ep_per_cu only for a class laid out as groups).
#include "nsk_class_plan.h"

namespace nsk {

static void put_general(int32_t *r, const GeneralLaunch &L, int ngroups) {
    r[NSK_CLS_GEN_ON] = L.on;
    if (!L.on) return;
    r[NSK_CLS_GEN_ITEMS] = L.ep ? ngroups : L.ntiles;
    r[NSK_CLS_GEN_GRID] = L.grid; r[NSK_CLS_GEN_STREAM] = L.stream;
    r[NSK_CLS_GEN_EP] = L.ep; r[NSK_CLS_GEN_MAXC] = L.maxc; r[NSK_CLS_GEN_CAPPED] = L.capped;
    r[NSK_CLS_GEN_TILE0] = L.tile0; r[NSK_CLS_GEN_NTILES] = L.ntiles;
    r[NSK_CLS_GEN_HBLOCKS] = L.hblocks; r[NSK_CLS_GEN_GBLOCKS] = L.gblocks; r[NSK_CLS_GEN_RBLOCKS] = L.rblocks;
    r[NSK_CLS_GEN_NREST] = L.nrest;
    r[NSK_CLS_GEN_BEHIND] = L.behind_generic; r[NSK_CLS_GEN_NBLOCKS] = L.nblocks;
}
static void put_simple(int32_t *r, const SimpleLaunch &L) {     // on, items, grid, stream
    r[0] = L.on;
    if (!L.on) return;
    r[1] = L.n; r[2] = L.grid; r[3] = L.stream;
}

void compiled_class_records(const Compiled &c, bool learning, const PlanOpts &base, int32_t *rec) {
    const size_t nphase = c.phase_start.empty() ? 0 : c.phase_start.size() - 1;
    const int ep_per_cu = base.ep_per_cu;
    PlanOpts o = base;
    o.ep_per_cu = 0;
    for (size_t ph = 0; ph < nphase; ph++) {
        int32_t *r = rec + ph * NSK_CLASS_REC;
        for (int i = 0; i < NSK_CLASS_REC; i++) r[i] = 0;
        const ClassShape s = class_shape(c, ph);
        r[NSK_CLS_FB] = s.fb; r[NSK_CLS_FE] = s.fe; r[NSK_CLS_HE] = s.he; r[NSK_CLS_E] = s.e;
        r[NSK_CLS_NTILES] = s.ntiles;
        r[NSK_CLS_NHUB] = s.he - s.fe; r[NSK_CLS_NBH] = s.nbh; r[NSK_CLS_NGROUPS] = s.ngroups;
        r[NSK_CLS_NDYN] = s.ndyn; r[NSK_CLS_NLREST] = s.nlrest; r[NSK_CLS_NREST] = s.nrest;
        r[NSK_CLS_NGENERIC] = s.e - s.he;
        if (learning) {
            o.seg_tiles = 0;
            for (const Compiled::SegLaunch &sl : c.learn_seg)
                if (sl.phase == (int)ph) o.seg_tiles += sl.tile_start[sl.n];
            if (s.ep && s.e > s.fb) o.ep_per_cu = ep_per_cu;            // (from the first such class on, as the driver's)
            const LearnClassPlan p = plan_learn_class(s, o);
            r[NSK_CLS_SEG_TILES] = o.seg_tiles;
            r[NSK_CLS_SKIP] = p.skip;
            put_general(r, p.general, s.ngroups);
            put_simple(r + NSK_CLS_GENERIC, p.generic);
            put_simple(r + NSK_CLS_HEAVY, p.heavy);
            put_simple(r + NSK_CLS_FAST, p.fast);
            put_simple(r + NSK_CLS_DYN, p.dyn);
            r[NSK_CLS_KSTAT] = p.kstat; r[NSK_CLS_UPDATE] = p.update;
            r[NSK_CLS_SEGMENTS] = o.seg_tiles > 0;
        } else {
            if (s.ep && s.fe > s.fb) o.ep_per_cu = ep_per_cu;
            const GibbsClassPlan p = plan_gibbs_class(s, o);
            put_general(r, p.general, s.ngroups);
            put_simple(r + NSK_CLS_GENERIC, p.generic);
            put_simple(r + NSK_CLS_FAST, p.fast);
            r[NSK_CLS_SEGMENTS] = p.segments;
        }
    }
}

}  // namespace nsk
