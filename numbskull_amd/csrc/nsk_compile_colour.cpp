// nsk_compile_colour.cpp -- graph compiler, first stage: which variables a handle samples, what they reach and read,
// and their colours.  Decides: the validation errors of reachable factors, the read lists, the colour classes.
// Fills: repeated_factors, has_ufo, literal_heads, logtab, color, ghost_needs (and ncolors, sampled, the read lists
// of the context).
#include <cmath>

#include "nsk_compile_ctx.h"

namespace nsk {

// Validation of every factor reachable from a sampled variable (errors as the reference raises them: SURVEY.md
// section 8b); marks the variables this handle samples, sets c.has_ufo / c.literal_heads / c.repeated_factors and fills
// c.logtab up to the largest arity of a RATIO factor.
int CompileCtx::validate_reachable() {
    const int64_t nvar = d->nvar, nfac = d->nfactor, nedge = d->nedge, nw = d->nweight;
    const int64_t nfi = d->nfactor_index;
    // ---- which variables does this handle sample? -------------------------------------------
    sampled.assign((size_t)nvar, 0);
    for (int64_t v = c.own_begin; v < c.own_end; v++) sampled[v] = d->variable[v].isEvidence != 4;   // inference.py:21-23
    // ---- validate every factor reachable from a sampled variable ------------------------------
    // Two parallel phases over index blocks: (1) every sampled variable's lists -- bounds, factor ids -- mark
    // the factors they reach; (2) every reached factor is checked.  Each thread keeps the first error of its
    // block (lowest variable / factor index); the lowest block's error is reported, list errors first, so
    // the message does not depend on the thread count.
    std::vector<uint8_t> checked(nfac, 0);
    int64_t max_ratio_arity = 0;
    struct Issue { int rc = NSK_OK; std::string msg; bool ufo = false, literal = false; int64_t ratio = 0; };
    auto check_factor = [&](int64_t f, Issue &is) -> int {
        const nsk_factor &fa = d->factor[f];
        const int fn = fa.factorFunction;
        if (!known_function(fn)) {
            is.msg = fmt("Factor function %lld (used in factor %lld) is not implemented.", fn, f);
            return NSK_E_FACTOR_FUNC;
        }
        if (fa.weightId < 0 || fa.weightId >= nw) {      // potential() reads it even for NOOP
            is.msg = fmt("factor %lld: weightId %lld outside weights", f, fa.weightId);
            return NSK_E_INDEX;
        }
        if (fn == -1) return NSK_OK;
        const int64_t s = fa.ftv_offset, e = fa.ftv_offset + fa.arity;
        if (fa.arity < 0 || s < 0 || e > nedge) {
            is.msg = fmt("factor %lld: members [%lld, %lld) outside fmap", f, s, e);
            return NSK_E_INDEX;
        }
        int64_t need = 0;       // member positions the function reads regardless of arity
        switch (fn) {
        case 3: need = 1; break;
        case 0: case 7: case 8: case 9: case 13: case 16: case 17:
            if (fa.arity < 1) { is.msg = fmt("factor %lld: function %lld needs arity >= 1", f, fn); return NSK_E_INDEX; }
            break;
        case 18: case 19: case 20: case 30: need = 1; break;
        case 21: case 22: case 25: case 26: need = 2; break;
        case 23: case 24: need = 3; break;
        default: break;
        }
        const int64_t last = std::max(e, s + need);
        if (s + need > nedge) {
            is.msg = fmt("factor %lld: function %lld reads member %lld beyond fmap", f, fn, s + need - 1);
            return NSK_E_INDEX;
        }
        for (int64_t l = s; l < last; l++) {
            if (d->fmap[l].vid < 0 || d->fmap[l].vid >= nvar) {
                is.msg = fmt("factor %lld: member variable %lld outside variables", f, d->fmap[l].vid);
                return NSK_E_INDEX;
            }
        }
        if (fn == 30) is.ufo = true;
        if (fn == 30) {   // UFO reads member (value of first member) - 1
            int64_t reach = s + d->variable[d->fmap[s].vid].cardinality - 2;
            if (reach >= nedge) { is.msg = fmt("factor %lld: UFO member index beyond fmap", f); return NSK_E_INDEX; }
            for (int64_t l = s; l <= reach; l++)
                if (d->fmap[l].vid < 0 || d->fmap[l].vid >= nvar) {
                    is.msg = fmt("factor %lld: member variable outside variables", f);
                    return NSK_E_INDEX;
                }
        }
        if (literal_head_function(fn) && !head_by_vid) is.literal = true;
        if (literal_head_function(fn) && !head_by_vid && e - 1 >= nvar) {
            is.msg = fmt("factor %lld: the reference reads var_value[%lld] for the head of function %lld "
                         "(inference.py:243,277,292), outside the variable array; pass NSK_FLAG_HEAD_BY_VID "
                         "for the fmap[l].vid lookup", f, e - 1, fn);
            return NSK_E_INDEX;
        }
        if (fn == 8) is.ratio = std::max(is.ratio, fa.arity);
        return NSK_OK;
    };
    {
        std::vector<Issue> issues((size_t)compile_threads());
        parallel_for(nvar, [&](int64_t vb0, int64_t vb1, int t) {
            Issue &is = issues[(size_t)t];
            std::vector<int64_t> sorted_list;
            for (int64_t v = vb0; v < vb1 && !is.rc; v++) {
                if (!sampled[v]) continue;
                const nsk_variable &var = d->variable[v];
                const int64_t nslots = var.dataType == 0 ? 1 : var.cardinality;
                for (int64_t k = 0; k < nslots && !is.rc; k++) {
                    const nsk_vtf &vt = d->vmap[var.vtf_offset + k];
                    if (vt.factor_index_length < 0 || vt.factor_index_offset < 0 ||
                        vt.factor_index_offset + vt.factor_index_length > nfi) {
                        is.msg = fmt("variable %lld: factor list outside factor_index", v);
                        is.rc = NSK_E_INDEX;
                        break;
                    }
                    // a factor twice in ONE list (compute_var_map never produces that, dataloading.py:68-81; a
                    // caller of the C-ABI may, and need not hand in sorted lists): its weight is then visited twice by
                    // one variable in one class and must not be updated in place at "its one visit"
                    // (find_direct_weights).  Bit 1 of checked[f] marks it: found on a sorted copy of the list when
                    // the list is not ascending already; the marks are atomic ORs (several threads reach one factor).
                    const int64_t *fl = d->factor_index + vt.factor_index_offset;
                    bool ascending = true;
                    for (int64_t j = 0; j < vt.factor_index_length; j++) {
                        const int64_t f = fl[j];
                        if (f < 0 || f >= nfac) {
                            is.msg = fmt("variable %lld: factor id %lld outside factors", v, f);
                            is.rc = NSK_E_INDEX;
                            break;
                        }
                        if (j > 0 && fl[j - 1] > f) ascending = false;
                    }
                    if (is.rc) break;
                    if (ascending) {
                        for (int64_t j = 0; j < vt.factor_index_length; j++)
                            __atomic_fetch_or(&checked[fl[j]], (uint8_t)((j > 0 && fl[j - 1] == fl[j]) ? 3 : 1), __ATOMIC_RELAXED);
                    } else {
                        sorted_list.assign(fl, fl + vt.factor_index_length);
                        std::sort(sorted_list.begin(), sorted_list.end());
                        for (size_t j = 0; j < sorted_list.size(); j++)
                            __atomic_fetch_or(&checked[sorted_list[j]], (uint8_t)((j > 0 && sorted_list[j - 1] == sorted_list[j]) ? 3 : 1), __ATOMIC_RELAXED);
                    }
                }
            }
        });
        for (const Issue &is : issues) if (is.rc) { err = is.msg; return is.rc; }      // blocks are in index order
        for (Issue &is : issues) is = Issue();
        parallel_for(nfac, [&](int64_t fb0, int64_t fb1, int t) {
            Issue &is = issues[(size_t)t];
            for (int64_t f = fb0; f < fb1 && !is.rc; f++)
                if (checked[f]) is.rc = check_factor(f, is);
        });
        c.repeated_factors.clear();
        for (int64_t f = 0; f < nfac; f++) if (checked[f] & 2) c.repeated_factors.push_back(f);
        for (const Issue &is : issues) {
            if (is.rc) { err = is.msg; return is.rc; }
            c.has_ufo = c.has_ufo || is.ufo;
            c.literal_heads = c.literal_heads || is.literal;
            max_ratio_arity = std::max(max_ratio_arity, is.ratio);
        }
    }
    c.logtab.resize((size_t)max_ratio_arity + 2);
    c.logtab[0] = 0.0;
    for (size_t k = 1; k < c.logtab.size(); k++) c.logtab[k] = std::log((double)k);   // math.log, inference.py:222
    return NSK_OK;
}

// Compact read lists: reads of v, sorted and unique, self excluded, as int32 -- built once, in
// parallel, from the packed records; every colouring pass walks these 4-byte lists
// instead of chasing vmap -> factor_index -> factor -> fmap again (for_each_read, nsk_compile_ctx.h).
void CompileCtx::build_read_lists() {
    const int64_t nvar = c.nvar;
    rd_off.assign((size_t)nvar + 1, 0);
    rd_len.assign((size_t)nvar, 0);
    {
        parallel_for(nvar, [&](int64_t b0, int64_t b1, int) {
            for (int64_t v = b0; v < b1; v++) {
                if (!sampled[v]) continue;
                int64_t n = 0;
                for_each_read_slow(v, [&](int64_t b) { if (b != v) n++; });
                rd_off[v + 1] = n;
            }
        });
        for (int64_t v = 0; v < nvar; v++) rd_off[v + 1] += rd_off[v];
        // (factors with a huge arity make the lists quadratic: beyond 2^32 entries walk the records)
        use_rd = rd_off[nvar] < ((int64_t)1 << 32);
        rd.resize(use_rd ? (size_t)rd_off[nvar] : 0);
        if (use_rd) parallel_for(nvar, [&](int64_t b0, int64_t b1, int) {
            for (int64_t v = b0; v < b1; v++) {
                if (!sampled[v]) continue;
                int32_t *out = rd.data() + rd_off[v];
                int64_t n = 0;
                for_each_read_slow(v, [&](int64_t b) { if (b != v) out[n++] = (int32_t)b; });
                std::sort(out, out + n);
                rd_len[v] = (int32_t)(std::unique(out, out + n) - out);
            }
        });
    }
}

// Colouring of the sampled variables: no two variables of a colour may read each other.  Greedy first fit in id
// order, a symmetry check of the reads (repaired with reverse lists when a raw index is asymmetric), iterated greedy
// (class by class, the classes of a pass over the host threads) and a balancing pass.  for_each_read(v, fn) calls
// fn(b) for every variable b that v reads; lap(name) closes a timed stage.  Sets ncolors.
void CompileCtx::colour_sampled() {
    const int64_t nvar = c.nvar;
    c.color.assign(nvar, -1);
    std::vector<int64_t> stamp(1, -1), load;
    ncolors = 0;
    // greedy first fit in id order, then a balancing pass (below)
    auto pick = [&](int64_t v) -> int32_t {
        int32_t col = 0;
        while (col < ncolors && stamp[col] == v) col++;
        if (col == ncolors) { ncolors++; stamp.push_back(-1); load.push_back(0); }
        load[col]++;
        return col;
    };
    for (int64_t v = 0; v < nvar; v++) {
        if (!sampled[v]) continue;
        for_each_read(v, [&](int64_t b) {
            if (b != v && c.color[b] >= 0) stamp[c.color[b]] = v;
        });
        c.color[v] = pick(v);
    }
    lap("greedy colouring");
    // the greedy pass assumes reads are symmetric (true for compute_var_map output); verify, and
    // repair with explicit reverse-read lists when a raw index is asymmetric
    auto has_conflict = [&]() {
        std::vector<uint8_t> bad((size_t)compile_threads(), 0);
        parallel_for(nvar, [&](int64_t b0, int64_t b1, int t) {
            for (int64_t v = b0; v < b1 && !bad[(size_t)t]; v++) {
                if (!sampled[v]) continue;
                for_each_read(v, [&](int64_t b) {
                    if (b != v && c.color[b] == c.color[v]) bad[(size_t)t] = 1;
                });
            }
        });
        bool any = false;
        for (uint8_t x : bad) any = any || x;
        return any;
    };
    auto repair = [&]() {
        std::vector<int64_t> rcount(nvar + 1, 0);
        for (int64_t v = 0; v < nvar; v++)
            if (sampled[v]) for_each_read(v, [&](int64_t b) { if (b != v) rcount[b + 1]++; });
        for (int64_t v = 0; v < nvar; v++) rcount[v + 1] += rcount[v];
        std::vector<int32_t> readers((size_t)rcount[nvar]);
        std::vector<int64_t> fill(rcount.begin(), rcount.end() - 1);
        for (int64_t v = 0; v < nvar; v++)
            if (sampled[v]) for_each_read(v, [&](int64_t b) { if (b != v) readers[fill[b]++] = (int32_t)v; });
        std::fill(c.color.begin(), c.color.end(), -1);
        stamp.assign(1, -1);
        load.clear();
        ncolors = 0;
        for (int64_t v = 0; v < nvar; v++) {
            if (!sampled[v]) continue;
            for_each_read(v, [&](int64_t b) {
                if (b != v && c.color[b] >= 0) stamp[c.color[b]] = v;
            });
            for (int64_t j = rcount[v]; j < rcount[v + 1]; j++) {
                int32_t a = readers[j];
                if (c.color[a] >= 0) stamp[c.color[a]] = v;
            }
            c.color[v] = pick(v);
        }
    };
    bool conflict = has_conflict();
    if (conflict) repair();

    lap("symmetry check");
    // fewer classes: iterated greedy (Culberson) -- recolour first fit with the vertices taken class
    // by class in a permuted class order; a class stays independent, so the count never grows, and
    // a few passes typically drop one or two classes (LR graph: 9 -> 7).  Every class costs a
    // kernel's latency floor, so this is sweep time.
    if (!conflict && ncolors > 2 && !knobs.no_recolour) {
        std::vector<int32_t> newc(nvar), seq;
        seq.reserve((size_t)nvar);
        const int npass = knobs.recolour_passes;
        int stale = 0;                                   // passes in a row that dropped no class
        for (int pass = 0; pass < npass && stale < 2; pass++) {       // (each pass is a serial walk of the graph)
            std::vector<int64_t> size((size_t)ncolors, 0);
            for (int64_t v = 0; v < nvar; v++) if (c.color[v] >= 0) size[c.color[v]]++;
            std::vector<int32_t> cls((size_t)ncolors);
            for (int32_t k = 0; k < ncolors; k++) cls[k] = k;
            if (pass % 3 == 0) std::reverse(cls.begin(), cls.end());
            else std::stable_sort(cls.begin(), cls.end(), [&](int32_t a, int32_t b) {
                return pass % 3 == 1 ? size[a] > size[b] : size[a] < size[b]; });
            std::vector<int64_t> at((size_t)ncolors + 1, 0);           // counting sort by class rank
            std::vector<int32_t> rank((size_t)ncolors);
            for (int32_t r = 0; r < ncolors; r++) rank[cls[r]] = r;
            for (int32_t k = 0; k < ncolors; k++) at[rank[k] + 1] = size[k];
            for (int32_t r = 0; r < ncolors; r++) at[r + 1] += at[r];
            seq.assign((size_t)at[ncolors], 0);
            for (int64_t v = 0; v < nvar; v++) if (c.color[v] >= 0) seq[at[rank[c.color[v]]]++] = (int32_t)v;
            std::fill(newc.begin(), newc.end(), -1);
            // The vertices of one old class are not adjacent, so first fit gives each of them the same
            // colour whether they are taken one after the other or all at once: class by class, the
            // class's vertices over the host threads (each reads only colours of earlier classes).
            int32_t nnew = 0;
            for (int32_t r = 0; r < ncolors; r++) {
                const int64_t a0 = r ? at[r - 1] : 0, a1 = at[r];       // (at[] now holds the classes' ends in seq)
                std::vector<int32_t> tmax((size_t)compile_threads(), -1);
                parallel_for(a1 - a0, [&](int64_t b0, int64_t b1, int t) {
                    std::vector<int64_t> st((size_t)ncolors + 1, -1);
                    int32_t mx = -1;
                    for (int64_t i = a0 + b0; i < a0 + b1; i++) {
                        const int32_t v = seq[(size_t)i];
                        for_each_read(v, [&](int64_t b) {
                            if (b != v && newc[b] >= 0) st[newc[b]] = v;
                        });
                        int32_t col = 0;
                        while (st[col] == v) col++;                  // (at most ncolors colours are in use)
                        newc[v] = col;
                        mx = std::max(mx, col);
                    }
                    tmax[(size_t)t] = mx;
                });
                for (int32_t m : tmax) nnew = std::max(nnew, m + 1);
            }
            for (int64_t v = 0; v < nvar; v++) if (c.color[v] >= 0) c.color[v] = newc[v];
            stale = nnew < ncolors ? 0 : stale + 1;
            ncolors = nnew;
        }
        stamp.assign((size_t)ncolors, -1);
        load.assign((size_t)ncolors, 0);
        for (int64_t v = 0; v < nvar; v++) if (c.color[v] >= 0) load[c.color[v]]++;
    }

    lap("iterated greedy");
    // balancing: first fit leaves a few huge classes and a tail of tiny ones, and every class costs
    // a kernel's latency floor however few variables it holds.  Move variables, in id order, from
    // their class to the least populated class none of their neighbours is in (reads are symmetric
    // here -- the asymmetric repair above skips this pass).
    if (!conflict && ncolors > 2 && !knobs.no_balance) {
        for (int pass = 0; pass < 2; pass++)
            for (int64_t v = 0; v < nvar; v++) {
                if (!sampled[v]) continue;
                const int32_t cur = c.color[v];
                // (no class is more than one variable lighter than this one's: nothing below can move it, and its
                // neighbours need not be looked at -- most variables once the classes are level)
                int64_t lightest = load[0];
                for (int32_t k = 1; k < ncolors; k++) lightest = std::min(lightest, load[k]);
                if (lightest + 1 >= load[cur]) continue;
                for_each_read(v, [&](int64_t b) {
                    if (b != v && c.color[b] >= 0) stamp[c.color[b]] = v;
                });
                int32_t best = cur;
                for (int32_t k = 0; k < ncolors; k++)
                    if (k != cur && stamp[k] != v && load[k] + 1 < load[best]) best = k;
                if (best != cur) { load[cur]--; load[best]++; c.color[v] = best; }
            }
    }
    // Greedy in id order hides an asymmetric read whenever the variable that is read comes first: a literal head index
    // (inference.py:243) that names a variable of no factor in common, say.  The two passes above take the variables
    // in other orders and may then put reader and read into one class.  Checked once more; such a graph gets the
    // repaired greedy colours and neither pass.
    if (!conflict && ncolors > 2 && !(knobs.no_recolour && knobs.no_balance) && has_conflict()) repair();
}

// Ghosts: variables outside the owned range read by a sampled variable (c.ghost_needs, sorted).
void CompileCtx::find_ghosts() {
    const int64_t nvar = c.nvar, ob = c.own_begin, oe = c.own_end;
    if (ob > 0 || oe < nvar) {
        std::vector<uint8_t> need(nvar, 0);
        for (int64_t v = 0; v < nvar; v++)
            if (sampled[v]) for_each_read(v, [&](int64_t b) { if (b < ob || b >= oe) need[b] = 1; });
        for (int64_t v = 0; v < nvar; v++) if (need[v]) c.ghost_needs.push_back((int32_t)v);
    }
}

}  // namespace nsk
