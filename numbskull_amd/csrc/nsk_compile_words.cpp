// nsk_compile_words.cpp -- graph compiler: the per-variable word lists every later stage lays out.  Decides: which
// variables take the fast path (mark_fast) or a general tile (mark_general), and the words of a variable's factor
// lists in either form (lane_words, general_words_walk / general_words with the word cache).
// Fills: nothing of Compiled; fast[] and the word cache of the context.
#include "nsk_compile_ctx.h"

namespace nsk {

// Fast-path eligibility (DESIGN.md "fast path"): a binary dataType-0 variable whose every
// factor is a symmetric boolean function it is a member of, with <= 6 other members and a
// weight id below 2^24; and featureValue == 1 so that learning can use the same stream.  Sets fast[v] = 1.
void CompileCtx::mark_fast() {
    const int64_t nvar = c.nvar;
    fast.assign((size_t)nvar, 0);
    auto fast_function = [](int fn) { return fn == -1 || (fn >= 0 && fn <= 4); };
    const bool no_fast = knobs.no_fast;      // diagnostic: everything on the generic path
    parallel_for(nvar, [&](int64_t vb0, int64_t vb1, int) {
    for (int64_t v = vb0; v < vb1; v++) {
        if (c.color[v] < 0 || no_fast) continue;
        const nsk_variable &var = d->variable[v];
        if (var.cardinality != 2 || var.dataType != 0) continue;
        const nsk_vtf &vt = d->vmap[var.vtf_offset];
        bool ok = vt.factor_index_length <= 4096;
        for (int64_t j = 0; ok && j < vt.factor_index_length; j++) {
            const nsk_factor &fa = d->factor[d->factor_index[vt.factor_index_offset + j]];
            if (!fast_function(fa.factorFunction) || fa.weightId >= (1 << 24) || fa.featureValue != 1.0 ||
                fa.arity > 64) { ok = false; break; }
            if (fa.factorFunction == -1) continue;
            int64_t others = 0;
            bool member = false;
            for (int64_t l = fa.ftv_offset; l < fa.ftv_offset + fa.arity; l++) {
                if (d->fmap[l].vid == v) member = true; else others++;
            }
            if (!member || others > 6) ok = false;
        }
        fast[v] = ok;
    }
    });
}

// General tiles (kind 6): variables of cardinality <= 8 and any dataType whose factors are
// boolean symmetric functions, IMPLY_MLN or the categorical *_CAT functions.  Stream words per
// entry: W0 = weight id; W1 = code | others << 4 | own role << 7 (1 body, 2 head of a positional
// function) | own dense_equal_to << 9 | owning candidate value << 14 (15 = every candidate,
// dataType 0; 14 = none, padding entry); then one word per other member: id |
// dense_equal_to << 27 (id NSK_GEN_NULL = empty slot).  Every such entry evaluates to
// (candidate == c) ? A : B with c, A, B known once the other members have been read.
static int general_code(int fn) {
    switch (fn) {
    case -1: return 0; case 0: return 1; case 1: return 2; case 2: case 4: return 3; case 3: return 4;
    case 13: return 5; case 12: case 15: return 6; case 14: return 7; case 16: return 8; case 17: return 9;
    default: return -1;
    }
}

// Longer lists (knobs.gen_max_entries) go to the wave-per-variable kernel: a tile is walked by one wave, so its longest
// lane sets a serial chain of memory round trips and the longest tile the kernel's run time
// (hub = true lifts the per-lane size caps: the entry-parallel hub kernels take up to 256 entries)
//
// The variable may occur SEVERAL times in one factor (the config-#5 generator draws the other
// members from [v - 1024, v + 1024], v included): as body member and head of a positional
// function, or with different dense_equal_to values.  With x = the candidate value c at every
// own edge, eval_factor still reduces to (c == cstar) ? A : B:
//   * positional function, own body edges (all with dense_equal_to db) AND own head (dh) -> role 3:
//     the head test is the constant (db == dh) [IMPLY_MLN: true -- the head is only reached with
//     every body member, the variable included, non-zero], the body test is over the other members;
//   * own edges whose dense_equal_to disagree: the variable cannot match all of them -- AND_CAT /
//     EQUAL_CAT_CONST and IMPLY_NATURAL_CAT (own body edges) are constant 0, IMPLY_MLN_CAT (own
//     body edges) constant 1, OR_CAT over a binary variable with both values named constant 1
//     (codes 10 / 11; no member words); OR_CAT naming two of more than two values is not of the
//     one-cstar form and keeps the variable on the generic path.
// A dataType-1 variable finds such a factor in the list of EVERY dense_equal_to its own edges
// name (dataloading.py:34-38); the learning sweep visits a factor once per variable
// (learning.py:76-95), so the entry in the list of the larger value names the smaller one as its
// `partner` (descriptor bits 19-22) and is skipped when the partner's list is selected too.
bool CompileCtx::general_words_walk(int64_t v, std::vector<uint32_t> *out, bool hub, size_t hub_cap) const {
    const nsk_variable &var = d->variable[v];
    if (var.cardinality > 8 || var.cardinality < 2) return false;
    // (an evidence value outside the domain is kept off the tiles: their saved facts hold the
    // variable's own values in 4 bits)
    if (var.initialValue < 0 || var.initialValue >= var.cardinality) return false;
    const int64_t nslots = var.dataType == 0 ? 1 : var.cardinality;
    size_t nwords = 0, nentries = 0;
    if (out) out->clear();
    for (int64_t k = 0; k < nslots; k++) {
        const nsk_vtf &vt = d->vmap[var.vtf_offset + k];
        for (int64_t j = 0; j < vt.factor_index_length; j++) {
            const nsk_factor &fa = d->factor[d->factor_index[vt.factor_index_offset + j]];
            int code = general_code(fa.factorFunction);
            if (code < 0 || fa.featureValue != 1.0 || fa.arity > 64) return false;
            const bool positional = code == 5 || code == 8 || code == 9;
            const bool cat = code >= 6;
            const int64_t s = fa.ftv_offset, e = s + fa.arity;
            int64_t others = 0, self_body = 0, self_head = 0;
            int64_t body_deo = -1, head_deo = -1;      // dense_equal_to of the own body edges / own head
            bool body_deo_mixed = false;
            int64_t own_deo[2] = {-1, -1};             // distinct dense_equal_to of all own edges
            int n_own_deo = 0;
            uint32_t mem[8];
            const bool keyed = cat || var.dataType != 0;      // own dense_equal_to matters
            for (int64_t l = s; l < e; l++) {
                const int64_t vid = d->fmap[l].vid, deo = d->fmap[l].dense_equal_to;
                if (vid == v) {
                    if (keyed) {
                        if (cat && (deo < 0 || deo > 31)) return false;
                        if (n_own_deo == 0 || (own_deo[0] != deo && (n_own_deo < 2 || own_deo[1] != deo))) {
                            if (n_own_deo == 2) return false;          // three different own values: generic path
                            own_deo[n_own_deo++] = deo;
                        }
                    }
                    if (code == 0) continue;
                    if (positional && l == e - 1) { self_head++; head_deo = deo; }
                    else {
                        self_body++;
                        if (body_deo >= 0 && body_deo != deo) body_deo_mixed = true;
                        body_deo = deo;
                    }
                } else if (code != 0) {
                    if (others >= 6) return false;
                    int64_t rd = vid;                                  // index the value is read at
                    if (positional && l == e - 1 && !head_by_vid) rd = l;   // inference.py:243,277,292
                    if (rd >= (int64_t)NSK_GEN_NULL) return false;
                    int64_t dd = cat ? deo : 0;
                    if (dd < 0 || dd > 31) return false;
                    mem[others++] = (uint32_t)rd | ((uint32_t)dd << 27);
                }
            }
            if (code != 0 && self_body + self_head == 0) return false;
            // a non-categorical function over a dataType-1 variable whose own edges disagree:
            // rare and not of the tile form (the lists are keyed by values the function ignores)
            if (!cat && var.dataType != 0 && n_own_deo > 1 && code != 0) return false;
            if (code == 0 && var.dataType != 0 && n_own_deo > 1) return false;
            uint32_t role = 0, hbit = 0;
            int64_t self_deo = keyed && n_own_deo > 0 ? own_deo[0] : -1;
            if (code != 0 && positional) {
                if (self_body > 0 && cat && body_deo_mixed) {            // the body can never match
                    code = code == 9 ? 11 : 10;
                    others = 0;
                } else if (self_body > 0 && self_head > 0) {
                    role = 3; self_deo = body_deo;
                    hbit = cat ? (body_deo == head_deo ? 1u : 0u) : 1u;
                } else if (self_body > 0) { role = 1; self_deo = body_deo; }
                else { role = 2; self_deo = head_deo; }
            } else if (code != 0 && cat && n_own_deo > 1) {             // AND_CAT / EQUAL_CAT_CONST / OR_CAT
                if (code == 6) { code = 10; others = 0; }
                else if (var.cardinality == 2) { code = 11; others = 0; }     // own edges name 0 and 1
                else return false;
            }
            uint32_t partner = 0;                       // bit 19: has one; bits 20-22: its value
            if (var.dataType != 0 && n_own_deo > 1) {
                const int64_t lo = std::min(own_deo[0], own_deo[1]), hi = std::max(own_deo[0], own_deo[1]);
                if (lo < 0 || hi > 7) return false;
                if (k == hi) partner = 1u | ((uint32_t)lo << 1);
            }
            const uint32_t kslot = var.dataType == 0 ? 15u : (uint32_t)k;
            nwords += 2 + (size_t)others;
            if (hub ? (++nentries > (hub_cap ? hub_cap : 256)) : (nwords > 120 || (int64_t)++nentries > knobs.gen_max_entries)) return false;
            if (out) {
                out->push_back((uint32_t)fa.weightId);          // (the caller's id: general_words numbers it)
                out->push_back((uint32_t)code | ((uint32_t)others << 4) | (role << 7) |
                               ((uint32_t)(cat && self_deo > 0 ? self_deo : 0) << 9) | (kslot << 14) |
                               (hbit << 18) | (partner << 19));
                for (int64_t m = 0; m < others; m++) out->push_back(mem[m]);
            }
        }
    }
    return true;
}

// The entry lists are read five times on the way to the streams (eligibility, lane order, tile shapes, the two
// passes of the entry-parallel groups), the later ones in position order, where a walk through the caller's
// records -- variable, value slots, factor ids, factors, members: six to ten cache lines a variable -- has no
// locality left (50M LR graph: 4.7 - 5.6 s a pass against 1.1 s in id order).  The eligibility pass keeps what it
// found: the words of every variable it sends to the general tiles, id order, one or two cache lines a variable.
// One chunk per thread of that pass, read where it was written (a flat copy would fault the pages in twice).
bool CompileCtx::general_words(int64_t v, std::vector<uint32_t> *out, bool hub, size_t hub_cap) const {
    if (out && !hub && !gw_len.empty() && gw_len[(size_t)v]) {
        const size_t t = (size_t)(std::upper_bound(gw_v0.begin(), gw_v0.end(), v) - gw_v0.begin()) - 1;
        const uint32_t *src = gw_chunk[t].data() + gw_at[(size_t)v];
        out->assign(src, src + gw_len[(size_t)v]);
    } else if (!general_words_walk(v, out, hub, hub_cap)) return false;
    if (out && !c.wmap.empty())             // the weight's slot in the device table, once the numbering exists
        for (size_t j = 0; j < out->size(); j += 2 + (((*out)[j + 1] >> 4) & 7u)) (*out)[j] = slot_of_weight((int64_t)(*out)[j]);
    return true;
}

// General-tile eligibility: every coloured variable the fast path did not take and general_words_walk accepts gets
// fast[v] = 2; its words are kept in the word cache (gw_chunk, gw_v0, gw_at, gw_len) for the later passes.
void CompileCtx::mark_general() {
    const int64_t nvar = c.nvar;
    const bool no_fast = knobs.no_fast, keep = !knobs.no_word_cache && !no_fast && !no_general;
    const size_t T = (size_t)compile_threads();
    std::vector<uint8_t> overflow(T, 0);
    if (keep) { gw_chunk.resize(T); gw_v0.assign(T, nvar); gw_at.resize((size_t)nvar); gw_len.assign((size_t)nvar, 0); }
    parallel_for(nvar, [&](int64_t vb0, int64_t vb1, int t) {
        std::vector<uint32_t> w;
        if (keep) { gw_v0[(size_t)t] = vb0; gw_chunk[(size_t)t].reserve((size_t)(vb1 - vb0) * 12); }
        for (int64_t v = vb0; v < vb1; v++) {
            if (c.color[v] < 0 || fast[v] || no_fast || no_general || !general_words_walk(v, keep ? &w : nullptr, false, 0)) continue;
            fast[v] = 2;
            if (!keep || overflow[(size_t)t]) continue;
            std::vector<uint32_t> &ch = gw_chunk[(size_t)t];
            if (ch.size() + w.size() > (size_t)0xFFFFFFFFu) { overflow[(size_t)t] = 1; continue; }
            gw_at[(size_t)v] = (uint32_t)ch.size();
            gw_len[(size_t)v] = (uint8_t)w.size();
            ch.insert(ch.end(), w.begin(), w.end());
        }
    });
    // (parallel_for hands out ascending ranges: gw_v0 is ascending, threads that took no part keep nvar at its end)
    if (knobs.verbose) { int64_t n2 = 0, n1 = 0; for (int64_t v = 0; v < nvar; v++) { n2 += fast[v] == 2; n1 += fast[v] == 1; } fprintf(stderr, "[nsk] eligibility: %lld general-tile variables (entry lists kept), %lld fast\n", (long long)n2, (long long)n1); }
}

// Words of one lane of the fast path: per factor of the variable, in list order, a header then the ids of
// the members other than the variable itself
void CompileCtx::lane_words(int64_t v, std::vector<uint32_t> &out) const {
    out.clear();
    const nsk_variable &var = d->variable[v];
    const nsk_vtf &vt = d->vmap[var.vtf_offset];
    for (int64_t j = 0; j < vt.factor_index_length; j++) {
        const nsk_factor &fa = d->factor[d->factor_index[vt.factor_index_offset + j]];
        const size_t at = out.size();
        out.push_back(0);
        uint32_t others = 0;
        if (fa.factorFunction != -1)
            for (int64_t l = fa.ftv_offset; l < fa.ftv_offset + fa.arity; l++)
                if (d->fmap[l].vid != v) { out.push_back((uint32_t)d->fmap[l].vid); others++; }
        out[at] = ((uint32_t)(fa.factorFunction + 1) << 27) | (others << 24) | slot_of_weight(fa.weightId);
    }
}

}  // namespace nsk
