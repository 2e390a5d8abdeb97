// nsk_compile_groups.cpp -- graph compiler: the lane-per-entry layouts.  Decides: the rows of the entry-parallel groups
// of a colour's general tiles (build_ep_groups) and of the hub variables (build_hub_streams).
// Fills: phase_ep_base, ep_desc, ep_adj, ep_wrow, ep_win, ep_win_off, ep_kstat; phase_hub_base, hub_desc, hub_adj,
// bighub_pos, phase_bighub_base, nhub_ep.
#include "nsk_compile_ctx.h"

namespace nsk {

// Entry-parallel groups (nsk_compile.h ep_desc): the general tiles of an EP colour, four at a time, as rows of 64
// list entries sorted by their member count.  general_words(v, &out) is the compiler's per-variable entry list (nsk_compile_words.cpp);
// lap(name) closes a timed stage.
int CompileCtx::build_ep_groups() {
    const int64_t nw = c.nweight;
    // ---- entry-parallel groups (nsk_compile.h ep_desc): the general tiles of an EP colour, four at a
    // time, as rows of 64 list entries sorted by their member count
    c.phase_ep_base.assign((size_t)ncolors + 1, 0);
    for (int32_t k = 0; k < ncolors; k++) {
        const int64_t ngt = (c.phase_wb_base[k + 1] - c.phase_wb_base[k]) - c.phase_gen_tile[k];
        c.phase_ep_base[k + 1] = c.phase_ep_base[k] + (c.phase_ep[k] ? (ngt + 3) / 4 : 0);
    }
    {
        const int64_t ngroups = c.phase_ep_base[ncolors];
        c.ep_desc.assign((size_t)ngroups * 4 + 4, 0u);
        c.ep_wrow.assign((size_t)ngroups + 1, 0u);
        std::vector<int32_t> group_colour((size_t)ngroups);
        for (int32_t k = 0; k < ncolors; k++)
            for (int64_t gi = c.phase_ep_base[k]; gi < c.phase_ep_base[k + 1]; gi++) group_colour[gi] = k;
        auto group_range = [&](int64_t gi, int64_t &p0, int64_t &p1) {
            const int32_t k = group_colour[gi];
            p0 = c.phase_start[k] + 64 * (c.phase_gen_tile[k] + 4 * (gi - c.phase_ep_base[k]));
            p1 = std::min(p0 + 256, c.phase_fast_end[k]);
        };
        std::vector<uint64_t> subrows((size_t)ngroups + 1, 0);
        // row classes: member count M = 0..3 of the entries with ordinal < 8 ("base", classes 0-3),
        // then the same for ordinals 8..15 ("overflow", classes 4-7): the kernels hold 8 list positions
        // per variable in LDS and take a group with longer lists in two passes
        auto row_class = [](uint32_t m, uint32_t ordinal) { return m + (ordinal >= 8 ? 4u : 0u); };
        parallel_for(ngroups, [&](int64_t g0, int64_t g1, int) {          // pass A: rows per class
            std::vector<uint32_t> w;
            for (int64_t gi = g0; gi < g1; gi++) {
                int64_t p0, p1;
                group_range(gi, p0, p1);
                uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, emax = 0, maxcard = 2;
                for (int64_t p = p0; p < p1; p++) {
                    if (c.p_vid[p] < 0) continue;
                    general_words(c.p_vid[p], &w);
                    uint32_t ne = 0;
                    for (size_t j = 0; j < w.size(); j += 2 + ((w[j + 1] >> 4) & 7u)) { cnt[row_class((w[j + 1] >> 4) & 7u, ne)]++; ne++; }
                    emax = std::max(emax, ne);
                    maxcard = std::max(maxcard, (uint32_t)d->variable[c.p_vid[p]].cardinality);
                }
                uint32_t *gd = &c.ep_desc[(size_t)gi * 4];
                uint64_t sr = 0;
                gd[1] = 0; gd[3] = 0;
                for (uint32_t cl = 0; cl < 8; cl++) {
                    const uint32_t rows = (cnt[cl] + 63) / 64;
                    gd[cl < 4 ? 1 : 3] |= rows << (8 * (cl & 3u));
                    sr += (uint64_t)rows * (2 + (cl & 3u));
                }
                gd[2] = emax | (maxcard << 8);
                subrows[gi + 1] = sr;
                uint32_t nrows = 0;
                for (uint32_t cl = 0; cl < 8; cl++) nrows += (cnt[cl] + 63) / 64;
                c.ep_wrow[gi + 1] = nrows;
            }
        }, 8);                                      // (a group is 256 variables' worth of work)
        lap("entry-parallel groups: rows");
        for (int64_t gi = 0; gi < ngroups; gi++) {
            const uint64_t next = (uint64_t)c.ep_wrow[gi] + c.ep_wrow[gi + 1];
            if (next >= ((uint64_t)1 << 31)) { err = "entry-parallel stream too large"; return NSK_E_RANGE; }
            c.ep_wrow[gi + 1] = (uint32_t)next;
        }
        for (int64_t gi = 0; gi < ngroups; gi++) subrows[gi + 1] += subrows[gi];
        if (subrows[ngroups] * 64 >= ((uint64_t)1 << 31)) { err = "entry-parallel stream too large"; return NSK_E_RANGE; }
        c.ep_adj.assign((size_t)subrows[ngroups] * 64 + 64, 0u);
        // structural visit counts (nsk_compile.h ep_kstat): global accumulators only (graphs with few
        // weights accumulate in LDS tables, where an update costs nothing); counted in pass B (atomic
        // increments: a weight's entries are spread over the groups, contention is negligible)
        const bool want_kstat = ngroups > 0 && nw > 256 && (int64_t)ncolors * nw * 2 <= ((int64_t)1 << 26) && !knobs.no_kstat &&
                                c.ndirect == 0;      // (direct weights are updated at their visit: every visit must reach the kernel)
        if (want_kstat) c.ep_kstat.assign((size_t)ncolors * 2 * (size_t)nw, 0u);
        lap("entry-parallel groups: allocation");
        parallel_for(ngroups, [&](int64_t g0, int64_t g1, int) {          // pass B: fill
            std::vector<uint32_t> w;
            for (int64_t gi = g0; gi < g1; gi++) {
                int64_t p0, p1;
                group_range(gi, p0, p1);
                uint32_t *gd = &c.ep_desc[(size_t)gi * 4];
                gd[0] = (uint32_t)subrows[gi];
                uint64_t base[8], at[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // first sub-row / entries placed, per class
                uint64_t sr = subrows[gi];
                for (uint32_t cl = 0; cl < 8; cl++) {
                    const uint32_t m = cl & 3u;
                    base[cl] = sr;
                    const uint32_t rows = (gd[cl < 4 ? 1 : 3] >> (8 * m)) & 255u;
                    // padding entries of the last row: owned by no candidate, empty member slots
                    for (uint64_t r = 0; r < rows; r++)
                        for (uint32_t e = 0; e < 64; e++) {
                            uint32_t *row = &c.ep_adj[(sr + r * (2 + m)) * 64];
                            row[2 * e] = 0u; row[2 * e + 1] = 14u << 14;
                            for (uint32_t mm = 0; mm < m; mm++) row[(2 + mm) * 64 + e] = NSK_GEN_NULL;
                        }
                    sr += (uint64_t)rows * (2 + m);
                }
                const int32_t gk = group_colour[gi];
                for (int64_t p = p0; p < p1; p++) {
                    if (c.p_vid[p] < 0) continue;
                    general_words(c.p_vid[p], &w);
                    const nsk_variable &var = d->variable[c.p_vid[p]];
                    if (want_kstat && var.dataType == 0) {
                        const size_t o = var.isEvidence == 1 ? 0 : 1;
                        for (size_t j = 0; j < w.size(); j += 2 + ((w[j + 1] >> 4) & 7u))
                            if (!c.w_fixed[w[j]])
                                __atomic_fetch_add(&c.ep_kstat[((size_t)gk * 2 + o) * (size_t)nw + w[j]], 1u, __ATOMIC_RELAXED);
                    }
                    uint32_t ordinal = 0;
                    for (size_t j = 0; j < w.size(); ordinal++) {
                        const uint32_t m = (w[j + 1] >> 4) & 7u, cl = row_class(m, ordinal);
                        const uint64_t r = at[cl] / 64, e = at[cl] % 64;
                        at[cl]++;
                        uint32_t *row = &c.ep_adj[(base[cl] + r * (2 + m)) * 64];
                        const uint32_t wid = w[j];
                        row[2 * e] = wid | (ordinal << 27);
                        row[2 * e + 1] = w[j + 1] | ((uint32_t)(p - p0) << 23) | (c.w_fixed[wid] ? 0x80000000u : 0u);
                        for (uint32_t mm = 0; mm < m; mm++)
                            row[(2 + mm) * 64 + e] = (uint32_t)c.iid[w[j + 2 + mm] & NSK_GEN_NULL] | (w[j + 2 + mm] & ~NSK_GEN_NULL);
                        j += 2 + m;
                    }
                }
            }
        }, 8);
        // ---- value windows (nsk_compile.h ep_win): per group the 16-byte chunks of the value array its members
        // lie in; member ids inside the kept chunks become offsets into the group's LDS copy
        c.ep_win.clear();
        c.ep_win_off.assign((size_t)ngroups + 1, 0u);
#ifdef NSK_EP_WIN
        const bool want_win = ngroups > 0 && c.vbytes == 1 && !knobs.no_ep_win && c.nid < (int64_t)NSK_EP_WIN_BASE;
#else
        const bool want_win = false;            // (measured and not kept: nsk_compile.h ep_win)
#endif
        if (want_win) {
            std::vector<std::vector<uint32_t>> kept((size_t)ngroups);
            std::vector<int64_t> st((size_t)compile_threads() * 2, 0);     // members in a window / members
            parallel_for(ngroups, [&](int64_t g0, int64_t g1, int t) {
                std::vector<uint32_t> ch;
                std::vector<std::pair<uint32_t, uint32_t>> cnt;        // (uses, chunk)
                for (int64_t gi = g0; gi < g1; gi++) {
                    const uint32_t *gd = &c.ep_desc[(size_t)gi * 4];
                    // every member word of the group's rows
                    ch.clear();
                    auto each_member = [&](auto &&fn) {
                        uint64_t sr = subrows[gi];
                        for (uint32_t cl = 0; cl < 8; cl++) {
                            const uint32_t m = cl & 3u, rows = (gd[cl < 4 ? 1 : 3] >> (8 * m)) & 255u;
                            for (uint64_t r = 0; r < rows; r++)
                                for (uint32_t mm = 0; mm < m; mm++) {
                                    uint32_t *row = &c.ep_adj[(sr + r * (2 + m) + 2 + mm) * 64];
                                    for (uint32_t e = 0; e < 64; e++) if ((row[e] & NSK_GEN_NULL) != NSK_GEN_NULL) fn(row[e]);
                                }
                            sr += (uint64_t)rows * (2 + m);
                        }
                    };
                    each_member([&](uint32_t &wd) { ch.push_back((wd & NSK_GEN_NULL) >> 4); });
                    std::sort(ch.begin(), ch.end());
                    cnt.clear();
                    for (size_t i = 0; i < ch.size();) {
                        size_t j = i;
                        while (j < ch.size() && ch[j] == ch[i]) j++;
                        cnt.emplace_back((uint32_t)(j - i), ch[i]);
                        i = j;
                    }
                    if (cnt.size() > NSK_EP_WIN_CHUNKS) {                // keep the most used chunks (ties: lowest id)
                        std::sort(cnt.begin(), cnt.end(), [](const std::pair<uint32_t, uint32_t> &a, const std::pair<uint32_t, uint32_t> &b) {
                            return a.first != b.first ? a.first > b.first : a.second < b.second; });
                        cnt.resize(NSK_EP_WIN_CHUNKS);
                    }
                    std::vector<uint32_t> &kp = kept[(size_t)gi];
                    kp.clear();
                    for (const auto &x : cnt) kp.push_back(x.second);
                    std::sort(kp.begin(), kp.end());
                    each_member([&](uint32_t &wd) {
                        const uint32_t id = wd & NSK_GEN_NULL;
                        const auto it = std::lower_bound(kp.begin(), kp.end(), id >> 4);
                        st[2 * (size_t)t + 1]++;
                        if (it == kp.end() || *it != (id >> 4)) return;
                        wd = (wd & ~NSK_GEN_NULL) | (NSK_EP_WIN_BASE + (uint32_t)(it - kp.begin()) * 16u + (id & 15u));
                        st[2 * (size_t)t]++;
                    });
                }
            }, 8);
            for (int64_t gi = 0; gi < ngroups; gi++) c.ep_win_off[gi + 1] = c.ep_win_off[gi] + (uint32_t)kept[(size_t)gi].size();
            c.ep_win.resize((size_t)c.ep_win_off[ngroups]);
            parallel_for(ngroups, [&](int64_t g0, int64_t g1, int) {
                for (int64_t gi = g0; gi < g1; gi++)
                    std::copy(kept[(size_t)gi].begin(), kept[(size_t)gi].end(), c.ep_win.begin() + c.ep_win_off[gi]);
            }, 64);
            if (knobs.verbose) {
                int64_t in = 0, all = 0;
                for (size_t t = 0; t < st.size(); t += 2) { in += st[t]; all += st[t + 1]; }
                fprintf(stderr, "[nsk] value windows: %.1f chunks per group, %.2f %% of %lld members inside\n",
                        (double)c.ep_win.size() / (double)ngroups, all ? 100.0 * (double)in / (double)all : 0.0, (long long)all);
            }
        }
        lap("entry-parallel groups: value windows");
        if (knobs.verbose && ngroups)
            fprintf(stderr, "[nsk] entry-parallel groups %lld, stream %.1f MB\n", (long long)ngroups,
                    (double)subrows[ngroups] * 256 / 1e6);
    }
    return NSK_OK;
}

// Hub streams: the long-list variables a whole wave (or workgroup) samples, laid out like the entry-parallel rows.
// general_words(v, &out, hub, cap) is the compiler's per-variable entry list (nsk_compile_words.cpp).
void CompileCtx::build_hub_streams() {
    // ---- entry-parallel hub streams: a hub (a long-list variable sampled by a whole wave) whose
    // factors are all of the general-tile kind gets its entries laid out one per LANE -- word j of
    // entry e of round r at hub_adj[off + (r * (2 + M) + j) * 64 + e] -- so that one coalesced row
    // load per word, one gather per member and a list-order sum over the lanes replace the
    // dependent fidx -> factor -> edge -> value chain of the generic hub walk.
    c.phase_hub_base.assign((size_t)ncolors + 1, 0);            // descriptors: hub ranges only, colour-major
    for (int32_t k = 0; k < ncolors; k++)
        c.phase_hub_base[k + 1] = c.phase_hub_base[k] + (c.phase_heavy_end[k] - c.phase_fast_end[k]);
    c.hub_desc.assign((size_t)(c.phase_hub_base[ncolors] + 1) * 4, 0u);
    c.phase_bighub_base.assign((size_t)ncolors + 1, 0);
    std::vector<int32_t> hub_colour;
    if (!knobs.no_hub_ep && !no_general) {
        std::vector<int64_t> hubs;
        for (int32_t k = 0; k < ncolors; k++)
            for (int64_t p = c.phase_fast_end[k]; p < c.phase_heavy_end[k]; p++)
                if (c.p_vid[p] >= 0) { hubs.push_back(p); hub_colour.push_back(k); }
        std::vector<uint32_t> nent(hubs.size(), 0), mh(hubs.size(), 0);
        parallel_for((int64_t)hubs.size(), [&](int64_t b0, int64_t b1, int) {
            std::vector<uint32_t> w;
            for (int64_t h = b0; h < b1; h++) {
                // (a colour laid out as entry-parallel groups has the block-per-hub kernels for long lists)
                if (!general_words(c.p_vid[hubs[h]], &w, true, c.phase_ep[hub_colour[h]] ? 16384 : 256)) continue;
                uint32_t ne = 0, mo = 0;
                for (size_t j = 0; j < w.size(); j += 2 + ((w[j + 1] >> 4) & 7u)) { ne++; mo = std::max(mo, (w[j + 1] >> 4) & 7u); }
                nent[h] = ne; mh[h] = mo;
            }
        }, 4);
        uint64_t total = 0;
        std::vector<uint64_t> off(hubs.size(), 0);
        for (size_t h = 0; h < hubs.size(); h++) {
            if (!nent[h]) continue;
            off[h] = total;
            total += (uint64_t)((nent[h] + 63) / 64) * (2 + mh[h]) * 64;
        }
        if (total < ((uint64_t)1 << 31)) {
            c.hub_adj.assign((size_t)total + 64, 0u);
            parallel_for((int64_t)hubs.size(), [&](int64_t b0, int64_t b1, int) {
                std::vector<uint32_t> w;
                for (int64_t h = b0; h < b1; h++) {
                    if (!nent[h]) continue;
                    const int64_t p = hubs[h];
                    const nsk_variable &var = d->variable[c.p_vid[p]];
                    general_words(c.p_vid[p], &w, true, 16384);
                    const uint32_t rows = 2 + mh[h], rounds = (nent[h] + 63) / 64;
                    uint32_t *base = &c.hub_adj[off[h]];
                    for (uint32_t r = 0; r < rounds; r++)              // padding entries: owned by no candidate
                        for (uint32_t e = 0; e < 64; e++) {
                            base[(r * rows + 0) * 64 + e] = 0u;
                            base[(r * rows + 1) * 64 + e] = 14u << 14;
                            for (uint32_t m = 0; m < mh[h]; m++) base[(r * rows + 2 + m) * 64 + e] = NSK_GEN_NULL;
                        }
                    uint32_t e = 0;
                    for (size_t j = 0; j < w.size(); e++) {
                        const uint32_t no = (w[j + 1] >> 4) & 7u, r = e / 64, l = e % 64;
                        base[(r * rows + 0) * 64 + l] = w[j];
                        base[(r * rows + 1) * 64 + l] = w[j + 1];
                        for (uint32_t m = 0; m < no; m++)
                            base[(r * rows + 2 + m) * 64 + l] = (uint32_t)c.iid[w[j + 2 + m] & NSK_GEN_NULL] | (w[j + 2 + m] & ~NSK_GEN_NULL);
                        j += 2 + no;
                    }
                    const int32_t hk = hub_colour[h];
                    uint32_t *hd = &c.hub_desc[(size_t)(c.phase_hub_base[hk] + (p - c.phase_fast_end[hk])) * 4];
                    // hd[3] = 1: a long list, evaluated by a whole workgroup (k_gibbs_ep / k_learn_ep)
                    hd[0] = (uint32_t)off[h]; hd[1] = nent[h]; hd[2] = mh[h] | ((uint32_t)var.cardinality << 8);
                    hd[3] = (c.phase_ep[hk] && nent[h] > 128) ? 1u : 0u;
                }
            }, 4);
            for (size_t h = 0; h < hubs.size(); h++) {          // (hubs are listed colour by colour)
                const int32_t hk = hub_colour[h];
                if (!c.hub_desc[(size_t)(c.phase_hub_base[hk] + (hubs[h] - c.phase_fast_end[hk])) * 4 + 3]) continue;
                c.bighub_pos.push_back((uint32_t)hubs[h]);
                c.phase_bighub_base[hk + 1]++;
            }
            c.nhub_ep = 0;
            for (size_t h = 0; h < hubs.size(); h++) if (nent[h]) c.nhub_ep++;
            if (knobs.verbose) fprintf(stderr, "[nsk] hubs %zu, entry-parallel %lld, stream %.1f MB\n", hubs.size(),
                                 (long long)c.nhub_ep, (double)total * 4 / 1e6);
        }
    }
    for (int32_t k = 0; k < ncolors; k++) c.phase_bighub_base[k + 1] += c.phase_bighub_base[k];
    if (c.bighub_pos.empty()) c.bighub_pos.push_back(0);
}

}  // namespace nsk
