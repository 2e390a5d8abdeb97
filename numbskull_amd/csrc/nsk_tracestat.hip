// nsk_tracestat.hip -- statistics of the sample trace computed where it lies (nsk_trace_ess, nsk_trace_autocov_counts,
// nsk_trace_pair_counts on bit-packed rows; nsk_trace_value_ess, nsk_trace_value_autocov_counts,
// nsk_trace_value_pair_counts on plain ones): the checks, the scratch and result buffers (allocated for the call alone),
// the launches of k_trace_autocov (nsk_kernels_tracestat.h), of k_trace_transpose / k_trace_pair_counts
// (nsk_kernels_tracepairs.h) and of k_trace_onehot / k_trace_autocov_planes (nsk_kernels_tracevalues.h) on the handle's
// stream and the permutation of the results to the caller's columns.  They read the trace and change nothing on the
// handle; the profiling bracket does not count their launches (sweep kernels only).
#include <hip/hip_runtime.h>

#include "nsk_internal.h"
#include "nsk_kernels_tracepairs.h"
#include "nsk_kernels_tracestat.h"
#include "nsk_kernels_tracevalues.h"

using namespace nsk;

// the result buffers of one call: off the books again wherever the call returns
struct TraceStatBuffers {
    nsk_graph *g;
    std::vector<void *> held;
    explicit TraceStatBuffers(nsk_graph *g_) : g(g_) {}
    TraceStatBuffers(const TraceStatBuffers &) = delete;
    ~TraceStatBuffers() { for (size_t i = held.size(); i-- > 0;) dev_free(g, held[i]); }
    template <typename T>
    int alloc(T **ptr, size_t n) {
        int rc = dev_alloc(g, ptr, n);
        if (!rc) held.push_back(*ptr);
        return rc;
    }
};

// The refusals both entry points share, and the window: n rows a half-chain, lags 0 .. L.  What depends on the
// arguments and the chain count alone (the int64 range among it) is decided before the rows recorded are looked at.
static int tracestat_window(const nsk_graph *g, const char *what, int64_t first_row, int64_t nrows, int64_t max_lag, TraceStatArgs &a) {
    const NskTrace &t = g->trace;
    const std::string w(what);
    if (t.capacity == 0) return fail(NSK_E_INVALID, w + ": no trace is set up");
    if (!t.packed) return fail(NSK_E_INVALID, w + ": the rows are not bit-packed (some traced variable is not binary)");
    if (nrows < 4) return fail(NSK_E_INVALID, w + ": at least 4 rows are needed");
    if (max_lag < 1 || max_lag > 63) return fail(NSK_E_INVALID, w + ": max_lag must lie in [1, 63]");
    if (first_row < 0) return fail(NSK_E_INVALID, w + ": rows beyond those recorded");
    const int64_t n = nrows / 2, H = 2 * (int64_t)t.chains;
    if (n >= ((int64_t)1 << 21) || (unsigned __int128)4 * (unsigned __int128)H * (unsigned __int128)n * (unsigned __int128)n * (unsigned __int128)n >= ((unsigned __int128)1 << 63))
        return fail(NSK_E_RANGE, w + ": 4 x half-chains x (rows / 2)^3 reaches 2^63: the counts do not fit int64 (fewer rows, or thin more)");
    if (nrows > t.rows || first_row > t.rows - nrows) return fail(NSK_E_INVALID, w + ": rows beyond those recorded");
    a.nwords = (long long)(t.row_bytes / 8);
    a.chains = t.chains;
    a.rows = (const unsigned long long *)t.buf + (size_t)first_row * (size_t)t.chains * (size_t)a.nwords;
    a.n = n;
    a.second = nrows - n;
    a.L = (int)std::min<int64_t>(max_lag, n - 1);
    // (each product rounded once, left to right: DESIGN.md section 4, diagnostics.ess_from_counts)
    a.D = (double)H * (double)n * (double)n * (double)(n - 1);
    a.Bden = (double)H * (double)(H - 1) * (double)n * (double)n;
    a.c1 = (double)(n - 1) / (double)n;
    a.Hn = (double)(H * n);
    return NSK_OK;
}

template <bool SUMMARY>
static int tracestat_launch(nsk_graph *g, const TraceStatArgs &a) {
    const dim3 grid((unsigned int)((a.nslots + NSK_TRACESTAT_BLOCK / 64 - 1) / (NSK_TRACESTAT_BLOCK / 64))), block(NSK_TRACESTAT_BLOCK);
    if (a.L <= 15) k_trace_autocov<15, SUMMARY><<<grid, block, 0, g->stream>>>(a);
    else if (a.L <= 31) k_trace_autocov<31, SUMMARY><<<grid, block, 0, g->stream>>>(a);
    else k_trace_autocov<63, SUMMARY><<<grid, block, 0, g->stream>>>(a);
    HIPCHECK(hipGetLastError());
    return NSK_OK;
}

static int tracestat_nomem(const char *what, double bytes, const char *which = "result") {
    return fail(NSK_E_NOMEM, std::string(what) + ": the " + which + " buffers (" + std::to_string((long long)(bytes / 1048576.0)) + " MB) do not fit on the device");
}

// ---- plain rows: indicators (trace column, value) -----------------------------------------------------------------------

// The indicators of a call: the caller's (column, value) entries as distinct (device column, value), sorted, with the
// column tiles of k_trace_onehot and the way back.
struct ValueIndicators {
    std::vector<uint64_t> keys;        // device column << 32 | value, sorted, each once
    std::vector<int32_t> ind;          // ... as (column, value)
    std::vector<int32_t> tiles;        // (column / 64, first indicator, one past the last) per tile that has any
    std::vector<int64_t> where;        // the caller's entry e is indicator where[e]
    size_t n() const { return keys.size(); }
    size_t npad() const { return (keys.size() + 63) / 64 * 64; }
};

// what every nsk_trace_value_* call refuses first
static int values_trace(const nsk_graph *g, const std::string &w, const char *binary) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    const NskTrace &t = g->trace;
    if (t.capacity == 0) return fail(NSK_E_INVALID, w + ": no trace is set up");
    if (t.packed) return fail(NSK_E_INVALID, w + ": the rows are bit-packed (every traced variable is binary): " + binary + " serves them");
    return NSK_OK;
}

// entries: count x (caller's column, value); every column is looked at before any value
static int values_indicators(const nsk_graph *g, const std::string &w, const int64_t *entries, int64_t count, ValueIndicators &vi) {
    const NskTrace &t = g->trace;
    for (int64_t e = 0; e < count; e++)
        if (entries[2 * e] < 0 || entries[2 * e] >= t.ncols) return fail(NSK_E_INDEX, w + ": column index out of range");
    for (int64_t e = 0; e < count; e++)
        if (entries[2 * e + 1] < 0 || entries[2 * e + 1] >= (int64_t)t.card[(size_t)entries[2 * e]])
            return fail(NSK_E_RANGE, w + ": a value lies outside [0, cardinality) of its column's variable");
    vi.keys.resize((size_t)count);
    for (int64_t e = 0; e < count; e++) vi.keys[(size_t)e] = ((uint64_t)t.pos[(size_t)entries[2 * e]] << 32) | (uint64_t)entries[2 * e + 1];
    std::sort(vi.keys.begin(), vi.keys.end());
    vi.keys.erase(std::unique(vi.keys.begin(), vi.keys.end()), vi.keys.end());
    vi.where.resize((size_t)count);
    nsk::parallel_for(count, [&](int64_t b0, int64_t b1, int) {
        for (int64_t e = b0; e < b1; e++) {
            const uint64_t key = ((uint64_t)t.pos[(size_t)entries[2 * e]] << 32) | (uint64_t)entries[2 * e + 1];
            vi.where[(size_t)e] = std::lower_bound(vi.keys.begin(), vi.keys.end(), key) - vi.keys.begin();
        }
    });
    vi.ind.resize(2 * vi.n());
    for (size_t i = 0; i < vi.n(); i++) {
        const int32_t col = (int32_t)(vi.keys[i] >> 32);
        vi.ind[2 * i] = col;
        vi.ind[2 * i + 1] = (int32_t)(vi.keys[i] & 0xffffffffull);
        if (vi.tiles.empty() || vi.tiles[vi.tiles.size() - 3] != col / 64) {
            vi.tiles.push_back(col / 64); vi.tiles.push_back((int32_t)i); vi.tiles.push_back((int32_t)i);
        }
        vi.tiles.back() = (int32_t)(i + 1);
    }
    return NSK_OK;
}

// bytes of the lists values_planes uploads
static double values_list_bytes(const ValueIndicators &vi, size_t nsegs) {
    return 8.0 * (double)vi.n() + 4.0 * (double)vi.tiles.size() + 24.0 * (double)nsegs;
}

// The planes of the window: uploads the lists (vi and segs must live until the stream is synchronised) and launches
// k_trace_onehot.  segs: (chain, first row, length) a segment, all of `length` rows.
static int values_planes(nsk_graph *g, TraceStatBuffers &buf, const ValueIndicators &vi, const std::vector<long long> &segs, long long length,
                         long long s_ind, long long s_seg, long long s_blk, size_t plane_words, unsigned long long **planes) {
    const NskTrace &t = g->trace;
    TraceOnehotArgs o = {};
    o.buf = t.buf;
    o.chains = t.chains;
    o.ndev = t.ndev;
    o.ntiles = (long long)(vi.tiles.size() / 3);
    o.nsegs = (long long)(segs.size() / 3);
    o.nb = (length + 63) / 64;
    o.s_ind = s_ind; o.s_seg = s_seg; o.s_blk = s_blk;
    int32_t *dind = nullptr, *dtiles = nullptr;
    long long *dsegs = nullptr;
    int rc = buf.alloc(&dind, vi.ind.size());
    if (!rc) rc = buf.alloc(&dtiles, vi.tiles.size());
    if (!rc) rc = buf.alloc(&dsegs, segs.size());
    if (!rc) rc = buf.alloc(planes, plane_words);
    if (rc) return rc;
    HIPCHECK(hipMemcpyAsync(dind, vi.ind.data(), vi.ind.size() * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    HIPCHECK(hipMemcpyAsync(dtiles, vi.tiles.data(), vi.tiles.size() * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    HIPCHECK(hipMemcpyAsync(dsegs, segs.data(), segs.size() * sizeof(long long), hipMemcpyHostToDevice, g->stream));
    o.ind = dind; o.tiles = dtiles; o.segs = dsegs; o.out = *planes;
    const dim3 grid((unsigned int)(o.ntiles * o.nsegs * o.nb)), block(NSK_TRACEVALUES_OBLOCK);
    if (g->c.vbytes == 1) k_trace_onehot<int8_t><<<grid, block, 0, g->stream>>>(o);
    else k_trace_onehot<int32_t><<<grid, block, 0, g->stream>>>(o);
    HIPCHECK(hipGetLastError());
    return NSK_OK;
}

// nsk_trace_value_autocov_counts (SUMMARY = false: out) and nsk_trace_value_ess (the four arrays), one body
template <bool SUMMARY>
static int values_autocov(nsk_graph *g, const char *what, int64_t first_row, int64_t nrows, int64_t max_lag, const int64_t *sel, int64_t nsel,
                          int64_t *out, double *mean, double *tau, double *rhat2, uint8_t *truncated) {
    const std::string w(what);
    if (int rc = values_trace(g, w, SUMMARY ? "nsk_trace_ess" : "nsk_trace_autocov_counts")) return rc;
    const NskTrace &t = g->trace;
    if (nrows < 4) return fail(NSK_E_INVALID, w + ": at least 4 rows are needed");
    if (max_lag < 1 || max_lag > 63) return fail(NSK_E_INVALID, w + ": max_lag must lie in [1, 63]");
    if (first_row < 0) return fail(NSK_E_INVALID, w + ": rows beyond those recorded");
    if (nsel < 0 || (nsel > 0 && (!sel || (!SUMMARY && !out)))) return fail(NSK_E_INVALID, w + ": null argument");
    const int64_t n = nrows / 2, R = t.chains, H = 2 * R;
    if (n >= ((int64_t)1 << 21) || (unsigned __int128)4 * (unsigned __int128)H * (unsigned __int128)n * (unsigned __int128)n * (unsigned __int128)n >= ((unsigned __int128)1 << 63))
        return fail(NSK_E_RANGE, w + ": 4 x half-chains x (rows / 2)^3 reaches 2^63: the counts do not fit int64 (fewer rows, or thin more)");
    ValueIndicators vi;
    if (int rc = values_indicators(g, w, sel, nsel, vi)) return rc;
    if (nrows > t.rows || first_row > t.rows - nrows) return fail(NSK_E_INVALID, w + ": rows beyond those recorded");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    if (nsel == 0) return NSK_OK;
    TraceValuesArgs a = {};
    a.s.chains = R;
    a.s.n = n;
    a.s.second = nrows - n;
    a.s.L = (int)std::min<int64_t>(max_lag, n - 1);
    // (each product rounded once, left to right: DESIGN.md section 4, diagnostics.ess_from_counts)
    a.s.D = (double)H * (double)n * (double)n * (double)(n - 1);
    a.s.Bden = (double)H * (double)(H - 1) * (double)n * (double)n;
    a.s.c1 = (double)(n - 1) / (double)n;
    a.s.Hn = (double)(H * n);
    a.nind = (long long)vi.n();
    a.npad = (long long)vi.npad();
    // the half-chains of diagnostics._split as segments
    std::vector<long long> segs;
    for (int64_t h = 0; h < H; h++) {
        segs.push_back(h < R ? h : h - R);
        segs.push_back(first_row + (h < R ? 0 : nrows - n));
        segs.push_back(n);
    }
    const long long nb = (n + 63) / 64;
    const size_t per = (size_t)(a.s.L + 3), nres = vi.npad() * (SUMMARY ? 1 : per);
    const double plane_words = (double)vi.npad() * (double)H * (double)nb;
    const double bytes = values_list_bytes(vi, (size_t)H) + 8.0 * plane_words + (SUMMARY ? 25.0 : 8.0) * (double)nres;
    const double ogrid = (double)(vi.tiles.size() / 3) * (double)H * (double)nb;
    if (bytes >= 9.0e18 || ogrid >= 2147483648.0 || vi.npad() / NSK_TRACEVALUES_ABLOCK >= 2147483647ull)
        return tracestat_nomem(what, bytes, "indicator list, plane and result");
    TraceStatBuffers buf(g);
    unsigned long long *planes = nullptr;
    double *dev = nullptr;
    // [half-chain][blk][indicator]
    int rc = values_planes(g, buf, vi, segs, n, 1, nb * a.npad, a.npad, (size_t)plane_words, &planes);
    if (!rc && SUMMARY) rc = buf.alloc(&dev, 3 * nres);
    if (!rc && SUMMARY) rc = buf.alloc(&a.s.truncated, nres);
    if (!rc && !SUMMARY) rc = buf.alloc(&a.s.counts, nres);
    if (rc) return rc == NSK_E_NOMEM ? tracestat_nomem(what, bytes, "indicator list, plane and result") : rc;
    a.planes = planes;
    a.s.mean = dev; a.s.tau = dev + nres; a.s.rhat2 = dev + 2 * nres;
    const dim3 grid((unsigned int)((vi.npad() + NSK_TRACEVALUES_ABLOCK - 1) / NSK_TRACEVALUES_ABLOCK)), block(NSK_TRACEVALUES_ABLOCK);
    if (a.s.L <= 15) k_trace_autocov_planes<15, SUMMARY><<<grid, block, 0, g->stream>>>(a);
    else if (a.s.L <= 31) k_trace_autocov_planes<31, SUMMARY><<<grid, block, 0, g->stream>>>(a);
    else k_trace_autocov_planes<63, SUMMARY><<<grid, block, 0, g->stream>>>(a);
    HIPCHECK(hipGetLastError());
    if (!SUMMARY) {
        std::vector<long long> hc(vi.n() * per);
        HIPCHECK(hipMemcpyAsync(hc.data(), a.s.counts, hc.size() * sizeof(long long), hipMemcpyDeviceToHost, g->stream));
        HIPCHECK(hipStreamSynchronize(g->stream));
        nsk::parallel_for(nsel, [&](int64_t b0, int64_t b1, int) {
            for (int64_t j = b0; j < b1; j++) {
                const long long *src = hc.data() + (size_t)vi.where[(size_t)j] * per;
                for (size_t k = 0; k < per; k++) out[(size_t)j * per + k] = (int64_t)src[k];
            }
        });
        return NSK_OK;
    }
    // only what the caller asked for crosses to the host
    double *const want[3] = {mean, tau, rhat2};
    std::vector<double> hd(mean || tau || rhat2 ? 3 * nres : 0);
    std::vector<uint8_t> ht(truncated ? nres : 0);
    for (int i = 0; i < 3; i++)
        if (want[i]) HIPCHECK(hipMemcpyAsync(hd.data() + (size_t)i * nres, dev + (size_t)i * nres, vi.n() * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    if (truncated) HIPCHECK(hipMemcpyAsync(ht.data(), a.s.truncated, vi.n(), hipMemcpyDeviceToHost, g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    nsk::parallel_for(nsel, [&](int64_t b0, int64_t b1, int) {
        for (int64_t j = b0; j < b1; j++) {
            const size_t p = (size_t)vi.where[(size_t)j];
            if (mean) mean[j] = hd[p];
            if (tau) tau[j] = hd[nres + p];
            if (rhat2) rhat2[j] = hd[2 * nres + p];
            if (truncated) truncated[j] = ht[p];
        }
    });
    return NSK_OK;
}

extern "C" {

int nsk_trace_ess(nsk_graph *g, int64_t first_row, int64_t nrows, int64_t max_lag, double *mean, double *tau, double *rhat2, uint8_t *truncated) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    TraceStatArgs a = {};
    if (int rc = tracestat_window(g, "nsk_trace_ess", first_row, nrows, max_lag, a)) return rc;
    const NskTrace &t = g->trace;
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    a.nslots = a.nwords;
    const size_t nd = (size_t)a.nwords * 64;
    if (nd == 0) return NSK_OK;
    TraceStatBuffers buf(g);
    double *dev = nullptr;
    int rc = buf.alloc(&dev, 3 * nd);
    if (!rc) rc = buf.alloc(&a.truncated, nd);
    if (rc) return rc == NSK_E_NOMEM ? tracestat_nomem("nsk_trace_ess", 25.0 * (double)nd) : rc;
    a.mean = dev; a.tau = dev + nd; a.rhat2 = dev + 2 * nd;
    if ((rc = tracestat_launch<true>(g, a))) return rc;
    // only what the caller asked for crosses to the host
    double *const want[3] = {mean, tau, rhat2};
    std::vector<double> hd(mean || tau || rhat2 ? 3 * nd : 0);
    std::vector<uint8_t> ht(truncated ? nd : 0);
    for (int i = 0; i < 3; i++)
        if (want[i]) HIPCHECK(hipMemcpyAsync(hd.data() + (size_t)i * nd, dev + (size_t)i * nd, nd * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    if (truncated) HIPCHECK(hipMemcpyAsync(ht.data(), a.truncated, nd, hipMemcpyDeviceToHost, g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    if (!mean && !tau && !rhat2 && !truncated) return NSK_OK;
    // device columns -> the caller's, over the host threads
    const int64_t *pos = t.pos.data();
    const double *hm = hd.data(), *hta = hd.data() + nd, *hr = hd.data() + 2 * nd;
    nsk::parallel_for(t.ncols, [&](int64_t b0, int64_t b1, int) {
        for (int64_t j = b0; j < b1; j++) {
            const int64_t p = pos[j];
            if (mean) mean[j] = hm[p];
            if (tau) tau[j] = hta[p];
            if (rhat2) rhat2[j] = hr[p];
            if (truncated) truncated[j] = ht[(size_t)p];
        }
    });
    return NSK_OK;
}

int nsk_trace_autocov_counts(nsk_graph *g, int64_t first_row, int64_t nrows, int64_t max_lag, const int64_t *cols, int64_t ncols_sel, int64_t *out) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    TraceStatArgs a = {};
    if (int rc = tracestat_window(g, "nsk_trace_autocov_counts", first_row, nrows, max_lag, a)) return rc;
    const NskTrace &t = g->trace;
    if (ncols_sel < 0 || (ncols_sel > 0 && (!cols || !out))) return fail(NSK_E_INVALID, "nsk_trace_autocov_counts: null argument");
    for (int64_t j = 0; j < ncols_sel; j++)
        if (cols[j] < 0 || cols[j] >= t.ncols) return fail(NSK_E_INDEX, "nsk_trace_autocov_counts: column index out of range");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    if (ncols_sel == 0) return NSK_OK;
    // the words the selection touches, each served once
    std::vector<int32_t> words((size_t)ncols_sel);
    for (int64_t j = 0; j < ncols_sel; j++) words[(size_t)j] = (int32_t)(t.pos[(size_t)cols[j]] >> 6);
    std::sort(words.begin(), words.end());
    words.erase(std::unique(words.begin(), words.end()), words.end());
    a.nslots = (long long)words.size();
    const size_t per = (size_t)(a.L + 3), nc = words.size() * 64 * per;
    TraceStatBuffers buf(g);
    int32_t *dwords = nullptr;
    int rc = buf.alloc(&dwords, words.size());
    if (!rc) rc = buf.alloc(&a.counts, nc);
    if (rc) return rc == NSK_E_NOMEM ? tracestat_nomem("nsk_trace_autocov_counts", 8.0 * (double)nc + 4.0 * (double)words.size()) : rc;
    HIPCHECK(hipMemcpyAsync(dwords, words.data(), words.size() * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    a.words = dwords;
    if ((rc = tracestat_launch<false>(g, a))) return rc;
    std::vector<long long> hc(nc);
    HIPCHECK(hipMemcpyAsync(hc.data(), a.counts, nc * sizeof(long long), hipMemcpyDeviceToHost, g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    nsk::parallel_for(ncols_sel, [&](int64_t b0, int64_t b1, int) {
        for (int64_t j = b0; j < b1; j++) {
            const int64_t p = t.pos[(size_t)cols[j]];
            const size_t slot = (size_t)(std::lower_bound(words.begin(), words.end(), (int32_t)(p >> 6)) - words.begin());
            const long long *src = hc.data() + (slot * 64 + (size_t)(p & 63)) * per;
            for (size_t k = 0; k < per; k++) out[(size_t)j * per + k] = (int64_t)src[k];
        }
    });
    return NSK_OK;
}

int nsk_trace_pair_counts(nsk_graph *g, int64_t first_row, int64_t nrows, const int64_t *pairs, int64_t npairs, int64_t *out) {
    const std::string w("nsk_trace_pair_counts");
    if (!g) return fail(NSK_E_INVALID, "null graph");
    const NskTrace &t = g->trace;
    if (t.capacity == 0) return fail(NSK_E_INVALID, w + ": no trace is set up");
    if (!t.packed) return fail(NSK_E_INVALID, w + ": the rows are not bit-packed (some traced variable is not binary)");
    if (nrows < 1) return fail(NSK_E_INVALID, w + ": at least 1 row is needed");
    if (first_row < 0) return fail(NSK_E_INVALID, w + ": rows beyond those recorded");
    if (npairs < 0 || (npairs > 0 && (!pairs || !out))) return fail(NSK_E_INVALID, w + ": null argument");
    if (nrows > t.rows || first_row > t.rows - nrows) return fail(NSK_E_INVALID, w + ": rows beyond those recorded");
    for (int64_t j = 0; j < 2 * npairs; j++)
        if (pairs[j] < 0 || pairs[j] >= t.ncols) return fail(NSK_E_INDEX, w + ": column index out of range");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    if (npairs == 0) return NSK_OK;
    // the words the pairs touch, each transposed once
    std::vector<int32_t> words((size_t)(2 * npairs));
    for (int64_t j = 0; j < 2 * npairs; j++) words[(size_t)j] = (int32_t)(t.pos[(size_t)pairs[j]] >> 6);
    std::sort(words.begin(), words.end());
    words.erase(std::unique(words.begin(), words.end()), words.end());
    // ... and the pairs as columns of T
    std::vector<long long> tcols((size_t)(2 * npairs));
    nsk::parallel_for(2 * npairs, [&](int64_t b0, int64_t b1, int) {
        for (int64_t j = b0; j < b1; j++) {
            const int64_t p = t.pos[(size_t)pairs[j]];
            const int64_t slot = std::lower_bound(words.begin(), words.end(), (int32_t)(p >> 6)) - words.begin();
            tcols[(size_t)j] = (long long)(slot * 64 + (p & 63));
        }
    });
    TracePairsArgs a = {};
    a.nwords = (long long)(t.row_bytes / 8);
    a.chains = t.chains;
    a.rows = (const unsigned long long *)t.buf + (size_t)first_row * (size_t)t.chains * (size_t)a.nwords;
    a.nslots = (long long)words.size();
    a.nrows = nrows;
    a.nb = (nrows + 63) / 64;
    a.bgroups = (a.nb + NSK_TRACEPAIRS_TBLKS - 1) / NSK_TRACEPAIRS_TBLKS;
    a.npairs = npairs;
    a.G = 1;
    while (a.G < 64 && a.G < a.nb) a.G *= 2;
    const double tiles = (double)words.size() * (double)a.chains * (double)a.nb, nres = 3.0 * (double)npairs * (double)a.chains;
    const double bytes = 512.0 * tiles + 4.0 * (double)words.size() + 16.0 * (double)npairs + 8.0 * nres;
    const long long sgroups = (a.nslots + NSK_TRACEPAIRS_TBLOCK / 64 - 1) / (NSK_TRACEPAIRS_TBLOCK / 64);
    const double tgrid = (double)sgroups * (double)a.chains * (double)a.bgroups;
    const long long pgrid = (npairs + NSK_TRACEPAIRS_PBLOCK / 64 - 1) / (NSK_TRACEPAIRS_PBLOCK / 64);
    if (bytes >= 9.0e18 || tgrid >= 2147483648.0 || pgrid >= 2147483648ll) return tracestat_nomem("nsk_trace_pair_counts", bytes, "scratch and result");
    const size_t nT = words.size() * 64 * (size_t)a.chains * (size_t)a.nb, nc = 3 * (size_t)npairs * (size_t)a.chains;
    TraceStatBuffers buf(g);
    int32_t *dwords = nullptr;
    long long *dpairs = nullptr;
    int rc = buf.alloc(&dwords, words.size());
    if (!rc) rc = buf.alloc(&dpairs, tcols.size());
    if (!rc) rc = buf.alloc(&a.T, nT);
    if (!rc) rc = buf.alloc(&a.counts, nc);
    if (rc) return rc == NSK_E_NOMEM ? tracestat_nomem("nsk_trace_pair_counts", bytes, "scratch and result") : rc;
    HIPCHECK(hipMemcpyAsync(dwords, words.data(), words.size() * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    HIPCHECK(hipMemcpyAsync(dpairs, tcols.data(), tcols.size() * sizeof(long long), hipMemcpyHostToDevice, g->stream));
    a.words = dwords;
    a.pairs = dpairs;
    k_trace_transpose<<<dim3((unsigned int)(sgroups * a.chains * a.bgroups)), dim3(NSK_TRACEPAIRS_TBLOCK), 0, g->stream>>>(a);
    HIPCHECK(hipGetLastError());
    k_trace_pair_counts<<<dim3((unsigned int)pgrid), dim3(NSK_TRACEPAIRS_PBLOCK), 0, g->stream>>>(a);
    HIPCHECK(hipGetLastError());
    static_assert(sizeof(long long) == sizeof(int64_t), "the counts go to the caller as they are");
    HIPCHECK(hipMemcpyAsync(out, a.counts, nc * sizeof(long long), hipMemcpyDeviceToHost, g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    return NSK_OK;
}

int nsk_trace_value_autocov_counts(nsk_graph *g, int64_t first_row, int64_t nrows, int64_t max_lag, const int64_t *sel, int64_t nsel, int64_t *out) {
    return values_autocov<false>(g, "nsk_trace_value_autocov_counts", first_row, nrows, max_lag, sel, nsel, out, nullptr, nullptr, nullptr, nullptr);
}

int nsk_trace_value_ess(nsk_graph *g, int64_t first_row, int64_t nrows, int64_t max_lag, const int64_t *sel, int64_t nsel,
                        double *mean, double *tau, double *rhat2, uint8_t *truncated) {
    return values_autocov<true>(g, "nsk_trace_value_ess", first_row, nrows, max_lag, sel, nsel, nullptr, mean, tau, rhat2, truncated);
}

int nsk_trace_value_pair_counts(nsk_graph *g, int64_t first_row, int64_t nrows, const int64_t *quads, int64_t npairs, int64_t *out) {
    const char *what = "nsk_trace_value_pair_counts";
    const std::string w(what);
    if (int rc = values_trace(g, w, "nsk_trace_pair_counts")) return rc;
    const NskTrace &t = g->trace;
    if (nrows < 1) return fail(NSK_E_INVALID, w + ": at least 1 row is needed");
    if (first_row < 0) return fail(NSK_E_INVALID, w + ": rows beyond those recorded");
    if (npairs < 0 || (npairs > 0 && (!quads || !out))) return fail(NSK_E_INVALID, w + ": null argument");
    ValueIndicators vi;
    if (int rc = values_indicators(g, w, quads, 2 * npairs, vi)) return rc;     // (a quad is two entries)
    if (nrows > t.rows || first_row > t.rows - nrows) return fail(NSK_E_INVALID, w + ": rows beyond those recorded");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    if (npairs == 0) return NSK_OK;
    // the planes are the T of k_trace_pair_counts: [indicator][chain][blk] over the whole window
    std::vector<long long> segs;
    for (int64_t r = 0; r < t.chains; r++) { segs.push_back(r); segs.push_back(first_row); segs.push_back(nrows); }
    TracePairsArgs a = {};
    a.chains = t.chains;
    a.nrows = nrows;
    a.nb = (nrows + 63) / 64;
    a.npairs = npairs;
    a.G = 1;
    while (a.G < 64 && a.G < a.nb) a.G *= 2;
    const double plane_words = (double)vi.n() * (double)a.chains * (double)a.nb, nres = 3.0 * (double)npairs * (double)a.chains;
    const double bytes = values_list_bytes(vi, (size_t)a.chains) + 8.0 * plane_words + 16.0 * (double)npairs + 8.0 * nres;
    const double ogrid = (double)(vi.tiles.size() / 3) * (double)a.chains * (double)a.nb;
    const long long pgrid = (npairs + NSK_TRACEPAIRS_PBLOCK / 64 - 1) / (NSK_TRACEPAIRS_PBLOCK / 64);
    if (bytes >= 9.0e18 || ogrid >= 2147483648.0 || pgrid >= 2147483648ll) return tracestat_nomem(what, bytes, "indicator list, plane and result");
    const size_t nc = 3 * (size_t)npairs * (size_t)a.chains;
    TraceStatBuffers buf(g);
    long long *dpairs = nullptr;
    int rc = values_planes(g, buf, vi, segs, nrows, a.chains * a.nb, a.nb, 1, (size_t)plane_words, &a.T);
    if (!rc) rc = buf.alloc(&dpairs, vi.where.size());
    if (!rc) rc = buf.alloc(&a.counts, nc);
    if (rc) return rc == NSK_E_NOMEM ? tracestat_nomem(what, bytes, "indicator list, plane and result") : rc;
    static_assert(sizeof(long long) == sizeof(int64_t), "the indicator indices go to the device, the counts to the caller, as they are");
    HIPCHECK(hipMemcpyAsync(dpairs, vi.where.data(), vi.where.size() * sizeof(long long), hipMemcpyHostToDevice, g->stream));
    a.pairs = dpairs;
    k_trace_pair_counts<<<dim3((unsigned int)pgrid), dim3(NSK_TRACEPAIRS_PBLOCK), 0, g->stream>>>(a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(out, a.counts, nc * sizeof(long long), hipMemcpyDeviceToHost, g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    return NSK_OK;
}

}  // extern "C"
