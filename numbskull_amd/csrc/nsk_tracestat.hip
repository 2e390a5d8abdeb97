// nsk_tracestat.hip -- statistics of the sample trace computed where it lies (nsk_trace_ess, nsk_trace_autocov_counts,
// nsk_trace_pair_counts): the checks, the scratch and result buffers (allocated for the call alone), the launches of
// k_trace_autocov (nsk_kernels_tracestat.h) and of k_trace_transpose / k_trace_pair_counts (nsk_kernels_tracepairs.h)
// on the handle's stream and the permutation of the results to the caller's columns.  They read the trace and change
// nothing on the handle; the profiling bracket does not count their launches (sweep kernels only).
#include <hip/hip_runtime.h>

#include "nsk_internal.h"
#include "nsk_kernels_tracepairs.h"
#include "nsk_kernels_tracestat.h"

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

}  // extern "C"
