// nsk_trace.hip -- the sample trace (nsk_internal.h NskTrace): set-up, the record launch behind a tallied sweep (called by
// nsk_gibbs_sweeps where a row is due), download.  Its lp column lives in nsk_energy.hip, its stats column in nsk_wstats.hip,
// its accumulators of conditionals in nsk_cond.hip.
#include <hip/hip_runtime.h>

#include "nsk_internal.h"
#include "nsk_kernels_misc.h"

using namespace nsk;

// rows as downloaded (device column order, packed or plain) -> the caller's columns, over the host threads
template <typename VT>
static void trace_unpack(const NskTrace &t, const uint8_t *host, int64_t nrows, VT *out) {
    const int64_t ncols = t.ncols, nrc = nrows * t.chains;
    const int64_t *pos = t.pos.data();
    nsk::parallel_for(nrc * ncols, [&](int64_t b0, int64_t b1, int) {
        int64_t rc = ncols ? b0 / ncols : 0, j = ncols ? b0 % ncols : 0;
        for (int64_t e = b0; e < b1; e++) {
            const uint8_t *row = host + (size_t)rc * t.row_bytes;
            const int64_t p = pos[j];
            out[e] = t.packed ? (VT)((((const unsigned long long *)row)[p >> 6] >> (p & 63)) & 1ull) : ((const VT *)row)[p];
            if (++j == ncols) { j = 0; rc++; }
        }
    });
}

static void trace_free(nsk_graph *g) {
    NskTrace &t = g->trace;
    dev_free(g, t.buf);
    dev_free(g, t.cols);
    dev_free(g, t.lp);
    dev_free(g, t.ws);
    wstats_plan_free(g, t.ws_plan);
    dev_free(g, t.cond);
    nsk_cond_sel_free(g, t.cond_sel);
    t = NskTrace();
}

extern "C" {

int nsk_trace_setup(nsk_graph *g, const int64_t *vids, int64_t nvids, int64_t every, int64_t capacity) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));          // (record launches into the buffer that goes)
    if (capacity == 0) { if (g->trace.capacity > 0) trace_free(g); return NSK_OK; }
    const Compiled &c = g->c;
    if (int rc = energy_whole_graph(g, "nsk_trace_setup")) return rc;       // (the same two refusals, word for word)
    if (every < 1 || capacity < 1) return fail(NSK_E_INVALID, "nsk_trace_setup: every and capacity must be at least 1");
    if (vids && nvids < 1) return fail(NSK_E_INVALID, "nsk_trace_setup: a list of variable ids needs at least one");
    if (!vids && c.nvar < 1) return fail(NSK_E_INVALID, "nsk_trace_setup: the graph has no variables");
    NskTrace t;
    t.ncols = vids ? nvids : c.nvar;
    t.every = every;
    t.chains = g->nchains;
    t.packed = true;
    t.pos.resize((size_t)t.ncols);
    t.card.resize((size_t)t.ncols);
    std::vector<int32_t> cols;
    if (vids) {
        for (int64_t j = 0; j < nvids; j++) {
            if (vids[j] < 0 || vids[j] >= c.nvar) return fail(NSK_E_INDEX, "nsk_trace_setup: variable id out of range");
            t.packed = t.packed && c.v_card[(size_t)vids[j]] == 2;
            t.card[(size_t)j] = c.v_card[(size_t)vids[j]];
            cols.push_back(c.iid[(size_t)vids[j]]);
        }
        std::sort(cols.begin(), cols.end());            // a full-state trace reads the value array front to back
        cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
        for (int64_t j = 0; j < nvids; j++)
            t.pos[(size_t)j] = std::lower_bound(cols.begin(), cols.end(), c.iid[(size_t)vids[j]]) - cols.begin();
        t.ndev = (int64_t)cols.size();
    } else {                                            // every variable: the device records every internal id, no index list
        for (int64_t v = 0; v < c.nvar; v++) { t.packed = t.packed && c.v_card[(size_t)v] == 2; t.pos[(size_t)v] = c.iid[(size_t)v]; t.card[(size_t)v] = c.v_card[(size_t)v]; }
        t.ndev = c.nid;
    }
    t.row_bytes = t.packed ? (size_t)((t.ndev + 63) / 64) * 8 : (size_t)t.ndev * (size_t)c.vbytes;
    const double total = (double)capacity * (double)t.chains * (double)t.row_bytes;
    if (total >= 281474976710656.0) return fail(NSK_E_NOMEM, "nsk_trace_setup: the trace does not fit");
    // the arguments hold: the trace this one replaces goes now, before the new buffer is asked for (the two need not fit
    // side by side; a set-up that fails for lack of memory leaves no trace)
    if (g->trace.capacity > 0) trace_free(g);
    NskRollback rb(g->mem, nsk_free_raw);
    uint8_t *buf = nullptr;
    int rc = dev_alloc(g, &buf, (size_t)capacity * (size_t)t.chains * t.row_bytes);
    if (rc) return rc;
    t.buf = buf;
    if (vids) {
        rc = dev_upload(g, &t.cols, cols);
        if (rc) return rc;
        HIPCHECK(hipStreamSynchronize(g->stream));      // (the upload reads a local vector)
    }
    rb.commit();
    t.capacity = capacity;
    g->trace = std::move(t);
    return NSK_OK;
}

int nsk_trace_rows(nsk_graph *g, int64_t *rows, int64_t *capacity, int64_t *packed) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (rows) *rows = g->trace.rows;
    if (capacity) *capacity = g->trace.capacity;
    if (packed) *packed = g->trace.capacity > 0 && g->trace.packed ? 1 : 0;
    return NSK_OK;
}

int nsk_trace_clear(nsk_graph *g) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (g->trace.capacity == 0) return fail(NSK_E_INVALID, "nsk_trace_clear: no trace is set up");
    g->trace.rows = g->trace.phase = 0;
    g->trace.sweep_index.clear();
    if (g->trace.cond) {    // the accumulators start over (behind the launches that still add to them)
        HIPCHECK(hipSetDevice(g->device));
        HIPCHECK(hipMemsetAsync(g->trace.cond, 0, std::max<size_t>(1, (size_t)g->trace.chains * (size_t)g->trace.cond_sel.dtotal()) * sizeof(double), g->stream));
        g->trace.cond_rows = 0;
    }
    return NSK_OK;
}

int nsk_trace_download(nsk_graph *g, int64_t first_row, int64_t nrows, void *out, int64_t *sweep_index) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    const NskTrace &t = g->trace;
    if (t.capacity == 0) return fail(NSK_E_INVALID, "nsk_trace_download: no trace is set up");
    if (first_row < 0 || nrows < 0 || first_row + nrows > t.rows) return fail(NSK_E_INVALID, "nsk_trace_download: rows beyond those recorded");
    if (nrows > 0 && !out) return fail(NSK_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    const size_t per_row = (size_t)t.chains * t.row_bytes, vb = (size_t)g->c.vbytes;
    const int64_t step = std::max<int64_t>(1, (int64_t)(((size_t)256 << 20) / std::max<size_t>(per_row, 1)));   // staging of 256 MB at most
    std::vector<uint8_t> host((size_t)std::min(step, std::max<int64_t>(nrows, 1)) * per_row + 8);
    for (int64_t r0 = 0; r0 < nrows; r0 += step) {
        const int64_t n = std::min(step, nrows - r0);
        if (per_row) HIPCHECK(hipMemcpy(host.data(), (const char *)t.buf + (size_t)(first_row + r0) * per_row, (size_t)n * per_row, hipMemcpyDeviceToHost));
        const size_t off = (size_t)r0 * (size_t)t.chains * (size_t)t.ncols;
        if (vb == 1) trace_unpack<int8_t>(t, host.data(), n, (int8_t *)out + off);
        else trace_unpack<int32_t>(t, host.data(), n, (int32_t *)out + off);
    }
    if (sweep_index) for (int64_t i = 0; i < nrows; i++) sweep_index[i] = t.sweep_index[(size_t)(first_row + i)];
    return NSK_OK;
}

}  // extern "C"

// One row behind whatever the stream holds: every chain's traced values as they are then (called by nsk_gibbs_sweeps
// where a row is due; the caller has checked the capacity before it enqueued a sweep)
int nsk_trace_record(nsk_graph *g) {
    NskTrace &t = g->trace;
    if (t.rows >= t.capacity) return fail(NSK_E_RANGE, "the sample trace is full");
    char *row = (char *)t.buf + (size_t)t.rows * (size_t)t.chains * t.row_bytes;
    const unsigned R = (unsigned)t.chains;
    const long long stride = (long long)g->chain_stride, ndev = t.ndev;
    const bool bytes = g->c.vbytes == 1;
    const auto blocks = [](long long items, long long per_block) { return (unsigned)std::max<long long>(1, std::min<long long>(2048, (items + per_block - 1) / per_block)); };
    if (ndev > 0 && t.packed) {
        const long long nwords = (long long)(t.row_bytes / 8);
        if (!t.cols && bytes)
            k_trace_record_dense<<<dim3(blocks(nwords * 4, NSK_BLOCK), R), dim3(NSK_BLOCK), 0, g->stream>>>((const signed char *)g->val, stride, ndev, (unsigned short *)row, nwords);
        else if (bytes)
            k_trace_record_bits<int8_t><<<dim3(blocks(nwords, NSK_BLOCK / 64), R), dim3(NSK_BLOCK), 0, g->stream>>>((const int8_t *)g->val, stride, t.cols, ndev, (unsigned long long *)row, nwords);
        else
            k_trace_record_bits<int32_t><<<dim3(blocks(nwords, NSK_BLOCK / 64), R), dim3(NSK_BLOCK), 0, g->stream>>>((const int32_t *)g->val, stride, t.cols, ndev, (unsigned long long *)row, nwords);
    } else if (ndev > 0) {
        if (bytes) k_trace_record_plain<int8_t><<<dim3(blocks(ndev, NSK_BLOCK), R), dim3(NSK_BLOCK), 0, g->stream>>>((const int8_t *)g->val, stride, t.cols, ndev, (int8_t *)row);
        else k_trace_record_plain<int32_t><<<dim3(blocks(ndev, NSK_BLOCK), R), dim3(NSK_BLOCK), 0, g->stream>>>((const int32_t *)g->val, stride, t.cols, ndev, (int32_t *)row);
    }
    HIPCHECK(hipGetLastError());
    if (t.lp) {     // the lp column: the state just recorded, every chain (a tally kept in the value bytes leaves bit 0 the value)
        int rc = nsk_energy_enqueue(g, g->val, t.chains, g->packed_sweeps > 0, t.lp + (size_t)t.rows * (size_t)t.chains);
        if (rc) return rc;
    }
    if (t.ws) {     // the stats column: likewise, the weights of its selection
        const size_t row = (size_t)t.chains * (size_t)t.ws_plan.ncols;
        int rc = nsk_wstats_enqueue(g, t.ws_plan, g->val, t.chains, g->packed_sweeps > 0, t.ws_scaled, t.ws + (size_t)t.rows * row, t.ws_plan.ncols);
        if (rc) return rc;
    }
    if (t.cond) {   // the accumulators: likewise, the conditionals of their selection added to the sums
        int rc = nsk_cond_accumulate(g, t.cond_sel, g->val, t.chains, g->packed_sweeps > 0, t.cond);
        if (rc) return rc;
        t.cond_rows++;
    }
    t.sweep_index.push_back((int64_t)g->sweep);
    t.rows++;
    return NSK_OK;
}
