// nsk_cond.hip -- per-variable conditionals (nsk_kernels_cond.h): the entry points (nsk_conditionals, the accumulators of
// a sample trace), the selection (caller's order <-> device columns), the lazily uploaded arrays of the list walk and its
// launch on the handle's stream; the sample trace calls nsk_cond_accumulate behind every record launch when its
// accumulators are on.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "nsk_internal.h"
#include "nsk_kernels_cond.h"

using namespace nsk;

// The arrays potential() reads, each where the handle lacks it: the slot index (p_slot, slot_off, fidx) and the records
// it shares with the log-potential (nsk_records_ensure).  Not gstream / gs_off / f_feat, and generic_uploaded stays
// nsk_ensure_generic's: it uploads what is still missing when it runs later, and this finds everything in place when
// it ran before.  Every factor of a positioned variable's list was validated at nsk_graph_create.
int cond_ensure(nsk_graph *g, const char *what) {
    Compiled &c = g->c;
    HIPCHECK(hipSetDevice(g->device));
    if (int rc = nsk_records_ensure(g, c.literal_heads, what)) return rc;
    if (g->p_slot && g->slot_off && g->fidx) return NSK_OK;
    int32_t *p_slot = nullptr, *slot_off = nullptr, *fidx = nullptr;
    NskRollback rb(g->mem, nsk_free_raw);
    int rc = NSK_OK;
    if (!g->p_slot) rc = dev_upload(g, &p_slot, c.p_slot);
    if (!rc && !g->slot_off) rc = dev_upload(g, &slot_off, c.slot_off);
    if (!rc && !g->fidx) rc = dev_upload(g, &fidx, c.fidx);
    if (!rc && hipStreamSynchronize(g->stream) != hipSuccess) rc = fail(NSK_E_DEVICE, "hipStreamSynchronize failed");
    if (rc) {
        if (rc != NSK_E_NOMEM) return rc;
        const double mb = ((double)c.p_slot.size() * 4 + (double)c.slot_off.size() * 4 + (double)c.fidx.size() * 4) / 1048576.0;
        return fail(NSK_E_NOMEM, std::string(what) + ": the factor lists of the variables (" + std::to_string((long long)mb) +
                                 " MB) do not fit on the device");
    }
    rb.commit();
    if (p_slot) g->p_slot = p_slot;
    if (slot_off) g->slot_off = slot_off;
    if (fidx) g->fidx = fidx;
    return NSK_OK;
}

// vids (NULL: all nvar variables) -> the selection; the ids have been checked
static int cond_sel_build(const nsk_graph *g, const int64_t *vids, int64_t nvids, NskCondSel &s, const char *what) {
    const Compiled &c = g->c;
    const int64_t n = vids ? nvids : c.nvar;
    s.off.assign((size_t)n + 1, 0);
    s.col.assign((size_t)n, -1);
    for (int64_t j = 0; j < n; j++) {
        const int64_t v = vids ? vids[j] : j;
        s.off[(size_t)j + 1] = s.off[(size_t)j] + c.v_card[(size_t)v];
        if (c.iid[(size_t)v] < c.npos) s.sel.push_back(c.iid[(size_t)v]);      // (a variable this handle does not sample has no position)
    }
    std::sort(s.sel.begin(), s.sel.end());
    s.sel.erase(std::unique(s.sel.begin(), s.sel.end()), s.sel.end());
    s.doff.assign(s.sel.size() + 1, 0);
    for (size_t i = 0; i < s.sel.size(); i++) s.doff[i + 1] = s.doff[i] + NSK_INFO_CARD(c.p_info[(size_t)s.sel[i]]);
    for (int64_t j = 0; j < n; j++) {
        const int64_t v = vids ? vids[j] : j;
        if (c.iid[(size_t)v] >= c.npos) continue;
        const int64_t i = std::lower_bound(s.sel.begin(), s.sel.end(), c.iid[(size_t)v]) - s.sel.begin();
        if (s.doff[(size_t)i + 1] - s.doff[(size_t)i] != c.v_card[(size_t)v])       // (the kernel stores as many doubles as the layout says)
            return fail(NSK_E_INVALID, std::string(what) + ": the compiled layout and the variable records disagree on a cardinality");
        s.col[(size_t)j] = i;
    }
    return NSK_OK;
}

static int cond_sel_upload(nsk_graph *g, NskCondSel &s) {
    int rc = dev_upload(g, &s.d_sel, s.sel);
    if (!rc) rc = dev_upload(g, &s.d_off, s.doff);
    return rc;
}

void nsk_cond_sel_free(nsk_graph *g, NskCondSel &s) {
    dev_free(g, s.d_sel);
    dev_free(g, s.d_off);
    s = NskCondSel();
}

// chain-major device output (nchains x dtotal) -> the caller's layout (nchains x total); NaN where there is no position
static void cond_scatter(const NskCondSel &s, const double *dev, int64_t nchains, double *out) {
    const int64_t total = s.total(), dtotal = s.dtotal();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    nsk::parallel_for(s.ncols(), [&](int64_t b0, int64_t b1, int) {
        for (int64_t r = 0; r < nchains; r++)
            for (int64_t j = b0; j < b1; j++) {
                double *o = out + r * total + s.off[(size_t)j];
                const int64_t n = s.off[(size_t)j + 1] - s.off[(size_t)j], i = s.col[(size_t)j];
                if (i < 0) { for (int64_t k = 0; k < n; k++) o[k] = nan; continue; }
                const double *d = dev + r * dtotal + s.doff[(size_t)i];
                for (int64_t k = 0; k < n; k++) o[k] = d[k];
            }
    });
}

template <int MODE>
static int cond_launch(nsk_graph *g, const NskCondSel &s, const void *val, int nchains, bool packed_bytes, double *out) {
    if (s.ndev() == 0) return NSK_OK;
    CondArgs a;
    a.p_info = g->p_info; a.p_slot = g->p_slot; a.slot_off = g->slot_off; a.fidx = g->fidx;
    a.f_rec = (const uint4 *)g->f_rec; a.m_rec = (const int2 *)g->m_rec;
    a.v_card = g->v_card; a.iid_of_vid = g->iid_of_vid;
    a.w = g->w; a.logtab = g->logtab;
    a.sel = s.d_sel; a.off = s.d_off;
    a.nsel = (long long)s.ndev(); a.total = (long long)s.dtotal(); a.chain_stride = (long long)g->chain_stride;
    a.head_by_vid = (g->c.flags & NSK_FLAG_HEAD_BY_VID) ? 1 : 0;
    const unsigned nb = (unsigned)std::max<long long>(1, std::min<long long>(2048, (a.nsel + NSK_BLOCK - 1) / NSK_BLOCK));
    const dim3 grid(nb, (unsigned)nchains), block(NSK_BLOCK);
    if (g->c.vbytes == 4) k_cond<int32_t, MODE><<<grid, block, 0, g->stream>>>(a, (const int32_t *)val, out);
    else if (packed_bytes) k_cond<PackedByte, MODE><<<grid, block, 0, g->stream>>>(a, (const PackedByte *)val, out);
    else k_cond<int8_t, MODE><<<grid, block, 0, g->stream>>>(a, (const int8_t *)val, out);
    HIPCHECK(hipGetLastError());
    return NSK_OK;
}

// One launch behind whatever the stream holds; not counted by the profiling bracket (sweep kernels only)
int nsk_cond_accumulate(nsk_graph *g, const NskCondSel &sel, const void *val, int nchains, bool packed_bytes, double *sums) {
    return cond_launch<COND_ACCUMULATE>(g, sel, val, nchains, packed_bytes, sums);
}

// the checks nsk_conditionals and nsk_trace_conditionals share on a list of variable ids
static int cond_check_vids(const nsk_graph *g, const int64_t *vids, int64_t nvids, const char *what) {
    if (vids ? nvids < 0 : nvids != 0)
        return fail(NSK_E_INVALID, std::string(what) + ": a list of variable ids with its length, or NULL with 0 for all variables");
    for (int64_t j = 0; vids && j < nvids; j++)
        if (vids[j] < 0 || vids[j] >= g->c.nvar) return fail(NSK_E_INDEX, std::string(what) + ": variable id out of range");
    return NSK_OK;
}

extern "C" {

int nsk_conditionals(nsk_graph *g, int which, int64_t first_chain, int64_t nchains, const int64_t *vids, int64_t nvids,
                     int what, double *out) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    int rc = chain_select(g, which, first_chain, nchains, "nsk_conditionals");
    if (rc) return rc;
    if (what != 0 && what != 1) return fail(NSK_E_INVALID, "nsk_conditionals: what must be 0 (potentials) or 1 (probabilities)");
    if ((rc = energy_whole_graph(g, "nsk_conditionals"))) return rc;
    if ((rc = cond_check_vids(g, vids, nvids, "nsk_conditionals"))) return rc;
    NskCondSel s;
    if ((rc = cond_sel_build(g, vids, nvids, s, "nsk_conditionals"))) return rc;
    if (s.total() == 0) return NSK_OK;
    if (!out) return fail(NSK_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(g->device));
    std::vector<double> host((size_t)nchains * (size_t)s.dtotal());
    if (s.ndev() > 0) {
        if ((rc = cond_ensure(g, "nsk_conditionals"))) return rc;
        // the selection and the values cross PCIe through buffers that live for this call only
        double *dev = nullptr;
        {
            NskRollback rb(g->mem, nsk_free_raw);
            rc = cond_sel_upload(g, s);
            if (!rc) rc = dev_alloc(g, &dev, host.size());
            if (rc == NSK_E_NOMEM)
                return fail(NSK_E_NOMEM, "nsk_conditionals: the selection and chains x total doubles (" +
                                         std::to_string((long long)((host.size() * 8 + (size_t)s.ndev() * 12) / 1048576)) + " MB) do not fit on the device");
            if (rc) return rc;
            rb.commit();
        }
        const char *val = chain_val(g, which, first_chain);
        rc = what == 0 ? cond_launch<COND_POTENTIALS>(g, s, val, (int)nchains, g->packed_sweeps > 0, dev)
                       : cond_launch<COND_PROBABILITIES>(g, s, val, (int)nchains, g->packed_sweeps > 0, dev);
        hipError_t e = hipSuccess;
        if (!rc) e = hipMemcpyAsync(host.data(), dev, host.size() * sizeof(double), hipMemcpyDeviceToHost, g->stream);
        const hipError_t e2 = hipStreamSynchronize(g->stream);      // (also: the uploads read the selection's vectors)
        dev_free(g, dev);
        dev_free(g, s.d_sel); dev_free(g, s.d_off);
        if (rc) return rc;
        HIPCHECK(e);
        HIPCHECK(e2);
    }
    cond_scatter(s, host.data(), nchains, out);
    return NSK_OK;
}

int nsk_trace_conditionals(nsk_graph *g, const int64_t *vids, int64_t nvids) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    NskTrace &t = g->trace;
    if (t.capacity == 0) return fail(NSK_E_INVALID, "nsk_trace_conditionals: no trace is set up");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));          // (accumulate launches into the buffer that goes)
    if (nvids < 0) {
        dev_free(g, t.cond);
        t.cond = nullptr; t.cond_rows = 0;
        nsk_cond_sel_free(g, t.cond_sel);
        return NSK_OK;
    }
    int rc = cond_check_vids(g, vids, nvids, "nsk_trace_conditionals");
    if (rc) return rc;
    NskCondSel s;
    if ((rc = cond_sel_build(g, vids, nvids, s, "nsk_trace_conditionals"))) return rc;
    if (s.ndev() > 0 && (rc = cond_ensure(g, "nsk_trace_conditionals"))) return rc;
    // the arguments hold: the accumulators these replace go now, before the new ones are asked for
    dev_free(g, t.cond);
    t.cond = nullptr; t.cond_rows = 0;
    nsk_cond_sel_free(g, t.cond_sel);
    const size_t n = (size_t)t.chains * (size_t)s.dtotal();
    double *sums = nullptr;
    {
        NskRollback rb(g->mem, nsk_free_raw);
        rc = cond_sel_upload(g, s);
        if (!rc) rc = dev_alloc(g, &sums, n);
        if (rc == NSK_E_NOMEM)
            return fail(NSK_E_NOMEM, "nsk_trace_conditionals: the selection and chains x total doubles (" +
                                     std::to_string((long long)((n * 8 + (size_t)s.ndev() * 12) / 1048576)) + " MB) do not fit on the device");
        if (rc) return rc;
        if (hipMemsetAsync(sums, 0, (n ? n : 1) * sizeof(double), g->stream) != hipSuccess || hipStreamSynchronize(g->stream) != hipSuccess)
            return fail(NSK_E_DEVICE, "nsk_trace_conditionals: clearing the accumulators failed");      // (the uploads read s's vectors)
        rb.commit();
    }
    t.cond_sel = std::move(s);
    t.cond = sums;
    return NSK_OK;
}

int nsk_trace_download_conditionals(nsk_graph *g, double *sums, int64_t *rows) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    const NskTrace &t = g->trace;
    if (t.capacity == 0) return fail(NSK_E_INVALID, "nsk_trace_download_conditionals: no trace is set up");
    if (!t.cond) return fail(NSK_E_INVALID, "nsk_trace_download_conditionals: the trace keeps no accumulators (nsk_trace_conditionals)");
    const NskCondSel &s = t.cond_sel;
    if (s.total() > 0 && !sums) return fail(NSK_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    std::vector<double> host((size_t)t.chains * (size_t)s.dtotal());
    if (!host.empty()) HIPCHECK(hipMemcpy(host.data(), t.cond, host.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (s.total() > 0) cond_scatter(s, host.data(), t.chains, sums);
    if (rows) *rows = t.cond_rows;
    return NSK_OK;
}

}  // extern "C"
