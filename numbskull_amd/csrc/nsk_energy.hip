// nsk_energy.hip -- the log-potential (nsk_internal.h NskEnergy): the entry points (nsk_log_potential, nsk_factor_values, the
// sample trace's lp column), the lazily uploaded arrays of the factor walk and its launches (nsk_kernels_energy.h) on the
// handle's stream; the sample trace calls nsk_energy_enqueue behind every record launch when its lp column is on.
#include <hip/hip_runtime.h>

#include "nsk_internal.h"
#include "nsk_kernels_energy.h"

using namespace nsk;

EnergyArgs energy_args(const nsk_graph *g) {
    EnergyArgs a;
    a.f_rec = (const uint4 *)g->f_rec; a.m_rec = (const int2 *)g->m_rec;
    a.v_card = g->v_card; a.iid_of_vid = g->iid_of_vid;
    a.w = g->w; a.logtab = g->logtab;
    a.nfactor = (long long)g->c.nfactor;
    a.chain_stride = (long long)g->chain_stride;
    a.head_by_vid = (g->c.flags & NSK_FLAG_HEAD_BY_VID) ? 1 : 0;
    return a;
}

// out[r] = log-potential of chain r, r < nchains, of the chains that start at `val` (device pointers; nchains at most
// the chains the partials were sized for, energy_ensure).  packed_bytes: the value is bit 0 of a value byte.
// Two launches behind whatever the stream holds; not counted by the profiling bracket (sweep kernels only).
int nsk_energy_enqueue(nsk_graph *g, const void *val, int nchains, bool packed_bytes, double *out) {
    const NskEnergy &en = g->energy;
    if (!en.ready || nchains < 1 || nchains > en.chains) return fail(NSK_E_INVALID, "log-potential: the factor records are not set up");
    const EnergyArgs a = energy_args(g);
    const unsigned int nb = nsk_energy_blocks(a.nfactor);
    const dim3 grid(nb, (unsigned)nchains), block(NSK_BLOCK);
    if (g->c.vbytes == 4) k_energy_partial<int32_t><<<grid, block, 0, g->stream>>>(a, (const int32_t *)val, en.partial);
    else if (packed_bytes) k_energy_partial<PackedByte><<<grid, block, 0, g->stream>>>(a, (const PackedByte *)val, en.partial);
    else k_energy_partial<int8_t><<<grid, block, 0, g->stream>>>(a, (const int8_t *)val, en.partial);
    k_energy_reduce<<<dim3((unsigned)nchains), block, 0, g->stream>>>(en.partial, (int)nb, out);
    HIPCHECK(hipGetLastError());
    return NSK_OK;
}

// out[f] = eval_factor(f) on the state at `val` (one chain), f in the caller's factor order
int nsk_factor_values_enqueue(nsk_graph *g, const void *val, double *out) {
    if (!g->energy.ready) return fail(NSK_E_INVALID, "factor values: the factor records are not set up");
    const EnergyArgs a = energy_args(g);
    const dim3 grid(nsk_energy_blocks(a.nfactor)), block(NSK_BLOCK);
    if (g->c.vbytes == 4) k_factor_values<int32_t><<<grid, block, 0, g->stream>>>(a, (const int32_t *)val, out);
    else k_factor_values<int8_t><<<grid, block, 0, g->stream>>>(a, (const int8_t *)val, out);
    HIPCHECK(hipGetLastError());
    return NSK_OK;
}

// ---- log-potential (nsk_internal.h NskEnergy, nsk_kernels_energy.h) ---------------------------------------------------
// The handles the sample trace serves: a shard's sum is not the graph's, and ghosts are stale between exchanges
int energy_whole_graph(const nsk_graph *g, const char *what) {
    const Compiled &c = g->c;
    if ((c.flags & NSK_FLAG_PARTITION) || c.own_begin != 0 || c.own_end != c.nvar)
        return fail(NSK_E_INVALID, std::string(what) + ": the handle must own the whole graph (no own_range / NSK_FLAG_PARTITION)");
    if (g->gather.world > 0 || g->p2p.world > 0 || g->gather.comm)
        return fail(NSK_E_INVALID, std::string(what) + ": the handle exchanges a boundary (exchange, RCCL or peer-to-peer set up)");
    return NSK_OK;
}

// nsk_graph_create validates the factors a sampled variable reaches (nsk_compile_colour.cpp validate_reachable); the walk
// evaluates EVERY factor, so the others are held to the same rules here, on the compiled records.  Returns the lowest
// factor that breaks one (-1: none) and whether some factor reads its head at the literal edge index.
static int64_t energy_check_factors(const nsk_graph *g, bool *literal_out) {
    const Compiled &c = g->c;
    const int64_t nedge = c.nedge, nid = c.nid, nw = c.nweight, nvar = c.nvar;
    const bool head_by_vid = (c.flags & NSK_FLAG_HEAD_BY_VID) != 0;
    const int nt = nsk::compile_threads();
    std::vector<int64_t> first((size_t)nt, -1);
    std::vector<int> literal((size_t)nt, 0);
    nsk::parallel_for(c.nfactor, [&](int64_t b0, int64_t b1, int t) {
        auto members_ok = [&](int64_t lo, int64_t hi) {
            for (int64_t l = lo; l < hi; l++) if (c.m_rec[2 * (size_t)l] < 0 || c.m_rec[2 * (size_t)l] >= nid) return false;
            return true;
        };
        for (int64_t f = b0; f < b1; f++) {
            const uint32_t head = c.f_rec[4 * (size_t)f];
            const int fn = (int)(head & 0xffu) - 1;
            const int64_t ar = (int64_t)(head >> 8), s = (int32_t)c.f_rec[4 * (size_t)f + 1], wz = (int32_t)c.f_rec[4 * (size_t)f + 2];
            bool ok = known_function(fn) && wz >= 0 && wz < nw;
            if (ok && fn != -1) {
                int64_t need = 0;       // member positions the function reads regardless of arity
                bool arity1 = false;
                switch (fn) {
                case 0: case 7: case 8: case 9: case 13: case 16: case 17: arity1 = true; break;
                case 3: case 18: case 19: case 20: case 30: need = 1; break;
                case 21: case 22: case 25: case 26: need = 2; break;
                case 23: case 24: need = 3; break;
                default: break;
                }
                const int64_t e = s + ar;
                ok = s >= 0 && e <= nedge && s + need <= nedge && !(arity1 && ar < 1) && members_ok(s, std::max(e, s + need));
                if (ok && fn == 30) {   // UFO: the first member's value indexes the member list (values are kept regular then)
                    const int64_t reach = s + c.v_card_i[(size_t)c.m_rec[2 * (size_t)s]] - 2;
                    ok = c.has_ufo && reach < nedge && members_ok(s, reach + 1);
                }
                if (ok && (fn == 13 || fn == 16 || fn == 17) && !head_by_vid) { literal[(size_t)t] = 1; ok = e - 1 < nvar; }
                if (ok && fn == 8) ok = ar < (int64_t)c.logtab.size();
            }
            if (!ok) { first[(size_t)t] = f; return; }
        }
    });
    *literal_out = false;
    for (int x : literal) if (x) *literal_out = true;
    int64_t bad = -1;
    for (int64_t x : first) if (x >= 0 && (bad < 0 || x < bad)) bad = x;
    return bad;
}

// The factor and member records, the cardinalities and -- `literal`: a factor the caller evaluates reads its head at the
// literal edge index -- the internal ids, each where the handle lacks it (nsk_ensure_generic uploads the same arrays and
// takes these when it runs later); all of them or none
int nsk_records_ensure(nsk_graph *g, bool literal, const char *what) {
    Compiled &c = g->c;
    uint32_t *f_rec = nullptr;
    int32_t *m_rec = nullptr, *v_card = nullptr, *iid = nullptr;
    NskRollback rb(g->mem, nsk_free_raw);
    int rc = NSK_OK;
    if (!g->f_rec) rc = dev_upload(g, &f_rec, c.f_rec);
    if (!rc && !g->m_rec) rc = dev_upload(g, &m_rec, c.m_rec);
    if (!rc && !g->v_card) rc = dev_upload(g, &v_card, c.v_card_i);
    if (!rc && literal && !g->iid_of_vid && !g->xfer_iid) rc = dev_upload(g, &iid, c.iid);
    if (!rc && hipStreamSynchronize(g->stream) != hipSuccess) rc = fail(NSK_E_DEVICE, "hipStreamSynchronize failed");
    if (rc) {
        if (rc != NSK_E_NOMEM) return rc;
        const double mb = ((double)c.f_rec.size() * 4 + (double)c.m_rec.size() * 4 + (double)c.v_card_i.size() * 4) / 1048576.0;
        return fail(NSK_E_NOMEM, std::string(what) + ": the factor and member records the evaluation reads (" +
                                 std::to_string((long long)mb) + " MB) do not fit on the device");
    }
    rb.commit();
    if (f_rec) g->f_rec = f_rec;
    if (m_rec) g->m_rec = m_rec;
    if (v_card) g->v_card = v_card;
    if (literal && !g->iid_of_vid) g->iid_of_vid = iid ? iid : g->xfer_iid;     // (the state transfers hold the same table)
    return NSK_OK;
}

// The arrays of the walk and the partial sums for `chains` chains, at the first use (and when more chains ask)
int energy_ensure(nsk_graph *g, int chains, const char *what) {
    NskEnergy &en = g->energy;
    Compiled &c = g->c;
    HIPCHECK(hipSetDevice(g->device));
    if (!en.ready) {
        bool literal = false;
        const int64_t bad = energy_check_factors(g, &literal);
        if (bad >= 0)
            return fail(NSK_E_INVALID, std::string(what) + ": factor " + std::to_string(bad) + ", which no sampled variable reaches, cannot be "
                                       "evaluated (unknown function, or a weight, member or head index outside the arrays)");
        if (int rc = nsk_records_ensure(g, literal, what)) return rc;
        en.ready = true;
    }
    if (chains > en.chains) {
        const size_t nb = (size_t)nsk_energy_blocks((long long)c.nfactor);
        double *partial = nullptr, *result = nullptr;
        NskRollback rb(g->mem, nsk_free_raw);
        int rc = dev_alloc(g, &partial, (size_t)chains * nb);
        if (!rc) rc = dev_alloc(g, &result, (size_t)chains);
        if (rc) return rc;
        HIPCHECK(hipStreamSynchronize(g->stream));      // (launches that write the buffers that go)
        rb.commit();
        dev_free(g, en.partial); dev_free(g, en.result);
        en.partial = partial; en.result = result; en.chains = chains;
    }
    return NSK_OK;
}

extern "C" {

int nsk_log_potential(nsk_graph *g, int which, int64_t first_chain, int64_t nchains, double *out) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!out) return fail(NSK_E_INVALID, "null argument");
    int rc = chain_select(g, which, first_chain, nchains, "nsk_log_potential");
    if (!rc) rc = energy_whole_graph(g, "nsk_log_potential");
    if (rc) return rc;
    if ((rc = energy_ensure(g, (int)nchains, "nsk_log_potential"))) return rc;
    if ((rc = nsk_energy_enqueue(g, chain_val(g, which, first_chain), (int)nchains, g->packed_sweeps > 0, g->energy.result))) return rc;
    HIPCHECK(hipMemcpyAsync(out, g->energy.result, (size_t)nchains * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    HIPCHECK(hipStreamSynchronize(g->stream));
    return NSK_OK;
}

int nsk_factor_values(nsk_graph *g, int which, int64_t chain, double *out) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    int rc = chain_select(g, which, chain, 1, "nsk_factor_values", true);
    if (!rc) rc = energy_whole_graph(g, "nsk_factor_values");
    if (rc) return rc;
    if (g->c.nfactor == 0) return NSK_OK;
    if (!out) return fail(NSK_E_INVALID, "null argument");
    if ((rc = energy_ensure(g, 0, "nsk_factor_values"))) return rc;
    // the values cross PCIe from a buffer that lives for this call only (8 bytes a factor)
    double *dev = nullptr;
    const size_t n = (size_t)g->c.nfactor;
    if ((rc = dev_alloc(g, &dev, n))) return fail(NSK_E_NOMEM, "nsk_factor_values: one double per factor does not fit on the device");
    rc = nsk_factor_values_enqueue(g, chain_val(g, which, chain), dev);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(out, dev, n * sizeof(double), hipMemcpyDeviceToHost, g->stream);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(g->stream);
    dev_free(g, dev);
    if (rc) return rc;
    HIPCHECK(e);
    return NSK_OK;
}

int nsk_trace_log_potential(nsk_graph *g, int on) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    NskTrace &t = g->trace;
    if (t.capacity == 0) return fail(NSK_E_INVALID, "nsk_trace_log_potential: no trace is set up");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    if (!on) {
        dev_free(g, t.lp);
        t.lp = nullptr;
        return NSK_OK;
    }
    if (t.lp) return NSK_OK;
    int rc = energy_ensure(g, t.chains, "nsk_trace_log_potential");
    if (rc) return rc;
    double *lp = nullptr;
    if ((rc = dev_alloc(g, &lp, (size_t)t.capacity * (size_t)t.chains))) return rc;
    HIPCHECK(hipMemsetAsync(lp, 0, (size_t)t.capacity * (size_t)t.chains * sizeof(double), g->stream));     // (rows recorded while it was off read 0)
    t.lp = lp;
    return NSK_OK;
}

int nsk_trace_download_log_potential(nsk_graph *g, int64_t first_row, int64_t nrows, double *out) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    const NskTrace &t = g->trace;
    if (t.capacity == 0) return fail(NSK_E_INVALID, "nsk_trace_download_log_potential: no trace is set up");
    if (!t.lp) return fail(NSK_E_INVALID, "nsk_trace_download_log_potential: the trace keeps no lp column (nsk_trace_log_potential)");
    if (first_row < 0 || nrows < 0 || first_row + nrows > t.rows) return fail(NSK_E_INVALID, "nsk_trace_download_log_potential: rows beyond those recorded");
    if (nrows > 0 && !out) return fail(NSK_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(g->device));
    HIPCHECK(hipStreamSynchronize(g->stream));
    if (nrows > 0)
        HIPCHECK(hipMemcpy(out, t.lp + (size_t)first_row * (size_t)t.chains, (size_t)nrows * (size_t)t.chains * sizeof(double), hipMemcpyDeviceToHost));
    return NSK_OK;
}

}  // extern "C"
