// nsk_plgrad.hip -- the pseudo-likelihood gradient and maximum pseudo-likelihood learning (nsk_kernels_plgrad.h): the entry
// points nsk_pl_gradient and nsk_mple_steps.  They read the arrays the conditionals read (nsk_cond.hip cond_ensure); the
// selection (a set of variables, sorted by position), the int64 sums and the per-step outputs live for the call only.
// nsk_mple_steps enqueues (zero the sums, k_plgrad, k_mple_update) per step on the handle's stream without a host wait
// and synchronises once.
#include <hip/hip_runtime.h>

#include <cmath>

#include "nsk_internal.h"
#include "nsk_kernels_plgrad.h"

using namespace nsk;

namespace {

// what both entry points check of their arguments, in nsk_conditionals' order; the selection: the positions of the
// selected variables that have one, ascending
int plgrad_selection(const nsk_graph *g, int which, int64_t first_chain, int64_t nchains, const int64_t *vids, int64_t nvids,
                     std::vector<int32_t> &sel, const std::string &what) {
    int rc = chain_select(g, which, first_chain, nchains, what);
    if (!rc) rc = energy_whole_graph(g, what.c_str());
    if (rc) return rc;
    if (vids ? nvids < 0 : nvids != 0)
        return fail(NSK_E_INVALID, what + ": a list of variable ids with its length, or NULL with 0 for all variables");
    const Compiled &c = g->c;
    for (int64_t j = 0; vids && j < nvids; j++)
        if (vids[j] < 0 || vids[j] >= c.nvar) return fail(NSK_E_INDEX, what + ": variable id out of range");
    const int64_t n = vids ? nvids : c.nvar;
    if (vids) {         // the selection is a set
        std::vector<uint32_t> seen((size_t)(c.nvar + 31) / 32, 0u);
        for (int64_t j = 0; j < n; j++) {
            const int64_t v = vids[j];
            if ((seen[(size_t)v >> 5] >> (v & 31)) & 1u) return fail(NSK_E_INVALID, what + ": variable " + std::to_string((long long)v) + " is selected twice");
            seen[(size_t)v >> 5] |= 1u << (v & 31);
        }
    }
    sel.clear();
    for (int64_t j = 0; j < n; j++) {
        const int64_t v = vids ? vids[j] : j;
        if (c.iid[(size_t)v] < c.npos) sel.push_back(c.iid[(size_t)v]);      // (a variable this handle does not sample has no position)
    }
    std::sort(sel.begin(), sel.end());
    return NSK_OK;
}

// The range of the int64 sums, from the graph and the selection alone: B_w = the sum over the selected variables' list
// entries of m * vmax(f), m = 2 for an entry of a dataType-0 list (visited with every k; sum_k |c_k| <= 2) and 1 for a
// dataType-1 one, vmax the per-function bound of the learning accumulators' format (nsk_compile_tiles.cpp
// choose_gradient_format).  Every term is below m * vmax * 2^32 in magnitude, so B_w * nchains < 2^30 keeps a weight's
// sum over all chains below 2^62.
double plgrad_vmax(uint32_t head) {
    const int fn = NSK_FHEAD_FUNC(head);
    const double ar = (double)std::max(NSK_FHEAD_ARITY(head), 1);
    return fn == F_LINEAR ? ar : fn == F_RATIO ? std::log(ar + 1.0) : fn == F_UFO ? 1e6 : 1.0;
}

template <typename F>
void plgrad_entries(const Compiled &c, const std::vector<int32_t> &sel, int64_t i0, int64_t i1, F &&visit) {
    for (int64_t i = i0; i < i1; i++) {
        const size_t p = (size_t)sel[(size_t)i];
        const uint32_t info = c.p_info[p];
        const bool dt1 = NSK_INFO_DT1(info) != 0;
        const int64_t nslots = dt1 ? NSK_INFO_CARD(info) : 1;
        const int64_t b = c.slot_off[(size_t)c.p_slot[p]], e = c.slot_off[(size_t)(c.p_slot[p] + nslots)];
        for (int64_t j = b; j < e; j++) {
            const uint32_t *rec = &c.f_rec[4 * (size_t)c.fidx[(size_t)j]];
            visit(rec[2], (dt1 ? 1.0 : 2.0) * plgrad_vmax(rec[0]));
        }
    }
}

int plgrad_range(const nsk_graph *g, const std::vector<int32_t> &sel, int64_t nchains, const std::string &what) {
    const Compiled &c = g->c;
    const double limit = 1073741824.0 / (double)nchains;
    // every B_w is at most the sum over ALL entries: most calls are decided by that one number (with a factor of two to
    // spare, so that the order of the threads' partial sums cannot matter)
    std::vector<double> part((size_t)nsk::compile_threads(), 0.0);
    nsk::parallel_for((int64_t)sel.size(), [&](int64_t b0, int64_t b1, int t) {
        double s = 0.0;
        plgrad_entries(c, sel, b0, b1, [&](uint32_t, double x) { s += x; });
        part[(size_t)t] = s;
    });
    double total = 0.0;
    for (double x : part) total += x;
    if (total < 0.5 * limit) return NSK_OK;
    std::vector<double> B((size_t)c.nweight, 0.0);
    plgrad_entries(c, sel, 0, (int64_t)sel.size(), [&](uint32_t slot, double x) { B[slot] += x; });
    for (int64_t s = 0; s < c.nweight; s++)
        if (B[(size_t)s] >= limit) {
            const int64_t wid = c.wuser.empty() ? s : (int64_t)c.wuser[(size_t)s];
            return fail(NSK_E_RANGE, what + ": the gradient sum of weight " + std::to_string((long long)wid) + " over " +
                                     std::to_string((long long)nchains) + " chain(s) may reach 2^62 (its bound B = " + std::to_string(B[(size_t)s]) +
                                     "; B x chains must stay below 2^30): select fewer variables or chains");
        }
    return NSK_OK;
}

// the buffers of one call: the selection, and ONE array zeroed per step: nchains x nweight sums, then nchains skip counts
struct PlgradBufs {
    nsk_graph *g;
    int32_t *sel = nullptr;
    unsigned long long *acc = nullptr;
    long long *steps = nullptr;            // nsk_mple_steps: gmax[nsteps], skipped[nsteps]
    size_t nacc = 0;
    explicit PlgradBufs(nsk_graph *g_) : g(g_) {}
    ~PlgradBufs() { dev_free(g, steps); dev_free(g, acc); dev_free(g, sel); }
};

int plgrad_alloc(nsk_graph *g, PlgradBufs &b, const std::vector<int32_t> &sel, size_t nchains, size_t nsteps, const std::string &what) {
    b.nacc = nchains * (size_t)g->c.nweight + nchains;
    int rc = dev_upload(g, &b.sel, sel);
    if (!rc) rc = dev_alloc(g, &b.acc, b.nacc);
    if (!rc && nsteps) rc = dev_alloc(g, &b.steps, 2 * nsteps);
    if (rc == NSK_E_NOMEM)
        return fail(NSK_E_NOMEM, what + ": the selection (4 bytes a variable), chains x (weights + 1) int64 sums and the per-step outputs (" +
                                 std::to_string((long long)(sel.size() * 4 + b.nacc * 8 + nsteps * 16)) + " bytes) do not fit on the device");
    return rc;
}

CondArgs plgrad_args(const nsk_graph *g, const PlgradBufs &b, size_t nsel) {
    CondArgs a = {};
    a.p_info = g->p_info; a.p_slot = g->p_slot; a.slot_off = g->slot_off; a.fidx = g->fidx;
    a.f_rec = (const uint4 *)g->f_rec; a.m_rec = (const int2 *)g->m_rec;
    a.v_card = g->v_card; a.iid_of_vid = g->iid_of_vid;
    a.w = g->w; a.logtab = g->logtab;
    a.sel = b.sel;
    a.nsel = (long long)nsel; a.chain_stride = (long long)g->chain_stride;
    a.head_by_vid = (g->c.flags & NSK_FLAG_HEAD_BY_VID) ? 1 : 0;
    return a;
}

// zero the sums and the skip counts, then one k_plgrad launch; not counted by the profiling bracket (sweep kernels only)
hipError_t plgrad_enqueue(nsk_graph *g, const CondArgs &a, const PlgradBufs &b, const char *val, int nchains) {
    hipError_t e = hipMemsetAsync(b.acc, 0, b.nacc * sizeof(unsigned long long), g->stream);
    if (e != hipSuccess) return e;
    const int nw = (int)g->c.nweight;
    const dim3 grid(nsk_plgrad_blocks(a.nsel), (unsigned)nchains), block(NSK_BLOCK);
    unsigned long long *skipped = b.acc + (size_t)nchains * (size_t)nw;
    if (g->c.vbytes == 4) k_plgrad<int32_t><<<grid, block, 0, g->stream>>>(a, (const int32_t *)val, nw, b.acc, skipped);
    else k_plgrad<int8_t><<<grid, block, 0, g->stream>>>(a, (const int8_t *)val, nw, b.acc, skipped);
    return hipGetLastError();
}

}  // namespace

extern "C" {

int nsk_pl_gradient(nsk_graph *g, int which, int64_t first_chain, int64_t nchains, const int64_t *vids, int64_t nvids,
                    int64_t *grad_q, double *grad, int64_t *skipped) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    std::vector<int32_t> sel;
    int rc = plgrad_selection(g, which, first_chain, nchains, vids, nvids, sel, "nsk_pl_gradient");
    if (rc) return rc;
    const Compiled &c = g->c;
    const size_t R = (size_t)nchains, nw = (size_t)c.nweight;
    if (sel.empty()) {          // nothing selected has a position: every sum is 0
        for (size_t i = 0; i < R * nw; i++) { if (grad_q) grad_q[i] = 0; if (grad) grad[i] = 0.0; }
        for (size_t r = 0; skipped && r < R; r++) skipped[r] = 0;
        return NSK_OK;
    }
    if ((rc = plgrad_range(g, sel, nchains, "nsk_pl_gradient"))) return rc;
    HIPCHECK(hipSetDevice(g->device));
    if ((rc = cond_ensure(g, "nsk_pl_gradient"))) return rc;
    // a tally kept in bits 1-7 of the value bytes goes back to its array first, as in nsk_icm: the kernel sees plain values
    if ((rc = nsk_unpack_tally(g))) return rc;
    PlgradBufs b(g);
    if ((rc = plgrad_alloc(g, b, sel, R, 0, "nsk_pl_gradient"))) return rc;
    std::vector<long long> host(b.nacc);
    hipError_t e = plgrad_enqueue(g, plgrad_args(g, b, sel.size()), b, chain_val(g, which, first_chain), (int)nchains);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), b.acc, b.nacc * sizeof(long long), hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);      // (also: the upload read the selection's vector)
    HIPCHECK(e);
    HIPCHECK(e2);
    // slots -> the caller's weight ids, as nsk_state_download maps the weights
    const SlotMap map(c);
    for (size_t r = 0; r < R; r++) {
        for (size_t i = 0; i < nw; i++) {
            const long long q = host[r * nw + map.slot(i)];
            if (grad_q) grad_q[r * nw + i] = (int64_t)q;
            if (grad) grad[r * nw + i] = (double)q * (1.0 / NSK_GRAD_SCALE);
        }
        if (skipped) skipped[r] = (int64_t)host[R * nw + r];
    }
    return NSK_OK;
}

int nsk_mple_steps(nsk_graph *g, int which, int64_t first_chain, int64_t nchains, const int64_t *vids, int64_t nvids,
                   int64_t nsteps, double step, double decay, double reg_param, int64_t *gmax, int64_t *skipped) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    std::vector<int32_t> sel;
    int rc = plgrad_selection(g, which, first_chain, nchains, vids, nvids, sel, "nsk_mple_steps");
    if (rc) return rc;
    if ((rc = refuse(check_nsteps("nsk_mple_steps", nsteps, 65536)))) return rc;
    if ((rc = refuse(check_rates("nsk_mple_steps", step, decay, reg_param)))) return rc;
    const Compiled &c = g->c;
    const size_t R = (size_t)nchains, T = (size_t)nsteps;
    for (size_t t = 0; t < T; t++) { if (gmax) gmax[t] = 0; if (skipped) skipped[t] = 0; }
    if (sel.empty()) return NSK_OK;         // N == 0: nothing to learn from
    if ((rc = plgrad_range(g, sel, nchains, "nsk_mple_steps"))) return rc;
    HIPCHECK(hipSetDevice(g->device));
    if ((rc = cond_ensure(g, "nsk_mple_steps"))) return rc;
    if ((rc = nsk_unpack_tally(g))) return rc;
    PlgradBufs b(g);
    if ((rc = plgrad_alloc(g, b, sel, R, T, "nsk_mple_steps"))) return rc;
    const char *val = chain_val(g, which, first_chain);
    const CondArgs a = plgrad_args(g, b, sel.size());
    const int nw = (int)c.nweight;
    const double n = (double)sel.size() * (double)nchains;
    const unsigned wblocks = (unsigned)std::max<int64_t>(1, (c.nweight + NSK_BLOCK - 1) / NSK_BLOCK);
    hipError_t e = hipMemsetAsync(b.steps, 0, 2 * T * sizeof(long long), g->stream);
    double st = step;           // step_0 = step, step_{t+1} = step_t * decay: the products are formed here, in t order
    for (size_t t = 0; t < T && e == hipSuccess; t++) {
        e = plgrad_enqueue(g, a, b, val, (int)nchains);
        if (e != hipSuccess) break;
        // (w_fixed by slot: a renumbered weight is a direct one, and those are never fixed -- nsk_compile.h wmap)
        k_mple_update<<<dim3(wblocks), dim3(NSK_BLOCK), 0, g->stream>>>((const long long *)b.acc, (int)nchains, nw, g->w, g->w_fixed, n, st, reg_param,
                                                                       b.steps + t, b.acc + R * (size_t)nw, b.steps + T + t);
        e = hipGetLastError();
        g->weights_dirty = true;            // the next sweep call rebuilds what derives from the weights
        st = st * decay;
    }
    std::vector<long long> host(2 * T);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), b.steps, 2 * T * sizeof(long long), hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);
    HIPCHECK(e);
    HIPCHECK(e2);
    for (size_t t = 0; t < T; t++) { if (gmax) gmax[t] = (int64_t)host[t]; if (skipped) skipped[t] = (int64_t)host[T + t]; }
    return NSK_OK;
}

}  // extern "C"
