// nsk_temper.hip -- sweeps under a schedule of inverse temperatures (nsk_kernels_temper.h): the entry point
// nsk_tempered_sweeps.  A step scales the weight table from a copy of the base weights, runs the burn-in sweeps of
// nsk_gibbs_sweeps under it (the refresh in front of a sweep call rebuilds what is derived from the weights), scores every
// chain under the BASE weights by the factor walk of the log-potential, and folds the annealed-importance-sampling weight
// and the best state so far on the device.  Every step is enqueued on the handle's stream without a wait; the call
// restores the base weights by a copy, synchronises once and downloads what was asked for.
#include <hip/hip_runtime.h>

#include <cmath>

#include "nsk_internal.h"
#include "nsk_kernels_temper.h"

using namespace nsk;

namespace {

// the buffers of one call: entered in the ledger, gone when the call returns
struct TemperBufs {
    nsk_graph *g;
    double *base = nullptr, *lp = nullptr, *log_weight = nullptr, *best_u = nullptr;
    unsigned int *improved = nullptr;
    char *best = nullptr;
    explicit TemperBufs(nsk_graph *g_) : g(g_) {}
    ~TemperBufs() {
        dev_free(g, best); dev_free(g, improved); dev_free(g, best_u); dev_free(g, log_weight); dev_free(g, lp); dev_free(g, base);
    }
};

}  // namespace

extern "C" int nsk_tempered_sweeps(nsk_graph *g, const double *betas, int64_t nsteps, int64_t sweeps_per_step, int sample_evidence,
                                   double *log_weight, double *lp, int64_t *best_values, double *best_lp) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!betas) return fail(NSK_E_INVALID, "null argument");
    if (nsteps < 1 || nsteps > 65536) return fail(NSK_E_INVALID, "nsk_tempered_sweeps: nsteps must lie in [1, 65536]");
    if (sweeps_per_step < 1 || sweeps_per_step > INT32_MAX / nsteps)
        return fail(NSK_E_INVALID, "nsk_tempered_sweeps: sweeps_per_step must be at least 1 and nsteps x sweeps_per_step at most 2^31 - 1");
    for (int64_t t = 0; t < nsteps; t++)
        if (!(betas[t] >= 0.0) || std::isinf(betas[t]))
            return fail(NSK_E_INVALID, "nsk_tempered_sweeps: step " + std::to_string((long long)t) + " has an inverse temperature that is negative, infinite or NaN");
    if (g->scan != NSK_SCAN_CHROMATIC) return fail(NSK_E_INVALID, "nsk_tempered_sweeps: the sequential scan is not served");
    int rc = energy_whole_graph(g, "nsk_tempered_sweeps");
    if (rc) return rc;
    HIPCHECK(hipSetDevice(g->device));
    const Compiled &c = g->c;
    const int R = g->nchains;
    const size_t T = (size_t)nsteps, nw = (size_t)c.nweight, nvar = (size_t)c.nvar;
    const bool keep = best_values || best_lp;
    if ((rc = energy_ensure(g, R, "nsk_tempered_sweeps"))) return rc;
    // a tally kept in bits 1-7 of the value bytes goes back to its array first: the walk and the kept states see plain values
    if ((rc = nsk_unpack_tally(g))) return rc;

    // one chain's values, and the stride of the kept states (16-byte accesses on both sides: a chain's values start on
    // a 256-byte boundary)
    const size_t vbytes = (size_t)c.nid * (size_t)c.vbytes, bstride = (vbytes + 15) / 16 * 16;
    TemperBufs b(g);
    if ((rc = temper_alloc(g, &b.base, nw, "nsk_tempered_sweeps", "the copy of the base weights"))) return rc;
    if (lp && (rc = temper_alloc(g, &b.lp, T * (size_t)R, "nsk_tempered_sweeps", "the log-potentials, nsteps x chains float64"))) return rc;
    if (log_weight && (rc = temper_alloc(g, &b.log_weight, (size_t)R, "nsk_tempered_sweeps", "the log-weights, one float64 a chain"))) return rc;
    if (keep) {
        if ((rc = temper_alloc(g, &b.best_u, (size_t)R, "nsk_tempered_sweeps", "the best log-potentials, one float64 a chain"))) return rc;
        if ((rc = temper_alloc(g, &b.improved, (size_t)R, "nsk_tempered_sweeps", "the flags, one word a chain"))) return rc;
        if (best_values && (rc = temper_alloc(g, &b.best, (size_t)R * bstride, "nsk_tempered_sweeps", "the best states, chains x the bytes of a chain's values"))) return rc;
    }
    if (b.log_weight) HIPCHECK(hipMemsetAsync(b.log_weight, 0, (size_t)R * sizeof(double), g->stream));
    if (nw) HIPCHECK(hipMemcpyAsync(b.base, g->w, nw * sizeof(double), hipMemcpyDeviceToDevice, g->stream));

    const unsigned int wblocks = (unsigned int)((nw + NSK_BLOCK - 1) / NSK_BLOCK);
    const unsigned int kblocks = (unsigned int)std::min<size_t>(256, std::max<size_t>(1, (vbytes / 16 + NSK_BLOCK - 1) / NSK_BLOCK));
    hipError_t e = hipSuccess;
    for (size_t t = 0; t < T && !rc && e == hipSuccess; t++) {
        // 1. scale (from here on an error still restores the base weights below)
        if (nw) k_temper_scale<<<dim3(wblocks), dim3(NSK_BLOCK), 0, g->stream>>>(b.base, betas[t], g->w, (long long)nw);
        g->weights_dirty = true;
        // 2. sweep: what a burn-in call enqueues (nothing tallied, no trace row); it refreshes the tables first
        if ((rc = nsk_gibbs_sweeps(g, sweeps_per_step, sample_evidence, 1))) break;
        // 3. - 5. score under the base weights, fold, keep the best
        TemperFold f = {};
        f.lp_row = b.lp ? b.lp + t * (size_t)R : nullptr;
        f.log_weight = b.log_weight;
        f.best_u = b.best_u;
        f.improved = b.improved;
        f.fold = t + 1 < T ? 1 : 0;
        f.dbeta = f.fold ? betas[t + 1] - betas[t] : 0.0;
        f.first = t == 0 ? 1 : 0;
        if (c.vbytes == 4) temper_score<int32_t>(g, b.base, R, f);
        else temper_score<int8_t>(g, b.base, R, f);
        if (b.best)
            k_temper_keep<<<dim3(kblocks, (unsigned)R), dim3(NSK_BLOCK), 0, g->stream>>>(b.improved, (const char *)g->val, (long long)g->chain_stride,
                                                                                       b.best, (long long)bstride, (long long)vbytes);
        e = hipGetLastError();
    }
    // the base weights come back by a copy, bit for bit, whatever happened above; the next sweep call refreshes the tables
    hipError_t e2 = nw ? hipMemcpyAsync(g->w, b.base, nw * sizeof(double), hipMemcpyDeviceToDevice, g->stream) : hipSuccess;
    g->weights_dirty = true;
    const bool ok = !rc && e == hipSuccess && e2 == hipSuccess;
    if (ok && lp) e2 = hipMemcpyAsync(lp, b.lp, T * (size_t)R * sizeof(double), hipMemcpyDeviceToHost, g->stream);
    if (ok && log_weight && e2 == hipSuccess) e2 = hipMemcpyAsync(log_weight, b.log_weight, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, g->stream);
    if (ok && best_lp && e2 == hipSuccess) e2 = hipMemcpyAsync(best_lp, b.best_u, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, g->stream);
    const hipError_t e3 = hipStreamSynchronize(g->stream);
    if (rc) return rc;
    HIPCHECK(e);
    HIPCHECK(e2);
    HIPCHECK(e3);
    // the kept states leave through the gather of nsk_chains_download: the caller's variable ids, int64
    if (best_values)
        for (size_t r = 0; r < (size_t)R; r++)
            if ((rc = nsk_download_values(g, b.best + r * bstride, best_values + r * nvar, 0))) return rc;
    return NSK_OK;
}
