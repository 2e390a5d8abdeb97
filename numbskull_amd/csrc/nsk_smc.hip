// nsk_smc.hip -- population annealing (nsk_kernels_smc.h): the entry point nsk_smc_sweeps.  A step is the step of
// nsk_tempered_sweeps (nsk_temper.hip) -- scale the weight table from a copy of the base weights, run the burn-in sweeps,
// score every chain under the BASE weights, fold the log-weights, with the very kernels of that call -- and behind the fold
// of every step but the last the population decides on the device whether its weights have degenerated, draws the
// ancestors and copies the surviving chains over the dead ones in place.  Nothing waits for the host: the call restores
// the base weights, synchronises once and downloads what was asked for.  The sweep generators are keyed by the chain's
// slot, so two copies of one state part ways at the next sweep.
#include <hip/hip_runtime.h>

#include <cmath>

#include "nsk_internal.h"
#include "nsk_kernels_temper.h"
#include "nsk_kernels_smc.h"

using namespace nsk;

namespace {

// the buffers of one call: entered in the ledger, gone when the call returns
struct SmcBufs {
    nsk_graph *g;
    double *base = nullptr, *lp = nullptr, *log_weight = nullptr, *logw_pre = nullptr;
    int32_t *anc = nullptr, *resampled = nullptr;
    explicit SmcBufs(nsk_graph *g_) : g(g_) {}
    ~SmcBufs() {
        dev_free(g, resampled); dev_free(g, anc); dev_free(g, logw_pre); dev_free(g, log_weight); dev_free(g, lp); dev_free(g, base);
    }
};

}  // namespace

extern "C" int nsk_smc_sweeps(nsk_graph *g, const double *betas, int64_t nsteps, int64_t sweeps_per_step, int sample_evidence,
                              double threshold, const double *offsets, double *log_weight, double *lp, double *logw_pre,
                              int32_t *ancestors, int32_t *resampled) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!betas) return fail(NSK_E_INVALID, "null argument");
    if (nsteps < 1 || nsteps > 65536) return fail(NSK_E_INVALID, "nsk_smc_sweeps: nsteps must lie in [1, 65536]");
    if (sweeps_per_step < 1 || sweeps_per_step > INT32_MAX / nsteps)
        return fail(NSK_E_INVALID, "nsk_smc_sweeps: sweeps_per_step must be at least 1 and nsteps x sweeps_per_step at most 2^31 - 1");
    for (int64_t t = 0; t < nsteps; t++)
        if (!(betas[t] >= 0.0) || std::isinf(betas[t]))
            return fail(NSK_E_INVALID, "nsk_smc_sweeps: step " + std::to_string((long long)t) + " has an inverse temperature that is negative, infinite or NaN");
    if (!(threshold >= 0.0 && threshold <= 1.0)) return fail(NSK_E_INVALID, "nsk_smc_sweeps: the threshold must lie in [0, 1]");
    if (!offsets && nsteps > 1 && threshold > 0.0) return fail(NSK_E_INVALID, "nsk_smc_sweeps: a threshold above 0 needs the offsets, one a step but the last");
    for (int64_t t = 0; offsets && t + 1 < nsteps; t++)
        if (!(offsets[t] >= 0.0 && offsets[t] < 1.0))
            return fail(NSK_E_INVALID, "nsk_smc_sweeps: the offset of step " + std::to_string((long long)t) + " lies outside [0, 1) or is NaN");
    if (g->scan != NSK_SCAN_CHROMATIC) return fail(NSK_E_INVALID, "nsk_smc_sweeps: the sequential scan is not served");
    int rc = energy_whole_graph(g, "nsk_smc_sweeps");
    if (rc) return rc;
    HIPCHECK(hipSetDevice(g->device));
    const Compiled &c = g->c;
    const int R = g->nchains;
    if (R > NSK_SMC_MAX) return fail(NSK_E_INVALID, "nsk_smc_sweeps: more chains than one block decides for");
    const size_t T = (size_t)nsteps, nw = (size_t)c.nweight;
    if ((rc = energy_ensure(g, R, "nsk_smc_sweeps"))) return rc;
    // a tally kept in bits 1-7 of the value bytes goes back to its array first: the walk and the copies see plain values
    if ((rc = nsk_unpack_tally(g))) return rc;

    const size_t vbytes = (size_t)c.nid * (size_t)c.vbytes, rows = (T - 1) * (size_t)R;
    SmcBufs b(g);
    if ((rc = temper_alloc(g, &b.base, nw, "nsk_smc_sweeps", "the copy of the base weights"))) return rc;
    if (lp && (rc = temper_alloc(g, &b.lp, T * (size_t)R, "nsk_smc_sweeps", "the log-potentials, nsteps x chains float64"))) return rc;
    if ((rc = temper_alloc(g, &b.log_weight, (size_t)R, "nsk_smc_sweeps", "the log-weights, one float64 a chain"))) return rc;
    if (T > 1) {
        if (logw_pre && (rc = temper_alloc(g, &b.logw_pre, rows, "nsk_smc_sweeps", "the log-weights before every decision, (nsteps - 1) x chains float64"))) return rc;
        if ((rc = temper_alloc(g, &b.anc, rows, "nsk_smc_sweeps", "the ancestors, (nsteps - 1) x chains int32"))) return rc;
        if ((rc = temper_alloc(g, &b.resampled, T - 1, "nsk_smc_sweeps", "the flags, one word a step"))) return rc;
    }
    HIPCHECK(hipMemsetAsync(b.log_weight, 0, (size_t)R * sizeof(double), g->stream));
    if (nw) HIPCHECK(hipMemcpyAsync(b.base, g->w, nw * sizeof(double), hipMemcpyDeviceToDevice, g->stream));

    const unsigned int wblocks = (unsigned int)((nw + NSK_BLOCK - 1) / NSK_BLOCK);
    const unsigned int cblocks = (unsigned int)std::min<size_t>(256, std::max<size_t>(1, (vbytes / 16 + NSK_BLOCK - 1) / NSK_BLOCK));
    // without a threshold, or with one chain, no step resamples: the decision still keeps its records, nothing is copied
    const bool copies = threshold > 0.0 && R > 1;
    const double thrR = threshold * (double)R;
    hipError_t e = hipSuccess;
    for (size_t t = 0; t < T && !rc && e == hipSuccess; t++) {
        // 1. scale (from here on an error still restores the base weights below)
        if (nw) k_temper_scale<<<dim3(wblocks), dim3(NSK_BLOCK), 0, g->stream>>>(b.base, betas[t], g->w, (long long)nw);
        g->weights_dirty = true;
        // 2. sweep: what a burn-in call enqueues (nothing tallied, no trace row); it refreshes the tables first
        if ((rc = nsk_gibbs_sweeps(g, sweeps_per_step, sample_evidence, 1))) break;
        // 3., 4. score under the base weights, fold
        TemperFold f = {};
        f.lp_row = b.lp ? b.lp + t * (size_t)R : nullptr;
        f.log_weight = b.log_weight;
        f.fold = t + 1 < T ? 1 : 0;
        f.dbeta = f.fold ? betas[t + 1] - betas[t] : 0.0;
        if (c.vbytes == 4) temper_score<int32_t>(g, b.base, R, f);
        else temper_score<int8_t>(g, b.base, R, f);
        // 5., 6. decide and copy
        if (t + 1 < T) {
            SmcDecide d = {};
            d.log_weight = b.log_weight;
            d.logw_pre = b.logw_pre ? b.logw_pre + t * (size_t)R : nullptr;
            d.anc = b.anc + t * (size_t)R;
            d.resampled = b.resampled + t;
            d.thrR = thrR;
            d.offset = offsets ? offsets[t] : 0.0;
            d.R = R;
            k_smc_decide<<<dim3(1), dim3((unsigned)((R + 63) / 64 * 64)), 0, g->stream>>>(d);
            if (copies)
                k_smc_copy<<<dim3(cblocks, (unsigned)R), dim3(NSK_BLOCK), 0, g->stream>>>(d.anc, (char *)g->val, (long long)g->chain_stride, (long long)vbytes);
        }
        e = hipGetLastError();
    }
    // a copy may have carried a value outside its domain from any slot into any other: chain 0 and the chains behind it
    // are regular only if all were (values_regular, their conjunction, stays what it is)
    if (copies && T > 1) g->chain_regular[0] = g->chains_regular = g->chain_regular[0] && g->chains_regular;
    // the base weights come back by a copy, bit for bit, whatever happened above; the next sweep call refreshes the tables
    hipError_t e2 = nw ? hipMemcpyAsync(g->w, b.base, nw * sizeof(double), hipMemcpyDeviceToDevice, g->stream) : hipSuccess;
    g->weights_dirty = true;
    const bool ok = !rc && e == hipSuccess && e2 == hipSuccess;
    if (ok && lp) e2 = hipMemcpyAsync(lp, b.lp, T * (size_t)R * sizeof(double), hipMemcpyDeviceToHost, g->stream);
    if (ok && log_weight && e2 == hipSuccess) e2 = hipMemcpyAsync(log_weight, b.log_weight, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, g->stream);
    if (ok && T > 1) {
        if (logw_pre && e2 == hipSuccess) e2 = hipMemcpyAsync(logw_pre, b.logw_pre, rows * sizeof(double), hipMemcpyDeviceToHost, g->stream);
        if (ancestors && e2 == hipSuccess) e2 = hipMemcpyAsync(ancestors, b.anc, rows * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream);
        if (resampled && e2 == hipSuccess) e2 = hipMemcpyAsync(resampled, b.resampled, (T - 1) * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream);
    }
    const hipError_t e3 = hipStreamSynchronize(g->stream);
    if (rc) return rc;
    HIPCHECK(e);
    HIPCHECK(e2);
    HIPCHECK(e3);
    return NSK_OK;
}
