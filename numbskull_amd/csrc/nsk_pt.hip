// nsk_pt.hip -- parallel tempering (nsk_kernels_pt.h): the entry point nsk_pt_sweeps.  Every chain of the handle is a
// replica at a FIXED inverse temperature; a step sweeps each replica alone under its own scaled weight table (the scale
// kernel of nsk_tempered_sweeps, the one-chain launches of nsk_gibbs.hip through nsk_gibbs_chain, the tables rebuilt in
// front of every replica), scores all chains under the BASE weights in one walk (temper_score), decides the Metropolis
// swaps of the step's pairs on the device and exchanges the accepted pairs' states in place.  No sweep kernel, kernel
// argument, plan or captured sequence knows of it.  Nothing waits for the host: the call restores the base weights,
// synchronises once and downloads what was asked for.  The sweep generators are keyed by the chain's slot, so a state
// that moved goes on under the stream of the slot it moved to.
#include <hip/hip_runtime.h>

#include <cmath>

#include "nsk_class_plan.h"         // plan_grid_cap
#include "nsk_internal.h"
#include "nsk_kernels_temper.h"
#include "nsk_kernels_pt.h"

using namespace nsk;

namespace {

// the buffers of one call: entered in the ledger, gone when the call returns
struct PtBufs {
    nsk_graph *g;
    double *base = nullptr, *lp = nullptr, *betas = nullptr, *uniforms = nullptr;
    int32_t *accepted = nullptr, *partner = nullptr;
    explicit PtBufs(nsk_graph *g_) : g(g_) {}
    ~PtBufs() {
        dev_free(g, partner); dev_free(g, accepted); dev_free(g, uniforms); dev_free(g, betas); dev_free(g, lp); dev_free(g, base);
    }
};

}  // namespace

extern "C" int nsk_pt_sweeps(nsk_graph *g, const double *betas, int64_t nsteps, int64_t sweeps_per_step, int sample_evidence,
                             const double *uniforms, int tally_chain, double *lp, int32_t *accepted) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!betas) return fail(NSK_E_INVALID, "null argument");
    if (nsteps < 1 || nsteps > 65536) return fail(NSK_E_INVALID, "nsk_pt_sweeps: nsteps must lie in [1, 65536]");
    if (sweeps_per_step < 1 || sweeps_per_step > INT32_MAX / nsteps)
        return fail(NSK_E_INVALID, "nsk_pt_sweeps: sweeps_per_step must be at least 1 and nsteps x sweeps_per_step at most 2^31 - 1");
    const int R = g->nchains;
    const size_t T = (size_t)nsteps, P = (size_t)(R - 1);
    for (int r = 0; r < R; r++)
        if (!(betas[r] >= 0.0) || std::isinf(betas[r]))
            return fail(NSK_E_INVALID, "nsk_pt_sweeps: chain " + std::to_string(r) + " has an inverse temperature that is negative, infinite or NaN");
    if (!uniforms && R > 1) return fail(NSK_E_INVALID, "nsk_pt_sweeps: several chains need the uniforms, one a step and pair");
    for (size_t i = 0; uniforms && i < T * P; i++)
        if (!(uniforms[i] >= 0.0 && uniforms[i] < 1.0))
            return fail(NSK_E_INVALID, "nsk_pt_sweeps: the uniform of step " + std::to_string((long long)(i / P)) + ", pair " +
                                       std::to_string((long long)(i % P)) + " lies outside [0, 1) or is NaN");
    if (tally_chain < -1 || tally_chain >= R) return fail(NSK_E_INVALID, "nsk_pt_sweeps: tally_chain must be -1 or a chain of the handle");
    NSK_NO_TRACE(g, "nsk_pt_sweeps");
    if (g->scan != NSK_SCAN_CHROMATIC) return fail(NSK_E_INVALID, "nsk_pt_sweeps: the sequential scan is not served");
    int rc = energy_whole_graph(g, "nsk_pt_sweeps");
    if (rc) return rc;
    HIPCHECK(hipSetDevice(g->device));
    const Compiled &c = g->c;
    const size_t nw = (size_t)c.nweight;
    if ((rc = energy_ensure(g, R, "nsk_pt_sweeps"))) return rc;

    const size_t vbytes = (size_t)c.nid * (size_t)c.vbytes;
    PtBufs b(g);
    // (a caller that does not ask for lp or accepted leaves one row of each, which every step reuses)
    if ((rc = temper_alloc(g, &b.base, nw, "nsk_pt_sweeps", "the copy of the base weights"))) return rc;
    if ((rc = temper_alloc(g, &b.lp, (lp ? T : 1) * (size_t)R, "nsk_pt_sweeps", "the log-potentials, nsteps x chains float64"))) return rc;
    if (R > 1) {
        if ((rc = temper_alloc(g, &b.betas, (size_t)R, "nsk_pt_sweeps", "the inverse temperatures, one float64 a chain"))) return rc;
        if ((rc = temper_alloc(g, &b.uniforms, T * P, "nsk_pt_sweeps", "the uniforms, nsteps x (chains - 1) float64"))) return rc;
        if ((rc = temper_alloc(g, &b.accepted, (accepted ? T : 1) * P, "nsk_pt_sweeps", "the decisions, nsteps x (chains - 1) int32"))) return rc;
        if ((rc = temper_alloc(g, &b.partner, (size_t)R, "nsk_pt_sweeps", "the partners, one word a chain"))) return rc;
    }
    // a tally kept in bits 1-7 of the value bytes goes back to its array, and what the uint8 position tally holds goes
    // into the masters: the walk and the swaps see plain values, and from here on only tally_chain's tally grows
    if ((rc = nsk_fold_position_tally(g))) return rc;
    if (R > 1) {
        HIPCHECK(hipMemcpyAsync(b.betas, betas, (size_t)R * sizeof(double), hipMemcpyHostToDevice, g->stream));
        HIPCHECK(hipMemcpyAsync(b.uniforms, uniforms, T * P * sizeof(double), hipMemcpyHostToDevice, g->stream));
    }
    if (nw) HIPCHECK(hipMemcpyAsync(b.base, g->w, nw * sizeof(double), hipMemcpyDeviceToDevice, g->stream));

    const unsigned int wblocks = (unsigned int)((nw + NSK_BLOCK - 1) / NSK_BLOCK);
    unsigned int sblocks = (unsigned int)std::min<size_t>(256, std::max<size_t>(1, (vbytes / 16 + NSK_BLOCK - 1) / NSK_BLOCK));
    const int cap = plan_grid_cap(nsk::diag_env("NSK_PT_SWAP_GRID_CAP"));       // (diagnostic: a small swap grid, later trips)
    if (cap > 0) sblocks = std::min(sblocks, (unsigned int)cap);
    const uint64_t sweep0 = g->sweep;
    const int64_t done0 = g->sweeps_done;
    hipError_t e = hipSuccess;
    for (size_t t = 0; t < T && !rc && e == hipSuccess; t++) {
        // 1. sweep: every replica alone under its own table, all from the step's first sweep index on (from the first
        // scale on an error still restores the base weights below)
        const uint64_t s_t = sweep0 + (uint64_t)t * (uint64_t)sweeps_per_step;
        for (int r = 0; r < R && !rc; r++) {
            if (nw) k_temper_scale<<<dim3(wblocks), dim3(NSK_BLOCK), 0, g->stream>>>(b.base, betas[r], g->w, (long long)nw);
            g->weights_dirty = true;
            g->sweep = s_t;
            g->sweeps_done = done0 + (int64_t)t * sweeps_per_step;
            rc = nsk_gibbs_chain(g, r, sweeps_per_step, sample_evidence, r == tally_chain ? 0 : 1);
        }
        if (rc) break;
        // 2. score under the base weights: all chains in one walk, U with the bits of nsk_log_potential
        double *U = b.lp + (lp ? t * (size_t)R : 0);
        TemperFold f = {};
        f.lp_row = U;
        if (c.vbytes == 4) temper_score<int32_t>(g, b.base, R, f);
        else temper_score<int8_t>(g, b.base, R, f);
        // 3., 4. decide and swap
        if (R > 1) {
            PtDecide d = {};
            d.betas = b.betas;
            d.U = U;
            d.uniforms = b.uniforms + t * P;
            d.accepted = b.accepted + (accepted ? t * P : 0);
            d.partner = b.partner;
            d.R = R;
            d.parity = (int)(t & 1);
            k_pt_decide<<<dim3(1), dim3((unsigned)((R - 1 + 63) / 64 * 64)), 0, g->stream>>>(d);
            const unsigned int npairs = (unsigned int)((R - d.parity) / 2);
            if (npairs)
                k_pt_swap<<<dim3(sblocks, npairs), dim3(NSK_BLOCK), 0, g->stream>>>(b.partner, (char *)g->val, (long long)g->chain_stride,
                                                                                   (long long)vbytes, d.parity);
        }
        e = hipGetLastError();
    }
    // what tally_chain's sweeps left in its uint8 position tally goes into its master: the handle-wide count is 0 again
    if (tally_chain >= 0) { ChainSwap cs(g, tally_chain); (void)nsk_fold_position_tally(g); }
    // a swap may have carried a value outside its domain from any slot into its neighbour: chain 0 and the chains behind
    // it are regular only if all were (values_regular, their conjunction, stays what it is)
    if (R > 1) g->chain_regular[0] = g->chains_regular = g->chain_regular[0] && g->chains_regular;
    // the base weights come back by a copy, bit for bit, whatever happened above; the next sweep call refreshes the tables
    hipError_t e2 = nw ? hipMemcpyAsync(g->w, b.base, nw * sizeof(double), hipMemcpyDeviceToDevice, g->stream) : hipSuccess;
    g->weights_dirty = true;
    const bool ok = !rc && e == hipSuccess && e2 == hipSuccess;
    if (ok && lp) e2 = hipMemcpyAsync(lp, b.lp, T * (size_t)R * sizeof(double), hipMemcpyDeviceToHost, g->stream);
    if (ok && accepted && R > 1 && e2 == hipSuccess) e2 = hipMemcpyAsync(accepted, b.accepted, T * P * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream);
    const hipError_t e3 = hipStreamSynchronize(g->stream);
    if (rc) return rc;
    HIPCHECK(e);
    HIPCHECK(e2);
    HIPCHECK(e3);
    return NSK_OK;
}
