// nsk_bp_residual.hip -- sum-product belief propagation under a residual schedule on the selected resident set-up
// (nsk_internal.h NskBp rs_*, nsk_kernels_bpres.h): a round recomputes the candidate messages of the edges whose inputs
// moved, commits those whose pending change is at least `frac` of the largest one and walks the variables they touch.
// It shares f2v, v2f and the beliefs with nsk_bp_run, so beliefs, factor beliefs, moments and a following nsk_bp_run work
// on what it leaves.  The first call on a set-up allocates the candidates, the pending changes, the flags, the queues
// and the edge -> v_list position map, which the set-up owns from then on (nsk_bp_clear, a replacing set-up and
// nsk_graph_destroy free them with the rest).  A call enqueues every round on the handle's stream -- five launches a
// round (four without a binary variable, or with nothing else) sized for the full index ranges, the lanes striding over
// the queue counters of the round -- without a synchronisation between them, the early exit on the device as in
// nsk_bp_run, and copies residuals and counters back once.  The launches are not counted by the profiling bracket.
#include <hip/hip_runtime.h>

#include <cstring>

#include "nsk_internal.h"
#include "nsk_kernels_bpres.h"

using namespace nsk;

static size_t round4(size_t n) { return (n + 3) / 4 * 4; }

// the arrays of the first run on a set-up; on a failure none of them stays
static int rs_ensure(nsk_graph *g, bool &fresh) {
    NskBp &b = g->bp;
    fresh = false;
    if (b.rs_cand) return NSK_OK;
    const size_t nmsg = (size_t)b.info.nmsg, E = (size_t)b.info.nedges, nv = (size_t)b.nvlist, at = b.owned.size();
    auto keep = [&](int rc, void *p) { if (!rc) b.owned.push_back(p); return rc; };
    int rc = keep(dev_alloc(g, &b.rs_cand, nmsg), b.rs_cand);
    if (!rc) rc = keep(dev_alloc(g, &b.rs_r, E), b.rs_r);
    if (!rc && b.rs_walk) rc = keep(dev_alloc(g, &b.rs_pre, nmsg), b.rs_pre);
    if (!rc && b.rs_walk) rc = keep(dev_alloc(g, &b.rs_chg, E), b.rs_chg);
    if (!rc) rc = keep(dev_alloc(g, &b.rs_dflag, round4(E)), b.rs_dflag);
    if (!rc) rc = keep(dev_alloc(g, &b.rs_vflag, round4(nv)), b.rs_vflag);
    if (!rc) rc = keep(dev_alloc(g, &b.rs_dq, E), b.rs_dq);
    if (!rc) rc = keep(dev_alloc(g, &b.rs_vq, nv), b.rs_vq);
    if (!rc) rc = keep(dev_alloc(g, &b.rs_vpos, E), b.rs_vpos);
    if (rc) {
        for (size_t i = at; i < b.owned.size(); i++) dev_free(g, b.owned[i]);
        b.owned.resize(at);
        b.rs_cand = b.rs_r = b.rs_pre = nullptr;
        b.rs_chg = b.rs_dflag = b.rs_vflag = nullptr;
        b.rs_dq = b.rs_vq = b.rs_vpos = nullptr;
        if (rc != NSK_E_NOMEM) return rc;
        const long long bytes = (b.rs_walk ? 16ll : 8ll) * (long long)nmsg + (b.rs_walk ? 18ll : 17ll) * (long long)E + 5ll * (long long)nv;
        return fail(NSK_E_NOMEM, "nsk_bp_residual_run: the candidates, the pending changes, the flags, the queues and the position map (" +
                                 std::to_string(bytes) + " bytes) do not fit on the device");
    }
    fresh = true;
    return NSK_OK;
}

extern "C" {

int nsk_bp_residual_run(nsk_graph *g, int64_t max_rounds, double frac, double damping, double tol, int warm, int64_t *rounds,
                        double *residual, int64_t *updates, int64_t *recomputed) {
    const char *who = "nsk_bp_residual_run";
    if (!g) return fail(NSK_E_INVALID, "null graph");
    int rc = energy_whole_graph(g, who);
    if (rc) return rc;
    if (!g->bp.ready) return fail(NSK_E_INVALID, std::string(who) + ": no belief propagation is set up (nsk_bp_setup)");
    if ((rc = bp_refuse_wide(g->bp, who))) return rc;
    if (!rounds) return fail(NSK_E_INVALID, "null argument");
    if (max_rounds < 1 || max_rounds > 4096) return fail(NSK_E_INVALID, std::string(who) + ": max_rounds must lie in [1, 4096]");
    if (!(frac >= 0.0 && frac <= 1.0)) return fail(NSK_E_INVALID, std::string(who) + ": frac must lie in [0, 1]");
    if (!(damping >= 0.0 && damping < 1.0)) return fail(NSK_E_INVALID, std::string(who) + ": damping must lie in [0, 1)");
    if (!(tol >= 0.0)) return fail(NSK_E_INVALID, std::string(who) + ": tol must be at least 0");
    if (warm != 0 && warm != 1) return fail(NSK_E_INVALID, std::string(who) + ": warm must be 0 or 1");
    HIPCHECK(hipSetDevice(g->device));
    bool fresh = false;
    if ((rc = rs_ensure(g, fresh))) return rc;
    NskBp &b = g->bp;
    const size_t S = (size_t)max_rounds, ncall = 5 * S + 1;
    unsigned long long *call = nullptr;             // for this call only: res[S] upd[S] nD[S + 1] nV[2 S]
    if ((rc = call_alloc(g, &call, ncall, who, "the residuals and the counters, 40 bytes a round"))) return rc;

    ResArgs q = {};
    q.b = bp_args(g, b);
    q.cand = b.rs_cand; q.r = b.rs_r; q.pre = b.rs_pre; q.chg = b.rs_chg; q.dflag = b.rs_dflag; q.vflag = b.rs_vflag;
    q.dq = b.rs_dq; q.vq = b.rs_vq; q.e_vpos = b.rs_vpos;
    q.res = call; q.upd = call + S; q.nD = call + 2 * S; q.nV = call + 3 * S + 1;
    q.nvbin = b.nvbin;
    const BpArgs &a = q.b;
    const int E = a.nedge, nbin = b.nvbin, nall = a.nvlist, cold = (fresh || !warm) ? 1 : 0;
    const double oml = 1.0 - damping;
    const dim3 block(NSK_BLOCK), ge(bp_blocks(E, NSK_BLOCK)), vblock(NSK_BP_VAR_BLOCK), gb(bp_blocks(nbin, NSK_BP_VAR_BLOCK)),
               gr(bp_blocks(nall - nbin, NSK_BP_VAR_BLOCK));
    hipError_t e = hipMemsetAsync(call, 0, ncall * 8, g->stream);
    if (e == hipSuccess && fresh) {
        if (E > 0) e = hipMemsetAsync(b.rs_dflag, 0, round4((size_t)E), g->stream);
        if (e == hipSuccess && nall > 0) e = hipMemsetAsync(b.rs_vflag, 0, round4((size_t)nall), g->stream);
        if (e == hipSuccess && nall > 0) {
            k_bpres_vpos<<<dim3(bp_blocks(nall, NSK_BLOCK)), block, 0, g->stream>>>(q);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess && cold && E > 0) {         // a cold start; new arrays start cold whatever the caller says
        k_bp_reset<<<ge, block, 0, g->stream>>>(a);
        e = hipGetLastError();
    }
    if (E > 0)
        for (size_t t = 0; t < S && e == hipSuccess; t++) {
            const int first = t == 0 ? 1 : 0, every = first && cold;
            k_bpres_cand<<<ge, block, 0, g->stream>>>(q, (int)t, first, tol, damping, oml);
            k_bpres_max<<<ge, block, 0, g->stream>>>(q, (int)t, tol);
            k_bpres_commit<<<ge, block, 0, g->stream>>>(q, (int)t, tol, frac, damping, oml, every ? 0 : 1);
            if (nbin > 0) k_bpres_var<true><<<gb, vblock, 0, g->stream>>>(q, (int)t, every, tol);
            if (nall > nbin) k_bpres_var<false><<<gr, vblock, 0, g->stream>>>(q, (int)t, every, tol);
            e = hipGetLastError();
        }
    std::vector<unsigned long long> host(ncall);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), call, ncall * 8, hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);
    dev_free(g, call);
    HIPCHECK(e);
    HIPCHECK(e2);
    int64_t ran = -max_rounds;
    for (size_t t = 0; t < S; t++) {
        double r;
        memcpy(&r, &host[t], 8);
        const bool live = ran < 0;                  // round t ran: no earlier round met the tolerance
        if (residual) residual[t] = r;
        if (updates) updates[t] = (int64_t)host[S + t];
        if (recomputed) recomputed[t] = !live ? 0 : (t == 0 ? (int64_t)E : (int64_t)host[2 * S + t]);
        if (live && r <= tol) ran = (int64_t)t + 1;
    }
    *rounds = ran;
    return NSK_OK;
}

}  // extern "C"
