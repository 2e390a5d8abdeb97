// nsk_icm.hip -- greedy MAP search, iterated conditional modes (nsk_kernels_icm.h): the entry point nsk_icm.  It reads
// the arrays the conditionals read (nsk_cond.hip cond_ensure) and the colour ranges of the compiled layout, enqueues every
// class launch of every sweep on the handle's stream without a synchronisation between them -- a chain that has reached
// its fixed point ends its later launches on the device -- and copies the per-sweep change counters back once.
#include <hip/hip_runtime.h>

#include "nsk_internal.h"
#include "nsk_kernels_icm.h"

using namespace nsk;

extern "C" {

int nsk_icm(nsk_graph *g, int which, int64_t first_chain, int64_t nchains, int64_t max_sweeps, int sample_evidence,
            int64_t *sweeps, int64_t *changed) {
    if (!g) return fail(NSK_E_INVALID, "null graph");
    if (!sweeps) return fail(NSK_E_INVALID, "null argument");
    int rc = chain_select(g, which, first_chain, nchains, "nsk_icm");
    if (rc) return rc;
    if (max_sweeps < 1 || max_sweeps > 4096) return fail(NSK_E_INVALID, "nsk_icm: max_sweeps must lie in [1, 4096]");
    if ((rc = energy_whole_graph(g, "nsk_icm"))) return rc;
    HIPCHECK(hipSetDevice(g->device));
    if ((rc = cond_ensure(g, "nsk_icm"))) return rc;
    // a tally kept in bits 1-7 of the value bytes goes back to its array first, as before a state download: the kernel
    // sees plain values (only a one-chain handle keeps its tally there)
    if ((rc = nsk_unpack_tally(g))) return rc;
    const Compiled &c = g->c;
    const size_t S = (size_t)max_sweeps, N = (size_t)nchains;
    long long *counters = nullptr;          // [max_sweeps][nchains], for this call only
    if ((rc = dev_alloc(g, &counters, S * N))) {
        if (rc != NSK_E_NOMEM) return rc;
        return fail(NSK_E_NOMEM, "nsk_icm: the change counters, max_sweeps x chains int64 (" + std::to_string((long long)(S * N * 8)) +
                                 " bytes), do not fit on the device");
    }
    hipError_t e = hipMemsetAsync(counters, 0, S * N * sizeof(long long), g->stream);
    CondArgs a = {};
    a.p_info = g->p_info; a.p_slot = g->p_slot; a.slot_off = g->slot_off; a.fidx = g->fidx;
    a.f_rec = (const uint4 *)g->f_rec; a.m_rec = (const int2 *)g->m_rec;
    a.v_card = g->v_card; a.iid_of_vid = g->iid_of_vid;
    a.w = g->w; a.logtab = g->logtab;
    a.chain_stride = (long long)g->chain_stride;
    a.head_by_vid = (c.flags & NSK_FLAG_HEAD_BY_VID) ? 1 : 0;
    char *val = chain_val(g, which, first_chain);
    const size_t ncolors = c.phase_end.size();
    for (size_t s = 0; s < S && e == hipSuccess; s++) {
        const long long *prev = s ? counters + (s - 1) * N : nullptr;
        unsigned long long *cur = (unsigned long long *)(counters + s * N);
        for (size_t k = 0; k < ncolors; k++) {
            const long long lo = (long long)c.phase_start[k], hi = (long long)c.phase_end[k];
            if (hi <= lo) continue;
            const unsigned nb = (unsigned)std::min<long long>(2048, (hi - lo + NSK_BLOCK - 1) / NSK_BLOCK);
            const dim3 grid(nb, (unsigned)nchains), block(NSK_BLOCK);
            if (c.vbytes == 4) k_icm<int32_t><<<grid, block, 0, g->stream>>>(a, g->p_vid, (int32_t *)val, lo, hi, sample_evidence ? 1 : 0, prev, cur);
            else k_icm<int8_t><<<grid, block, 0, g->stream>>>(a, g->p_vid, (int8_t *)val, lo, hi, sample_evidence ? 1 : 0, prev, cur);
        }
        e = hipGetLastError();
    }
    std::vector<long long> host(S * N);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), counters, S * N * sizeof(long long), hipMemcpyDeviceToHost, g->stream);
    const hipError_t e2 = hipStreamSynchronize(g->stream);
    dev_free(g, counters);
    HIPCHECK(e);
    HIPCHECK(e2);
    for (size_t i = 0; i < N; i++) {
        int64_t ran = -max_sweeps;          // every sweep changed something: not converged
        for (size_t s = 0; s < S; s++) {
            if (changed) changed[i * S + s] = (int64_t)host[s * N + i];
            if (ran < 0 && host[s * N + i] == 0) ran = (int64_t)s + 1;
        }
        sweeps[i] = ran;
    }
    return NSK_OK;
}

}  // extern "C"
