"""FactorGraph: owner of the graph/state arrays and driver of burn-in, inference and learning.

Keeps the public face of the reference class (numbskull/factorgraph.py:27-229: constructor
signature, attributes, method names, text dumps) so that callers -- the CLI, the reference's
smoke scripts, code that patches ``var_value`` / ``weight_value`` between epochs -- keep working.
What changed is what happens below ``burnIn`` / ``inference`` / ``learn``: the reference fans
``gibbsthread`` / ``learnthread`` out over a thread pool (run_pool, factorgraph.py:13-24, called
at :141, :163, :202); here those three call sites go through the C-ABI to HIP kernels on the
MI355X.  The STATE arrays -- ``var_value``, ``var_value_evid``, ``weight_value``, ``count`` -- are
uploaded when a call starts and downloaded when it returns, so in-place edits of them between
calls are honoured exactly like in the reference.  The STRUCTURE (``variable`` incl. isEvidence /
initialValue of evidence, ``weight['isFixed']``, ``factor``, ``fmap``, ``vmap``,
``factor_index``) is compiled into the device layout once, at the first call; after editing it in
place call ``invalidate()`` so that the next call recompiles.
"""

import collections
import ctypes as C
import sys
import warnings

import numpy as np

from . import _lib
from .timer import Timer


def _all_copies(var_copy):
    return isinstance(var_copy, str) and var_copy == "all"


# what FactorGraph.mixing returns, one entry per selected variable (samples: the samples the figures rest on)
Mixing = collections.namedtuple("Mixing", ["ess", "tau", "rhat", "mean", "truncated", "samples"])
# what FactorGraph.mixing_values returns, one entry per indicator (variable id, value)
MixingValues = collections.namedtuple("MixingValues", ["ess", "tau", "rhat", "mean", "truncated", "samples", "var", "value", "offset"])


def split_rhat(half_counts, n):
    """Split-R-hat per tally slot: ``half_counts`` (M, ncount) holds each half-chain's tally over ``n``
    sweeps (M = 2 x chains).  With half-chain means p_j: B = n / (M - 1) sum (p_j - mean p)^2,
    W = mean(n / (n - 1) p_j (1 - p_j)), R-hat = sqrt(((n - 1) / n W + B / n) / W); NaN where W = 0 or n < 2."""
    hc = np.asarray(half_counts, np.float64)
    out = np.full(hc.shape[1] if hc.ndim == 2 else 0, np.nan)
    m = hc.shape[0] if hc.ndim == 2 else 0
    if n < 2 or m < 2:
        return out
    p = hc / float(n)
    b = n / (m - 1.0) * ((p - p.mean(axis=0)) ** 2).sum(axis=0)
    w = (n / (n - 1.0) * p * (1.0 - p)).mean(axis=0)
    ok = w > 0
    out[ok] = np.sqrt(((n - 1.0) / n * w[ok] + b[ok] / n) / w[ok])
    return out


class FactorGraph(object):
    """A factor graph resident on one MI355X.

    Positional parameters are the reference's (factorgraph.py:30-31).  Keyword-only extras:
    ``device`` (HIP ordinal), ``seed`` (Philox key / MT19937 seed), ``scan`` ("chromatic" or
    "sequential"), ``head_by_vid`` (intended head lookup for IMPLY_MLN-type factors instead of
    the literal inference.py:243 indexing), ``own_range`` ((begin, end) variable ids sampled by
    this handle when the graph is range-partitioned over several GPUs), ``learn_cap`` / ``learn_lag``
    (chromatic learning: cap on visits x stepsize per weight and colour class; the weight update of a
    class overlapped with the next class's sampling, nsk_set_learn_lag).
    """

    def __init__(self, weight, variable, factor, fmap, vmap, factor_index, var_copies,
                 weight_copies, fid, workers, *, device=0, seed=0, scan="chromatic",
                 head_by_vid=False, own_range=None, learn_cap=0.5, global_ids=None, learn_lag=True):
        self.weight, self.variable, self.factor = weight, variable, factor
        self.fmap, self.vmap, self.factor_index = fmap, vmap, factor_index

        nvar = variable.shape[0]
        # tally layout: one slot for a binary variable, `cardinality` slots otherwise (native: the records are packed
        # 27-byte structs, numpy's strided field reads take seconds at 50M variables)
        self.cstart = np.zeros(nvar + 1, np.int64)
        init = np.empty(nvar, np.int64)
        max_card, longest = C.c_int64(), C.c_int64()
        vc, mc = _lib.as_c(variable), _lib.as_c(vmap)
        if vc.dtype.itemsize != 27 or mc.dtype.itemsize != 24:
            raise TypeError("variable / vmap records of %d / %d bytes, expected 27 / 24 (numbskulltypes)" % (vc.dtype.itemsize, mc.dtype.itemsize))
        _lib.check(_lib.lib().nsk_state_layout(nvar, _lib.ptr(vc), len(mc), _lib.ptr(mc), _lib.ptr(self.cstart), _lib.ptr(init),
                                               C.byref(max_card), C.byref(longest)))
        ncount = int(self.cstart[nvar])
        self.count = np.zeros(ncount, np.int64)

        self.var_value_evid = np.tile(init, (var_copies, 1))
        self.var_value = np.tile(init, (var_copies, 1))
        self.weight_value = np.tile(weight["initialValue"], (weight_copies, 1))

        # scratch arrays of the reference's CPU threads; kept for attribute compatibility only
        self.Z = np.zeros((workers, int(max_card.value) if nvar else 0))
        self.fids = np.zeros((workers, 2 * int(longest.value)), factor_index.dtype)

        self.fid = fid
        assert workers > 0
        self.threads = workers          # accepted for compatibility; the GPU ignores it
        self.threadpool = None
        self.marginals = np.zeros(ncount)
        # var_copy="all" (one chain per row of var_value): each chain's own tally, and split-R-hat per tally slot
        self.chain_count = np.zeros((var_copies, ncount), np.int64)
        self.rhat = np.full(ncount, np.nan)
        self.inference_epoch_time = 0.0
        self.inference_total_time = 0.0
        self.learning_epoch_time = 0.0
        self.learning_total_time = 0.0

        self.device = int(device)
        self.seed = int(seed)
        self.scan = scan
        self.learn_cap = float(learn_cap)
        self.learn_lag = bool(learn_lag)
        self.head_by_vid = bool(head_by_vid)
        self.own_range = own_range
        # shard-local graph (graphgen.extract_shard): global id of every local variable; the shard's
        # generator streams are tagged with the GLOBAL id of its first owned variable
        self.global_ids = None if global_ids is None else np.ascontiguousarray(global_ids, np.int64)
        self._handle = None
        self._keep = None
        self._clipped_seen = 0

    # ------------------------------------------------------------------ device handle
    def _descriptor(self):
        """nsk_graph_desc over the arrays this object owns (plus the arrays kept alive)."""
        arrays = [_lib.as_c(a) for a in (self.weight, self.variable, self.factor, self.fmap,
                                         self.vmap)]
        fi = _lib.as_c(self.factor_index, np.int64)
        sizes = (9, 27, 34, 16, 24)
        for a, s in zip(arrays, sizes):
            if a.dtype.itemsize != s:
                raise TypeError("record array with itemsize %d, expected %d" % (a.dtype.itemsize, s))
        w, v, f, fm, vm = arrays
        ob, oe = self.own_range if self.own_range is not None else (0, 0)
        desc = _lib.GraphDesc(len(w), len(v), len(f), len(fm), len(vm), len(fi),
                              w.ctypes.data, v.ctypes.data, f.ctypes.data, fm.ctypes.data,
                              vm.ctypes.data, fi.ctypes.data,
                              (_lib.FLAG_HEAD_BY_VID if self.head_by_vid else 0) |
                              (_lib.FLAG_PARTITION if self.own_range is not None else 0), self.device,
                              int(ob), int(oe))
        return desc, (arrays, fi)

    def plan(self):
        """Host-only: validate and colour the graph as the device build would (no GPU needed).
        Returns (color[nvar] with -1 for variables this handle does not sample, info dict)."""
        desc, keep = self._descriptor()
        color = np.zeros(self.variable.shape[0], np.int32)
        inf = _lib.GraphInfo()
        _lib.check(_lib.lib().nsk_graph_plan(C.byref(desc), _lib.ptr(color), C.byref(inf)))
        return color, {k: getattr(inf, k) for k, _ in inf._fields_}

    def plan_routes(self):
        """Host-only: the route word of every variable (which kernel family would sample it, with the sizes of its
        tile or group: nsk_graph_plan_routes; ``_lib.route_fields`` names the fields)."""
        desc, keep = self._descriptor()
        out = np.zeros(self.variable.shape[0], np.int32)
        _lib.check(_lib.lib().nsk_graph_plan_routes(C.byref(desc), _lib.ptr(out)))
        return out

    def plan_classes(self, learning, regularization=2, grid_cap=0):
        """Host-only: the launches a sweep would give every colour class (nsk_graph_plan_classes), one int32 record per
        class -- ``_lib.class_fields`` names the fields.  ``learning``: the learning sweep under ``regularization``, else
        the inference sweep; ``grid_cap``: what a sweep reads from NSK_CLASS_GRID_CAP (0: none)."""
        desc, keep = self._descriptor()
        n = C.c_int64()
        L = _lib.lib()
        _lib.check(L.nsk_graph_plan_classes(C.byref(desc), int(bool(learning)), int(regularization), int(grid_cap), None, C.byref(n)))
        out = np.zeros((n.value, _lib.CLASS_REC), np.int32)
        _lib.check(L.nsk_graph_plan_classes(C.byref(desc), int(bool(learning)), int(regularization), int(grid_cap),
                                            _lib.ptr(out), C.byref(n)))
        return out

    def routes(self):
        """The route word of every variable on this handle's compiled layout (nsk_graph_get_routes)."""
        out = np.zeros(self.variable.shape[0], np.int32)
        _lib.check(_lib.lib().nsk_graph_get_routes(self._engine(), _lib.ptr(out)))
        return out

    def ghost_needs(self, host_only=False):
        """Sorted ids of the variables outside ``own_range`` that this partition's variables read
        (what the boundary exchange must deliver).  ``host_only`` plans without touching a GPU."""
        L = _lib.lib()
        n = C.c_int64()
        if host_only:
            desc, keep = self._descriptor()
            _lib.check(L.nsk_graph_plan_needs(C.byref(desc), C.byref(n), None))
            out = np.zeros(n.value, np.int32)
            _lib.check(L.nsk_graph_plan_needs(C.byref(desc), C.byref(n), _lib.ptr(out)))
            return out
        h = self._engine()
        _lib.check(L.nsk_ghost_needs(h, C.byref(n), None))
        out = np.zeros(n.value, np.int32)
        _lib.check(L.nsk_ghost_needs(h, C.byref(n), _lib.ptr(out)))
        return out

    def _engine(self):
        """Create (once) the device-side graph.  Fails loudly without a GPU."""
        if self._handle is not None:
            return self._handle
        L = _lib.lib()
        desc, keep = self._descriptor()
        h = C.c_void_p()
        _lib.check(L.nsk_graph_create(C.byref(desc), C.byref(h)))
        self._handle = h
        self._keep = keep
        _lib.check(L.nsk_set_seed(h, self.seed, 0))
        if self.global_ids is not None and self.own_range is not None and len(self.global_ids):
            lo = int(self.own_range[0])
            tag = int(self.global_ids[lo]) if lo < len(self.global_ids) else int(self.global_ids[-1]) + 1
            _lib.check(L.nsk_set_rng_tag(h, tag & 0xFFFFFFFF))
        scan = {"chromatic": _lib.SCAN_CHROMATIC, "sequential": _lib.SCAN_SEQUENTIAL}[self.scan]
        _lib.check(L.nsk_set_scan(h, scan))
        _lib.check(L.nsk_set_learn_cap(h, self.learn_cap))
        _lib.check(L.nsk_set_learn_lag(h, int(self.learn_lag)))
        return h

    def close(self):
        if self._handle is not None:
            _lib.lib().nsk_graph_destroy(self._handle)
            self._handle = None
            self._clipped_seen = 0

    def invalidate(self):
        """Drop the compiled device graph: the next burnIn / inference / learn call recompiles it
        from the current contents of the structural arrays (the reference reads them on every
        sweep, e.g. after its master marks ownership with isEvidence == 4)."""
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_seed(self, seed, sweep0=0):
        self.seed = int(seed)
        if self._handle is not None:
            _lib.check(_lib.lib().nsk_set_seed(self._handle, self.seed, int(sweep0)))

    def info(self):
        inf = _lib.GraphInfo()
        _lib.check(_lib.lib().nsk_graph_get_info(self._engine(), C.byref(inf)))
        return {k: getattr(inf, k) for k, _ in inf._fields_}

    def layout(self):
        """Internal id of every variable (its index in the device's value arrays; for a sampled
        variable its position in the compiled layout = its generator id in the chromatic scan)."""
        iid = np.zeros(self.variable.shape[0], np.int32)
        nid = C.c_int64()
        _lib.check(_lib.lib().nsk_graph_get_layout(self._engine(), _lib.ptr(iid), C.byref(nid)))
        return iid.astype(np.int64)

    def generators(self):
        """The chromatic scan's generator of every variable (nsk_graph_get_generators): position in the
        compiled layout | quad-scheme flag << 40; -1 for variables this handle does not sample."""
        out = np.zeros(self.variable.shape[0], np.int64)
        _lib.check(_lib.lib().nsk_graph_get_generators(self._engine(), _lib.ptr(out)))
        return out

    def weight_slots(self):
        """Slot of every weight in the device table (nsk_graph_get_weight_slots); the identity unless the
        handle renumbered its single-factor weights."""
        out = np.zeros(self.weight.shape[0], np.int64)
        rc = _lib.lib().nsk_graph_get_weight_slots(self._engine(), _lib.ptr(out))
        if rc < 0:
            _lib.check(rc)
        return out

    def colors(self):
        out = np.zeros(self.variable.shape[0], np.int32)
        _lib.check(_lib.lib().nsk_graph_get_colors(self._engine(), _lib.ptr(out)))
        return out

    def _push(self, var_copy, weight_copy):
        if self._handle is not None and _lib.lib().nsk_get_chains(self._handle) != 1:
            _lib.check(_lib.lib().nsk_set_chains(self._handle, 1))      # back from var_copy="all": chain 0 only
        vv = _lib.as_c(self.var_value[var_copy], np.int64)
        ve = _lib.as_c(self.var_value_evid[var_copy], np.int64)
        wv = _lib.as_c(self.weight_value[weight_copy], np.float64)
        cnt = _lib.as_c(self.count, np.int64)
        _lib.check(_lib.lib().nsk_state_upload(self._engine(), _lib.ptr(vv), _lib.ptr(ve),
                                               _lib.ptr(wv), _lib.ptr(cnt)))

    def _pull(self, var_copy, weight_copy, values=True, weights=True, count=True):
        """Download state into the arrays the caller sees.  Straight into their memory when it is a
        C-contiguous array of the right type (the usual case: rows of ``var_value`` etc.) -- a fresh
        buffer per call costs more in page faults than the transfer itself (240 MB at 10M variables)."""
        def target(a, dtype, n):
            # (the library writes n elements: an array the caller replaced by a shorter one takes the
            # temporary buffer and fails in the assignment below, as it did in the reference)
            ok = (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous and a.flags.writeable
                  and a.shape == (n,))
            return (a, None) if ok else (np.empty(n, dtype), a)
        nv, nw, nc = self.variable.shape[0], self.weight.shape[0], int(self.cstart[-1]) if len(self.cstart) else 0
        vv, vv_to = target(self.var_value[var_copy], np.int64, nv) if values else (None, None)
        ve, ve_to = target(self.var_value_evid[var_copy], np.int64, nv) if values else (None, None)
        wv, wv_to = target(self.weight_value[weight_copy], np.float64, nw) if weights else (None, None)
        cnt, cnt_to = target(self.count, np.int64, nc) if count else (None, None)
        _lib.check(_lib.lib().nsk_state_download(self._engine(), _lib.ptr(vv), _lib.ptr(ve),
                                                 _lib.ptr(wv), _lib.ptr(cnt)))
        for buf, to in ((vv, vv_to), (ve, ve_to), (wv, wv_to), (cnt, cnt_to)):
            if to is not None:
                to[:] = buf

    # ------------------------------------------------------------------ reference API
    def clear(self):
        self.count[:] = 0
        self.chain_count[:] = 0

    def getWeights(self, weight_copy=0):
        return self.weight_value[weight_copy][:]

    def getMarginals(self, varIds=None):
        return self.marginals if not varIds else self.marginals[varIds]

    def diagnostics(self, epochs):
        print('Inference took %.03f sec.' % self.inference_total_time)
        epochs = epochs or 1
        bins = 10
        assert self.count.min(initial=0) >= 0
        assert self.count.max(initial=0) <= epochs
        which = np.minimum(self.count * bins // epochs, bins - 1)
        hist = np.bincount(which, minlength=bins)
        for i in range(bins):
            print("Prob. " + str(i / 10.0) + ".." + str((i + 1) / 10.0) + ": \
                  " + str(hist[i]) + " variables")

    def diagnosticsLearning(self, weight_copy=0):
        print('Learning epoch took %.03f sec.' % self.learning_epoch_time)
        print("Weights:")
        for i, w in enumerate(self.weight):
            print("    weightId:", i)
            print("        isFixed:", w["isFixed"])
            print("        weight: ", self.weight_value[weight_copy][i])
            print()

    def _sweep(self, nsweeps, sample_evidence, burnin):
        h = self._engine()
        _lib.check(_lib.lib().nsk_gibbs_sweeps(h, int(nsweeps), int(bool(sample_evidence)),
                                               int(bool(burnin))))

    def burnIn(self, epochs, sample_evidence, diagnostics=False, var_copy=0, weight_copy=0):
        """factorgraph.py:129-143 -- `epochs` sweeps that do not touch the tally.  ``var_copy="all"``:
        every row of ``var_value`` is one chain, all swept by the same calls (nsk_set_chains)."""
        if diagnostics:
            print("FACTOR " + str(self.fid) + ": STARTED BURN-IN...")
        if epochs > 0:
            if _all_copies(var_copy):
                self._push_chains(weight_copy, count=False)
                self._sweep(epochs, sample_evidence, True)
                self._pull_chains(count=False)
            else:
                self._push(var_copy, weight_copy)
                self._sweep(epochs, sample_evidence, True)
                self._pull(var_copy, weight_copy, weights=False, count=False)
        if diagnostics:
            print("FACTOR " + str(self.fid) + ": DONE WITH BURN-IN")

    def inference(self, burnin_epochs, epochs, sample_evidence=False, diagnostics=False,
                  var_copy=0, weight_copy=0):
        """factorgraph.py:145-175.  ``var_copy="all"``: one chain per row of ``var_value``; ``count``
        grows by the sum of the chains' tallies, ``chain_count`` keeps them apart, ``marginals`` pools
        them and ``rhat`` is the split-R-hat of every tally slot over this call's sweeps."""
        if _all_copies(var_copy):
            return self._inference_chains(burnin_epochs, epochs, sample_evidence, diagnostics, weight_copy)
        if burnin_epochs > 0:
            self.burnIn(burnin_epochs, sample_evidence, diagnostics=diagnostics,
                        var_copy=var_copy, weight_copy=weight_copy)
        if diagnostics:
            print("FACTOR " + str(self.fid) + ": STARTED INFERENCE")
        if epochs > 0:
            L, h = _lib.lib(), self._engine()
            self._push(var_copy, weight_copy)
            if diagnostics:     # per-epoch timing lines, like the reference prints them
                for ep in range(epochs):
                    with Timer() as timer:
                        self._sweep(1, sample_evidence, False)
                        _lib.check(L.nsk_synchronize(h))
                    self.inference_epoch_time = timer.interval
                    self.inference_total_time += timer.interval
                    print('Inference epoch #%d took %.03f sec.' % (ep, self.inference_epoch_time))
            else:
                with Timer() as timer:
                    self._sweep(epochs, sample_evidence, False)
                    _lib.check(L.nsk_synchronize(h))
                self.inference_epoch_time = timer.interval / epochs
                self.inference_total_time += timer.interval
            self._pull(var_copy, weight_copy, weights=False)
        if diagnostics:
            print("FACTOR " + str(self.fid) + ": DONE WITH INFERENCE")
        if epochs != 0:
            self.marginals = self.count / float(epochs)
        if diagnostics:
            self.diagnostics(epochs)

    # ------------------------------------------------------------------ several chains (var_copy="all")
    def _chains(self):
        """Point the handle at one chain per row of ``var_value``; returns the number of chains."""
        nchains = int(self.var_value.shape[0])
        L, h = _lib.lib(), self._engine()
        if L.nsk_get_chains(h) != nchains:
            _lib.check(L.nsk_set_chains(h, nchains))
        ncount = len(self.count)
        if not (isinstance(self.chain_count, np.ndarray) and self.chain_count.shape == (nchains, ncount)):
            self.chain_count = np.zeros((nchains, ncount), np.int64)
        return nchains

    def _push_chains(self, weight_copy, count=True):
        nchains = self._chains()
        L, h = _lib.lib(), self._engine()
        ve = _lib.as_c(self.var_value_evid[0], np.int64)
        wv = _lib.as_c(self.weight_value[weight_copy], np.float64)
        _lib.check(L.nsk_state_upload(h, None, _lib.ptr(ve), _lib.ptr(wv), None))
        vv = _lib.as_c(self.var_value, np.int64)
        cc = _lib.as_c(self.chain_count, np.int64) if count else None
        _lib.check(L.nsk_chains_upload(h, _lib.ptr(vv), _lib.ptr(cc)))
        return nchains

    def _pull_chains(self, values=True, count=True):
        """Download every chain's values into ``var_value`` (and returns the per-chain tallies)."""
        L, h = _lib.lib(), self._engine()
        vv = np.empty(self.var_value.shape, np.int64) if values else None
        cc = np.empty(self.chain_count.shape, np.int64) if count else None
        _lib.check(L.nsk_chains_download(h, _lib.ptr(vv), _lib.ptr(cc)))
        if values:
            self.var_value[:] = vv
        return cc

    def _inference_chains(self, burnin_epochs, epochs, sample_evidence, diagnostics, weight_copy):
        nchains = self._chains()
        if burnin_epochs > 0:
            self.burnIn(burnin_epochs, sample_evidence, diagnostics=diagnostics, var_copy="all",
                        weight_copy=weight_copy)
        if diagnostics:
            print("FACTOR " + str(self.fid) + ": STARTED INFERENCE")
        self.rhat = np.full(len(self.count), np.nan)
        if epochs > 0:
            L, h = _lib.lib(), self._engine()
            self._push_chains(weight_copy)
            # split-R-hat: the per-chain tallies after h and after 2 h sweeps (h = epochs // 2) give 2 R half-chains
            half = epochs // 2
            parts = [half, half, epochs - 2 * half] if half >= 2 else [epochs]
            snaps = [self.chain_count.copy()]
            ep = 0
            for k, n in enumerate(parts):
                if n == 0:
                    continue
                if diagnostics:
                    for _ in range(n):
                        with Timer() as timer:
                            self._sweep(1, sample_evidence, False)
                            _lib.check(L.nsk_synchronize(h))
                        self.inference_epoch_time = timer.interval
                        self.inference_total_time += timer.interval
                        print('Inference epoch #%d took %.03f sec.' % (ep, self.inference_epoch_time))
                        ep += 1
                else:
                    with Timer() as timer:
                        self._sweep(n, sample_evidence, False)
                        _lib.check(L.nsk_synchronize(h))
                    self.inference_epoch_time = timer.interval / n
                    self.inference_total_time += timer.interval
                if k < 2 and len(parts) > 1:
                    snaps.append(self._pull_chains(values=False))
            cc = self._pull_chains()
            self.count += (cc - snaps[0]).sum(axis=0)
            self.chain_count[:] = cc
            if len(snaps) == 3:
                self.rhat = split_rhat(np.concatenate([snaps[1] - snaps[0], snaps[2] - snaps[1]]), half)
        if diagnostics:
            print("FACTOR " + str(self.fid) + ": DONE WITH INFERENCE")
        if epochs != 0:
            self.marginals = self.count / float(epochs * nchains)
        if diagnostics:
            self.diagnostics(epochs * nchains)
            finite = self.rhat[np.isfinite(self.rhat)]
            print("Largest split R-hat over %d chains: %s" % (nchains, "%.4f" % finite.max() if len(finite) else "nan"))

    # ------------------------------------------------------------------ sample traces
    def sample(self, epochs, var_ids=None, thin=1, burnin_epochs=0, sample_evidence=False, var_copy=0,
               weight_copy=0, log_potential=False, weight_statistics=None, feature_scaled=False):
        """``inference(burnin_epochs, epochs, sample_evidence, var_copy=..., weight_copy=...)`` that also returns
        the joint samples: after every ``thin``-th tallied sweep the device records the values of ``var_ids``
        (any variables, any order; None = all) without returning to the host (nsk_trace_setup).  Returns an array
        ``(epochs // thin, chains, len(var_ids))`` of int8 or int32 (the handle's value type); one chain unless
        ``var_copy="all"``.  State, ``count``, ``chain_count``, ``marginals``, ``rhat`` and the timing attributes
        come out as ``inference`` leaves them, and the trace is torn down before the call returns.
        ``numbskull_amd.diagnostics`` computes autocorrelation and effective sample size of the result.
        ``log_potential=True`` returns ``(samples, lp)``: ``lp[i, r]``, float64 ``(epochs // thin, chains)``, is the
        log-potential of the whole state of chain ``r`` when row ``i`` was taken, whatever ``var_ids`` keeps --
        the doubles ``log_potential()`` gives for that state, evaluated on the device behind the row
        (nsk_trace_log_potential).
        ``weight_statistics=True`` or a list of weight ids (any order, repeats allowed) adds a LAST element to the
        returned tuple: float64 ``(epochs // thin, chains, nsel)``, the per-weight sufficient statistics
        ``weight_statistics()`` gives for the state of every row, evaluated on the device behind the row for the
        selected weights only (nsk_trace_weight_stats); ``feature_scaled`` as in ``weight_statistics``.
        ``numbskull_amd.diagnostics.moment_gap`` compares them with a target."""
        epochs, thin = int(epochs), int(thin)
        if thin < 1:
            raise ValueError("thin must be at least 1")
        stats_on = weight_statistics is not None and weight_statistics is not False
        wids = None
        if stats_on and weight_statistics is not True:
            wids = np.asarray(weight_statistics)
            if wids.ndim != 1 or wids.size == 0 or wids.dtype.kind not in "iu":
                raise ValueError("weight_statistics is True or a non-empty list of weight ids")
            if wids.min() < 0 or wids.max() >= self.weight.shape[0]:
                raise IndexError("weight_statistics: weight id out of range")
            wids = _lib.as_c(wids, np.int64)
        if feature_scaled and not stats_on:
            raise ValueError("feature_scaled goes with weight_statistics")
        L, h = _lib.lib(), self._engine()
        if burnin_epochs > 0:
            self.burnIn(burnin_epochs, sample_evidence, var_copy=var_copy, weight_copy=weight_copy)
        # the chain count of the call, before the trace is sized for it
        nchains = self._chains() if _all_copies(var_copy) else 1
        if L.nsk_get_chains(h) != nchains:
            _lib.check(L.nsk_set_chains(h, nchains))
        vids = None if var_ids is None else _lib.as_c(np.asarray(var_ids).reshape(-1), np.int64)
        ncols = self.variable.shape[0] if vids is None else len(vids)
        rows = epochs // thin
        dtype = np.int8 if self.info()["value_bytes"] == 1 else np.int32
        out = np.zeros((rows, nchains, ncols), dtype)
        traced = rows > 0 and ncols > 0         # (an empty result needs no trace)
        lp = np.zeros((rows, nchains), np.float64) if log_potential else None
        nsel = 0 if not stats_on else (self.weight.shape[0] if wids is None else len(wids))
        stats = np.zeros((rows, nchains, nsel), np.float64) if stats_on else None
        stats_traced = stats_on and nsel > 0
        if (log_potential or stats_traced) and rows > 0 and not traced:      # no columns asked for: the lp and stats columns ride on a one-column trace
            first = _lib.as_c(np.zeros(1), np.int64)
            _lib.check(L.nsk_trace_setup(h, _lib.ptr(first), 1, thin, rows))
            traced = True
        elif traced:
            _lib.check(L.nsk_trace_setup(h, _lib.ptr(vids), ncols, thin, rows))
        try:
            if traced and log_potential:
                _lib.check(L.nsk_trace_log_potential(h, 1))
            if traced and stats_traced:
                _lib.check(L.nsk_trace_weight_stats(h, _lib.ptr(wids), 0 if wids is None else nsel, 1 if feature_scaled else 0))
            self.inference(0, epochs, sample_evidence, var_copy=var_copy, weight_copy=weight_copy)
            if traced and ncols > 0:
                _lib.check(L.nsk_trace_download(h, 0, rows, _lib.ptr(out), None))
            if traced and log_potential:
                _lib.check(L.nsk_trace_download_log_potential(h, 0, rows, _lib.ptr(lp)))
            if traced and stats_traced:
                _lib.check(L.nsk_trace_download_weight_stats(h, 0, rows, _lib.ptr(stats)))
        except BaseException:
            if traced:
                L.nsk_trace_setup(h, None, 0, 1, 0)     # (its status must not replace the exception under way)
            raise
        if traced:
            _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
        if stats_on:
            return (out, lp, stats) if log_potential else (out, stats)
        return (out, lp) if log_potential else out

    def mixing(self, epochs, var_ids=None, thin=1, burnin_epochs=0, sample_evidence=False, max_lag=63):
        """How well every selected variable has mixed, computed on the device from the trace and without downloading
        a row: ``inference(burnin_epochs, epochs, sample_evidence, var_copy="all")`` -- one chain per row of
        ``var_value`` -- under a trace of ``var_ids`` (binary variables, any order, repeats allowed; None = all), a row
        after every ``thin``-th sweep, then nsk_trace_ess over the ``epochs // thin`` rows.  Returns the named tuple
        ``Mixing(ess, tau, rhat, mean, truncated, samples)``: per variable the effective sample size, the
        autocorrelation time, split R-hat, the mean and a uint8 flag, and the number of samples they rest on
        (``2 x (rows // 2) x chains``).  It is the estimator of ``diagnostics.effective_sample_size`` with the lags
        cut at ``max_lag`` (1 .. 63; the same estimator while ``rows // 2 <= max_lag + 1``): where ``truncated`` is 1
        the autocorrelation had not decayed inside the window, ``tau`` is a lower bound and ``ess`` an upper bound --
        thin more.  A constant column (an evidence variable) reads NaN.  With one chain, or fewer than 4 rows, every
        figure is NaN, as in ``diagnostics``.  State, ``count``, ``chain_count``, ``marginals`` and ``rhat`` come out
        as ``inference`` leaves them; the trace is torn down before the call returns.  ValueError when a selected
        variable is not binary."""
        epochs, thin, max_lag = int(epochs), int(thin), int(max_lag)
        if thin < 1:
            raise ValueError("thin must be at least 1")
        if max_lag < 1 or max_lag > 63:
            raise ValueError("max_lag must lie in [1, 63]")
        vids = None if var_ids is None else _lib.as_c(np.asarray(var_ids).reshape(-1), np.int64)
        if vids is not None and len(vids) and (vids.min() < 0 or vids.max() >= self.variable.shape[0]):
            raise IndexError("mixing: variable id out of range")
        card = self.variable["cardinality"] if vids is None else self.variable["cardinality"][vids]
        if (card != 2).any():
            raise ValueError("mixing: every selected variable must be binary (cardinality 2)")
        L, h = _lib.lib(), self._engine()
        if burnin_epochs > 0:
            self.burnIn(burnin_epochs, sample_evidence, var_copy="all")
        nchains = self._chains()
        ncols = self.variable.shape[0] if vids is None else len(vids)
        rows = epochs // thin
        mean, tau, rhat2 = (np.full(ncols, np.nan) for _ in range(3))
        truncated = np.zeros(ncols, np.uint8)
        measured = nchains >= 2 and rows >= 4 and ncols > 0
        if measured:
            _lib.check(L.nsk_trace_setup(h, _lib.ptr(vids), ncols, thin, rows))
        try:
            self.inference(0, epochs, sample_evidence, var_copy="all")
            if measured:
                _lib.check(L.nsk_trace_ess(h, 0, rows, max_lag, _lib.ptr(mean), _lib.ptr(tau), _lib.ptr(rhat2), _lib.ptr(truncated)))
        except BaseException:
            if measured:
                L.nsk_trace_setup(h, None, 0, 1, 0)     # (its status must not replace the exception under way)
            raise
        if measured:
            _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
        samples = 2 * (rows // 2) * nchains
        with np.errstate(invalid="ignore"):
            return Mixing(samples / tau, tau, np.sqrt(rhat2), mean, truncated, samples)

    def pairwise(self, epochs, pairs, thin=1, burnin_epochs=0, sample_evidence=False):
        """The joint marginal of pairs of variables, counted on the device from the trace and without downloading a
        row: ``inference(burnin_epochs, epochs, sample_evidence, var_copy="all")`` -- one chain per row of
        ``var_value``; one chain is fine -- under a trace of the distinct variables of ``pairs``, a row after every
        ``thin``-th sweep, then nsk_trace_pair_counts over the ``epochs // thin`` rows.  ``pairs`` is an ``(npairs, 2)``
        array of variable ids (binary variables; any order, repeats and ``a == b`` allowed) or the string
        ``"factors"``: the two ends of every arity-2 factor of the graph, in factor order
        (``diagnostics.factor_pairs``).  Returns ``diagnostics.pair_tables`` of the counts, the named tuple
        ``Pairwise(joint, cov, corr, mi, counts, samples)``: per pair the 2 x 2 table ``joint[j][value of a][value of
        b]``, covariance, correlation (NaN when a column is constant, an evidence variable for one) and mutual
        information in nats, the chains pooled; the per-chain integers ``counts`` ``(npairs, chains, 3)`` = n11, n1(a),
        n1(b); and ``samples = rows x chains``.  With zero rows or zero pairs the arrays are NaN or empty and no trace
        is set up.  State, ``count``, ``chain_count``, ``marginals`` and ``rhat`` come out as ``inference`` leaves them;
        the trace is torn down before the call returns.  ValueError when a variable of a pair is not binary, on
        ``thin < 1`` and on a bad shape; IndexError on an id out of range."""
        from .diagnostics import factor_pairs, pair_tables
        epochs, thin = int(epochs), int(thin)
        if thin < 1:
            raise ValueError("thin must be at least 1")
        if isinstance(pairs, str):
            if pairs != "factors":
                raise ValueError('pairwise: pairs is an (npairs, 2) array of variable ids or "factors"')
            pairs = factor_pairs(self.factor, self.fmap)
        pairs = np.asarray(pairs)
        if pairs.size == 0 and pairs.ndim <= 2:
            pairs = np.zeros((0, 2), np.int64)
        if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
            raise ValueError("pairwise: pairs have shape (npairs, 2) and an integer type, got %r %s" % (pairs.shape, pairs.dtype))
        pairs = pairs.astype(np.int64)
        if len(pairs) and (pairs.min() < 0 or pairs.max() >= self.variable.shape[0]):
            raise IndexError("pairwise: variable id out of range")
        vids, cols = np.unique(pairs, return_inverse=True)
        if (self.variable["cardinality"][vids] != 2).any():
            raise ValueError("pairwise: every variable of a pair must be binary (cardinality 2)")
        vids, cols = _lib.as_c(vids, np.int64), _lib.as_c(cols.reshape(-1, 2), np.int64)
        L, h = _lib.lib(), self._engine()
        if burnin_epochs > 0:
            self.burnIn(burnin_epochs, sample_evidence, var_copy="all")
        nchains = self._chains()
        rows = epochs // thin
        counts = np.zeros((len(pairs), nchains, 3), np.int64)
        measured = rows > 0 and len(pairs) > 0
        if measured:
            _lib.check(L.nsk_trace_setup(h, _lib.ptr(vids), len(vids), thin, rows))
        try:
            self.inference(0, epochs, sample_evidence, var_copy="all")
            if measured:
                _lib.check(L.nsk_trace_pair_counts(h, 0, rows, _lib.ptr(cols), len(cols), _lib.ptr(counts)))
        except BaseException:
            if measured:
                L.nsk_trace_setup(h, None, 0, 1, 0)     # (its status must not replace the exception under way)
            raise
        if measured:
            _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
        return pair_tables(counts, rows)

    def mixing_values(self, epochs, var_ids=None, indicators=None, thin=1, burnin_epochs=0, sample_evidence=False, max_lag=63):
        """``mixing`` for categorical variables: how well every selected VALUE of every selected variable has mixed,
        computed on the device from the trace and without downloading a row.  An indicator is a pair (variable id,
        value); its series is the 0 / 1 sequence ``x == value``, and the figures are those of ``mixing`` for that
        series (nsk_trace_value_ess; ``mean`` is the marginal of the value).  ``indicators`` is an ``(nind, 2)`` array
        of (variable id, value) -- any order, repeats allowed -- or None for every value ``0 .. cardinality - 1`` of
        every variable of ``var_ids`` in order (None = all variables); with ``indicators`` given ``var_ids`` is
        ignored.  Runs ``inference(burnin_epochs, epochs, sample_evidence, var_copy="all")`` under a trace of the
        distinct variables, a row after every ``thin``-th sweep.  Returns the named tuple ``MixingValues(ess, tau,
        rhat, mean, truncated, samples, var, value, offset)``: the first five are arrays of length ``nind``,
        ``var[i]`` and ``value[i]`` name indicator ``i``, and with ``indicators=None`` ``offset`` (length
        ``nvars + 1``) brackets each variable's run -- variable ``j`` of the selection is indicators
        ``offset[j] .. offset[j + 1] - 1`` -- else it is None.  NaN as in ``mixing``: one chain, fewer than 4 rows, a
        series that never changes (a value an evidence variable holds, or one no row holds).  State, ``count``,
        ``chain_count``, ``marginals`` and ``rhat`` come out as ``inference`` leaves them; the trace is torn down before
        the call returns.  ValueError when every traced variable is binary (the trace would be bit-packed: ``mixing``
        serves it), on ``thin < 1``, ``max_lag`` outside [1, 63], a bad shape and a value outside its variable's
        domain; IndexError on a variable id out of range."""
        epochs, thin, max_lag = int(epochs), int(thin), int(max_lag)
        if thin < 1:
            raise ValueError("thin must be at least 1")
        if max_lag < 1 or max_lag > 63:
            raise ValueError("max_lag must lie in [1, 63]")
        nvar = self.variable.shape[0]
        card = self.variable["cardinality"].astype(np.int64)
        offset = None
        if indicators is None:
            ids = np.arange(nvar, dtype=np.int64) if var_ids is None else np.asarray(var_ids).reshape(-1)
            if ids.size and ids.dtype.kind not in "iu":
                raise ValueError("mixing_values: var_ids are integers")
            ids = ids.astype(np.int64)
            if len(ids) and (ids.min() < 0 or ids.max() >= nvar):
                raise IndexError("mixing_values: variable id out of range")
            offset = np.concatenate([[0], np.cumsum(card[ids])]).astype(np.int64)
            var = np.repeat(ids, card[ids])
            value = np.arange(offset[-1], dtype=np.int64) - np.repeat(offset[:-1], card[ids])
        else:
            ind = np.asarray(indicators)
            if ind.size == 0 and ind.ndim <= 2:
                ind = np.zeros((0, 2), np.int64)
            if ind.ndim != 2 or ind.shape[1] != 2 or ind.dtype.kind not in "iu":
                raise ValueError("mixing_values: indicators have shape (nind, 2) and an integer type, got %r %s" % (ind.shape, ind.dtype))
            var, value = ind[:, 0].astype(np.int64), ind[:, 1].astype(np.int64)
            if len(var) and (var.min() < 0 or var.max() >= nvar):
                raise IndexError("mixing_values: variable id out of range")
            if ((value < 0) | (value >= card[var])).any():
                raise ValueError("mixing_values: a value lies outside its variable's domain")
        vids, cols = np.unique(var, return_inverse=True)
        if len(vids) and (card[vids] == 2).all():
            raise ValueError("mixing_values: every traced variable is binary (cardinality 2): the trace would be bit-packed, use mixing")
        nind = len(var)
        sel = _lib.as_c(np.stack([cols.reshape(-1), value], axis=1).reshape(-1, 2), np.int64)
        vids = _lib.as_c(vids, np.int64)
        L, h = _lib.lib(), self._engine()
        if burnin_epochs > 0:
            self.burnIn(burnin_epochs, sample_evidence, var_copy="all")
        nchains = self._chains()
        rows = epochs // thin
        mean, tau, rhat2 = (np.full(nind, np.nan) for _ in range(3))
        truncated = np.zeros(nind, np.uint8)
        measured = nchains >= 2 and rows >= 4 and nind > 0
        if measured:
            _lib.check(L.nsk_trace_setup(h, _lib.ptr(vids), len(vids), thin, rows))
        try:
            self.inference(0, epochs, sample_evidence, var_copy="all")
            if measured:
                _lib.check(L.nsk_trace_value_ess(h, 0, rows, max_lag, _lib.ptr(sel), nind, _lib.ptr(mean), _lib.ptr(tau), _lib.ptr(rhat2),
                                                 _lib.ptr(truncated)))
        except BaseException:
            if measured:
                L.nsk_trace_setup(h, None, 0, 1, 0)     # (its status must not replace the exception under way)
            raise
        if measured:
            _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
        samples = 2 * (rows // 2) * nchains
        with np.errstate(invalid="ignore"):
            return MixingValues(samples / tau, tau, np.sqrt(rhat2), mean, truncated, samples, var, value, offset)

    def contingency(self, epochs, pairs, thin=1, burnin_epochs=0, sample_evidence=False):
        """``pairwise`` for categorical variables: the ``K_a x K_b`` joint table of pairs of variables, counted on the
        device from the trace and without downloading a row.  ``pairs`` is as in ``pairwise``: an ``(npairs, 2)`` array
        of variable ids (any order, repeats and ``a == b`` allowed) or ``"factors"``.  Runs
        ``inference(burnin_epochs, epochs, sample_evidence, var_copy="all")`` under a trace of the distinct variables, a
        row after every ``thin``-th sweep, then nsk_trace_value_pair_counts on all ``K_a x K_b`` cells of every pair
        over the ``epochs // thin`` rows.  Returns ``diagnostics.contingency_tables`` of the counts, the named tuple
        ``Contingency(joint, mi, counts, samples)``: per pair the table ``joint[j][value of a][value of b]`` (a list;
        chains pooled), mutual information in nats, the per-chain integers ``(chains, K_a, K_b)`` and
        ``samples = rows x chains``.  With zero rows or zero pairs no trace is set up.  State, ``count``,
        ``chain_count``, ``marginals`` and ``rhat`` come out as ``inference`` leaves them; the trace is torn down before
        the call returns.  ValueError when every variable involved is binary (the trace would be bit-packed:
        ``pairwise`` serves it), on ``thin < 1`` and on a bad shape; IndexError on an id out of range."""
        from .diagnostics import contingency_tables, factor_pairs
        epochs, thin = int(epochs), int(thin)
        if thin < 1:
            raise ValueError("thin must be at least 1")
        if isinstance(pairs, str):
            if pairs != "factors":
                raise ValueError('contingency: pairs is an (npairs, 2) array of variable ids or "factors"')
            pairs = factor_pairs(self.factor, self.fmap)
        pairs = np.asarray(pairs)
        if pairs.size == 0 and pairs.ndim <= 2:
            pairs = np.zeros((0, 2), np.int64)
        if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
            raise ValueError("contingency: pairs have shape (npairs, 2) and an integer type, got %r %s" % (pairs.shape, pairs.dtype))
        pairs = pairs.astype(np.int64)
        if len(pairs) and (pairs.min() < 0 or pairs.max() >= self.variable.shape[0]):
            raise IndexError("contingency: variable id out of range")
        card = self.variable["cardinality"].astype(np.int64)
        vids, cols = np.unique(pairs, return_inverse=True)
        if len(vids) and (card[vids] == 2).all():
            raise ValueError("contingency: every variable involved is binary (cardinality 2): the trace would be bit-packed, use pairwise")
        cols = cols.reshape(-1, 2)
        shapes = card[pairs].reshape(-1, 2)
        # all cells of every pair, a pair's in row-major order (value of a, value of b)
        ncell = shapes[:, 0] * shapes[:, 1]
        pair_of = np.repeat(np.arange(len(pairs)), ncell)
        within = np.arange(int(ncell.sum()), dtype=np.int64) - np.repeat(np.cumsum(ncell) - ncell, ncell)
        kb = shapes[pair_of, 1]
        quads = _lib.as_c(np.stack([cols[pair_of, 0], within // kb, cols[pair_of, 1], within % kb], axis=1).reshape(-1, 4), np.int64)
        vids = _lib.as_c(vids, np.int64)
        L, h = _lib.lib(), self._engine()
        if burnin_epochs > 0:
            self.burnIn(burnin_epochs, sample_evidence, var_copy="all")
        nchains = self._chains()
        rows = epochs // thin
        counts = np.zeros((len(quads), nchains, 3), np.int64)
        measured = rows > 0 and len(quads) > 0
        if measured:
            _lib.check(L.nsk_trace_setup(h, _lib.ptr(vids), len(vids), thin, rows))
        try:
            self.inference(0, epochs, sample_evidence, var_copy="all")
            if measured:
                _lib.check(L.nsk_trace_value_pair_counts(h, 0, rows, _lib.ptr(quads), len(quads), _lib.ptr(counts)))
        except BaseException:
            if measured:
                L.nsk_trace_setup(h, None, 0, 1, 0)     # (its status must not replace the exception under way)
            raise
        if measured:
            _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
        return contingency_tables(counts[:, :, 0], shapes, rows)

    # ------------------------------------------------------------------ conditionals
    def _cond_selection(self, var_ids, default, what):
        """(ids or None for all variables, offsets of the "full" layout); argument errors before any device work."""
        nvar = self.variable.shape[0]
        card = self.variable["cardinality"].astype(np.int64)
        if var_ids is None and default is None:
            return None, np.concatenate([[0], np.cumsum(card)]).astype(np.int64)
        ids = np.asarray(default if var_ids is None else var_ids)
        if ids.ndim != 1 or (ids.size and ids.dtype.kind not in "iu"):
            raise ValueError("%s: var_ids is a one-dimensional list of integer variable ids, got %r %s" % (what, ids.shape, ids.dtype))
        ids = _lib.as_c(ids, np.int64)
        if len(ids) and (ids.min() < 0 or ids.max() >= nvar):
            raise IndexError("%s: variable id out of range" % what)
        return ids, np.concatenate([[0], np.cumsum(card[ids])]).astype(np.int64)

    def conditionals(self, var_ids=None, var_copy=0, weight_copy=0, evidence_chain=False, potentials=False):
        """The distribution the sampler draws each selected variable from, ``P(x_v = k | every other variable)``, evaluated
        on the device (nsk_conditionals).  ``var_ids``: variable ids, any order, repeats allowed; None = all.  Returns
        ``(offsets, values)``: int64 ``(nsel + 1,)`` and float64 ``(total,)`` -- selected variable ``i`` owns the
        ``cardinality`` entries ``values[offsets[i] : offsets[i + 1]]``, one per value (a binary variable owns 2;
        ``diagnostics.tally_layout`` converts to the layout of ``count``).  ``potentials=True`` returns the potentials
        ``p_k`` the sampler exponentiates instead of the probabilities ``exp(p_k) / sum_j exp(p_j)``
        (``diagnostics.conditional_probabilities`` turns one into the other).  The state is ``var_value[var_copy]`` --
        ``var_value_evid[var_copy]`` with ``evidence_chain=True`` -- under ``weight_value[weight_copy]``, pushed as
        ``log_potential`` pushes them; ``var_copy="all"`` gives ``(chains, total)``.  A variable this handle does not
        sample (``isEvidence == 4``) reads NaN.  The sums are unshifted, as the sampler's: potentials beyond exp's range
        give what IEEE gives (inf / inf = NaN)."""
        ids, offsets = self._cond_selection(var_ids, None, "conditionals")
        if _all_copies(var_copy) and evidence_chain:
            raise ValueError('the evidence chain exists once: var_copy="all" is for the free chains')
        total = int(offsets[-1])
        if total == 0:
            return offsets, np.zeros((self.var_value.shape[0], 0) if _all_copies(var_copy) else 0, np.float64)
        L, h = _lib.lib(), self._engine()
        what = 0 if potentials else 1
        nsel = 0 if ids is None else len(ids)
        if _all_copies(var_copy):
            nchains = self._push_chains(weight_copy, count=False)
            out = np.zeros((nchains, total), np.float64)
            _lib.check(L.nsk_conditionals(h, _lib.BUF_VALUE, 0, nchains, _lib.ptr(ids), nsel, what, _lib.ptr(out)))
            return offsets, out
        self._push(var_copy, weight_copy)
        out = np.zeros(total, np.float64)
        _lib.check(L.nsk_conditionals(h, _lib.BUF_VALUE_EVID if evidence_chain else _lib.BUF_VALUE, 0, 1, _lib.ptr(ids), nsel, what,
                                      _lib.ptr(out)))
        return offsets, out

    def log_pseudo_likelihood(self, var_ids=None, var_copy=0, weight_copy=0, evidence_chain=False):
        """The log-pseudo-likelihood of a state: the sum over the selected variables (None = those with
        ``isEvidence == 0``) of ``log P(x_v | every other variable)`` at the variable's own value -- the usual cheap score
        for comparing weight vectors where no enumeration reaches.  The potentials come from the device
        (``conditionals(potentials=True)``); the logarithms are taken on the host
        (``diagnostics.log_pseudo_likelihood``, shifted by each variable's largest potential).  Returns a float;
        ``var_copy="all"`` a float64 array with one entry per row of ``var_value``."""
        default = np.nonzero(self.variable["isEvidence"] == 0)[0] if var_ids is None else None
        ids, _ = self._cond_selection(var_ids, default, "log_pseudo_likelihood")
        if _all_copies(var_copy) and evidence_chain:
            raise ValueError('the evidence chain exists once: var_copy="all" is for the free chains')
        from .diagnostics import log_pseudo_likelihood
        offsets, pot = self.conditionals(ids, var_copy, weight_copy, evidence_chain, potentials=True)
        if _all_copies(var_copy):
            values = np.asarray(self.var_value)[:, ids]
        else:
            values = np.asarray((self.var_value_evid if evidence_chain else self.var_value)[var_copy])[ids]
        return log_pseudo_likelihood(offsets, pot, values.astype(np.int64))

    # ------------------------------------------------------------------ pseudo-likelihood gradient, MPLE learning
    def _pl_selection(self, var_ids, var_copy, evidence_chain, what):
        """The selection of ``log_pseudo_likelihood`` (None = the variables with ``isEvidence == 0``), as a set; argument
        errors before any device work."""
        default = np.nonzero(self.variable["isEvidence"] == 0)[0] if var_ids is None else None
        ids, _ = self._cond_selection(var_ids, default, what)
        if len(np.unique(ids)) != len(ids):
            raise ValueError("%s: a variable id is repeated (the selection is a set)" % what)
        if _all_copies(var_copy) and evidence_chain:
            raise ValueError('the evidence chain exists once: var_copy="all" is for the free chains')
        return ids

    def pl_gradient(self, var_ids=None, var_copy=0, weight_copy=0, evidence_chain=False, counts=False):
        """The gradient of ``log_pseudo_likelihood`` with respect to the weights, summed on the device
        (nsk_pl_gradient): for every weight the sum, over the selected variables ``v`` (None = those with
        ``isEvidence == 0``), their values ``k`` and the factors ``f`` of the weight in the list of ``(v, k)``, of
        ``((k == x_v) - P(x_v = k | the others)) * f(x with v at k)``.  Every term is rounded to a multiple of ``2**-32``
        and the terms are added as int64, so the result is exact to within ``2**-33`` per term and does not depend on the
        order of execution (``diagnostics.pl_gradient_counts`` is the rule in numpy).  State and weights are pushed as
        ``conditionals`` pushes them.  Returns float64 ``(nweight,)`` in the order of ``weight`` -- fixed weights
        included; ``var_copy="all"`` gives ``(chains, nweight)``, one row per row of ``var_value``.  ``counts=True``
        returns ``(int64 sums, skipped)`` instead: the raw sums (gradient ``= sums * 2.0**-32``) and the number of
        selected variables skipped because their value lies outside its domain or their normaliser is not a finite
        positive number (an array per chain for ``"all"``).  Repeated ids raise ValueError: the selection is a set.
        With the reference's literal head lookup this is the derivative of the sum of the sampler's own conditionals,
        which are then not those of one joint distribution."""
        ids = self._pl_selection(var_ids, var_copy, evidence_chain, "pl_gradient")
        L, h = _lib.lib(), self._engine()
        nw = self.weight.shape[0]
        if _all_copies(var_copy):
            nchains = self._push_chains(weight_copy, count=False)
            which, shape = _lib.BUF_VALUE, (nchains, nw)
        else:
            self._push(var_copy, weight_copy)
            nchains, which, shape = 1, (_lib.BUF_VALUE_EVID if evidence_chain else _lib.BUF_VALUE), (nw,)
        gq, skipped = np.zeros(shape, np.int64), np.zeros(nchains, np.int64)
        if len(ids):
            _lib.check(L.nsk_pl_gradient(h, which, 0, nchains, _lib.ptr(ids), len(ids), _lib.ptr(gq), None, _lib.ptr(skipped)))
        if counts:
            return gq, (skipped if _all_copies(var_copy) else int(skipped[0]))
        return gq.astype(np.float64) * 2.0 ** -32

    # ------------------------------------------------------------------ what the full-batch learners share
    @staticmethod
    def _learn_steps(what, epochs, stepsize, decay, reg_param, max_epochs=65536, also=(False, "")):
        """(epochs, stepsize, decay, reg_param) converted and checked: epochs in [1, max_epochs] (None: the learner's own
        bound covers them), then ``also`` = (fails, message), a learner's own bound, then the rates"""
        epochs = int(epochs)
        if max_epochs is not None and (epochs < 1 or epochs > max_epochs):
            raise ValueError("%s: epochs must lie in [1, %d]" % (what, max_epochs))
        if also[0]:
            raise ValueError(also[1])
        stepsize, decay, reg_param = float(stepsize), float(decay), float(reg_param)
        if not (np.isfinite(stepsize) and np.isfinite(decay) and np.isfinite(reg_param)) or reg_param < 0:
            raise ValueError("%s: stepsize, decay and reg_param must be finite, reg_param not negative" % what)
        return epochs, stepsize, decay, reg_param

    def _learn_target(self, what, target):
        """an explicit target checked, None: the statistics of the evidence chain"""
        if target is None:
            return self.weight_moments(evidence_chain=True)
        target = np.ascontiguousarray(target, np.float64)
        if target.shape != self.weight.shape or not np.isfinite(target).all():
            raise ValueError("%s: target is finite float64 (nweight,) = (%d,)" % (what, self.weight.shape[0]))
        return target

    def _factors_per_weight(self):
        return np.bincount(self.factor["weightId"].astype(np.int64), minlength=self.weight.shape[0]).astype(np.int64)

    def learn_mple(self, epochs, stepsize, decay=1.0, reg_param=0.0, var_ids=None, var_copy=0, weight_copy=0,
                   evidence_chain=False):
        """Maximum pseudo-likelihood learning on the device (nsk_mple_steps): ``epochs`` steps of gradient ascent on the
        mean log-pseudo-likelihood of fully observed data, ``w += step * (pl_gradient / n - reg_param * w)`` with
        ``step = stepsize * decay**t`` -- deterministic, no sampling, every chain an example.  The data are
        ``var_value[var_copy]`` (``var_value_evid[var_copy]`` with ``evidence_chain=True``); ``var_copy="all"`` makes
        every row of ``var_value`` a training example.  ``var_ids`` selects the variables whose conditionals count
        (None = those with ``isEvidence == 0``; repeats raise ValueError).  State and weights are pushed as
        ``conditionals`` pushes them; all steps run on the device without returning to the host, and the learned weights
        are pulled back into ``weight_value[weight_copy]``, as ``learn`` does.  Fixed weights stay.  Nothing else
        changes: values, ``count`` and the generator are as before.  Returns a dict: ``grad_max`` -- float64
        ``(epochs,)``, the largest magnitude of the mean gradient over the weights that are not fixed at the weights
        each step started from (without the penalty); ``skipped`` -- int64 ``(epochs,)``, the variables skipped in each
        step, summed over the examples (see ``pl_gradient``); ``n`` -- selected variables with a position x examples
        (``diagnostics.mple_step`` is the update in numpy)."""
        epochs, stepsize, decay, reg_param = self._learn_steps("learn_mple", epochs, stepsize, decay, reg_param)
        ids = self._pl_selection(var_ids, var_copy, evidence_chain, "learn_mple")
        L, h = _lib.lib(), self._engine()
        if _all_copies(var_copy):
            nchains, which = self._push_chains(weight_copy, count=False), _lib.BUF_VALUE
        else:
            self._push(var_copy, weight_copy)
            nchains, which = 1, (_lib.BUF_VALUE_EVID if evidence_chain else _lib.BUF_VALUE)
        n = int(np.count_nonzero(self.variable["isEvidence"][ids] != 4)) * nchains
        gmax, skipped = np.zeros(epochs, np.int64), np.zeros(epochs, np.int64)
        if n > 0:
            _lib.check(L.nsk_mple_steps(h, which, 0, nchains, _lib.ptr(ids), len(ids), epochs, stepsize, decay, reg_param,
                                        _lib.ptr(gmax), _lib.ptr(skipped)))
            self._pull(0 if _all_copies(var_copy) else var_copy, weight_copy, values=False, count=False)
        grad_max = gmax.astype(np.float64) * 2.0 ** -32 / n if n > 0 else np.zeros(epochs)
        return {"grad_max": grad_max, "skipped": skipped, "n": n}

    # ------------------------------------------------------------------ chain-summed moments, PCD learning
    def weight_moments(self, var_copy=0, evidence_chain=False, counts=False, chains=None):
        """The mean per-weight statistics of chains, summed on the device in fixed point (nsk_weight_moments): every
        factor value is rounded to a multiple of ``2**-32`` and added as int64 into ONE sum per weight, whatever the
        number of chains, so the result is exact to within ``2**-33`` per factor and does not depend on the order of
        execution (``diagnostics.moment_counts`` is the rule in numpy).  The state is ``var_value[var_copy]`` --
        ``var_value_evid[var_copy]`` with ``evidence_chain=True`` --, pushed as ``weight_statistics`` pushes it;
        ``var_copy="all"`` sums over every row of ``var_value``.  Returns float64 ``(nweight,)`` in the order of
        ``weight``: the sums ``* 2.0**-32 / chains``, equal to ``weight_statistics(...)`` averaged over the chains where the
        factor values are integers.  ``counts=True`` returns ``(int64 sums, chains)`` instead.  A weight without a
        factor reads 0; ``featureValue`` plays no part.  ``chains=(first, n)`` sums over the rows ``first .. first + n - 1``
        of ``var_value`` alone (``var_copy`` is then not read): one population of ``learn_pcd(clamped=K)``."""
        first = 0
        if chains is not None:
            if evidence_chain:
                raise ValueError("the evidence chain exists once: chains=(first, n) names rows of var_value")
            first, n = (int(x) for x in chains)
            if first < 0 or n < 1 or first + n > int(self.var_value.shape[0]):
                raise ValueError("weight_moments: chains=(first, n) must name rows of var_value, n at least 1")
            var_copy = "all"
        if _all_copies(var_copy) and evidence_chain:
            raise ValueError('the evidence chain exists once: var_copy="all" is for the free chains')
        L, h = _lib.lib(), self._engine()
        if _all_copies(var_copy):
            nchains, which = self._push_chains(0, count=False), _lib.BUF_VALUE
            if chains is not None:
                nchains = n
        else:
            self._push(var_copy, 0)
            nchains, which = 1, (_lib.BUF_VALUE_EVID if evidence_chain else _lib.BUF_VALUE)
        m = np.zeros(self.weight.shape[0], np.int64)
        _lib.check(L.nsk_weight_moments(h, which, first, nchains, _lib.ptr(m)))
        if counts:
            return m, nchains
        return m.astype(np.float64) * 2.0 ** -32 / np.float64(nchains)

    def learn_pcd(self, epochs, stepsize, decay=1.0, reg_param=0.0, sweeps=1, sample_evidence=True, target=None,
                  normalize=True, weight_copy=0, moments=False, clamped=0, clamp=True):
        """Maximum-likelihood learning by persistent contrastive divergence on the device (nsk_pcd_steps).  The rows of
        ``var_value`` are the persistent chains ("fantasy particles"); each of the ``epochs`` steps sweeps all of them
        ``sweeps`` times under the current weights (burn-in sweeps: nothing is tallied), sums their per-weight statistics
        exactly (``weight_moments``) and moves every weight that is not fixed along ``target - model mean``:
        ``w += step * ((target - mean) / n_w - reg_param * w)`` with ``step = stepsize * decay**t`` and ``n_w`` the number
        of factors of the weight (``normalize=False``: no division).  Nothing returns to the host between steps.  Its
        fixed point is where the model's mean statistics equal the target -- the maximum-likelihood estimate when the
        target is the data's mean statistics -- unlike ``learn_mple``, which maximises the pseudo-likelihood, and unlike
        ``learn``, which takes one clipped SGD step per variable visit.

        ``target`` (nweight,) are the statistics to match; None means those of the evidence chain,
        ``weight_moments(evidence_chain=True)``, which is right for FULLY OBSERVED data.  ``sample_evidence=True`` lets the
        chains sample every variable (the free phase).

        With LATENT variables the target moves with the weights: it is the mean statistics of chains that sample the
        latent variables with the evidence held.  ``clamped=K > 0`` (nsk_pcd_latent_steps) makes the first ``K`` rows of
        ``var_value`` that clamped population and the other rows the free one; ``target`` must then be None.  Every step
        sweeps the clamped rows ``sweeps`` times with the evidence held, then the free rows ``sweeps`` times under
        ``sample_evidence``, and moves the weights along ``clamped mean - free mean`` by the same rule
        (``diagnostics.pcd_latent_step``).  ``clamp=True`` first writes ``initialValue`` into every evidence variable
        (``isEvidence`` 1, 2 or 3) of the clamped rows; ``clamp=False`` trusts the rows as they are -- each may hold the
        evidence of another training example.  Both populations persist across steps and calls.

        The chains are pushed as ``inference(var_copy="all")`` pushes them, without the tally; afterwards ``var_value``
        holds every chain's state and ``weight_value[weight_copy]`` the learned weights.  ``count`` is untouched.
        Returns a dict: ``grad_max`` -- float64 ``(epochs,)``, the largest ``|target - mean|`` (divided by ``n_w`` with
        ``normalize``) over the weights that are not fixed, at the weights each step swept under; ``target``; ``chains``;
        ``factors_per_weight`` -- int64 ``(nweight,)``; and with ``moments=True`` ``moments`` -- int64 ``(epochs,
        nweight)``, every step's sums (``diagnostics.pcd_step`` is the update in numpy).  With ``clamped=K``
        ``target`` is None, the dict gains ``clamped`` and ``moments`` is ``(epochs, 2, nweight)``: the clamped rows' sums, then the
        free rows'."""
        epochs, sweeps = int(epochs), int(sweeps)
        epochs, stepsize, decay, reg_param = self._learn_steps("learn_pcd", epochs, stepsize, decay, reg_param, also=(
            sweeps < 1 or epochs * sweeps > 2 ** 31 - 1, "learn_pcd: sweeps must be at least 1 and epochs x sweeps at most 2**31 - 1"))
        nw = self.weight.shape[0]
        clamped = int(clamped)
        if clamped != 0:
            if clamped < 1 or clamped > int(self.var_value.shape[0]) - 1:
                raise ValueError("learn_pcd: clamped must lie in [1, rows of var_value - 1]: a clamped and a free population")
            if target is not None:
                raise ValueError("learn_pcd: with clamped rows the target is their statistics; target must be None")
            if 2 * epochs * sweeps > 2 ** 31 - 1:
                raise ValueError("learn_pcd: 2 x epochs x sweeps must be at most 2**31 - 1 with clamped rows")
        else:
            target = self._learn_target("learn_pcd", target)
        L, h = _lib.lib(), self._engine()
        nchains = self._push_chains(weight_copy, count=False)
        gmax = np.zeros(epochs, np.float64)
        rows = np.zeros((epochs, 2, nw) if clamped else (epochs, nw), np.int64) if moments else None
        tail = (epochs, sweeps, int(bool(sample_evidence)), stepsize, decay, reg_param, int(bool(normalize)), _lib.ptr(gmax), _lib.ptr(rows))
        if clamped:
            _lib.check(L.nsk_pcd_latent_steps(h, clamped, int(bool(clamp)), *tail))
        else:
            _lib.check(L.nsk_pcd_steps(h, _lib.ptr(target), *tail))
        self._pull_chains(count=False)
        self._pull(0, weight_copy, values=False, count=False)
        out = {"grad_max": gmax, "target": target, "chains": nchains, "factors_per_weight": self._factors_per_weight()}
        if clamped:
            out["clamped"] = clamped
        if moments:
            out["moments"] = rows
        return out

    def rao_blackwell(self, epochs, var_ids=None, thin=1, burnin_epochs=0, sample_evidence=False):
        """Rao-Blackwellised marginals: ``inference(burnin_epochs, epochs, sample_evidence, var_copy="all")`` -- one chain
        per row of ``var_value``; one chain is fine -- during which, after every ``thin``-th tallied sweep, the device adds
        the conditionals ``P(x_v = k | the others)`` of every selected variable in every chain's state to running sums
        (nsk_trace_conditionals; no row leaves the device).  Their average estimates the same marginals as
        ``count / epochs`` at lower variance for the same sweeps.  ``var_ids``: variable ids, any order, repeats allowed;
        None = the variables the call samples.  Returns a dict: ``offsets`` (the layout of ``conditionals``),
        ``per_chain`` ``(chains, total)`` = sums / rows, ``marginals`` ``(total,)`` their mean over chains, ``stderr`` the
        standard deviation over chains divided by ``sqrt(chains)`` (NaN with one chain), ``rows = epochs // thin``.
        With zero rows or an empty selection the figures are NaN and no trace is set up.  State, ``count``,
        ``chain_count``, ``marginals`` and ``rhat`` come out as ``inference`` leaves them; the trace is torn down before
        the call returns."""
        epochs, thin = int(epochs), int(thin)
        if thin < 1:
            raise ValueError("thin must be at least 1")
        if epochs < 0:
            raise ValueError("epochs must not be negative")
        default = None
        if var_ids is None:
            ev = self.variable["isEvidence"]
            default = np.nonzero((ev != 4) if sample_evidence else (ev == 0))[0]
        ids, offsets = self._cond_selection(var_ids, default, "rao_blackwell")
        total = int(offsets[-1])
        L, h = _lib.lib(), self._engine()
        if burnin_epochs > 0:
            self.burnIn(burnin_epochs, sample_evidence, var_copy="all")
        nchains = self._chains()
        rows = epochs // thin
        sums = np.full((nchains, total), np.nan)
        got = C.c_int64(0)
        measured = rows > 0 and total > 0
        if measured:
            first = _lib.as_c(np.zeros(1), np.int64)            # the accumulators ride on a one-column trace
            _lib.check(L.nsk_trace_setup(h, _lib.ptr(first), 1, thin, rows))
        try:
            if measured:
                _lib.check(L.nsk_trace_conditionals(h, _lib.ptr(ids), len(ids)))
            self.inference(0, epochs, sample_evidence, var_copy="all")
            if measured:
                _lib.check(L.nsk_trace_download_conditionals(h, _lib.ptr(sums), C.byref(got)))
        except BaseException:
            if measured:
                L.nsk_trace_setup(h, None, 0, 1, 0)     # (its status must not replace the exception under way)
            raise
        if measured:
            _lib.check(L.nsk_trace_setup(h, None, 0, 1, 0))
        per_chain = sums / float(got.value) if measured else sums
        with np.errstate(invalid="ignore"):
            stderr = per_chain.std(axis=0, ddof=1) / np.sqrt(nchains) if nchains > 1 else np.full(total, np.nan)
        return {"offsets": offsets, "per_chain": per_chain, "marginals": per_chain.mean(axis=0), "stderr": stderr,
                "rows": int(got.value)}

    # ------------------------------------------------------------------ greedy MAP search
    def icm(self, max_sweeps=100, var_copy=0, weight_copy=0, evidence_chain=False, sample_evidence=False):
        """Iterated conditional modes on the device (nsk_icm): greedy coordinate ascent from ``var_value[var_copy]`` --
        ``var_value_evid[var_copy]`` with ``evidence_chain=True`` -- under ``weight_value[weight_copy]``, pushed as
        ``log_potential`` pushes them.  A sweep visits the colour classes in the chromatic scan's order; every variable
        with ``isEvidence == 0`` (every sampled variable with ``sample_evidence``) takes the value of largest potential
        given the others -- moving on strict improvement only, the smallest value among several maxima
        (``diagnostics.icm_choice`` is the rule in numpy).  Deterministic: no random numbers are drawn.  Up to
        ``max_sweeps`` (1 .. 4096) sweeps; the state reached replaces the row it started from, and nothing else changes
        (``count``, weights, the generator).  ``var_copy="all"`` polishes every row of ``var_value``, each on its own.
        Returns a dict: ``sweeps`` -- the sweeps run up to and including the first without a change, ``max_sweeps`` when
        every sweep changed something; ``converged`` -- whether a sweep without a change was reached (with the
        reference's literal head lookup the potentials are not the gradient of one energy, and cycles are possible);
        ``changed`` -- int64 ``(max_sweeps,)``, the changes of every sweep, 0 from the fixed point on.  For one copy an
        int, a bool and that array; for ``"all"`` arrays ``(chains,)``, ``(chains,)`` and ``(chains, max_sweeps)``."""
        max_sweeps = int(max_sweeps)
        if max_sweeps < 1 or max_sweeps > 4096:
            raise ValueError("icm: max_sweeps must lie in [1, 4096]")
        if _all_copies(var_copy) and evidence_chain:
            raise ValueError('the evidence chain exists once: var_copy="all" is for the free chains')
        L, h = _lib.lib(), self._engine()
        ev = int(bool(sample_evidence))
        if _all_copies(var_copy):
            nchains = self._push_chains(weight_copy, count=False)
            sweeps, changed = np.zeros(nchains, np.int64), np.zeros((nchains, max_sweeps), np.int64)
            _lib.check(L.nsk_icm(h, _lib.BUF_VALUE, 0, nchains, max_sweeps, ev, _lib.ptr(sweeps), _lib.ptr(changed)))
            self._pull_chains(count=False)
            return {"sweeps": np.abs(sweeps), "converged": sweeps > 0, "changed": changed}
        self._push(var_copy, weight_copy)
        sweeps, changed = np.zeros(1, np.int64), np.zeros(max_sweeps, np.int64)
        _lib.check(L.nsk_icm(h, _lib.BUF_VALUE_EVID if evidence_chain else _lib.BUF_VALUE, 0, 1, max_sweeps, ev, _lib.ptr(sweeps),
                             _lib.ptr(changed)))
        self._pull(var_copy, weight_copy, weights=False, count=False)
        return {"sweeps": abs(int(sweeps[0])), "converged": bool(sweeps[0] > 0), "changed": changed}

    def map_estimate(self, epochs, thin=1, burnin_epochs=0, sample_evidence=False, max_sweeps=100):
        """A MAP estimate: the most probable labelling the chains can find.  Runs ``sample(epochs, thin=thin,
        burnin_epochs=burnin_epochs, sample_evidence=sample_evidence, var_copy="all", log_potential=True)`` -- one chain
        per row of ``var_value``, all variables recorded -- takes every chain's best recorded row
        (``diagnostics.best_sample``), loads those rows as the chains' states, polishes them with ``icm(max_sweeps,
        var_copy="all")`` and evaluates ``log_potential(var_copy="all")``.  Returns a dict for the best polished chain:
        ``values`` (its state, int64 ``(nvar,)``), ``log_potential``, ``chain``, ``sampled_log_potential`` (that of the
        chain's best recorded row, before polishing), ``sweeps`` and ``converged`` (as ``icm``); and for all chains the
        arrays ``log_potentials`` and ``sampled_log_potentials``.  ``var_value`` is left holding the polished states;
        ``count``, ``chain_count``, ``marginals`` and ``rhat`` come out as ``inference`` leaves them.  ValueError when
        ``epochs // thin`` is 0: there is no recorded row to start from."""
        from .diagnostics import best_sample
        epochs, thin = int(epochs), int(thin)
        if thin < 1:
            raise ValueError("thin must be at least 1")
        if epochs // thin < 1:
            raise ValueError("map_estimate: epochs // thin must be at least 1 (no row would be recorded)")
        samples, lp = self.sample(epochs, None, thin, burnin_epochs, sample_evidence, var_copy="all", log_potential=True)
        nchains = samples.shape[1]
        rows = np.array([best_sample(lp[:, r:r + 1])[0] for r in range(nchains)])
        sampled = lp[rows, np.arange(nchains)]
        self.var_value[:] = samples[rows, np.arange(nchains)]
        res = self.icm(max_sweeps, var_copy="all", sample_evidence=sample_evidence)
        after = self.log_potential(var_copy="all")
        chain = int(np.argmax(after))
        return {"values": np.array(self.var_value[chain], np.int64), "log_potential": float(after[chain]), "chain": chain,
                "sampled_log_potential": float(sampled[chain]), "sweeps": int(res["sweeps"][chain]),
                "converged": bool(res["converged"][chain]), "log_potentials": after, "sampled_log_potentials": sampled}

    # ------------------------------------------------------------------ tempered schedules: log Z, annealing
    @staticmethod
    def _schedule(betas, what):
        b = np.ascontiguousarray(betas, np.float64)
        if b.ndim != 1 or len(b) < 1:
            raise ValueError("%s: betas is a 1-d schedule of at least one inverse temperature" % what)
        if not (np.isfinite(b).all() and (b >= 0).all()):
            raise ValueError("%s: an inverse temperature is negative, infinite or NaN" % what)
        return b

    def tempered_sweeps(self, betas, sweeps=1, sample_evidence=False, weight_copy=0, best=False):
        """Sweeps under a schedule of inverse temperatures, driven on the device (nsk_tempered_sweeps): for every
        ``betas[t]`` in turn the weights are scaled by it, ``sweeps`` burn-in sweeps run on every chain -- one chain per
        row of ``var_value``, pushed and pulled as ``icm(var_copy="all")`` does, under ``weight_value[weight_copy]`` --
        and every chain's log-potential under the UNSCALED weights is taken.  Sampling at beta is sampling under the weight
        table beta x w, so step t draws from ``exp(betas[t] U) / Z``; nothing is tallied (``count`` stays) and the weights
        come back as they were.  Returns a dict: ``log_potentials`` float64 ``(T, chains)``, the log-potential after
        every step, with the bits ``log_potential`` gives for that state; ``log_weights`` ``(chains,)``, the sum over
        ``t + 1 < T`` of ``(betas[t + 1] - betas[t]) * log_potentials[t]`` (``diagnostics.ais_log_weights``: with a
        schedule from 0 to 1 the log importance weights of annealed importance sampling); with ``best=True`` also
        ``best_values`` int64 ``(chains, nvar)`` and ``best_log_potentials`` ``(chains,)``, each chain's state of largest
        log-potential over the steps (the earliest among equals), kept on the device.  ``var_value`` is left holding the
        final states.  The schedule's order is free: annealing goes past 1."""
        b = self._schedule(betas, "tempered_sweeps")
        sweeps = int(sweeps)
        if sweeps < 1:
            raise ValueError("tempered_sweeps: sweeps must be at least 1")
        L, h = _lib.lib(), self._engine()
        nchains = self._push_chains(weight_copy, count=False)
        lp, logw = np.zeros((len(b), nchains), np.float64), np.zeros(nchains, np.float64)
        bv = np.zeros((nchains, self.variable.shape[0]), np.int64) if best else None
        bu = np.zeros(nchains, np.float64) if best else None
        _lib.check(L.nsk_tempered_sweeps(h, _lib.ptr(b), len(b), sweeps, int(bool(sample_evidence)), _lib.ptr(logw), _lib.ptr(lp),
                                         _lib.ptr(bv), _lib.ptr(bu)))
        self._pull_chains(count=False)
        out = {"log_weights": logw, "log_potentials": lp}
        if best:
            out["best_values"], out["best_log_potentials"] = bv, bu
        return out

    def smc_sweeps(self, betas, sweeps=1, threshold=0.5, seed=0, sample_evidence=False, weight_copy=0):
        """Population annealing, driven on the device (nsk_smc_sweeps): ``tempered_sweeps`` along ``betas`` with the
        resampling step of sequential Monte Carlo behind the fold of every step but the last.  When the effective sample
        size of the folded log-weights falls below ``threshold x chains`` the heavy chains are copied over the light ones
        -- systematic resampling, decided, drawn and copied on the device -- and the log-weights start again from 0.
        ``threshold`` lies in [0, 1]; 0 never resamples.  The one uniform a step needs comes from
        ``np.random.default_rng(seed).random(T - 1)``.  Chains are pushed and pulled as ``tempered_sweeps`` does; nothing
        is tallied, the weights come back as they were, ``var_value`` is left holding the final states.  Returns a dict:
        ``log_potentials`` float64 ``(T, chains)``; ``log_weights`` ``(chains,)``, the fold since the last resampling;
        ``logw_pre`` ``(T - 1, chains)``, the log-weights in front of every decision; ``ancestors`` int32 ``(T - 1,
        chains)``, the chain whose state slot r holds after step t (itself where nothing was copied); ``resampled``
        bool ``(T - 1,)``; ``offsets`` ``(T - 1,)``.  ``diagnostics.smc_resample`` restates the rule and
        ``diagnostics.smc_estimate`` turns the result into log Z."""
        b = self._schedule(betas, "smc_sweeps")
        sweeps = int(sweeps)
        if sweeps < 1:
            raise ValueError("smc_sweeps: sweeps must be at least 1")
        threshold = float(threshold)
        if not 0.0 <= threshold <= 1.0:
            raise ValueError("smc_sweeps: the threshold lies in [0, 1]")
        T = len(b)
        offsets = np.ascontiguousarray(np.random.default_rng(seed).random(T - 1), np.float64)
        L, h = _lib.lib(), self._engine()
        nchains = self._push_chains(weight_copy, count=False)
        lp, logw = np.zeros((T, nchains), np.float64), np.zeros(nchains, np.float64)
        pre = np.zeros((T - 1, nchains), np.float64)
        anc, flag = np.zeros((T - 1, nchains), np.int32), np.zeros(T - 1, np.int32)
        _lib.check(L.nsk_smc_sweeps(h, _lib.ptr(b), T, sweeps, int(bool(sample_evidence)), threshold, _lib.ptr(offsets),
                                    _lib.ptr(logw), _lib.ptr(lp), _lib.ptr(pre), _lib.ptr(anc), _lib.ptr(flag)))
        self._pull_chains(count=False)
        return {"log_weights": logw, "log_potentials": lp, "logw_pre": pre, "ancestors": anc, "resampled": flag != 0,
                "offsets": offsets}

    def parallel_tempering(self, betas, steps, sweeps=1, seed=0, sample_evidence=False, weight_copy=0, target=None):
        """Parallel tempering, driven on the device (nsk_pt_sweeps): replica exchange between the chains.  One chain per
        row of ``var_value``, pushed and pulled as ``tempered_sweeps`` does; chain r stays at ``betas[r]`` (``len(betas)``
        must equal the number of rows: ValueError) for all ``steps`` steps.  A step sweeps every chain ``sweeps`` times
        under its own temperature, takes every chain's log-potential under the unscaled weights and proposes to swap the
        STATES of neighbouring chains -- pairs (0, 1), (2, 3), ... at even steps, (1, 2), (3, 4), ... at odd ones -- each
        accepted with probability ``min(1, exp((betas[r] - betas[r + 1]) (U[r + 1] - U[r])))``, decided and exchanged on
        the device.  Temperatures do not move, so a chain at beta = 1 samples the target throughout while the hot chains
        carry it between its modes (``diagnostics.pt_ladder`` makes a ladder that ends there).  The uniforms come from
        ``np.random.RandomState(seed).random_sample((steps, chains - 1))``.  With ``target=r`` the sweeps of chain r are
        tallied: ``count`` grows by its tally and ``chain_count[r]`` keeps it, as after ``inference(var_copy="all")``;
        without, nothing is tallied.  The weights come back as they were and ``var_value`` is left holding the final
        states.  Returns a dict: ``lp`` float64 ``(steps, chains)``, the log-potentials behind every step's sweeps and in
        front of its swaps; ``accepted`` int32 ``(steps, chains - 1)``, 1, 0, or -1 for a pair not proposed at that step;
        ``swap_rate`` ``(chains - 1,)``, accepted over proposed per pair (NaN for a pair never proposed); ``paths`` and
        ``round_trips`` (``diagnostics.pt_paths``); ``uniforms``.  ``diagnostics.pt_swap_rule`` restates the decision."""
        from .diagnostics import pt_paths
        b = self._schedule(betas, "parallel_tempering")
        nchains = int(self.var_value.shape[0])
        if len(b) != nchains:
            raise ValueError("parallel_tempering: %d inverse temperatures for %d chains (rows of var_value)" % (len(b), nchains))
        steps, sweeps = int(steps), int(sweeps)
        if steps < 1 or sweeps < 1:
            raise ValueError("parallel_tempering: steps and sweeps must be at least 1")
        tally = -1 if target is None else int(target)
        if not -1 <= tally < nchains or (target is not None and tally < 0):
            raise ValueError("parallel_tempering: target is None or a chain in [0, %d)" % nchains)
        uniforms = np.ascontiguousarray(np.random.RandomState(seed).random_sample((steps, nchains - 1)), np.float64)
        L, h = _lib.lib(), self._engine()
        self._push_chains(weight_copy, count=tally >= 0)
        before = self.chain_count.copy()
        lp = np.zeros((steps, nchains), np.float64)
        acc = np.zeros((steps, nchains - 1), np.int32)
        _lib.check(L.nsk_pt_sweeps(h, _lib.ptr(b), steps, sweeps, int(bool(sample_evidence)), _lib.ptr(uniforms), tally,
                                   _lib.ptr(lp), _lib.ptr(acc)))
        cc = self._pull_chains(count=tally >= 0)
        if tally >= 0:
            self.count += (cc - before).sum(axis=0)
            self.chain_count[:] = cc
        proposed, taken = (acc >= 0).sum(axis=0), (acc == 1).sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            rate = np.where(proposed > 0, taken / np.maximum(proposed, 1), np.nan)
        paths, trips = pt_paths(acc)
        return {"lp": lp, "accepted": acc, "swap_rate": rate, "paths": paths, "round_trips": trips, "uniforms": uniforms}

    def _log_z0(self, sample_evidence):
        """the log of the number of states of the variables a sweep samples"""
        sampled = self.colors() >= 0
        if not sample_evidence:
            sampled &= np.asarray(self.variable["isEvidence"]) == 0
        return float(np.log(np.asarray(self.variable["cardinality"], np.float64)[sampled]).sum())

    def _log_partition_smc(self, b, sweeps, sample_evidence, weight_copy, resample):
        from .diagnostics import smc_estimate, thermodynamic_integral
        res = self.smc_sweeps(b, sweeps, resample, 0, sample_evidence, weight_copy)
        log_z0 = self._log_z0(sample_evidence)
        log_z, ess, events = smc_estimate(res["logw_pre"], res["resampled"], res["log_weights"], log_z0)
        return {"log_z": log_z, "stderr": float("nan"), "ess": ess, "log_z0": log_z0, "log_weights": res["log_weights"],
                "log_z_ti": thermodynamic_integral(b, res["log_potentials"], log_z0), "betas": b, "resamplings": events}

    def log_partition(self, steps=100, betas=None, sweeps=1, sample_evidence=False, weight_copy=0, resample=None):
        """log Z by annealed importance sampling (Neal 2001), the chains of ``var_value`` as the particles:
        ``tempered_sweeps`` along ``betas`` -- ``np.linspace(0, 1, steps + 1)`` unless given; a schedule must start at 0.0
        and end at 1.0 (ValueError, raised before the device is touched) -- and ``diagnostics.ais_estimate`` of the
        log-weights.  The first step's sweeps, at beta = 0, draw every sampled variable uniformly, so the rows of
        ``var_value`` need no preparation.  With ``sample_evidence=False`` Z is the partition function with the evidence
        variables clamped at their current values, with ``True`` the free one.  Returns a dict: ``log_z``; ``stderr``
        (NaN for one chain) and ``ess``, the effective number of chains behind the estimate (``diagnostics.ais_estimate``);
        ``log_z0`` = the sum of log(cardinality) over the variables the sweeps sample; ``log_weights``; ``log_z_ti``, the
        thermodynamic integral of the same log-potentials, an independent cross-check; ``betas``.  ``log Z -
        log_potential`` of a state is its negative log-likelihood.  Meaningless where ``potential()`` is not the gradient
        of one energy: the reference's literal head lookup of IMPLY_MLN-type functions (see ``icm``).
        ``resample``: ``None`` is plain AIS as above; a threshold in (0, 1] is population annealing -- ``smc_sweeps(betas,
        sweeps, threshold=resample)`` and ``diagnostics.smc_estimate``: chains are resampled on the device whenever the
        effective sample size falls below ``resample x chains``, which keeps the estimate from resting on one heavy
        chain where the couplings are strong.  The dict then has the same keys with ``stderr`` NaN (one run of a
        resampled population has no honest error bar; repeat it), ``ess`` and ``log_weights`` those of the last stage,
        and ``resamplings``, the number of events."""
        from .diagnostics import ais_estimate, thermodynamic_integral
        if resample is not None:
            resample = float(resample)
            if not 0.0 < resample <= 1.0:
                raise ValueError("log_partition: resample is None or a threshold in (0, 1]")
        if betas is None:
            steps = int(steps)
            if steps < 1:
                raise ValueError("log_partition: steps must be at least 1")
            b = np.linspace(0.0, 1.0, steps + 1)
        else:
            b = self._schedule(betas, "log_partition")
            if len(b) < 2 or b[0] != 0.0 or b[-1] != 1.0:
                raise ValueError("log_partition: the schedule must start at 0.0 and end at 1.0")
        if resample is not None:
            return self._log_partition_smc(b, sweeps, sample_evidence, weight_copy, resample)
        res = self.tempered_sweeps(b, sweeps, sample_evidence, weight_copy)
        log_z0 = self._log_z0(sample_evidence)
        log_z, stderr, ess = ais_estimate(res["log_weights"], log_z0)
        return {"log_z": log_z, "stderr": stderr, "ess": ess, "log_z0": log_z0, "log_weights": res["log_weights"],
                "log_z_ti": thermodynamic_integral(b, res["log_potentials"], log_z0), "betas": b}

    def log_evidence(self, steps=100, betas=None, sweeps=1, weight_copy=0, resample=None):
        """log P(the evidence variables hold their values in ``var_value``) = log Z with the evidence clamped minus log Z
        with every variable free: two ``log_partition`` runs from the same rows.  Every row of ``var_value`` must hold
        the same evidence values (the clamped Z is one number).  Returns a dict: ``log_evidence``; ``stderr``, the root of
        the two squared errors; ``clamped`` and ``free``, the two ``log_partition`` results.  ``var_value`` is restored to
        what it held before the call.  ``resample``: as in ``log_partition``, for both runs (``stderr`` is then NaN)."""
        keep = np.array(self.var_value, np.int64)
        try:
            clamped = self.log_partition(steps, betas, sweeps, False, weight_copy, resample)
            self.var_value[:] = keep
            free = self.log_partition(steps, betas, sweeps, True, weight_copy, resample)
        finally:
            self.var_value[:] = keep
        return {"log_evidence": clamped["log_z"] - free["log_z"],
                "stderr": float(np.sqrt(clamped["stderr"] ** 2 + free["stderr"] ** 2)), "clamped": clamped, "free": free}

    def anneal(self, betas, sweeps=1, sample_evidence=False, max_sweeps=100):
        """A MAP search that can leave a basin: simulated annealing with the best state tracked on the device.  Runs
        ``tempered_sweeps(betas, sweeps, sample_evidence, best=True)`` -- a schedule that rises past 1 cools the chains --
        loads every chain's best state, polishes it with ``icm(max_sweeps, var_copy="all")`` and evaluates
        ``log_potential(var_copy="all")``.  No trace is set up: nothing but the best states is kept.  Returns the dict
        ``map_estimate`` returns; ``sampled_log_potential(s)`` are the best ones kept on the device, before polishing.
        ``var_value`` is left holding the polished states; ``count`` is untouched."""
        res = self.tempered_sweeps(betas, sweeps, sample_evidence, best=True)
        sampled = res["best_log_potentials"]
        self.var_value[:] = res["best_values"]
        pol = self.icm(max_sweeps, var_copy="all", sample_evidence=sample_evidence)
        after = self.log_potential(var_copy="all")
        chain = int(np.argmax(after))
        return {"values": np.array(self.var_value[chain], np.int64), "log_potential": float(after[chain]), "chain": chain,
                "sampled_log_potential": float(sampled[chain]), "sweeps": int(pol["sweeps"][chain]),
                "converged": bool(pol["converged"][chain]), "log_potentials": after, "sampled_log_potentials": sampled}

    # ------------------------------------------------------------------ per-weight statistics
    def weight_statistics(self, var_copy=0, evidence_chain=False, feature_scaled=False):
        """The sufficient statistics of a state: for every weight the sum of the values of its factors (the
        log-potential's sum split by weight), evaluated on the device (nsk_weight_stats); with ``feature_scaled`` every
        factor value is multiplied by the factor's ``featureValue`` first.  The state is ``var_value[var_copy]`` --
        ``var_value_evid[var_copy]`` with ``evidence_chain=True`` -- pushed as ``log_potential`` pushes it.  Returns
        float64 ``(nweight,)``, in the order of ``weight``; ``var_copy="all"`` ``(chains, nweight)``.  A weight without a
        factor reads 0.  The sums are reproducible: equal states give equal doubles, whichever chain holds them."""
        if _all_copies(var_copy) and evidence_chain:
            raise ValueError('the evidence chain exists once: var_copy="all" is for the free chains')
        L, h = _lib.lib(), self._engine()
        nw, scaled = self.weight.shape[0], 1 if feature_scaled else 0
        if _all_copies(var_copy):
            nchains = self._push_chains(0, count=False)
            out = np.zeros((nchains, nw), np.float64)
            _lib.check(L.nsk_weight_stats(h, _lib.BUF_VALUE, 0, nchains, scaled, _lib.ptr(out)))
            return out
        self._push(var_copy, 0)
        out = np.zeros(nw, np.float64)
        _lib.check(L.nsk_weight_stats(h, _lib.BUF_VALUE_EVID if evidence_chain else _lib.BUF_VALUE, 0, 1, scaled, _lib.ptr(out)))
        return out

    # ------------------------------------------------------------------ belief propagation
    def belief_propagation(self, max_iters=100, damping=0.0, tol=1e-9, var_copy=0, weight_copy=0, evidence_chain=False,
                           sample_evidence=False, factor_beliefs=False):
        """Loopy belief propagation on the device (nsk_bp_setup / nsk_bp_run): sum-product message passing, every factor
        and every variable updated once per iteration -- deterministic inference beside the sampler.  The variables with
        ``isEvidence != 0`` are clamped at their values in ``var_value[var_copy]`` (``var_value_evid[var_copy]`` with
        ``evidence_chain=True``) unless ``sample_evidence``; state and ``weight_value[weight_copy]`` are pushed as
        ``log_potential`` pushes them, and nothing of the graph changes.  Exact where the free variables form a forest;
        on a graph with cycles the beliefs and ``log_z`` (the Bethe estimate) are approximations and the iteration may
        not converge: raise ``damping`` (in [0, 1)) then, and read ``converged``.  At most ``max_iters`` (1 .. 4096)
        iterations; they stop behind the first whose largest message change is ``<= tol``.  A factor takes part with
        at most 16 distinct members and 4096 table entries over its free members; UFO and, without ``head_by_vid``, the
        IMPLY_MLN-type factors are refused (ValueError naming the factor).  Two hard constraints that contradict each
        other give NaN, as in ``conditionals``.  ``diagnostics.bp_iterate`` is the rule in numpy.
        Returns a dict: ``offsets``, ``beliefs`` -- the layout of ``conditionals`` over all variables
        (``diagnostics.tally_layout`` converts to that of ``count``); ``iters``, ``converged``, ``residual`` (float64
        ``(max_iters,)``, 0 behind the stop); ``log_z``; with ``factor_beliefs=True`` also ``table_offsets``
        (nfactor + 1), ``theta`` and ``factor_beliefs``."""
        from .diagnostics import bethe_log_z
        max_iters = int(max_iters)
        if max_iters < 1 or max_iters > 4096:
            raise ValueError("belief_propagation: max_iters must lie in [1, 4096]")
        if _all_copies(var_copy):
            raise ValueError('belief_propagation serves one state: var_copy="all" is for the sampler')
        L, h = _lib.lib(), self._engine()
        self._push(var_copy, weight_copy)
        info = _lib.BpInfo()
        _lib.check(L.nsk_bp_setup(h, _lib.BUF_VALUE_EVID if evidence_chain else _lib.BUF_VALUE, 0, int(bool(sample_evidence)),
                                  C.byref(info)))
        try:
            iters, residual = C.c_int64(0), np.zeros(max_iters, np.float64)
            _lib.check(L.nsk_bp_run(h, max_iters, float(damping), float(tol), C.byref(iters), _lib.ptr(residual)))
            _, offsets = self._cond_selection(None, None, "belief_propagation")
            beliefs = np.zeros(int(offsets[-1]), np.float64)
            _lib.check(L.nsk_bp_beliefs(h, None, 0, _lib.ptr(beliefs)))
            theta, fb = np.zeros(info.ntable, np.float64), np.zeros(info.ntable, np.float64)
            _lib.check(L.nsk_bp_download(h, _lib.BP_THETA, _lib.ptr(theta)))
            _lib.check(L.nsk_bp_download(h, _lib.BP_FACTOR_BELIEFS, _lib.ptr(fb)))
            table_off, edge_var = np.zeros(self.factor.shape[0] + 1, np.int64), np.zeros(info.nedges, np.int64)
            _lib.check(L.nsk_bp_layout(h, _lib.ptr(table_off), None, _lib.ptr(edge_var), None))
        finally:
            L.nsk_bp_clear(h)
        ev = self.variable["isEvidence"]
        layout = {"card": self.variable["cardinality"].astype(np.int64), "edge_var": edge_var,
                  "clamped": (ev == 4) | ((ev != 0) & (not sample_evidence))}
        out = {"offsets": offsets, "beliefs": beliefs, "iters": abs(int(iters.value)), "converged": bool(iters.value > 0),
               "residual": residual, "log_z": bethe_log_z(layout, theta, fb, beliefs)}
        if factor_beliefs:
            out.update(table_offsets=table_off, theta=theta, factor_beliefs=fb)
        return out

    def bp_weight_moments(self, max_iters=100, damping=0.0, tol=1e-9, var_copy=0, weight_copy=0, evidence_chain=False,
                          sample_evidence=False, counts=False):
        """The expected per-weight statistics ``E[S_w]`` under belief propagation (nsk_bp_setup / nsk_bp_run /
        nsk_bp_moments): the sum over every factor of a weight and every entry of its table of factor belief x factor
        value, reduced on the device in the int64 fixed point of ``weight_moments`` -- exact to within ``2**-33`` per table
        entry wherever BP is exact (the free variables form a forest), the Bethe approximation on a graph with cycles.
        State, weights, clamping and the iteration's arguments are those of ``belief_propagation``.  A factor whose
        beliefs are NaN (two contradicting hard constraints) is left out and counted.  ``diagnostics.bp_moment_counts`` is
        the rule in numpy.  Returns a dict: ``moments`` -- float64 ``(nweight,)``, the sums ``* 2.0**-32``, or the int64
        sums with ``counts=True``; ``iters``, ``converged`` as ``belief_propagation`` returns them; ``skipped``.  On a state
        where every variable is clamped ``moments`` equal ``weight_moments`` of it."""
        max_iters = int(max_iters)
        if max_iters < 1 or max_iters > 4096:
            raise ValueError("bp_weight_moments: max_iters must lie in [1, 4096]")
        if _all_copies(var_copy):
            raise ValueError('bp_weight_moments serves one state: var_copy="all" is for the sampler')
        L, h = _lib.lib(), self._engine()
        self._push(var_copy, weight_copy)
        _lib.check(L.nsk_bp_setup(h, _lib.BUF_VALUE_EVID if evidence_chain else _lib.BUF_VALUE, 0, int(bool(sample_evidence)), None))
        try:
            iters, skipped = C.c_int64(0), C.c_int64(0)
            _lib.check(L.nsk_bp_run(h, max_iters, float(damping), float(tol), C.byref(iters), None))
            m = np.zeros(self.weight.shape[0], np.int64)
            _lib.check(L.nsk_bp_moments(h, _lib.ptr(m), C.byref(skipped)))
        finally:
            L.nsk_bp_clear(h)
        return {"moments": m if counts else m.astype(np.float64) * 2.0 ** -32, "iters": abs(int(iters.value)),
                "converged": bool(iters.value > 0), "skipped": int(skipped.value)}

    def learn_bp(self, epochs, stepsize, decay=1.0, reg_param=0.0, iters=20, damping=0.0, tol=1e-9, warm=True,
                 sample_evidence=True, target=None, normalize=True, var_copy=0, weight_copy=0, moments=False, latent=False):
        """Maximum-likelihood learning whose model expectations come from belief propagation instead of chains
        (nsk_bp_learn_steps): EXACT maximum likelihood where the free variables form a forest -- chains, stars, graphs
        that the evidence separates --, the Bethe approximation on a graph with cycles; no sampling noise, no chain
        count, no generator state, reproducible bit for bit.  Each of the ``epochs`` steps rebuilds the tables from the
        current weights, runs up to ``iters`` BP iterations (from the previous step's messages with ``warm``, from
        ``1 / cardinality`` without; they stop behind the first whose largest message change is ``<= tol``), takes
        ``bp_weight_moments`` and moves every weight that is not fixed as ``learn_pcd`` does:
        ``w += step * ((target - E[S_w]) / n_w - reg_param * w)`` with ``step = stepsize * decay**t``
        (``normalize=False``: no division by the factor count ``n_w``).  Nothing returns to the host between steps.

        Its signals: ``converged`` says per step whether the iterations reached ``tol`` -- where they do not on a graph
        with cycles, raise ``damping`` (in [0, 1)) or ``iters``; the gradient of a step that did not converge is that of
        the messages as they stood.  ``target`` (nweight,) are the statistics to match; None means those of the evidence
        chain, ``weight_moments(evidence_chain=True)``, which is right for FULLY OBSERVED data, as in ``learn_pcd``.
        ``sample_evidence=True`` frees every variable with a position (the free phase).

        ``latent=True`` is learning with LATENT variables (nsk_bp_latent_steps), the noise-free counterpart of
        ``learn_pcd(clamped=K)``: two set-ups of the same state live on the device, one with the evidence held and the
        other variables free (the positive phase), one with everything free (the negative phase); each step runs both --
        in the same launches -- and moves the weights along the difference of their Bethe moments,
        ``w += step * ((E[S_w | evidence] - E[S_w]) / n_w - reg_param * w)``, which ascends the Bethe estimate of the
        evidence's log-probability (``bp_log_evidence``; exact on forests).  ``target`` must be None then and
        ``sample_evidence`` is not read.  The dict has no ``target``; ``iters``, ``converged`` and ``skipped`` have the
        shape ``(epochs, 2)``, ``residual`` ``(epochs, 2, iters)`` and ``moments`` ``(epochs, 2, nweight)``, index 0 of
        the pair axis the clamped set-up, each set-up stopping at ``tol`` on its own
        (``diagnostics.pcd_latent_step`` with ``K = Rf = 1`` is the update in numpy).

        The state ``var_value[var_copy]`` and ``weight_value[weight_copy]`` are pushed as ``belief_propagation`` pushes
        them; afterwards ``weight_value[weight_copy]`` holds the learned weights, and the set-up is cleared whatever
        happens.  Values and ``count`` are untouched.  Returns a dict: ``grad_max`` -- float64 ``(epochs,)``, the largest
        ``|target - E[S_w]|`` (divided by ``n_w`` with ``normalize``) over the weights that are not fixed, at the weights
        each step ran under; ``iters`` (epochs,) the iterations each step ran; ``converged`` (epochs,) bool;
        ``residual`` (epochs, iters); ``skipped`` (epochs,) the factors left out for NaN beliefs; ``target``;
        ``factors_per_weight``; with ``moments=True`` also ``moments`` -- int64 ``(epochs, nweight)``
        (``diagnostics.bp_moment_counts``; ``diagnostics.pcd_step`` with ``R=1`` is the update in numpy)."""
        epochs, iters = int(epochs), int(iters)
        epochs, stepsize, decay, reg_param = self._learn_steps("learn_bp", epochs, stepsize, decay, reg_param, None, (
            epochs < 1 or epochs > 4096 or iters < 1 or iters > 4096 or epochs * iters > 65536,
            "learn_bp: epochs and iters must lie in [1, 4096], epochs x iters at most 65536"))
        if _all_copies(var_copy):
            raise ValueError('learn_bp serves one state: var_copy="all" is for the sampler')
        nw = self.weight.shape[0]
        if latent and target is not None:
            raise ValueError("learn_bp: latent=True takes no target (the clamped set-up's moments are the positive phase)")
        if not latent:
            target = self._learn_target("learn_bp", target)
        L, h = _lib.lib(), self._engine()
        # latent: slot 0 the clamped set-up, slot 1 the free one, and a pair axis in what is kept per set-up; else the selected slot
        slots, pair = ((0, 1), (2,)) if latent else ((L.nsk_bp_selected(h),), ())
        self._push(var_copy, weight_copy)
        try:
            for slot in slots:
                _lib.check(L.nsk_bp_select(h, slot))
                _lib.check(L.nsk_bp_setup(h, _lib.BUF_VALUE, 0, slot if latent else int(bool(sample_evidence)), None))
            gmax, ran, skipped = np.zeros(epochs, np.float64), np.zeros((epochs,) + pair, np.int64), np.zeros((epochs,) + pair, np.int64)
            residual = np.zeros((epochs,) + pair + (iters,), np.float64)
            rows = np.zeros((epochs,) + pair + (nw,), np.int64) if moments else None
            args = (epochs, iters, float(damping), float(tol), int(bool(warm)), stepsize, decay, reg_param, int(bool(normalize)),
                    _lib.ptr(gmax), _lib.ptr(ran), _lib.ptr(residual), _lib.ptr(rows), _lib.ptr(skipped))
            _lib.check(L.nsk_bp_latent_steps(h, *args) if latent else L.nsk_bp_learn_steps(h, _lib.ptr(target), *args))
            self._pull(var_copy, weight_copy, values=False, count=False)
        finally:
            for slot in reversed(slots):            # (latent: slot 0 stays selected)
                L.nsk_bp_select(h, slot)
                L.nsk_bp_clear(h)
        out = {"grad_max": gmax, "iters": np.abs(ran), "converged": ran > 0, "residual": residual, "skipped": skipped}
        if not latent:
            out["target"] = target
        out["factors_per_weight"] = self._factors_per_weight()
        if moments:
            out["moments"] = rows
        return out

    def bp_log_evidence(self, max_iters=100, damping=0.0, tol=1e-9, var_copy=0, weight_copy=0):
        """The Bethe estimate of ``log P(the evidence variables' values)`` under ``weight_value[weight_copy]``:
        ``log_z`` of ``belief_propagation`` with the evidence held minus ``log_z`` with everything free
        (``sample_evidence=True``), two runs composed on the host.  It is the objective ``learn_bp(latent=True)``
        ascends; exact where the graph is a forest and both runs converge, an approximation on a graph with cycles.
        The arguments are those of ``belief_propagation``.  Returns a dict: ``log_evidence``, ``log_z_clamped``,
        ``log_z_free``, ``converged`` -- bool ``(2,)`` -- and ``iters`` -- int64 ``(2,)`` --, the clamped run first."""
        runs = [self.belief_propagation(max_iters, damping, tol, var_copy, weight_copy, sample_evidence=sev) for sev in (False, True)]
        lz = [float(r["log_z"]) for r in runs]
        return {"log_evidence": lz[0] - lz[1], "log_z_clamped": lz[0], "log_z_free": lz[1],
                "converged": np.array([r["converged"] for r in runs], np.bool_), "iters": np.array([r["iters"] for r in runs], np.int64)}

    # ------------------------------------------------------------------ log-potential
    def log_potential(self, var_copy=0, weight_copy=0, evidence_chain=False):
        """The unnormalised log-probability of a state: the sum over all factors of weight x factor value, evaluated
        on the device (nsk_log_potential).  The state is ``var_value[var_copy]`` -- ``var_value_evid[var_copy]``
        with ``evidence_chain=True`` -- under ``weight_value[weight_copy]``, pushed as ``inference`` pushes them.
        Returns a float; ``var_copy="all"`` a float64 array with one entry per row of ``var_value``.  The sum is
        reproducible: equal states under equal weights give equal doubles, whichever chain holds them."""
        L, h = _lib.lib(), self._engine()
        if _all_copies(var_copy):
            if evidence_chain:
                raise ValueError('the evidence chain exists once: var_copy="all" is for the free chains')
            nchains = self._push_chains(weight_copy, count=False)
            out = np.zeros(nchains, np.float64)
            _lib.check(L.nsk_log_potential(h, _lib.BUF_VALUE, 0, nchains, _lib.ptr(out)))
            return out
        self._push(var_copy, weight_copy)
        out = np.zeros(1, np.float64)
        _lib.check(L.nsk_log_potential(h, _lib.BUF_VALUE_EVID if evidence_chain else _lib.BUF_VALUE, 0, 1, _lib.ptr(out)))
        return float(out[0])

    def factor_values(self, var_copy=0, evidence_chain=False):
        """The value of every factor on ``var_value[var_copy]`` (``var_value_evid[var_copy]`` with
        ``evidence_chain=True``): float64 ``(nfactor,)`` in the order of ``factor`` -- what the reference's
        ``eval_factor`` returns for the state as it is, head quirks included (nsk_factor_values)."""
        L, h = _lib.lib(), self._engine()
        self._push(var_copy, 0)
        out = np.zeros(self.factor.shape[0], np.float64)
        _lib.check(L.nsk_factor_values(h, _lib.BUF_VALUE_EVID if evidence_chain else _lib.BUF_VALUE, 0, _lib.ptr(out)))
        return out

    def learn(self, burnin_epochs, epochs, stepsize, decay, regularization, reg_param, truncation,
              diagnostics=False, verbose=False, learn_non_evidence=False, var_copy=0,
              weight_copy=0):
        """factorgraph.py:177-208."""
        if _all_copies(var_copy):
            raise ValueError('learning samples one chain: var_copy="all" is for burnIn / inference only')
        if burnin_epochs > 0:
            self.burnIn(burnin_epochs, True, diagnostics=diagnostics, var_copy=var_copy,
                        weight_copy=weight_copy)
        if diagnostics:
            print("FACTOR " + str(self.fid) + ": STARTED LEARNING")
        if epochs > 0:
            L, h = _lib.lib(), self._engine()
            self._push(var_copy, weight_copy)
            args = (int(regularization), float(reg_param), int(truncation),
                    int(bool(learn_non_evidence)))
            if diagnostics:
                for ep in range(epochs):
                    print("FACTOR " + str(self.fid) + ": EPOCH #" + str(ep))
                    print("Current stepsize = " + str(stepsize))
                    if verbose:
                        self._pull(var_copy, weight_copy, values=False, count=False)
                        self.diagnosticsLearning(weight_copy)
                    sys.stdout.flush()
                    with Timer() as timer:
                        _lib.check(L.nsk_learn_sweeps(h, 1, float(stepsize), float(decay), *args))
                        _lib.check(L.nsk_synchronize(h))
                    self.learning_epoch_time = timer.interval
                    self.learning_total_time += timer.interval
                    stepsize *= decay
            else:
                with Timer() as timer:
                    _lib.check(L.nsk_learn_sweeps(h, int(epochs), float(stepsize), float(decay),
                                                  *args))
                    _lib.check(L.nsk_synchronize(h))
                self.learning_epoch_time = timer.interval / epochs
                self.learning_total_time += timer.interval
            self._pull(var_copy, weight_copy, count=False)
            # Chromatic learning applies the SGD rule once per colour class and caps visits * step
            # of a weight at `learn_cap` (a weight tied to many factors then moves more slowly per
            # epoch than under the reference's per-visit rule, learning.py:110-125; same fixed
            # point).  Say so instead of leaving it to a counter nobody reads.
            clipped = self.info()["learn_clipped"]
            if self.scan == "chromatic" and clipped > self._clipped_seen:
                msg = ("numbskull_amd: %d weight update(s) used a step below stepsize because one "
                       "colour class visits the weight more than learn_cap / stepsize = %g times "
                       "(learn_cap=%g; pass learn_cap=0 for the uncapped batch rule, or "
                       "scan='sequential' for the reference's per-visit trajectory)"
                       % (clipped - self._clipped_seen, self.learn_cap / max(stepsize, 1e-300),
                          self.learn_cap))
                warnings.warn(msg, RuntimeWarning, stacklevel=2)
                if diagnostics:
                    print(msg)
            self._clipped_seen = clipped
        if diagnostics:
            print("FACTOR " + str(self.fid) + ": DONE WITH LEARNING")

    def dump_weights(self, fout, weight_copy=0):
        """<wid, weight> text file (factorgraph.py:210-214)."""
        w = self.weight_value[weight_copy]
        with open(fout, 'w') as out:
            out.write("".join('%d %f\n' % (i, w[i]) for i in range(self.weight.shape[0])))

    def dump_probabilities(self, fout, epochs):
        """<vid, value, prob> text file (factorgraph.py:216-229): binary variables print the
        probability of value 1, others one line per domain value (written natively,
        nsk_write_probabilities)."""
        epochs = epochs or 1
        v, vm = _lib.as_c(self.variable), _lib.as_c(self.vmap)
        cs, cnt = _lib.as_c(self.cstart, np.int64), _lib.as_c(self.count, np.int64)
        _lib.check(_lib.lib().nsk_write_probabilities(str(fout).encode(), len(v), _lib.ptr(v), _lib.ptr(vm),
                                                      len(vm), _lib.ptr(cs), _lib.ptr(cnt), len(cnt),
                                                      float(epochs)))

