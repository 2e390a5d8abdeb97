"""Diagnostics over a sample trace (``FactorGraph.sample``): autocorrelation and effective sample size.

Pure numpy, no GPU.  A trace is an array of shape ``(samples, chains, columns)``; every function works per
column.  The estimator is the one of Vehtari, Gelman, Simpson, Carpenter and Buerkner, "Rank-normalization,
folding, and localization: an improved R-hat for assessing convergence of MCMC" (Bayesian Analysis 16(2), 2021),
section 3.2 (the one Stan reports as ``ess_bulk`` without the rank normalisation; Gelman et al., Bayesian Data
Analysis, 3rd edition, section 11.5): every chain is split in halves as for split R-hat, the within-chain
variance W and the between-chain variance B give var+ = (n - 1) / n W + B / n, the autocorrelation at lag t is

    rho_t = 1 - (W - mean over half-chains of their autocovariance at lag t) / var+ ,

and the autocorrelation time sums the pairs P_k = rho_2k + rho_2k+1 while they stay positive (Geyer's initial
positive sequence; Geyer, "Practical Markov chain Monte Carlo", Statistical Science 7(4), 1992):

    tau = -1 + 2 sum_k P_k ,        ESS = (number of samples x number of chains) / tau .

The log-potentials ``lp`` of ``FactorGraph.sample(..., log_potential=True)``, shape ``(samples, chains)``, are one
more column: ``effective_sample_size(lp[:, :, None])`` is the ESS of the joint state, and ``best_sample(lp)`` finds
the most probable sample recorded.

The per-weight statistics of ``FactorGraph.sample(..., weight_statistics=...)``, shape ``(samples, chains, weights)``,
are a trace like any other; ``moment_gap`` compares their mean with a target (the evidence chain's statistics, or an
exact expectation): the log-likelihood gradient of weight learning, with its Monte-Carlo standard error.

``autocov_counts`` and ``ess_from_counts`` restate, in numpy, what ``FactorGraph.mixing`` computes on the device from
a bit-packed trace (nsk_trace_ess): for 0 / 1 columns the estimator above is integer counts --
exact in int64 -- and a short float64 epilogue, the lags cut at ``max_lag``.  With ``max_lag = n - 1`` it is the
estimator of ``effective_sample_size``.

``pair_counts`` restates what ``FactorGraph.pairwise`` counts on the device for pairs of 0 / 1 columns
(nsk_trace_pair_counts), and ``pair_tables`` turns such counts -- the device's or numpy's -- into the 2 x 2 joint
marginal, covariance, correlation and mutual information of every pair; ``factor_pairs`` lists the two ends of every
pairwise factor of a graph.

Categorical columns go through indicators: ``indicators(trace, sel)`` is the 0 / 1 trace of ``trace[..., column] ==
value`` for every (column, value) of ``sel``, to which ``autocov_counts``, ``ess_from_counts`` and ``pair_counts`` apply
unchanged -- the numpy side of ``FactorGraph.mixing_values`` and ``FactorGraph.contingency`` (nsk_trace_value_ess,
nsk_trace_value_pair_counts) -- and ``contingency_tables`` turns the co-occurrence counts of all cells of a pair into its
``K_a x K_b`` joint table and mutual information.

``conditional_probabilities`` restates what ``FactorGraph.conditionals`` computes on the device from the potentials of
every value of a variable (nsk_conditionals), ``log_pseudo_likelihood`` sums the logs of those
conditionals at a state's own values, and ``tally_layout`` brings the "full" layout of both (every variable owns
``cardinality`` slots) to the layout of ``count`` / ``marginals`` (a binary variable owns one), so that the Rao-Blackwell
marginals of ``FactorGraph.rao_blackwell`` can be compared with the tally's.

``icm_choice`` restates the rule by which ``FactorGraph.icm`` (nsk_icm) picks a variable's new value
from the same potentials: greedy coordinate ascent towards a MAP estimate.

``ais_log_weights``, ``log_mean_exp``, ``ais_estimate`` and ``thermodynamic_integral`` are the host side of
``FactorGraph.tempered_sweeps`` / ``log_partition`` (nsk_tempered_sweeps): the device runs the
sweeps under a schedule of inverse temperatures and hands back every step's log-potentials; the fold of the importance
weights restated with the device's roundings, and the estimators of log Z, which need a ``log`` and live here.

``smc_resample`` and ``smc_estimate`` are the host side of ``FactorGraph.smc_sweeps`` / ``log_partition(resample=...)``
(nsk_smc_sweeps): the device's resampling decision and ancestor choice restated operation by
operation, and the estimate of log Z from a resampled population.

``pt_swap_rule``, ``pt_paths`` and ``pt_ladder`` are the host side of ``FactorGraph.parallel_tempering`` (nsk_pt_sweeps;
DESIGN.md section 4): the device's Metropolis decision on the swaps of a step restated operation by operation, the walk of
every starting replica over the slots with its round trips, and a geometric ladder of inverse temperatures.

``pl_gradient_counts`` and ``mple_step`` restate ``FactorGraph.pl_gradient`` / ``learn_mple`` (nsk_pl_gradient,
nsk_mple_steps): the gradient of the log-pseudo-likelihood as int64 sums of quantised terms -- exact,
whatever the order -- and the weight update of maximum pseudo-likelihood learning, one rounded operation each.

``moment_counts`` and ``pcd_step`` restate ``FactorGraph.weight_moments`` / ``learn_pcd`` (nsk_weight_moments, nsk_pcd_steps;
DESIGN.md section 4): the per-weight statistics summed over chains as int64 sums of quantised factor values, and the weight
update of persistent contrastive divergence, one rounded operation each; ``pcd_latent_step`` is the update of
``learn_pcd(clamped=K)`` (nsk_pcd_latent_steps), whose target is the mean of a clamped population of chains.

``bp_layout``, ``bp_psi``, ``bp_iterate`` and ``bp_factor_beliefs`` restate ``FactorGraph.belief_propagation``
(nsk_bp_setup, nsk_bp_run, nsk_bp_download) operation by operation in plain loops: the structure of
clamped and free variables, tables, directed edges and message offsets, the sum-product iterations with damping, the
residual and the rescale rule, and the factor beliefs -- the device's doubles bit for bit when handed the library's exp.
``bethe_log_z`` is the Bethe estimate of log Z from the beliefs, which needs a ``log`` and lives here.
"""

import collections

import numpy as np

Pairwise = collections.namedtuple("Pairwise", ["joint", "cov", "corr", "mi", "counts", "samples"])
Contingency = collections.namedtuple("Contingency", ["joint", "mi", "counts", "samples"])

_CHUNK = 256          # columns per FFT batch (memory: ~ 64 bytes x samples x chains x _CHUNK)


def _split(trace):
    """(samples, chains, columns) -> float64 half-chains (n, 2 x chains, columns), or None where the estimators
    are undefined (one chain, or fewer than 4 samples)."""
    x = np.asarray(trace)
    if x.ndim != 3:
        raise ValueError("a trace has shape (samples, chains, columns), got %r" % (x.shape,))
    s, m, _ = x.shape
    if m < 2 or s < 4:
        return None
    n = s // 2
    return np.concatenate([x[:n], x[s - n:]], axis=1).astype(np.float64)


def _rho(h, max_lag):
    """Combined autocorrelation estimates rho_0 .. rho_max_lag of half-chains h (n, m, c): (max_lag + 1, c);
    NaN for a column without variance."""
    n, m, c = h.shape
    d = h - h.mean(axis=0)
    size = 1 << int(2 * n - 1).bit_length()
    f = np.fft.rfft(d, size, axis=0)
    acov = np.fft.irfft(f * np.conj(f), size, axis=0)[:max_lag + 1] / n          # biased, per half-chain
    w = acov[0].mean(axis=0) * n / (n - 1.0)
    b_over_n = h.mean(axis=0).var(axis=0, ddof=1)
    var_plus = (n - 1.0) / n * w + b_over_n
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = 1.0 - (w - acov.mean(axis=1) * n / (n - 1.0)) / var_plus
    rho[:, ~(var_plus > 0)] = np.nan
    return rho


def autocorrelation(trace, max_lag):
    """Autocorrelation of every column at lags 0 .. ``max_lag``: array ``(max_lag + 1, columns)``.  Within- and
    between-chain variances are combined as for split R-hat (module docstring), so chains that have not mixed show
    as autocorrelation that does not decay.  NaN for a constant column, for one chain and for fewer than 4 samples."""
    ncol = np.asarray(trace).shape[2] if np.asarray(trace).ndim == 3 else 0
    h = _split(trace)
    max_lag = int(max_lag)
    if max_lag < 0:
        raise ValueError("max_lag must not be negative")
    out = np.full((max_lag + 1, ncol), np.nan)
    if h is None:
        return out
    lag = min(max_lag, h.shape[0] - 1)
    for c0 in range(0, ncol, _CHUNK):
        out[:lag + 1, c0:c0 + _CHUNK] = _rho(h[:, :, c0:c0 + _CHUNK], lag)
    return out


def effective_sample_size(trace):
    """Effective sample size of every column of a ``(samples, chains, columns)`` trace: array ``(columns,)``.
    NaN for a constant column, for one chain and for fewer than 4 samples."""
    ncol = np.asarray(trace).shape[2] if np.asarray(trace).ndim == 3 else 0
    h = _split(trace)
    out = np.full(ncol, np.nan)
    if h is None:
        return out
    n, m, _ = h.shape
    for c0 in range(0, ncol, _CHUNK):
        rho = _rho(h[:, :, c0:c0 + _CHUNK], n - 1)
        npair = rho.shape[0] // 2
        pairs = rho[0:2 * npair:2] + rho[1:2 * npair:2]
        keep = np.cumprod(np.nan_to_num(pairs) > 0, axis=0)           # the initial positive sequence
        tau = -1.0 + 2.0 * (np.nan_to_num(pairs) * keep).sum(axis=0)
        ess = np.full(rho.shape[1], np.nan)
        ok = np.isfinite(rho[0]) & (tau > 0)
        ess[ok] = n * m / tau[ok]
        out[c0:c0 + _CHUNK] = ess
    return out


def counts_fit_int64(n, H):
    """Whether the integers of ``autocov_counts`` for ``H`` half-chains of ``n`` rows fit int64 with every
    intermediate: ``4 H n^3 < 2^63`` (the bound nsk_trace_ess refuses beyond, NSK_E_RANGE)."""
    return 4 * int(H) * int(n) ** 3 < 2 ** 63


def autocov_counts(trace, max_lag):
    """The integers of the device estimator from a downloaded 0 / 1 trace ``(samples, chains, columns)``:
    ``(n, H, A, S1, S2)`` with ``n = samples // 2`` rows in each of the ``H = 2 x chains`` half-chains (rows ``[0, n)``
    and ``[samples - n, samples)`` of every chain), and per column, in int64, for ``k = 0 .. L``,
    ``L = min(max_lag, n - 1)``,

        A[k] = sum over half-chains h of  n^2 c_h(k) - n S_h (head_h(k) + tail_h(k)) + (n - k) S_h^2

    (``S_h`` the half-chain's sum, ``c_h(k)`` the sum of ``x_t x_{t+k}`` over ``t < n - k``, ``head_h(k)`` / ``tail_h(k)``
    the sums of its first / last ``n - k`` rows; ``n^3`` times the summed biased autocovariance at lag ``k``), shape
    ``(L + 1, columns)``; ``S1`` the sum of the ``S_h`` and ``S2`` of their squares, shape ``(columns,)``.  One chain
    is allowed here (``H = 2``)."""
    x = np.asarray(trace)
    if x.ndim != 3:
        raise ValueError("a trace has shape (samples, chains, columns), got %r" % (x.shape,))
    s, m, ncol = x.shape
    max_lag = int(max_lag)
    if s < 4:
        raise ValueError("at least 4 samples are needed")
    if max_lag < 1:
        raise ValueError("max_lag must be at least 1")
    if x.size and not ((x == 0) | (x == 1)).all():
        raise ValueError("the counts are defined for 0 / 1 columns")
    n, H = s // 2, 2 * m
    if not counts_fit_int64(n, H):
        raise OverflowError("4 x half-chains x (samples // 2)^3 reaches 2^63: the counts do not fit int64")
    h = np.concatenate([x[:n], x[s - n:]], axis=1).astype(np.int64)       # (n, H, columns)
    L = min(max_lag, n - 1)
    S = h.sum(axis=0)                                                      # (H, columns)
    A = np.zeros((L + 1, ncol), np.int64)
    for k in range(L + 1):
        c = (h[:n - k] * h[k:]).sum(axis=0)
        head, tail = h[:n - k].sum(axis=0), h[k:].sum(axis=0)
        A[k] = (n * n * c - n * S * (head + tail) + (n - k) * S * S).sum(axis=0)
    return n, H, A, S.sum(axis=0), (S * S).sum(axis=0)


def ess_from_counts(n, H, A, S1, S2):
    """The float64 epilogue of the device estimator (nsk_trace_ess), element for element: from the integers of
    ``autocov_counts`` -- ``A`` of shape ``(L + 1, columns)``, ``L >= 1`` -- returns ``(mean, tau, rhat2, truncated)``
    per column.  Every step is one rounded float64 operation, in the device's order:

        D = H n n (n - 1) (left to right),  W = A[0] / D,  B = (H S2 - S1^2) / (H (H - 1) n n),
        V = (n - 1) / n W + B,  rho_k = 1 - ((A[0] - A[k]) / D) / V  (both integer forms in int64),
        P_j = rho_2j + rho_2j+1 for j < (L + 1) // 2,  tau = -1 + 2 x (the initial run of P_j > 0 added in ascending j).

    ``mean = S1 / (H n)``; ``tau`` is NaN unless ``V > 0`` and ``tau > 0``; ``rhat2 = V / W`` is NaN unless ``V > 0``;
    ``truncated`` (uint8) is 1 where every pair was positive and ``L < n - 1``: the sequence did not end inside the
    window, so ``tau`` is a lower bound and ``n H / tau`` an upper bound of the effective sample size."""
    n, H = int(n), int(H)
    A = np.asarray(A, np.int64)
    S1, S2 = np.asarray(S1, np.int64), np.asarray(S2, np.int64)
    L = A.shape[0] - 1
    D = np.float64(H) * np.float64(n) * np.float64(n) * np.float64(n - 1)
    Bden = np.float64(H) * np.float64(H - 1) * np.float64(n) * np.float64(n)
    c1 = np.float64(n - 1) / np.float64(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        W = A[0].astype(np.float64) / D
        B = (H * S2 - S1 * S1).astype(np.float64) / Bden
        V = c1 * W + B
        ok = V > 0
        run = ok.copy()
        total = np.zeros(A.shape[1], np.float64)
        for j in range((L + 1) // 2):
            r0 = 1.0 - ((A[0] - A[2 * j]).astype(np.float64) / D) / V
            r1 = 1.0 - ((A[0] - A[2 * j + 1]).astype(np.float64) / D) / V
            P = r0 + r1
            run &= P > 0
            total = np.where(run, total + P, total)
        tau = -1.0 + 2.0 * total
        tau[~(ok & (tau > 0))] = np.nan
        rhat2 = np.where(ok, V / W, np.nan)
        mean = S1.astype(np.float64) / np.float64(H * n)
    truncated = (run & (L < n - 1)).astype(np.uint8)
    return mean, tau, rhat2, truncated


def _pair_list(pairs, ncols, what):
    p = np.asarray(pairs)
    if p.size == 0 and p.ndim <= 2:
        return np.zeros((0, 2), np.int64)
    if p.ndim != 2 or p.shape[1] != 2 or p.dtype.kind not in "iu":
        raise ValueError("%s: pairs have shape (npairs, 2) and an integer type, got %r %s" % (what, p.shape, p.dtype))
    p = p.astype(np.int64)
    if p.min() < 0 or p.max() >= ncols:
        raise ValueError("%s: an index of a pair lies outside [0, %d)" % (what, ncols))
    return p


def pair_counts(trace, pairs):
    """The integers of ``FactorGraph.pairwise`` from a downloaded 0 / 1 trace ``(rows, chains, columns)``: for every
    pair ``(a, b)`` of ``pairs`` (``(npairs, 2)`` column indices; any order, repeats and ``a == b`` allowed) and every
    chain ``r`` the number of rows where both columns are 1, where column ``a`` is and where column ``b`` is --
    ``(n11, n1a, n1b)``, int64, shape ``(npairs, chains, 3)``.  ValueError on values other than 0 / 1, on a bad shape
    and on an index outside the columns."""
    x = np.asarray(trace)
    if x.ndim != 3:
        raise ValueError("a trace has shape (samples, chains, columns), got %r" % (x.shape,))
    if x.size and not ((x == 0) | (x == 1)).all():
        raise ValueError("the counts are defined for 0 / 1 columns")
    p = _pair_list(pairs, x.shape[2], "pair_counts")
    x = x.astype(np.int8)
    out = np.zeros((len(p), x.shape[1], 3), np.int64)
    n1 = x.sum(axis=0, dtype=np.int64)                                     # (chains, columns)
    for j0 in range(0, len(p), _CHUNK):
        a, b = p[j0:j0 + _CHUNK, 0], p[j0:j0 + _CHUNK, 1]
        out[j0:j0 + _CHUNK, :, 0] = (x[:, :, a] & x[:, :, b]).sum(axis=0, dtype=np.int64).T
        out[j0:j0 + _CHUNK, :, 1] = n1[:, a].T
        out[j0:j0 + _CHUNK, :, 2] = n1[:, b].T
    return out


def pair_tables(counts, nrows):
    """From the counts of ``pair_counts`` / nsk_trace_pair_counts -- ``(npairs, chains, 3)`` int64 over ``nrows`` rows a
    chain -- the named tuple ``Pairwise(joint, cov, corr, mi, counts, samples)``, the chains pooled.  With
    ``N = nrows x chains`` and the pooled integers ``n11, na, nb`` (sums over the chains, int64), every figure is an
    exact integer expression converted to float64 once and then, in this order, one rounded float64 operation a step:

        joint[j]  2 x 2, indexed [value of a][value of b]:  [1, 1] = n11 / N,  [1, 0] = (na - n11) / N,
                  [0, 1] = (nb - n11) / N,  [0, 0] = (N - na - nb + n11) / N;
        num = N n11 - na nb  (int64; ValueError when N >= 2^31, so that it fits);
        cov = float(num) / float(N N);
        corr = float(num) / sqrt(float(na (N - na)) x float(nb (N - nb))),  NaN when either column is constant;
        mi (nats) = the cells c > 0 added in the order [0, 0], [0, 1], [1, 0], [1, 1] of
                  (float(c) / N) x log(float(c N) / float(row total x column total)).

    ``counts`` is the input as int64 and ``samples`` is ``N``.  With ``N = 0`` every float is NaN.  The device path
    and the numpy path both go through this function: equal counts give equal floats."""
    c = np.asarray(counts)
    if c.ndim != 3 or c.shape[2] != 3 or (c.size and c.dtype.kind not in "iu"):
        raise ValueError("counts have shape (npairs, chains, 3) and an integer type, got %r %s" % (c.shape, c.dtype))
    c = c.astype(np.int64)
    nrows = int(nrows)
    if nrows < 0:
        raise ValueError("nrows must not be negative")
    N = nrows * c.shape[1]
    if N >= 2 ** 31:
        raise ValueError("rows x chains reaches 2^31: N n11 - na nb may not fit int64")
    if c.size and (c.min() < 0 or c[:, :, 1:].max() > nrows or (c[:, :, :1] > c[:, :, 1:]).any()):
        raise ValueError("not the counts of %d rows a chain" % nrows)
    n11, na, nb = (c[:, :, k].sum(axis=1) for k in range(3))
    if ((na + nb - n11) > N).any():
        raise ValueError("not the counts of %d rows a chain" % nrows)
    cells = np.empty((len(c), 2, 2), np.int64)
    cells[:, 0, 0] = N - na - nb + n11
    cells[:, 0, 1] = nb - n11
    cells[:, 1, 0] = na - n11
    cells[:, 1, 1] = n11
    rowtot = np.stack([N - na, na], axis=1)                                # by the value of a
    coltot = np.stack([N - nb, nb], axis=1)                                # by the value of b
    num = N * n11 - na * nb
    fN = np.float64(N)
    with np.errstate(divide="ignore", invalid="ignore"):
        joint = cells.astype(np.float64) / fN
        cov = num.astype(np.float64) / np.float64(N * N)
        va, vb = na * (N - na), nb * (N - nb)
        corr = num.astype(np.float64) / np.sqrt(va.astype(np.float64) * vb.astype(np.float64))
        corr[(va == 0) | (vb == 0)] = np.nan
        mi = np.zeros(len(c), np.float64)
        for i in (0, 1):
            for k in (0, 1):
                cc = cells[:, i, k]
                term = (cc.astype(np.float64) / fN) * np.log((cc * N).astype(np.float64) / (rowtot[:, i] * coltot[:, k]).astype(np.float64))
                mi = np.where(cc > 0, mi + term, mi)
        if N == 0:
            mi[:] = np.nan
    return Pairwise(joint, cov, corr, mi, c, N)


def indicators(trace, sel):
    """The 0 / 1 series of a categorical trace: for a ``(rows, chains, columns)`` integer array and ``sel`` of shape
    ``(nsel, 2)`` -- (column, value) pairs; any order, repeats allowed -- the uint8 array ``(rows, chains, nsel)`` of
    ``trace[..., column] == value``.  ``autocov_counts``, ``ess_from_counts`` and ``pair_counts`` apply to it as to any
    0 / 1 trace: it is what nsk_trace_value_autocov_counts, nsk_trace_value_ess and nsk_trace_value_pair_counts count
    on the device.  A value no row holds gives a column of zeros.  ValueError on a bad shape or a non-integer array,
    IndexError on a column outside the trace."""
    x = np.asarray(trace)
    if x.ndim != 3 or (x.size and x.dtype.kind not in "iu"):
        raise ValueError("a trace has shape (samples, chains, columns) and an integer type, got %r %s" % (x.shape, x.dtype))
    s = np.asarray(sel)
    if s.size == 0 and s.ndim <= 2:
        return np.zeros(x.shape[:2] + (0,), np.uint8)
    if s.ndim != 2 or s.shape[1] != 2 or s.dtype.kind not in "iu":
        raise ValueError("indicators: sel has shape (nsel, 2) and an integer type, got %r %s" % (s.shape, s.dtype))
    s = s.astype(np.int64)
    if s[:, 0].min() < 0 or s[:, 0].max() >= x.shape[2]:
        raise IndexError("indicators: a column lies outside [0, %d)" % x.shape[2])
    return (x[:, :, s[:, 0]] == s[:, 1]).astype(np.uint8)


def contingency_tables(counts, shapes, nrows):
    """From the co-occurrence counts of all cells of all pairs the named tuple ``Contingency(joint, mi, counts,
    samples)``.  ``shapes`` is ``(npairs, 2)``: the cardinalities ``(K_a, K_b)`` of every pair; ``counts`` is int64
    ``(ncells, chains)``, the per-chain ``n11`` of the cells -- pair after pair, a pair's ``K_a x K_b`` cells in row-major
    order (value of a, value of b), ``ncells`` the sum of ``K_a K_b`` -- over ``nrows`` rows a chain: column 0 of
    ``pair_counts`` / nsk_trace_value_pair_counts on those cells.  With ``N = nrows x chains`` and the integers pooled
    over the chains (int64), per pair:

        joint   (K_a, K_b) float64:  float(cell) / float(N), one division a cell;
        mi (nats):  row and column totals are int64 sums of the cells; the cells c > 0 in row-major order add
                    (float(c) / float(N)) x log(float(c N) / float(row total x column total)) -- both products int64,
                    one conversion each, then one rounded operation a step, the sum from 0.0 in that order
                    (0 log 0 = 0: an empty cell adds nothing);
        counts  the per-chain integers as (chains, K_a, K_b).

    ``joint`` and ``counts`` are lists (the pairs need not share a shape), ``mi`` is an array ``(npairs,)`` and
    ``samples`` is ``N``.  With ``N = 0`` every float is NaN.  ValueError on a bad shape, on negative counts, when a
    pair's cells do not sum to ``nrows`` in every chain, and when ``N >= 2^31`` (``c N`` must fit int64).  The device
    path and the numpy path both go through this function: equal counts give equal floats."""
    c = np.asarray(counts)
    sh = np.asarray(shapes)
    if sh.size == 0 and sh.ndim <= 2:
        sh = np.zeros((0, 2), np.int64)
    if sh.ndim != 2 or sh.shape[1] != 2 or sh.dtype.kind not in "iu" or (sh.size and sh.min() < 1):
        raise ValueError("shapes are (npairs, 2) positive integers, got %r %s" % (sh.shape, sh.dtype))
    sh = sh.astype(np.int64)
    ncells = int((sh[:, 0] * sh[:, 1]).sum())
    if c.ndim != 2 or c.shape[0] != ncells or (c.size and c.dtype.kind not in "iu"):
        raise ValueError("counts have shape (ncells, chains) = (%d, chains) and an integer type, got %r %s" % (ncells, c.shape, c.dtype))
    c = c.astype(np.int64)
    nrows = int(nrows)
    if nrows < 0:
        raise ValueError("nrows must not be negative")
    nchains = c.shape[1]
    N = nrows * nchains
    if N >= 2 ** 31:
        raise ValueError("rows x chains reaches 2^31: cell x N may not fit int64")
    if c.size and c.min() < 0:
        raise ValueError("not the counts of %d rows a chain" % nrows)
    fN = np.float64(N)
    joint, per_chain = [], []
    mi = np.zeros(len(sh), np.float64)
    at = 0
    for j, (ka, kb) in enumerate(sh):
        ka, kb = int(ka), int(kb)
        cells = c[at:at + ka * kb].T.reshape(nchains, ka, kb)
        at += ka * kb
        if (cells.sum(axis=(1, 2)) != nrows).any():
            raise ValueError("pair %d: not the counts of %d rows a chain" % (j, nrows))
        pooled = cells.sum(axis=0)
        rowtot, coltot = pooled.sum(axis=1), pooled.sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            joint.append(pooled.astype(np.float64) / fN)
            total = np.float64(0.0)
            for va in range(ka):
                for vb in range(kb):
                    cc = pooled[va, vb]
                    if cc > 0:
                        total = total + (np.float64(cc) / fN) * np.log(np.float64(cc * N) / np.float64(rowtot[va] * coltot[vb]))
        mi[j] = total if N > 0 else np.nan
        per_chain.append(cells.copy())
    return Contingency(joint, mi, per_chain, N)


def factor_pairs(factor, fmap):
    """The two member variable ids of every arity-2 factor of a graph, in factor order: int64 ``(nf2, 2)``, first and
    second member as ``fmap`` lists them."""
    factor, fmap = np.asarray(factor), np.asarray(fmap)
    off = factor["ftv_offset"][factor["arity"] == 2].astype(np.int64)
    if len(off) and (off.min() < 0 or off.max() + 1 >= len(fmap)):
        raise ValueError("factor_pairs: a factor's members lie outside fmap")
    return np.stack([fmap["vid"][off], fmap["vid"][off + 1]], axis=1).astype(np.int64).reshape(-1, 2)


def best_sample(lp):
    """``(row, chain)`` of the largest log-potential in ``lp`` (samples, chains): the most probable sample of a
    ``FactorGraph.sample(..., log_potential=True)`` call, a MAP estimate; ties go to the first in row-major order."""
    x = np.asarray(lp)
    if x.ndim != 2 or x.size == 0:
        raise ValueError("log-potentials have shape (samples, chains) with at least one entry, got %r" % (x.shape,))
    row, chain = np.unravel_index(int(np.argmax(x)), x.shape)
    return int(row), int(chain)


def moment_gap(stats, target):
    """``(gap, mcse)`` of per-weight statistics ``stats`` (samples, chains, weights) against ``target`` (weights,):
    ``gap`` is the mean over samples and chains minus ``target`` -- with ``target`` the statistics of the evidence
    chain, minus the log-likelihood gradient the learning sweeps estimate one visit at a time -- and ``mcse`` its
    Monte-Carlo standard error, the standard deviation over samples and chains divided by
    ``sqrt(effective_sample_size(stats))``.  ``mcse`` is NaN where the statistic never moves and wherever the
    effective sample size is undefined (one chain, fewer than 4 samples)."""
    x = np.asarray(stats, np.float64)
    t = np.asarray(target, np.float64)
    if x.ndim != 3 or x.shape[0] * x.shape[1] == 0:
        raise ValueError("statistics have shape (samples, chains, weights) with at least one sample, got %r" % (x.shape,))
    if t.shape != (x.shape[2],):
        raise ValueError("target has shape (weights,) = (%d,), got %r" % (x.shape[2], t.shape))
    flat = x.reshape(-1, x.shape[2])
    gap = flat.mean(axis=0) - t
    sd = flat.std(axis=0, ddof=1) if flat.shape[0] > 1 else np.full(x.shape[2], np.nan)
    ess = effective_sample_size(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        mcse = sd / np.sqrt(ess)
    mcse[~(sd > 0)] = np.nan
    return gap, mcse


def _full_layout(offsets, x, what):
    off = np.asarray(offsets)
    if off.ndim != 1 or len(off) < 1 or off.dtype.kind not in "iu" or off[0] != 0 or (np.diff(off) < 1).any():
        raise ValueError("%s: offsets are int64 (nsel + 1,), start at 0 and grow by each variable's cardinality" % what)
    off = off.astype(np.int64)
    x = np.asarray(x, np.float64)
    if x.ndim < 1 or x.shape[-1] != off[-1]:
        raise ValueError("%s: the last axis has offsets[-1] = %d entries, got shape %r" % (what, off[-1], x.shape))
    return off, x


def conditional_probabilities(offsets, potentials, exp=np.exp):
    """The conditionals of ``FactorGraph.conditionals(potentials=True)`` output: ``potentials`` (..., total) holds, for
    selected variable ``i``, the potentials ``p_k`` of its values ``k`` at ``offsets[i] + k``.  ``e_k = exp(p_k)``,
    unshifted; ``Z`` is the running sum ``e_0, Z + e_1, ...`` in ``k`` order; ``P_k = e_k / Z`` -- the operations of the
    device, one rounded float64 operation each, so with ``exp`` the library's specified exponential (the oracle's
    ``exp_det``) the result equals ``FactorGraph.conditionals()`` bit for bit; ``np.exp`` may differ in the last place.
    Where ``Z`` is 0, infinite or NaN the result is what IEEE gives (the sampler's own degenerate case), and the NaN
    slots of a variable without a position stay NaN."""
    off, p = _full_layout(offsets, potentials, "conditional_probabilities")
    card = np.diff(off)
    e = np.asarray(exp(p), np.float64).reshape(p.shape)
    z = np.zeros(p.shape[:-1] + (len(card),))
    for k in range(int(card.max()) if len(card) else 0):
        m = card > k
        ek = e[..., off[:-1][m] + k]
        z[..., m] = ek if k == 0 else z[..., m] + ek
    with np.errstate(divide="ignore", invalid="ignore"):
        return e / np.repeat(z, card, axis=-1)


def log_pseudo_likelihood(offsets, potentials, values):
    """The log-pseudo-likelihood of a state from the potentials of ``FactorGraph.conditionals(potentials=True)``: the
    sum over the selected variables ``v`` of ``log P(x_v | the others) = p_{x_v} - m_v - log(sum_k exp(p_k - m_v))``,
    ``m_v`` the variable's largest potential (the shift keeps the sum finite where the unshifted conditional
    overflows).  ``values`` (..., nsel) holds each selected variable's own value; ``potentials`` is (..., total).  Returns
    a float, or an array over the leading axes.  NaN when a selected variable has no position (its potentials are NaN);
    ValueError when a value lies outside its variable's domain."""
    off, p = _full_layout(offsets, potentials, "log_pseudo_likelihood")
    card = np.diff(off)
    x = np.asarray(values)
    if x.ndim < 1 or x.shape[-1] != len(card) or (x.size and x.dtype.kind not in "iu"):
        raise ValueError("log_pseudo_likelihood: values are integers (..., nsel) = (..., %d), got %r %s" % (len(card), x.shape, x.dtype))
    x = x.astype(np.int64)
    if ((x < 0) | (x >= card)).any():
        raise ValueError("log_pseudo_likelihood: a value lies outside its variable's domain")
    lead = np.broadcast_shapes(p.shape[:-1], x.shape[:-1])
    p = np.broadcast_to(p, lead + p.shape[-1:])
    x = np.broadcast_to(x, lead + x.shape[-1:])
    if len(card) == 0:
        out = np.zeros(lead)
    else:
        m = np.maximum.reduceat(p, off[:-1], axis=-1)
        with np.errstate(invalid="ignore"):
            s = np.add.reduceat(np.exp(p - np.repeat(m, card, axis=-1)), off[:-1], axis=-1)
            own = np.take_along_axis(p, off[:-1] + x, axis=-1)
            out = (own - m - np.log(s)).sum(axis=-1)
    return float(out) if out.ndim == 0 else out


def icm_choice(offsets, potentials, values):
    """The decision of one iterated-conditional-modes visit (``FactorGraph.icm``, nsk_icm), for every selected variable at
    once: ``potentials`` (..., total) is the "full" layout of ``FactorGraph.conditionals(potentials=True)``, ``values``
    (..., nsel) each selected variable's current value.  Per variable of cardinality ``C``: ``best = cur`` when
    ``0 <= cur < C``, else 0; then for ``k`` ascending ``if p_k > p_best: best = k``.  So a move needs a strict
    improvement, the smallest ``k`` wins among several maxima, a NaN potential never wins (and a NaN incumbent is never
    left).  Returns the new values, int64 (..., nsel).  The potentials must be those of the state the values come from
    with every OTHER variable as it is: decide one colour class at a time."""
    off, p = _full_layout(offsets, potentials, "icm_choice")
    card = np.diff(off)
    x = np.asarray(values)
    if x.ndim < 1 or x.shape[-1] != len(card) or (x.size and x.dtype.kind not in "iu"):
        raise ValueError("icm_choice: values are integers (..., nsel) = (..., %d), got %r %s" % (len(card), x.shape, x.dtype))
    x = x.astype(np.int64)
    lead = np.broadcast_shapes(p.shape[:-1], x.shape[:-1])
    p = np.broadcast_to(p, lead + p.shape[-1:])
    x = np.broadcast_to(x, lead + x.shape[-1:])
    best = np.where((x >= 0) & (x < card), x, 0)
    if len(card) == 0:
        return best
    best_p = np.take_along_axis(p, off[:-1] + best, axis=-1)
    for k in range(int(card.max())):
        m = card > k
        pk = p[..., off[:-1][m] + k]
        better = pk > best_p[..., m]            # (False wherever either side is NaN)
        best[..., m] = np.where(better, k, best[..., m])
        best_p[..., m] = np.where(better, pk, best_p[..., m])
    return best


def tally_layout(offsets, values):
    """``(tally_offsets, tally_values)``: the "full" layout of ``FactorGraph.conditionals`` / ``rao_blackwell`` (every
    variable owns ``cardinality`` slots) brought to the layout of ``count`` / ``marginals`` / ``cstart``: the value-0 slot
    of every binary variable dropped, so that it owns ONE slot, the probability of value 1.  With ``var_ids=None``
    ``tally_offsets`` equals ``FactorGraph.cstart`` and ``tally_values`` lines up with ``count``."""
    off, v = _full_layout(offsets, values, "tally_layout")
    card = np.diff(off)
    keep = np.ones(int(off[-1]), bool)
    keep[off[:-1][card == 2]] = False
    toff = np.concatenate([[0], np.cumsum(np.where(card == 2, 1, card))]).astype(np.int64)
    return toff, v[..., keep]


def pl_gradient_counts(offsets, probabilities, values, entry_var, entry_k, entry_weight, entry_eval, nweight):
    """The gradient of the log-pseudo-likelihood with respect to the weights, as ``FactorGraph.pl_gradient(counts=True)``
    sums it on the device (nsk_pl_gradient), for ONE state.  ``offsets`` / ``probabilities`` are the "full" layout of
    ``FactorGraph.conditionals()`` for the selection (``P_k`` of selected variable ``i`` at ``offsets[i] + k``), ``values``
    (nsel,) each selected variable's own value.  The entries are the walk: entry ``j`` says that the factor list of
    (selected variable ``entry_var[j]`` -- an index into the selection --, value ``entry_k[j]``) holds a factor of weight
    ``entry_weight[j]`` whose value with the variable at ``entry_k[j]`` is ``entry_eval[j]``; a factor of a dataType-0
    list appears once per value.  Per entry, with ``cur`` the variable's own value::

        c = (k == cur ? 1.0 : 0.0) - P_k;  t = c * e;  q = np.rint(t * 2.0**32).astype(np.int64);  counts[weight] += q

    A variable is SKIPPED -- no entry of it counts -- when its value lies outside its domain or its ``Z`` is not a finite
    positive number, which its probabilities show: one of them is NaN (``Z`` is 0, NaN, or infinite through an infinite
    term), or none is positive (a finite sum that overflowed).  Returns ``(counts, skipped)``: int64 ``(nweight,)`` and
    the number of skipped variables.  ``counts * 2.0**-32`` is the derivative, to within ``2**-33`` per entry; the sums
    are integers, so their order does not matter."""
    off, p = _full_layout(offsets, probabilities, "pl_gradient_counts")
    if p.ndim != 1:
        raise ValueError("pl_gradient_counts: one state at a time: probabilities are (total,), got %r" % (p.shape,))
    card = np.diff(off)
    x = np.asarray(values)
    if x.shape != (len(card),) or (x.size and x.dtype.kind not in "iu"):
        raise ValueError("pl_gradient_counts: values are integers (nsel,) = (%d,), got %r %s" % (len(card), x.shape, x.dtype))
    x = x.astype(np.int64)
    ev, ek = np.asarray(entry_var, np.int64), np.asarray(entry_k, np.int64)
    ew, ee = np.asarray(entry_weight, np.int64), np.asarray(entry_eval, np.float64)
    if not (ev.ndim == 1 and ev.shape == ek.shape == ew.shape == ee.shape):
        raise ValueError("pl_gradient_counts: the four entry arrays are one-dimensional and equally long")
    counts = np.zeros(int(nweight), np.int64)
    if len(card) == 0:
        return counts, 0
    if len(ev) and (ev.min() < 0 or ev.max() >= len(card) or ek.min() < 0 or (ek >= card[ev]).any()
                    or ew.min() < 0 or ew.max() >= nweight):
        raise IndexError("pl_gradient_counts: an entry names a variable, value or weight out of range")
    nan = np.isnan(p)
    skip = (x < 0) | (x >= card) | (np.add.reduceat(nan.astype(np.int64), off[:-1]) > 0) \
        | ~(np.maximum.reduceat(np.where(nan, 0.0, p), off[:-1]) > 0)
    keep = ~skip[ev]
    ev, ek, ew, ee = ev[keep], ek[keep], ew[keep], ee[keep]
    c = (ek == x[ev]).astype(np.float64) - p[off[ev] + ek]
    t = c * ee
    q = np.rint(t * 2.0 ** 32).astype(np.int64)
    np.add.at(counts, ew, q)
    return counts, int(skip.sum())


def mple_step(w, fixed, counts_sum, n, step, reg_param):
    """One step of maximum pseudo-likelihood learning as ``FactorGraph.learn_mple`` takes it on the device
    (nsk_mple_steps): ``counts_sum`` (nweight,) is the int64 sum of ``pl_gradient_counts`` over the training examples,
    ``n`` = selected variables x examples.  One rounded float64 operation each::

        gbar = (float(S) * 2.0**-32) / n;  a = reg_param * w;  b = gbar - a;  c = step * b;  w = w + c

    Weights with ``fixed`` set stay as they are.  Returns the new weights (a new array)."""
    w = np.asarray(w, np.float64)
    s = np.asarray(counts_sum)
    if s.dtype.kind not in "iu" or s.shape != w.shape:
        raise ValueError("mple_step: counts_sum is int64 with the shape of w")
    gbar = (s.astype(np.float64) * 2.0 ** -32) / np.float64(n)
    a = np.float64(reg_param) * w
    b = gbar - a
    c = np.float64(step) * b
    return np.where(np.asarray(fixed).astype(bool), w, w + c)


def moment_counts(values, weight_ids, nweight):
    """The chain-summed per-weight moments as ``FactorGraph.weight_moments(counts=True)`` sums them on the device
    (nsk_weight_moments): ``values`` ``(chains, nfactor)`` -- or ``(nfactor,)`` for one chain -- are the factors' values on
    every chain's state (``FactorGraph.factor_values``), ``weight_ids`` ``(nfactor,)`` each factor's weight.  Per factor and
    chain ``q = np.rint(e * 2.0**32).astype(np.int64)``, and ``M[w]`` is the int64 sum of ``q`` over the chains and the
    factors of ``w``: integers, so their order does not matter.  A weight without a factor reads 0.  Returns int64
    ``(nweight,)``; ``M * 2.0**-32 / chains`` are the mean statistics."""
    e = np.asarray(values, np.float64)
    if e.ndim == 1:
        e = e[None, :]
    wid = np.asarray(weight_ids)
    if e.ndim != 2 or wid.shape != (e.shape[1],) or (wid.size and wid.dtype.kind not in "iu"):
        raise ValueError("moment_counts: values are (chains, nfactor), weight_ids integers (nfactor,)")
    wid = wid.astype(np.int64)
    nweight = int(nweight)
    if wid.size and (wid.min() < 0 or wid.max() >= nweight):
        raise IndexError("moment_counts: a factor names a weight out of range")
    if not np.isfinite(e).all() or (e.size and np.abs(e).max() >= 2.0 ** 30):
        raise OverflowError("moment_counts: a factor value is not finite or does not fit the fixed point")
    q = np.rint(e * 2.0 ** 32).astype(np.int64)
    counts = np.zeros(nweight, np.int64)
    np.add.at(counts, wid, q.sum(axis=0, dtype=np.int64))
    return counts


def pcd_step(w, fixed, M, R, target, n_w, step, reg_param, normalize):
    """One step of persistent contrastive divergence as ``FactorGraph.learn_pcd`` takes it on the device (nsk_pcd_steps):
    ``M`` (nweight,) is the int64 ``moment_counts`` of the ``R`` chains, ``target`` the statistics to match, ``n_w`` the
    number of factors of every weight (a weight without a factor counts as 1).  One rounded float64 operation each::

        m = (float(M) * 2.0**-32) / R;  g = target - m;  if normalize: g = g / n_w
        a = reg_param * w;  b = g - a;  c = step * b;  w = w + c

    Weights with ``fixed`` set stay as they are.  Returns ``(w_new, gmax)``: the new weights (a new array) and the largest
    ``|g|`` over the weights that are not fixed (after the normalisation, before the penalty; 0.0 when all are fixed)."""
    w = np.asarray(w, np.float64)
    s = np.asarray(M)
    t = np.asarray(target, np.float64)
    if s.dtype.kind not in "iu" or s.shape != w.shape or t.shape != w.shape:
        raise ValueError("pcd_step: M is int64 and target float64, both with the shape of w")
    n = np.maximum(np.asarray(n_w, np.float64), 1.0)
    if n.shape != w.shape:
        raise ValueError("pcd_step: n_w has the shape of w")
    free = ~np.asarray(fixed).astype(bool)
    m = (s.astype(np.float64) * 2.0 ** -32) / np.float64(R)
    g = t - m
    if normalize:
        g = g / n
    a = np.float64(reg_param) * w
    b = g - a
    c = np.float64(step) * b
    gmax = float(np.abs(g[free]).max()) if free.any() else 0.0
    return np.where(free, w + c, w), gmax


def pcd_latent_step(w, fixed, Mc, K, Mf, Rf, n_w, step, reg_param, normalize):
    """One step of PCD with latent variables as ``FactorGraph.learn_pcd(clamped=K)`` takes it on the device
    (nsk_pcd_latent_steps): ``Mc`` (nweight,) is the int64 ``moment_counts`` of the ``K`` clamped chains, ``Mf`` that of the
    ``Rf`` free chains.  One rounded float64 operation each::

        mc = (float(Mc) * 2.0**-32) / K;  mf = (float(Mf) * 2.0**-32) / Rf;  g = mc - mf;  if normalize: g = g / n_w
        a = reg_param * w;  b = g - a;  c = step * b;  w = w + c

    which is ``pcd_step`` with ``target = mc`` and ``Rf`` chains.  Weights with ``fixed`` set stay as they are.  Returns
    ``(w_new, gmax)`` as ``pcd_step`` does."""
    w = np.asarray(w, np.float64)
    sc = np.asarray(Mc)
    if sc.dtype.kind not in "iu" or sc.shape != w.shape:
        raise ValueError("pcd_latent_step: Mc and Mf are int64 with the shape of w")
    if int(K) < 1 or int(Rf) < 1:
        raise ValueError("pcd_latent_step: each population has at least one chain")
    mc = (sc.astype(np.float64) * 2.0 ** -32) / np.float64(K)
    return pcd_step(w, fixed, Mf, Rf, mc, n_w, step, reg_param, normalize)


def _schedule(betas, lp, what):
    b = np.asarray(betas, np.float64)
    u = np.asarray(lp, np.float64)
    if b.ndim != 1 or u.ndim != 2 or u.shape[0] != len(b) or len(b) < 1:
        raise ValueError("%s: betas (T,) and log-potentials (T, chains), got %r and %r" % (what, b.shape, u.shape))
    return b, u


def ais_log_weights(betas, lp):
    """The log importance weights of annealed importance sampling (Neal, "Annealed importance sampling", Statistics and
    Computing 11, 2001) as nsk_tempered_sweeps folds them: ``betas`` (T,) the schedule, ``lp`` (T, chains) the
    log-potential of every chain after the sweeps of every step.  Per chain, from 0.0 and in step order,
    ``logw = logw + (betas[t + 1] - betas[t]) * lp[t]`` for ``t + 1 < T`` -- one rounded difference, one rounded product,
    one rounded addition, a plain loop: fed the device's ``lp`` it returns the device's ``log_weights`` bit for bit."""
    b, u = _schedule(betas, lp, "ais_log_weights")
    logw = np.zeros(u.shape[1], np.float64)
    for t in range(len(b) - 1):
        d = b[t + 1] - b[t]
        term = d * u[t]
        logw = logw + term
    return logw


def log_mean_exp(x):
    """``log(mean(exp(x)))`` of a 1-d array, shifted by its maximum so that nothing overflows; -inf when every entry is
    -inf, NaN for an empty array."""
    x = np.asarray(x, np.float64).ravel()
    if x.size == 0:
        return float("nan")
    m = float(x.max())
    if not np.isfinite(m):
        return m
    return m + float(np.log(np.mean(np.exp(x - m))))


def ais_estimate(log_weights, log_z0):
    """``(log_z, stderr, ess)`` from the AIS log-weights of R chains and ``log_z0``, the log of the number of states at
    beta = 0.  With ``w = exp(logw - max)``: ``log_z = log_z0 + max + log(mean w)``; ``stderr = std(w, ddof=1) / (mean(w)
    sqrt(R))``, the delta-method standard error of ``log_z`` (NaN for R = 1); ``ess = (sum w)^2 / sum w^2``, the
    effective number of chains behind the mean (between 1 and R)."""
    lw = np.asarray(log_weights, np.float64).ravel()
    n = lw.size
    if n < 1:
        raise ValueError("ais_estimate: no log-weights")
    m = float(lw.max())
    w = np.exp(lw - m)
    mean = float(w.mean())
    log_z = float(log_z0) + m + float(np.log(mean))
    stderr = float(np.std(w, ddof=1) / (mean * np.sqrt(n))) if n > 1 else float("nan")
    ess = float(w.sum() ** 2 / (w * w).sum())
    return log_z, stderr, ess


def smc_resample(log_weights, u, threshold, exp=np.exp):
    """The resampling decision and the ancestors of population annealing as nsk_smc_sweeps takes them behind the fold of a
    step (include/numbskull_amd.h, step 5): ``log_weights`` (R,) the folded log-weights, ``u`` the step's uniform in
    [0, 1), ``threshold`` in [0, 1].  Returns ``(resampled, ancestors, S, Q)``.  With ``m`` the largest log-weight,
    ``w = exp(log_weights - m)``, ``c = cumsum(w)`` and ``q = cumsum(w * w)`` in chain order, ``S = c[-1]``, ``Q = q[-1]``:
    the population is resampled iff ``S * S < (threshold * R) * Q`` -- its effective sample size fell below ``threshold x
    R`` -- and then systematically: ``target[i] = (i + u) * (S / R)``, ``a[i]`` = the number of ``c[j] <= target[i]``, at
    most ``R - 1``, chain j gets ``n[j] = #{i : a[i] = j}`` offspring.  A chain with offspring keeps its slot
    (``ancestors[j] = j``); the slots without, ascending, take the chains with more than one, ascending, each repeated
    ``n[j] - 1`` times -- so the copy ``x[r] = x[ancestors[r]]`` can run in place.  Without resampling the ancestors are
    the identity; a NaN log-weight or a maximum that is not finite means no resampling (``S`` and ``Q`` are then NaN).
    Every step is one rounded float64 operation, the two cumulative sums run in order: fed the device's ``logw_pre`` row
    and the oracle's ``exp_det`` as ``exp`` it returns the device's ancestors integer for integer; ``np.exp`` may differ in
    a last place and so, rarely, in an ancestor."""
    lw = np.ascontiguousarray(log_weights, np.float64)
    if lw.ndim != 1 or lw.size < 1:
        raise ValueError("smc_resample: log_weights is a 1-d array of at least one chain, got %r" % (lw.shape,))
    if not 0.0 <= threshold <= 1.0:
        raise ValueError("smc_resample: the threshold lies in [0, 1]")
    if not 0.0 <= u < 1.0:
        raise ValueError("smc_resample: the uniform lies in [0, 1)")
    R = lw.size
    ident = np.arange(R, dtype=np.int32)
    m = lw.max()                                            # (NaN if any entry is)
    if not np.isfinite(m):
        return False, ident, float("nan"), float("nan")
    w = np.ascontiguousarray(exp(lw - m), np.float64)
    c, q = np.cumsum(w), np.cumsum(w * w)                   # 1-d float64: sequential, one rounded addition an entry
    S, Q = c[-1], q[-1]
    if not S * S < (np.float64(threshold) * np.float64(R)) * Q:
        return False, ident, float(S), float(Q)
    step = S / np.float64(R)
    target = (np.arange(R, dtype=np.float64) + np.float64(u)) * step
    a = np.minimum(np.searchsorted(c, target, side="right"), R - 1)
    n = np.bincount(a, minlength=R)
    anc = ident.copy()
    anc[n == 0] = np.repeat(ident, np.maximum(n - 1, 0))
    return True, anc, float(S), float(Q)


def pt_swap_rule(betas, lp_row, uniforms_row, t, exp=np.exp):
    """The swap decisions of step ``t`` of parallel tempering as nsk_pt_sweeps takes them (include/numbskull_amd.h, step
    3): ``betas`` (R,) the chains' inverse temperatures, ``lp_row`` (R,) their log-potentials behind the step's sweeps,
    ``uniforms_row`` (R - 1,) the step's uniforms in [0, 1).  Returns int32 ``(R - 1,)``: for the pair of the chains r and
    r + 1, -1 where the pair is not proposed (r and t of different parity), else 1 or 0.  ``d = (betas[r] - betas[r + 1])
    * (lp_row[r + 1] - lp_row[r])`` -- two rounded differences, one rounded product -- and the swap is accepted iff ``d >=
    0``, or ``d >= -745`` and ``uniforms_row[r] < exp(d)``; a NaN ``d`` rejects.  Fed the device's ``lp`` row and the
    oracle's ``exp_det`` as ``exp`` it returns the device's decisions integer for integer; ``np.exp`` may differ in a last
    place and so, rarely, in a decision."""
    b = np.ascontiguousarray(betas, np.float64)
    u = np.ascontiguousarray(lp_row, np.float64)
    if b.ndim != 1 or b.size < 1 or u.shape != b.shape:
        raise ValueError("pt_swap_rule: betas and lp_row are 1-d arrays of one entry a chain, got %r and %r" % (b.shape, u.shape))
    R = b.size
    x = np.ascontiguousarray(uniforms_row if R > 1 else np.zeros(0), np.float64)
    if x.shape != (R - 1,):
        raise ValueError("pt_swap_rule: uniforms_row holds one uniform a pair, (R - 1,), got %r" % (x.shape,))
    if not ((x >= 0.0) & (x < 1.0)).all():
        raise ValueError("pt_swap_rule: a uniform lies outside [0, 1)")
    out = np.full(R - 1, -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(int(t) & 1, R - 1, 2):
            db = b[r] - b[r + 1]
            du = u[r + 1] - u[r]
            d = db * du
            if d >= 0.0:
                out[r] = 1
            elif d >= -745.0:
                out[r] = 1 if x[r] < float(np.asarray(exp(np.array([d], np.float64))).ravel()[0]) else 0
            else:
                out[r] = 0              # (a NaN d lands here)
    return out


def pt_paths(accepted):
    """The walk of the replicas over the slots of a parallel-tempering run: ``accepted`` int ``(T, R - 1)`` as
    nsk_pt_sweeps returns it (1: the states of the chains r and r + 1 changed places behind step t; 0 and -1: they did
    not).  Returns ``(paths, round_trips)``: ``paths`` int64 ``(T, R)``, ``paths[t, s]`` the starting slot of the state
    that sits in slot s behind step t; ``round_trips`` int64 ``(R,)``, per starting slot the number of completed round
    trips slot 0 -> slot R - 1 -> slot 0 of its state (a state that starts in slot 0 has visited it).  With one chain
    there is nowhere to go: no round trips."""
    a = np.asarray(accepted)
    if a.ndim != 2:
        raise ValueError("pt_paths: accepted is (T, R - 1), got %r" % (a.shape,))
    T, R = a.shape[0], a.shape[1] + 1
    where = np.arange(R, dtype=np.int64)            # slot -> the starting slot of its state
    paths, trips = np.zeros((T, R), np.int64), np.zeros(R, np.int64)
    leg = np.zeros(R, np.int64)                     # per state: 0 nothing yet, 1 has been at slot 0, 2 ... and then at R - 1
    leg[where[0]] = 1
    for t in range(T):
        acc = np.nonzero(a[t] == 1)[0]
        if len(acc) > 1 and (np.diff(acc) < 2).any():
            raise ValueError("pt_paths: step %d accepts two pairs that share a chain" % t)
        for r in acc:
            where[r], where[r + 1] = where[r + 1], where[r]
        paths[t] = where
        if R > 1:
            top, bottom = where[R - 1], where[0]
            if leg[top] == 1:
                leg[top] = 2
            if leg[bottom] == 2:
                trips[bottom] += 1
            if leg[bottom] != 1:
                leg[bottom] = 1
    return paths, trips


def pt_ladder(n, beta_min):
    """A geometric ladder of ``n`` inverse temperatures from ``beta_min`` up to 1.0: ``beta_min ** (1 - i / (n - 1))``,
    the last exactly 1.0 (the cold chain, which samples the target); ``n = 1`` is ``[1.0]``.  Neighbouring chains of a
    geometric ladder have equal ratios, which gives about equal swap rates where the heat capacity is flat."""
    n, beta_min = int(n), float(beta_min)
    if n < 1:
        raise ValueError("pt_ladder: at least one chain")
    if not 0.0 < beta_min <= 1.0:
        raise ValueError("pt_ladder: beta_min lies in (0, 1]")
    if n == 1:
        return np.ones(1)
    out = beta_min ** (1.0 - np.arange(n, dtype=np.float64) / (n - 1))
    out[0], out[-1] = beta_min, 1.0
    return out


def smc_estimate(logw_pre, resampled, log_weights, log_z0):
    """``(log_z, ess, resamplings)`` of one population-annealing run (``FactorGraph.smc_sweeps``): ``logw_pre`` (T - 1,
    R) the log-weights in front of every decision, ``resampled`` (T - 1,) the decisions, ``log_weights`` (R,) the fold
    since the last resampling, ``log_z0`` the log of the number of states at beta = 0.  Every resampling closes a stage
    whose ratio of normalisers is the mean weight, so ``log_z = log_z0 + sum over resampled t of log_mean_exp(logw_pre[t])
    + log_mean_exp(log_weights)``; ``ess = (sum w)^2 / sum w^2`` of the final weights; ``resamplings`` the number of
    events.  Without an event this is ``ais_estimate``'s ``log_z``.  There is NO standard error: the chains of a
    resampled population share ancestors, the spread of the final weights says nothing about the stages before, and one
    run has no honest error bar -- repeat the run with other seeds and take the spread of ``exp(log_z)``."""
    pre = np.asarray(logw_pre, np.float64)
    lw = np.asarray(log_weights, np.float64).ravel()
    flag = np.asarray(resampled).astype(bool).ravel()
    if lw.size < 1:
        raise ValueError("smc_estimate: no log-weights")
    if pre.size == 0:
        pre = pre.reshape(0, lw.size)
    if pre.ndim != 2 or pre.shape != (flag.size, lw.size):
        raise ValueError("smc_estimate: logw_pre (T - 1, R), resampled (T - 1,) and log_weights (R,), got %r, %r and %r" %
                         (pre.shape, flag.shape, lw.shape))
    log_z = float(log_z0)
    for t in np.nonzero(flag)[0]:
        log_z = log_z + log_mean_exp(pre[t])
    log_z = log_z + log_mean_exp(lw)
    w = np.exp(lw - lw.max())
    return log_z, float(w.sum() ** 2 / (w * w).sum()), int(flag.sum())


def thermodynamic_integral(betas, lp, log_z0):
    """``log_z0`` plus the trapezoid over beta of the chain-mean of ``lp``: d log Z_beta / d beta = E_beta[U], so the
    integral from 0 to 1 is log Z - log Z_0.  An independent cross-check of ``ais_estimate`` from the same numbers; its
    bias is the trapezoid's and the chains' lag behind the schedule, and it comes without an error bar."""
    b, u = _schedule(betas, lp, "thermodynamic_integral")
    mean = u.mean(axis=1)
    return float(log_z0) + float(np.sum(np.diff(b) * 0.5 * (mean[1:] + mean[:-1])))


# ------------------------------------------------------------------------------------------------- belief propagation
# member positions a function reads whatever its arity says (EQUAL 1, the DP_GEN_* functions 1 to 3)
_BP_NEED = {3: 1, 18: 1, 19: 1, 20: 1, 30: 1, 21: 2, 22: 2, 25: 2, 26: 2, 23: 3, 24: 3}


def bp_layout(factor, fmap, variable, values, sample_evidence=False):
    """The structure ``FactorGraph.belief_propagation`` (nsk_bp_setup) builds for the state ``values``: a variable is
    clamped at its value when ``isEvidence`` is 4, or non-zero without ``sample_evidence``, and free otherwise.  Per
    factor, in order: ``members[f]`` its distinct members in order of first occurrence (none for NOOP), ``slots[f]`` the
    local slot of every member position, ``axes[f]`` the free ones among the members, in that order -- the axes of the
    factor's table, the first the most significant digit (C order) -- and ``shapes[f]`` their cardinalities.
    ``table_off`` (nfactor + 1) the tables' entries, ``edge_off`` (nfactor + 1) the directed edges (f, j), factor-major,
    ``edge_var`` their variables, ``msg_off`` (nedges + 1): edge e owns ``cardinality`` doubles at ``msg_off[e]`` in
    either message array.  ``var_edges[v]`` the edges of a free variable, ascending.  ``offsets`` (nvar + 1) the "full"
    layout of the beliefs.  A dict; ``clamped``, ``values`` and ``card`` are kept in it."""
    values = np.asarray(values, np.int64)
    ev = np.asarray(variable["isEvidence"])
    card = np.asarray(variable["cardinality"]).astype(np.int64)
    clamped = (ev == 4) | ((ev != 0) & (not sample_evidence))
    vid = np.asarray(fmap["vid"]).astype(np.int64)
    members, slots, axes, shapes = [], [], [], []
    table_off, edge_off, edge_var, msg_off = [0], [0], [], [0]
    var_edges = [[] for _ in range(len(card))]
    for f in range(len(factor)):
        fn, ar, s = int(factor[f]["factorFunction"]), int(factor[f]["arity"]), int(factor[f]["ftv_offset"])
        npos = 0 if fn == -1 else max(ar, _BP_NEED.get(fn, 0))
        mine, slot = [], []
        for v in vid[s:s + npos]:
            v = int(v)
            if v not in mine:
                mine.append(v)
            slot.append(mine.index(v))
        ax = [v for v in mine if not clamped[v]]
        T = 1
        for v in ax:
            var_edges[v].append(len(edge_var))
            edge_var.append(v)
            msg_off.append(msg_off[-1] + int(card[v]))
            T *= int(card[v])
        members.append(mine)
        slots.append(slot)
        axes.append(ax)
        shapes.append([int(card[v]) for v in ax])
        table_off.append(table_off[-1] + T)
        edge_off.append(len(edge_var))
    i64 = lambda x: np.asarray(x, np.int64)             # noqa: E731
    return {"members": members, "slots": slots, "axes": axes, "shapes": shapes, "table_off": i64(table_off),
            "edge_off": i64(edge_off), "edge_var": i64(edge_var), "msg_off": i64(msg_off), "var_edges": var_edges,
            "offsets": np.concatenate([[0], np.cumsum(card)]).astype(np.int64), "clamped": clamped, "values": values,
            "card": card}


def _bp_digits(a, shape):
    out = [0] * len(shape)
    for i in range(len(shape) - 1, -1, -1):
        out[i] = a % shape[i]
        a //= shape[i]
    return out


def _bp_rescale(v):
    """while the largest entry is > 0 and < 2^-512: every entry times 2^512 (exact)"""
    tiny, big = 2.0 ** -512, 2.0 ** 512
    while True:
        mx = v[0]
        for x in v[1:]:
            if x > mx:
                mx = x
        if not (mx > 0.0 and mx < tiny):
            return v
        v = [x * big for x in v]


def _bp_sum(v):
    z = v[0]
    for x in v[1:]:
        z = z + x
    return z


def bp_psi(layout, theta, exp=np.exp):
    """``psi_f(a) = exp(theta_f(a) - max_a theta_f)`` for every table: the maximum by exact comparison (a NaN never
    wins over the first entry), the subtraction rounded once."""
    theta = np.asarray(theta, np.float64)
    psi = np.zeros(len(theta))
    to = layout["table_off"]
    for f in range(len(to) - 1):
        th = [float(x) for x in theta[to[f]:to[f + 1]]]
        mx = th[0]
        for x in th[1:]:
            if x > mx:
                mx = x
        psi[to[f]:to[f + 1]] = exp(np.array([x - mx for x in th]))
    return psi


def bp_iterate(layout, theta, iters, damping=0.0, tol=0.0, exp=np.exp, messages=None):
    """Sum-product belief propagation as nsk_bp_run performs it, in plain loops, operation by operation (the header
    states the rule): up to ``iters`` iterations of the factor phase -- per edge (f, j) the sums over the table
    entries of ``psi`` times the other axes' incoming messages, normalised in k order, damped with
    ``(1 - damping) * new + damping * old``, the residual the largest change of a message entry, NaN counting as inf --
    and the variable phase -- prefix products stored, the belief from the full product, suffix products multiplied in,
    each vector rescaled by 2^512 while its largest entry is positive and below 2^-512.  The iterations stop behind the
    first whose residual is ``<= tol``.  ``messages=(f2v, v2f)`` continues from those; None starts at ``1 / card``.
    Returns a dict: ``f2v``, ``v2f``, ``beliefs`` (the "full" layout of ``layout["offsets"]``: a clamped variable's
    indicator, a free variable's uniform law where it is in no table), ``residual`` (``iters`` entries, 0 behind the
    stop), ``iters`` (the iterations run up to and including the first with residual <= tol; ``-iters`` without one),
    ``psi`` and ``rescaled`` (how often the rescale rule fired)."""
    to, eo, mo = layout["table_off"], layout["edge_off"], layout["msg_off"]
    card, off = layout["card"], layout["offsets"]
    psi = bp_psi(layout, theta, exp)
    nmsg = int(mo[-1])
    if messages is None:
        f2v, v2f = np.zeros(nmsg), np.zeros(nmsg)
        for e in range(len(mo) - 1):
            f2v[mo[e]:mo[e + 1]] = v2f[mo[e]:mo[e + 1]] = 1.0 / float(mo[e + 1] - mo[e])
    else:
        f2v, v2f = (np.array(m, np.float64) for m in messages)
    beliefs = np.zeros(int(off[-1]))
    for v in range(len(card)):
        if layout["clamped"][v]:
            if 0 <= layout["values"][v] < card[v]:
                beliefs[off[v] + layout["values"][v]] = 1.0
        else:
            beliefs[off[v]:off[v + 1]] = 1.0 / float(card[v])
    lam, oml = float(damping), 1.0 - float(damping)
    residual = np.zeros(iters)
    ran, fired = -iters, 0
    count = [0]

    def rescale(v):
        w = _bp_rescale(v)
        if w is not v:
            count[0] += 1
        return w

    for t in range(iters):
        if t > 0 and residual[t - 1] <= tol:
            break
        res = 0.0
        new = f2v.copy()
        for f in range(len(to) - 1):
            shape = layout["shapes"][f]
            e0 = int(eo[f])
            for j in range(len(shape)):
                m = [0.0] * shape[j]
                for a in range(int(to[f + 1] - to[f])):
                    d = _bp_digits(a, shape)
                    x = float(psi[to[f] + a])
                    for i in range(len(shape)):
                        if i != j:
                            x = x * float(v2f[mo[e0 + i] + d[i]])
                    m[d[j]] = m[d[j]] + x
                z = _bp_sum(m)
                with np.errstate(all="ignore"):
                    for k in range(shape[j]):
                        nw = float(np.float64(m[k]) / np.float64(z))
                        old = float(f2v[mo[e0 + j] + k])
                        if lam > 0.0:
                            nw = oml * nw + lam * old
                        new[mo[e0 + j] + k] = nw
                        dd = abs(nw - old)
                        res = max(res, dd if dd == dd else np.inf)
        f2v = new
        residual[t] = res
        with np.errstate(all="ignore"):
            for v in range(len(card)):
                edges = layout["var_edges"][v]
                if layout["clamped"][v] or not edges:
                    continue
                n = int(card[v])
                P = [1.0] * n
                for e in edges:
                    v2f[mo[e]:mo[e + 1]] = P
                    P = rescale([P[k] * float(f2v[mo[e] + k]) for k in range(n)])
                z = np.float64(_bp_sum(P))
                beliefs[off[v]:off[v + 1]] = [np.float64(p) / z for p in P]
                S = [1.0] * n
                for e in reversed(edges):
                    T = rescale([float(v2f[mo[e] + k]) * S[k] for k in range(n)])
                    zt = np.float64(_bp_sum(T))
                    v2f[mo[e]:mo[e + 1]] = [np.float64(x) / zt for x in T]
                    S = rescale([S[k] * float(f2v[mo[e] + k]) for k in range(n)])
        if ran < 0 and res <= tol:
            ran = t + 1
    fired = count[0]
    return {"f2v": f2v, "v2f": v2f, "beliefs": beliefs, "residual": residual, "iters": ran, "psi": psi, "rescaled": fired}


def bp_factor_beliefs(layout, psi, v2f):
    """``b_f(a) = psi_f(a) * v2f[(f, 0)][a_0] * ..`` over the axes ascending, divided by their a-ordered sum; the
    layout of ``table_off`` (nsk_bp_download, NSK_BP_FACTOR_BELIEFS)."""
    to, eo, mo = layout["table_off"], layout["edge_off"], layout["msg_off"]
    out = np.zeros(int(to[-1]))
    for f in range(len(to) - 1):
        shape = layout["shapes"][f]
        b = []
        for a in range(int(to[f + 1] - to[f])):
            d = _bp_digits(a, shape)
            x = float(psi[to[f] + a])
            for i in range(len(shape)):
                x = x * float(v2f[mo[int(eo[f]) + i] + d[i]])
            b.append(x)
        with np.errstate(all="ignore"):
            z = np.float64(_bp_sum(b))
            out[to[f]:to[f + 1]] = [np.float64(x) / z for x in b]
    return out


def bp_moment_counts(layout, feat, psi, v2f, weight_ids, nweight):
    """The expected per-weight statistics under the factor beliefs as ``FactorGraph.bp_weight_moments(counts=True)`` sums
    them on the device (nsk_bp_moments): ``feat`` is the table of ``eval_factor`` without the weight (``table_off``'s
    layout; ``theta = w[weight] * feat``), ``psi`` and ``v2f`` those of a ``bp_iterate`` run, ``weight_ids`` (nfactor,)
    each factor's weight.  Per factor ``x(a)`` and their a-ordered sum ``Z`` exactly as ``bp_factor_beliefs`` forms them;
    a factor whose ``Z`` is not a finite positive number (two contradicting hard constraints: NaN) is skipped.
    Otherwise per entry, one rounded float64 operation each::

        b = x(a) / Z;  p = b * feat(a);  q = np.rint(p * 2.0**32).astype(np.int64);  M[weight] += q

    Integers, so their order does not matter; a factor without a free member adds ``rint(e * 2**32)``, what
    ``moment_counts`` adds for it.  Returns ``(int64 (nweight,), skipped)``; ``M * 2.0**-32`` are the expectations, each
    within ``2**-33`` per table entry of the sum of ``b * feat``."""
    to, eo, mo = layout["table_off"], layout["edge_off"], layout["msg_off"]
    feat = np.asarray(feat, np.float64)
    wid = np.asarray(weight_ids).astype(np.int64)
    nweight = int(nweight)
    if feat.shape != (int(to[-1]),) or wid.shape != (len(to) - 1,):
        raise ValueError("bp_moment_counts: feat has the layout of table_off, weight_ids one entry a factor")
    if wid.size and (wid.min() < 0 or wid.max() >= nweight):
        raise IndexError("bp_moment_counts: a factor names a weight out of range")
    counts = np.zeros(nweight, np.int64)
    skipped = 0
    psi, v2f = np.asarray(psi, np.float64), np.asarray(v2f, np.float64)
    for f in range(len(to) - 1):
        shape = layout["shapes"][f]
        # x(a) = ((psi(a) * v2f[(f,0)][a_0]) * ..): one elementwise product per axis, ascending -- per entry the same
        # rounded products in the same order as bp_factor_beliefs takes them one by one
        x = psi[to[f]:to[f + 1]].reshape(shape if shape else (1,))
        with np.errstate(invalid="ignore"):         # (0 * inf = NaN is what IEEE gives; it is caught below)
            for i in range(len(shape)):
                m = v2f[mo[int(eo[f]) + i]:mo[int(eo[f]) + i + 1]]
                x = x * m.reshape([-1 if k == i else 1 for k in range(len(shape))])
        x = x.ravel()
        z = _bp_sum(x.tolist())                     # the a-ordered sum, one addition after another
        if not (z > 0.0 and z < np.inf):            # (a NaN fails both: nothing of it reaches a conversion)
            skipped += 1
            continue
        b = x / np.float64(z)
        p = b * feat[to[f]:to[f + 1]]
        counts[wid[f]] += np.rint(p * 2.0 ** 32).astype(np.int64).sum(dtype=np.int64)
    return counts, skipped


def bethe_log_z(layout, theta, factor_beliefs, beliefs):
    """The Bethe estimate of log Z from the beliefs of a belief-propagation run: the sum over factors and table entries
    of ``b_f (theta_f - log b_f)``, plus the sum over free variables of ``(d_v - 1) sum_k b_v log b_v`` with ``d_v`` the
    variable's edges, plus ``log cardinality`` for every free variable without an edge; ``0 log 0 = 0``.  Exact where
    the free part of the graph is a forest and the run has converged.  Of ``layout`` it reads ``card``, ``clamped`` (per
    variable) and ``edge_var`` (nsk_bp_layout gives the same); ``beliefs`` is in the "full" layout over all variables."""
    theta = np.asarray(theta, np.float64)
    fb = np.asarray(factor_beliefs, np.float64)
    b = np.asarray(beliefs, np.float64)
    card, clamped = np.asarray(layout["card"], np.int64), np.asarray(layout["clamped"], bool)
    deg = np.bincount(np.asarray(layout["edge_var"], np.int64), minlength=len(card))
    with np.errstate(divide="ignore", invalid="ignore"):
        total = float(np.sum(np.where(fb > 0, fb * (theta - np.log(fb)), 0.0)))
        h = np.bincount(np.repeat(np.arange(len(card)), card), weights=np.where(b > 0, b * np.log(b), 0.0), minlength=len(card))
    walked = ~clamped & (deg > 0)
    total += float(np.sum((deg[walked] - 1) * h[walked]))
    total += float(np.sum(np.log(card[~clamped & (deg == 0)].astype(np.float64))))
    return total
