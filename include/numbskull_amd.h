/*
 * numbskull_amd.h -- C-ABI of the MI355X-native Gibbs-sweep engine (libnumbskull_amd.so).
 *
 * The reference (HazyResearch/numbskull) has no FFI layer: its seam is the three
 * run_pool(...) call sites in numbskull/factorgraph.py
 *     :141  burn-in   -> inference.gibbsthread(..., burnin=True)
 *     :163  inference -> inference.gibbsthread(..., burnin=False)
 *     :202  learning  -> learning.learnthread(...)
 * whose callee signatures are inference.py:10-13 and learning.py:12-16.  A maintainer makes the
 * reference GPU-backed by replacing those three calls with nsk_gibbs_sweeps / nsk_learn_sweeps on
 * a handle created from the very arrays FactorGraph already owns (INTEGRATION.md shows the ctypes
 * stub).  Everything crosses this boundary as plain pointers and sizes; the record layouts are
 * the reference's packed numpy dtypes (numbskulltypes.py:11-39), so record arrays are passed by
 * pointer without conversion.
 *
 * Conventions: every function returns NSK_OK (0) or a negative NSK_E_* code; nsk_last_error()
 * returns a thread-local human-readable message for the last failure.  Host pointers stay owned
 * by the caller; the library owns device memory.  One in-flight call per handle.
 */
#ifndef NUMBSKULL_AMD_H
#define NUMBSKULL_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSK_OK 0
#define NSK_E_INVALID (-1)      /* bad argument / inconsistent sizes                              */
#define NSK_E_FACTOR_FUNC (-2)  /* unknown factorFunction: reference raises NotImplementedError
                                   (inference.py:410-413)                                         */
#define NSK_E_INDEX (-3)        /* an index the reference would fault on (IndexError)             */
#define NSK_E_DEVICE (-4)       /* HIP runtime failure or no usable device                        */
#define NSK_E_RANGE (-5)        /* a value does not fit the device representation                 */
#define NSK_E_NOMEM (-6)

/* ---- record layouts = numbskull/numbskulltypes.py:11-39 (packed) ---- */
#pragma pack(push, 1)
typedef struct { uint8_t isFixed; double initialValue; } nsk_weight;                  /*  9 B */
typedef struct { int8_t isEvidence; int64_t initialValue; int16_t dataType;
                 int64_t cardinality; int64_t vtf_offset; } nsk_variable;             /* 27 B */
typedef struct { int16_t factorFunction; int64_t weightId; double featureValue;
                 int64_t arity; int64_t ftv_offset; } nsk_factor;                     /* 34 B */
typedef struct { int64_t vid; int64_t dense_equal_to; } nsk_ftv;                      /* 16 B */
typedef struct { int64_t value; int64_t factor_index_offset;
                 int64_t factor_index_length; } nsk_vtf;                              /* 24 B */
#pragma pack(pop)

/* nsk_graph_desc.flags */
#define NSK_FLAG_HEAD_BY_VID 1  /* IMPLY_MLN / IMPLY_NATURAL_CAT / IMPLY_MLN_CAT read their head as
                                   var_value[fmap[l].vid] instead of the reference's literal
                                   var_value[l] (inference.py:243,277,292)                        */

#define NSK_FLAG_PARTITION 2    /* [own_begin, own_end) is this handle's shard even when it is empty;
                                   without the flag own_begin == own_end == 0 means "the whole graph" */

/* scan orders (nsk_set_scan) */
#define NSK_SCAN_CHROMATIC 0    /* colour classes in parallel, Philox uniforms (default)          */
#define NSK_SCAN_SEQUENTIAL 1   /* one lane, variable-id order, MT19937: the reference's own
                                   trajectory (validation only; slow)                             */

/* The arrays a FactorGraph is constructed from (factorgraph.py:30-37). */
typedef struct {
    int64_t nweight, nvar, nfactor, nedge, nvtf, nfactor_index;
    const nsk_weight *weight;
    const nsk_variable *variable;
    const nsk_factor *factor;
    const nsk_ftv *fmap;
    const nsk_vtf *vmap;
    const int64_t *factor_index;
    int32_t flags;
    int32_t device;        /* HIP device ordinal                                                  */
    int64_t own_begin;     /* this handle samples variables [own_begin, own_end); the rest are     */
    int64_t own_end;       /* ghosts (= the reference's isEvidence==4, inference.py:21-23)         */
} nsk_graph_desc;

typedef struct nsk_graph nsk_graph;

/* Replaces FactorGraph.__init__'s state setup (factorgraph.py:39-63): validates the graph
 * (unknown factor functions -> NSK_E_FACTOR_FUNC, out-of-range indices -> NSK_E_INDEX), colours
 * it, compiles the device layout and uploads it.  State starts as the reference's: values and
 * evidence-chain values = initialValue, weights = initialValue, counts = 0. */
int nsk_graph_create(const nsk_graph_desc *desc, nsk_graph **out);
int nsk_graph_destroy(nsk_graph *g);

/* Host <-> device state sync.  Arrays are the FactorGraph attributes var_value[0],
 * var_value_evid[0], weight_value[0], count (factorgraph.py:46-53); NULL = leave alone. */
int nsk_state_upload(nsk_graph *g, const int64_t *var_value, const int64_t *var_value_evid,
                     const double *weight_value, const int64_t *count);
int nsk_state_download(nsk_graph *g, int64_t *var_value, int64_t *var_value_evid,
                       double *weight_value, int64_t *count);

/* Several chains on one handle (FactorGraph.inference(..., var_copy="all")).  A handle with R chains keeps
 * R value arrays and R tallies over ONE compiled layout and weight table; one nsk_gibbs_sweeps call sweeps
 * every chain, all at the same sweep index.  Chain r of a handle seeded s draws exactly what a one-chain
 * handle seeded s ^ ((uint64_t)r << 32) draws (Philox key word 1 XOR r): chain 0 is the one-chain handle.
 * Consequence: seeds that differ only in bits 32 and above give overlapping chains (chain r of seed s is
 * chain 0 of seed s ^ (r << 32)).
 * nsk_set_chains: 1 <= nchains <= 1024.  Chain 0 keeps its values and tally (as do the chains both counts
 * have); new chains start as nsk_graph_create leaves a handle: initialValue, tally 0.  NSK_E_NOMEM when the
 * state does not fit.  The value array moves: a pointer from nsk_device_buffer(NSK_BUF_VALUE) taken before is
 * stale.  With R > 1 only chromatic inference and burn-in sweeps serve the handle (and what is built on
 * them: nsk_pcd_steps learns from all R chains): the per-visit learning of nsk_learn_sweeps, the sequential
 * scan, own_range / NSK_FLAG_PARTITION handles, nsk_pf_setup and the exchange, RCCL and peer-to-peer entry
 * points return NSK_E_INVALID.
 * nsk_chains_upload / nsk_chains_download: var_value is R x nvar (row r = chain r, caller's variable ids),
 * count is R x ncount (chain r's tally); NULL = leave alone.  nsk_state_upload / nsk_state_download keep
 * meaning chain 0 (plus the evidence chain and the shared weights).  nsk_profile_* counts a launch that
 * serves every chain once. */
int nsk_set_chains(nsk_graph *g, int nchains);
int nsk_get_chains(nsk_graph *g);
int nsk_chains_upload(nsk_graph *g, const int64_t *var_value, const int64_t *count);
int nsk_chains_download(nsk_graph *g, int64_t *var_value, int64_t *count);

/* Sample traces (FactorGraph.sample): thinned joint samples recorded on the device.  While a trace is set up, one
 * launch behind every `every`-th TALLIED sweep of nsk_gibbs_sweeps (burnin = 0) appends a ROW: the values of the
 * traced variables in every chain of the handle, as they are after that sweep.  Burn-in sweeps are neither counted
 * nor recorded; the count of tallied sweeps since the last row carries over from call to call.  Nothing waits on
 * the host, and a traced call leaves exactly the values and tallies the same call leaves without a trace.  Rows are
 * kept bit-packed on the device when every traced variable has cardinality 2, else as one element of value_bytes
 * per column.
 * nsk_trace_setup: vids = the caller's variable ids (sampled or evidence, any order, repeats allowed), NULL = all
 * nvar variables; an id outside [0, nvar) is NSK_E_INDEX; every >= 1 and capacity >= 1 rows, else NSK_E_INVALID;
 * nvids >= 1 with a list; NSK_E_NOMEM when capacity x chains rows do not fit.  capacity = 0 tears the trace down and
 * frees it; setting up again replaces the trace (a call refused for its arguments leaves the old one; one that fails
 * for lack of memory leaves none).  NSK_E_INVALID on an own_range / NSK_FLAG_PARTITION handle and on one that exchanges
 * a boundary.
 * nsk_trace_rows: rows recorded so far, the capacity (0: no trace), 1 / 0 for bit-packed / plain rows (any may be NULL).
 * nsk_trace_download: synchronises, then writes rows first_row .. first_row + nrows - 1 as nrows x chains x nvids
 * elements of value_bytes (int8_t or int32_t, as NSK_BUF_VALUE) in the caller's column order, unpacked;
 * sweep_index[i] (may be NULL) = the handle's sweep index after which row first_row + i was taken.  Rows beyond
 * those recorded: NSK_E_INVALID.
 * nsk_trace_clear: rows and the count of sweeps since the last row back to 0; the buffer stays (and the accumulators of
 * nsk_trace_conditionals are zeroed).
 * A handle with a trace refuses, before it enqueues anything: a nsk_gibbs_sweeps call that needs more rows than
 * are left (NSK_E_RANGE; state and sweeps_done untouched), sweeps while values lie outside their domains and the
 * rows are bit-packed (NSK_E_RANGE), and with NSK_E_INVALID nsk_learn_sweeps, sweeps under the sequential scan,
 * the exchange, RCCL and peer-to-peer entry points, and nsk_set_chains with another count.  nsk_profile_* keeps
 * counting sweep-kernel launches only. */
int nsk_trace_setup(nsk_graph *g, const int64_t *vids, int64_t nvids, int64_t every, int64_t capacity);
int nsk_trace_rows(nsk_graph *g, int64_t *rows, int64_t *capacity, int64_t *packed);
int nsk_trace_download(nsk_graph *g, int64_t first_row, int64_t nrows, void *out, int64_t *sweep_index);
int nsk_trace_clear(nsk_graph *g);

/* Log-potential (FactorGraph.log_potential / factor_values / sample(..., log_potential=True)): the unnormalised
 * log-probability of a state, the sum over ALL factors f of weight[f.weightId] * eval_factor(f, state), evaluated on
 * the device one lane per factor.  Every term is one rounded float64 product; the sum is REPRODUCIBLE -- a function of
 * graph, weights and state only: the same bits for any chain index or chain count of the handle, from a query or from
 * a trace row, on every run (a fixed grid, fixed-order wave, block and final reductions, no floating-point atomics).  It
 * differs from the exactly rounded sum by at most (nfactor + 1) * 2^-53 * sum |term|.
 * The calls synchronise with the handle's stream and read values and weights as nsk_state_download /
 * nsk_chains_download would return them at that moment; they change nothing (values, tallies, sweeps_done, generator
 * state).  The first one uploads the factor and member records unless the handle's kernels read them already
 * (16 bytes a factor, 8 an edge, 4 a variable; reported by nsk_graph_info.device_bytes; NSK_E_NOMEM when they do not fit) and holds
 * the factors no sampled variable reaches to the rules nsk_graph_create applies to the others (NSK_E_INVALID names
 * the first that breaks one).  A handle that never calls them allocates and launches nothing for them.
 * which: NSK_BUF_VALUE (chains first_chain .. first_chain + nchains - 1 of the handle's chains) or NSK_BUF_VALUE_EVID
 * (the evidence chain exists once: first_chain = 0, nchains = 1); anything else, nchains < 1 and a chain the handle
 * does not have are NSK_E_INVALID, as are own_range / NSK_FLAG_PARTITION handles and handles that exchange a boundary
 * (a shard's sum is not the graph's, and its ghosts are stale between exchanges).  The sequential scan is fine.
 * nsk_log_potential: out[i] = log-potential of chain first_chain + i.
 * nsk_factor_values: out[f] = eval_factor(f, state of `chain`) for the nfactor factors in the caller's order.
 * nsk_trace_log_potential(g, 1): valid while a trace is set up (NSK_E_INVALID otherwise); allocates capacity x chains
 * doubles, and from then on every record launch is followed on the stream by the evaluation of the state just
 * recorded, every chain, whatever columns the trace keeps (rows recorded while it was off read 0).  0 switches it
 * off and frees the buffer; nsk_trace_setup (replace or tear down) resets it to off; nsk_trace_clear keeps it.
 * nsk_trace_download_log_potential: synchronises, then writes rows first_row .. first_row + nrows - 1 as
 * nrows x chains doubles; rows beyond those recorded, or no lp column: NSK_E_INVALID.
 * nsk_profile_* keeps counting sweep-kernel launches only. */
int nsk_log_potential(nsk_graph *g, int which, int64_t first_chain, int64_t nchains, double *out);
int nsk_factor_values(nsk_graph *g, int which, int64_t chain, double *out /* nfactor */);
int nsk_trace_log_potential(nsk_graph *g, int on);
int nsk_trace_download_log_potential(nsk_graph *g, int64_t first_row, int64_t nrows,
                                     double *out /* nrows x chains */);

/* Per-weight sufficient statistics (FactorGraph.weight_statistics / sample(..., weight_statistics=...)): the
 * log-potential's sum split by weight, S_w = the sum of eval_factor(f, state) over the factors f with weightId == w, in
 * the caller's weight numbering; a weight without a factor reads 0.  scaled != 0: every term is the one rounded product
 * featureValue[f] * eval_factor(f, state).  Evaluated on the device through a by-weight index list: one lane per weight
 * of at most 16 factors, one wave per piece of at most 2048 factors of a longer one, and a second launch that adds the
 * pieces of the weights that have several.  The sums are REPRODUCIBLE -- a function of graph, state and `scaled` only:
 * how a weight is cut depends on its own length, every addition has a fixed order, there are no floating-point atomics
 * and no constant is taken from the device; so S_w has the same bits for any chain index or chain count, for a query
 * of all weights or a trace column of some, on every run.  S_w differs from the exactly rounded sum of its n_w terms by
 * at most (n_w + 1) * 2^-53 * sum |term|, and is exact where the terms are integers.
 * The calls follow nsk_log_potential in every rule: `which`, the chains, the handles refused (NSK_E_INVALID), reading
 * without changing anything.  The first one uploads what nsk_log_potential uploads and, in addition, the by-weight list
 * (4 bytes a factor), the work list of the weights asked for (8 bytes a short weight, 16 a piece) and, with `scaled`,
 * the feature values (8 bytes a factor) -- all in nsk_graph_info.device_bytes; NSK_E_NOMEM names the size of what does
 * not fit.  A handle that never calls them allocates and launches nothing for them.
 * nsk_weight_stats: out[i * nweight + w] = S_w of chain first_chain + i.
 * nsk_trace_weight_stats: valid while a trace is set up (NSK_E_INVALID otherwise).  wids = the caller's weight ids
 * (nwids >= 1, repeats allowed, the column order kept; an id outside [0, nweight) is NSK_E_INDEX), or NULL with
 * nwids = 0 for all nweight weights.  Allocates capacity x chains x nwids doubles, zeroed (NSK_E_NOMEM otherwise); from
 * then on every record launch is followed on the stream by the evaluation of the state just recorded, every chain, of
 * the factors of THOSE weights only.  Calling it again replaces the column (a call refused for its arguments leaves the
 * old one); nwids < 0 switches it off and frees it; nsk_trace_setup (replace or tear down) resets it to off;
 * nsk_trace_clear keeps it.  It is independent of the lp column.
 * nsk_trace_download_weight_stats: synchronises, then writes rows first_row .. first_row + nrows - 1 as
 * nrows x chains x nwids doubles; rows beyond those recorded, or no stats column: NSK_E_INVALID.
 * nsk_profile_* keeps counting sweep-kernel launches only. */
int nsk_weight_stats(nsk_graph *g, int which, int64_t first_chain, int64_t nchains, int scaled,
                     double *out /* nchains x nweight */);
int nsk_trace_weight_stats(nsk_graph *g, const int64_t *wids, int64_t nwids, int scaled);
int nsk_trace_download_weight_stats(nsk_graph *g, int64_t first_row, int64_t nrows,
                                    double *out /* nrows x chains x nwids */);

/* Per-variable conditionals (FactorGraph.conditionals / log_pseudo_likelihood / rao_blackwell): the distribution the
 * sampler draws variable v from, P(x_v = k | every other variable), for the variables of a selection.  For a variable
 * of cardinality C that has a position in the compiled layout (every owned variable with isEvidence != 4) and a state x:
 *   potentials     p_k = potential(v, k, x), k = 0 .. C - 1: the reference's potential() with v hypothetically at k --
 *                  the walk of the factor list of (v, k) (one list for dataType 0), every term one rounded product
 *                  weight * eval_factor, added in list order, head quirks as the sampler sees them; the doubles the
 *                  sweep kernels exponentiate;
 *   probabilities  e_k = exp(p_k) by the library's specified exp, unshifted; Z the running sum
 *                  e_0, Z + e_1, ... in k order; P_k = e_k / Z, one IEEE float64 division.  Where Z is 0, infinite or
 *                  NaN the result is whatever IEEE gives: the sampler's own degenerate case.
 * Layout ("full"): selected variable i owns C_i consecutive doubles at off_i = the sum of C_j over j < i, in the
 * caller's order (a binary variable owns 2); total = the sum of all C_i.  A variable without a position reads NaN in all
 * its slots.  vids = the caller's variable ids, any order, repeats allowed; NULL with nvids = 0 = all nvar variables;
 * an id outside [0, nvar) is NSK_E_INDEX; NULL with another count, or a negative count: NSK_E_INVALID.
 * One lane per selected variable (the host sorts the selection by position and drops repeats, and scatters the results
 * back into the caller's order); every double is a function of graph, weights and state only.
 * nsk_conditionals: out[i * total + off_j + k] for chain first_chain + i; what = 0 potentials, 1 probabilities, anything
 * else NSK_E_INVALID.  `which`, the chains, the handles refused (NSK_E_INVALID) and reading without changing anything
 * follow nsk_log_potential rule for rule; the sequential scan is fine.  nvids == 0 with a list, or total == 0, is NSK_OK
 * with nothing done.  The first call uploads what potential() reads and the handle's kernels do not: the lists (4 bytes a
 * position, 4 a list slot + 4, 4 a list entry) and the records nsk_log_potential shares (16 bytes a factor, 8 an edge,
 * 4 a variable, 4 more with literal heads) -- kept, in nsk_graph_info.device_bytes; the selection (12 bytes a
 * variable) and chains x total doubles live for the call only.  NSK_E_NOMEM names the size of what does not fit.  A
 * handle that never calls them allocates and launches nothing for them.
 * nsk_trace_conditionals: Rao-Blackwell accumulators.  Valid while a trace is set up (NSK_E_INVALID otherwise);
 * allocates the selection and chains x total doubles, zeroed, and from then on every record launch is followed on the
 * stream by ONE launch that adds the probabilities of the state just recorded to them, S = S + P_k, every chain,
 * whatever columns the trace keeps: one lane owns a sum and adds once per row, in row order, so a sum equals the
 * sequential sum of the per-row probabilities bit for bit.  Calling it again replaces the selection and zeroes the
 * sums (a call refused for its arguments leaves the old ones); nvids < 0 switches it off and frees them;
 * nsk_trace_setup (replace or tear down) resets it to off; nsk_trace_clear ZEROES the sums and their row count -- unlike
 * the lp and stats columns, which it keeps: those are per row and have nothing to zero.
 * nsk_trace_download_conditionals: synchronises, then writes chains x total sums in the caller's order and *rows (may
 * be NULL) = the rows added since the selection was set or cleared; sums / rows estimates the marginals.
 * NSK_E_INVALID without a selection.  nsk_profile_* keeps counting sweep-kernel launches only. */
int nsk_conditionals(nsk_graph *g, int which, int64_t first_chain, int64_t nchains, const int64_t *vids, int64_t nvids,
                     int what, double *out /* nchains x total */);
int nsk_trace_conditionals(nsk_graph *g, const int64_t *vids, int64_t nvids);
int nsk_trace_download_conditionals(nsk_graph *g, double *sums /* chains x total */, int64_t *rows);

/* Greedy MAP search: iterated conditional modes (FactorGraph.icm / map_estimate).  Deterministic coordinate ascent on the
 * potentials above: no random numbers, no exponential.  One ICM sweep visits the colour classes in colour order, as the
 * chromatic scan does; inside a class every eligible variable is decided in parallel, which equals the sequential
 * decision because a variable reads none of its own class.  Eligible: a variable with a position and isEvidence == 0, or
 * any variable with a position when sample_evidence != 0 (the sweep kernels' test).  For an eligible variable of
 * cardinality C with current value cur and p_k = potential(v, k, x) -- the doubles nsk_conditionals(what = 0) returns:
 *   best = cur, best_p = p_cur when 0 <= cur < C, else best = 0, best_p = p_0;
 *   for k = 0 .. C - 1: if (p_k > best_p) { best = k; best_p = p_k; }
 * A move happens on strict improvement only, the smallest k wins among several maxima, and a NaN potential never wins.
 * The variable takes `best`; a value that differs from cur counts as one change.
 * nsk_icm runs up to max_sweeps sweeps on chains first_chain .. first_chain + nchains - 1, every chain on its own:
 *   sweeps[i]  = the sweeps chain first_chain + i ran up to and including its first sweep without a change (its fixed
 *                point: later sweeps could change nothing), or -max_sweeps when every sweep changed something -- the
 *                chain has NOT converged.  With the literal head lookup potential() is not the gradient of one energy,
 *                so cycles are possible; the negative count is how they are reported;
 *   changed    (may be NULL) [i * max_sweeps + s] = the changes of sweep s; 0 from the fixed point on.
 * All max_sweeps x ncolors launches are enqueued on the handle's stream without returning to the host; a chain that has
 * reached its fixed point ends its later launches on the device after one load.  The counters are integers: the result
 * does not depend on any order of execution.
 * `which`, the chains and the handles refused (NSK_E_INVALID) follow nsk_log_potential rule for rule; the sequential scan
 * is fine (the sweep is the chromatic one either way).  max_sweeps outside [1, 4096] and sweeps == NULL are
 * NSK_E_INVALID.  A handle with partial factors (nsk_pf_setup) is served: that set-up caches nothing that depends on the
 * values -- the aggregates are recomputed from the values at every exchange, before they are pushed.  A handle with a
 * sample trace is served; its rows and columns are untouched.
 * The call changes the values of the chains named and nothing else: tallies (a tally kept in the value bytes is first
 * brought back to its array, as before a state download), sweeps_done, the generator state and the weights stay.  The
 * first call uploads what nsk_conditionals uploads, or finds it in place; the counters (8 bytes x max_sweeps x nchains)
 * live for the call only; NSK_E_NOMEM names the size of what does not fit.  nsk_profile_* keeps counting sweep-kernel
 * launches only. */
int nsk_icm(nsk_graph *g, int which, int64_t first_chain, int64_t nchains, int64_t max_sweeps, int sample_evidence,
            int64_t *sweeps /* nchains */, int64_t *changed /* nchains x max_sweeps, may be NULL */);

/* Loopy belief propagation (FactorGraph.belief_propagation): sum-product message passing on the factor graph, flooding
 * schedule -- deterministic inference beside the sampler.  Exact on forests (after clamping), an approximation that may
 * not converge on graphs with cycles.  numbskull_amd.diagnostics.bp_layout / bp_iterate / bp_factor_beliefs are the rule
 * in numpy, bit for bit: every sum and product is taken in the order stated here, the exponential is the library's
 * specified one, nothing is fused or reassociated.
 * Scope: ONE state -- chain `chain` of NSK_BUF_VALUE or the evidence chain (NSK_BUF_VALUE_EVID, chain 0) -- under the
 * current weights.  A variable is CLAMPED at its value in that state when the sweep kernels would not sample it: without
 * a position (isEvidence == 4), or isEvidence != 0 with sample_evidence == 0; every other variable is FREE.
 * Structure, per factor f in the caller's order: its member positions are its `arity` edge positions (a function that
 * reads positions beyond its arity -- EQUAL reads 1, the DP_GEN_* functions 1 to 3 -- has those too; NOOP has none); its
 * DISTINCT members in order of first occurrence get the local slots 0, 1, ..; the free ones among them, in that order,
 * are the table's axes j = 0 .. A_f - 1, the first the most significant digit of a table index (C order); T_f = the
 * product of their cardinalities (1 without a free member, and then no edge).  Directed edges (f, j) are numbered
 * factor-major; edge e owns card(var(e)) doubles at msg_off[e] in each message array, f2v (factor to variable) and v2f.
 * Tables: theta_f(a) = weight * eval_factor, ONE rounded product, the factor asked as its first member sees it, the
 * free members at the digits of a, the clamped ones at their values; psi_f(a) = exp(theta_f(a) - max_a theta_f).
 * Messages start at 1 / card.  Iteration t:
 *   factor phase, per edge (f, j): m[k] = the sum over the table indices a with digit j equal to k, ascending, of
 *     ((psi_f(a) * v2f[(f,0)][a_0]) * ..) over the axes i != j ascending; Z = m[0] + m[1] + .. in k order;
 *     new[k] = m[k] / Z; with damping d > 0, new[k] = (1 - d) * new[k] + d * old[k] (two products, one sum; 1 - d
 *     computed once); the edge's residual is the largest |new[k] - old[k]|, a NaN counting as +inf; residual[t] = the
 *     largest over all edges;
 *   variable phase, per free variable with the edges e_0 < .. < e_{n-1}: P = all ones; for i ascending: v2f[e_i] = P,
 *     then P = P * f2v[e_i] entry by entry, then RESCALE(P): while the largest entry is > 0 and < 2^-512, every entry
 *     times 2^512 (exact).  belief = P / (P[0] + P[1] + ..).  Then S = all ones; for i descending: v2f[e_i] = v2f[e_i] * S,
 *     RESCALE, divided by its k-ordered sum; S = S * f2v[e_i], RESCALE.  (The product of all others, without a division.)
 * A clamped variable's belief is the indicator of its value, a free variable in no table has the uniform one.  Two hard
 * constraints that contradict each other give what IEEE gives (0 / 0 = NaN), as the conditionals do.
 * Factor beliefs: b_f(a) = (psi_f(a) * v2f[(f,0)][a_0]) * .., divided by their a-ordered sum.
 *   nsk_bp_setup     builds structure and tables for the state named and resets the messages; *info (may be NULL) = the
 *                    sizes.  A set-up that was there is replaced.  Refused, naming the lowest offending factor and before
 *                    anything is allocated: more than NSK_BP_MAX_MEMBERS distinct members, T_f > NSK_BP_MAX_TABLE, UFO
 *                    (it reads members by value), a factor of function 13, 16 or 17 on a handle without
 *                    NSK_FLAG_HEAD_BY_VID (the literal head lookup has no single energy), an index outside the arrays.
 *   nsk_bp_layout    table_off[nfactor + 1], edge_off[nfactor + 1], edge_var[nedges] (the caller's ids), msg_off[nedges + 1];
 *                    any may be NULL.
 *   nsk_bp_run       up to max_iters (1 .. 4096) iterations from the resident messages, damping in [0, 1), tol >= 0.
 *                    Everything is enqueued at once; the kernels of iteration t >= 1 return at once when
 *                    residual[t - 1] <= tol.  *iters = the iterations run up to and including the first with
 *                    residual <= tol, or -max_iters when there is none: NOT converged.  residual (may be NULL)
 *                    [max_iters]: 0 behind the early exit.  May be called again: it continues.
 *   nsk_bp_beliefs   the "full" layout of the conditionals above: variable i of the selection owns C_i doubles; vids as
 *                    there (NULL with nvids = 0 = all variables).
 *   nsk_bp_download  what = NSK_BP_THETA, NSK_BP_FACTOR_BELIEFS (computed by the call; both table_off's layout),
 *                    NSK_BP_F2V, NSK_BP_V2F (msg_off's layout).
 *   nsk_bp_clear     frees the set-up (NSK_OK without one).
 *   nsk_bp_select    a handle holds TWO resident set-ups, slots 0 and 1, and one of them is selected: slot 0 on a new
 *                    handle.  Every nsk_bp_* call above and below -- setup, layout, run, beliefs, download, refresh,
 *                    moments, learn_steps, clear -- acts on the selected set-up and on nothing else; the other keeps its
 *                    tables, messages, beliefs and bytes.  A slot outside {0, 1} is NSK_E_INVALID.  The call moves no
 *                    data and waits for nothing.  nsk_bp_clear frees only the selected set-up, nsk_graph_destroy both;
 *                    nsk_graph_info.device_bytes counts both, nsk_bp_info.device_bytes each its own.  The two share
 *                    nothing; only nsk_bp_latent_steps reads both.
 *   nsk_bp_selected  the selected slot.
 * Run, beliefs, layout and download without a set-up are NSK_E_INVALID.  `which` and the handles refused follow
 * nsk_log_potential; a tally kept in the value bytes is first brought back to its array, as in nsk_icm.  Nothing of the
 * handle changes: values, tallies, weights and the generator stay.  The set-up is resident and counted in
 * nsk_graph_info.device_bytes: 24 bytes a table entry (theta, psi and the feature table below), 16 a message entry + 20 an edge, 8 a member position + 8 a distinct
 * member, 24 a factor, 17 a variable + 8 a value (16 where a free variable of cardinality above 16 has an edge); NSK_E_NOMEM names the
 * bytes.  nsk_profile_* keeps counting sweep-kernel launches only.  (Diagnostic, NSK_DIAG=1 NSK_BP_GRID_CAP=blocks,
 * read at each call: caps every grid of these calls, so that small graphs run the later trips of the lanes' loops.) */
#define NSK_BP_MAX_MEMBERS 16
#define NSK_BP_MAX_TABLE 4096
#define NSK_BP_THETA 0
#define NSK_BP_FACTOR_BELIEFS 1
#define NSK_BP_F2V 2
#define NSK_BP_V2F 3
typedef struct {
    int64_t nfactor, nedges, ntable, nmsg;      /* factors, directed edges, table entries, doubles of one message array */
    int64_t nfree, nisolated, nclamped;         /* free variables; those among them in no table; clamped variables */
    int64_t nbelief, max_table, device_bytes;   /* doubles of all beliefs; the largest T_f; bytes the set-up holds */
} nsk_bp_info;
int nsk_bp_setup(nsk_graph *g, int which, int64_t chain, int sample_evidence, nsk_bp_info *info);
int nsk_bp_layout(nsk_graph *g, int64_t *table_off, int64_t *edge_off, int64_t *edge_var, int64_t *msg_off);
int nsk_bp_run(nsk_graph *g, int64_t max_iters, double damping, double tol, int64_t *iters,
               double *residual /* max_iters, may be NULL */);
int nsk_bp_beliefs(nsk_graph *g, const int64_t *vids, int64_t nvids, double *out /* total */);
int nsk_bp_download(nsk_graph *g, int what, double *out);
int nsk_bp_clear(nsk_graph *g);
int nsk_bp_select(nsk_graph *g, int slot);
int nsk_bp_selected(nsk_graph *g);

/* Learning by belief propagation (FactorGraph.bp_weight_moments / learn_bp): maximum-likelihood learning whose model
 * expectations come from the factor beliefs of the resident set-up above instead of from chains -- exact wherever BP is
 * exact (the free variables form a forest), the Bethe approximation on graphs with cycles, without sampling noise.
 * Every call here acts on the selected resident set-up (nsk_bp_select) and is NSK_E_INVALID without one, as nsk_bp_run is.
 * Feature table: feat_f(a) = eval_factor exactly as the set-up asks it for theta_f(a), without the weight, so that
 * theta_f(a) = w[weight of f] * feat_f(a) is ONE rounded product and reproduces the set-up's own theta bit for bit.  The
 * set-up fills it in the launch that fills theta (no further launch), owns it (nsk_bp_clear and a replacing set-up free
 * it) and counts its 8 bytes a table entry among its bytes above.
 * nsk_bp_refresh: theta[i] = w[slot] * feat[i] from the device weight table as it stands, then psi as the set-up forms
 *   it; messages and beliefs stay.  How a caller continues nsk_bp_run after uploading new weights (enqueued; no wait).
 * nsk_bp_moments: the expected per-weight statistics under the factor beliefs, in the int64 fixed point of
 *   nsk_weight_moments.  Per factor f, x(a) = (psi_f(a) * v2f[(f,0)][a_0]) * .. and Z_f = their a-ordered sum, exactly as
 *   the factor beliefs above form them.  A factor whose Z_f is not a finite positive number (two hard constraints that
 *   contradict each other: NaN) is SKIPPED: it adds nothing and counts one in *skipped (may be NULL).  Otherwise per entry
 *     b = x(a) / Z_f            the very bits of NSK_BP_FACTOR_BELIEFS
 *     p = b * feat_f(a)         one rounded product
 *     q = p * 2^32 rounded to the nearest int64, ties to even (numpy: np.rint(p * 2.0**32).astype(np.int64))
 *     M[weight of f] += q       int64: the order of execution is free
 *   M_w * 2^-32 is E_b[S_w] to within 2^-33 per table entry.  A factor without a free member (T_f = 1) contributes
 *   rint(e * 2^32): where every variable is clamped M equals nsk_weight_moments of that state integer for integer.
 *   moments[nweight] in the caller's weight ids; a weight without a factor reads 0.  NSK_E_RANGE: the rule of
 *   nsk_weight_moments with nchains = 1 (|b * feat| <= vmax(f)).  numbskull_amd.diagnostics.bp_moment_counts is the rule
 *   in numpy.  The sums, the counter and Z_f (8 bytes a factor) live for the call only.
 * nsk_bp_learn_steps: for t = 0 .. nsteps - 1, on the handle's stream without a host wait:
 *   1. nsk_bp_refresh; with warm == 0 also every message back to 1 / card;
 *   2. up to iters_per_step iterations exactly as nsk_bp_run enqueues them, with row t of the residuals: the early exit
 *      applies inside the row, iteration 0 of every step always runs;
 *   3. zero M and the skip counter, then the launches of nsk_bp_moments;
 *   4. nsk_pcd_steps' update launch with one chain (a division by 1.0 is exact): target, n_w, step_t = step * decay^t
 *      formed on the host in t order, reg_param and normalize as there; numbskull_amd.diagnostics.pcd_step with R = 1.
 *   After the last step one more refresh, so that the resident tables agree with the device weights and a following
 *   nsk_bp_run continues under the learned weights; then the call synchronises, once.  gmax[t] and moments[t * nweight
 *   + w] are what nsk_pcd_steps defines; iters[t] follows nsk_bp_run (negative: the step's iterations did not reach tol);
 *   residual[t * iters_per_step + i]; skipped[t].  Each output may be NULL.  The weights on the device change (fixed
 *   weights stay; the next sweep call rebuilds what derives from them); values, tallies, sweeps_done, the generator and
 *   the trace stay.  NSK_E_INVALID, before anything is allocated or enqueued: no set-up, a null target or a target entry
 *   that is not finite, nsteps or iters_per_step outside [1, 4096], nsteps x iters_per_step > 65536, damping or tol
 *   outside what nsk_bp_run accepts, warm or normalize other than 0 or 1, a step, decay or reg_param that is not
 *   finite, reg_param < 0.  NSK_E_RANGE as nsk_bp_moments.  nweight == 0 is NSK_OK with nothing done.  The sums, the
 *   target, the factor counts, Z_f and the per-step outputs live for the call only; NSK_E_NOMEM names the bytes.
 * nsk_bp_latent_steps: learning with LATENT variables, the gradient "statistics with the evidence held - statistics
 *   with everything free" from two set-ups instead of from two populations of chains (nsk_pcd_latent_steps).  Slot 0 is
 *   the positive phase, by convention set up with sample_evidence = 0 (evidence held, latent variables free), slot 1 the
 *   negative phase, set up with sample_evidence = 1; both must be set up, otherwise NSK_E_INVALID.  There is no target.
 *   For t = 0 .. nsteps - 1, on the handle's stream without a host wait:
 *   1. both set-ups refreshed from the device weights; with warm == 0 both message sets back to 1 / card;
 *   2. up to iters_per_step iterations of both, each set-up with its own row of residuals and its own early exit: one
 *      that has reached tol stops while the other goes on; iteration 0 of every step always runs for both;
 *   3. the Bethe moments of slot 0 into Mc and of slot 1 into M, the rule of nsk_bp_moments bit for bit, a skip counter
 *      per set-up;
 *   4. nsk_pcd_latent_steps' update launch with one chain a side: pos = (Mc * 2^-32) / 1.0, m = (M * 2^-32) / 1.0,
 *      g = pos - m, then as nsk_pcd_steps; step_t = step * decay^t formed on the host in t order;
 *      numbskull_amd.diagnostics.pcd_latent_step with K = Rf = 1.
 *   After the last step both set-ups are refreshed once more, then the call synchronises, once.  The two phases of a
 *   step share their launches (gridDim.y = 2, the grid what the larger set-up needs): a step costs the launches of one
 *   nsk_bp_learn_steps step, and each set-up computes what it computes alone, bit for bit.  In every output with an axis
 *   of 2, index 0 is the clamped set-up and index 1 the free one: iters[nsteps x 2], residual[nsteps x 2 x
 *   iters_per_step], skipped[nsteps x 2], moments[nsteps x 2 x nweight] (the clamped row first); gmax[nsteps].  Each may be
 *   NULL.  NSK_E_INVALID, before anything is allocated or enqueued: what nsk_bp_learn_steps refuses, without the target.
 *   NSK_E_RANGE as nsk_bp_moments.  nweight == 0 is NSK_OK with nothing done.  The sums, the factor counts, Z_f and the
 *   per-step outputs live for the call only; NSK_E_NOMEM names the bytes.  The weights change as in nsk_bp_learn_steps;
 *   the selected slot is the same after the call as before.
 * Every launch honours NSK_BP_GRID_CAP. */
int nsk_bp_refresh(nsk_graph *g);
int nsk_bp_moments(nsk_graph *g, int64_t *moments /* nweight */, int64_t *skipped /* may be NULL */);
int nsk_bp_learn_steps(nsk_graph *g, const double *target /* nweight, caller's ids */,
                       int64_t nsteps, int64_t iters_per_step, double damping, double tol, int warm,
                       double step, double decay, double reg_param, int normalize,
                       double *gmax /* nsteps */, int64_t *iters /* nsteps */, double *residual /* nsteps x iters_per_step */,
                       int64_t *moments /* nsteps x nweight */, int64_t *skipped /* nsteps */);
int nsk_bp_latent_steps(nsk_graph *g, int64_t nsteps, int64_t iters_per_step, double damping, double tol, int warm,
                        double step, double decay, double reg_param, int normalize,
                        double *gmax /* nsteps */, int64_t *iters /* nsteps x 2 */,
                        double *residual /* nsteps x 2 x iters_per_step */,
                        int64_t *moments /* nsteps x 2 x nweight */, int64_t *skipped /* nsteps x 2 */);

/* Pseudo-likelihood gradient and maximum pseudo-likelihood learning (FactorGraph.pl_gradient / learn_mple): the
 * derivative of sum_v log P(x_v | every other variable) over a selection of variables with respect to every weight, and
 * the deterministic, sampling-free learner built on it.  No random number is drawn and no logarithm is taken on the
 * device.  For a state x, the weight table w and a selected variable v that has a position, of cardinality C and own
 * value cur = x_v: P_k, k = 0 .. C - 1, are the very bits nsk_conditionals(what = 1) returns for v.  The variable is
 * SKIPPED when cur lies outside [0, C) or Z is not a finite positive number: it contributes nothing and adds one to the
 * chain's `skipped`.  Otherwise, for k = 0 .. C - 1 and every entry f of the factor list of (v, k) (one list for
 * dataType 0):
 *   c_k = (k == cur ? 1.0 : 0.0) - P_k        one rounded subtraction
 *   e   = eval_factor(f, v, k, x)             as potential() calls it, head quirks included
 *   t   = c_k * e                             one rounded product
 *   q   = t * 2^32 rounded to the nearest int64, ties to even (numpy: np.rint(t * 2.0**32).astype(np.int64))
 *   G[weight of f] += q                       int64
 * G_w * 2^-32 is the derivative with respect to weight w, to within 2^-33 per term.  The sums are integers, so no order
 * of execution changes a bit (numbskull_amd.diagnostics.pl_gradient_counts is the rule in numpy).  Fixed weights get
 * their sum like any other; featureValue plays no part, as in potential().  With the literal head lookup (IMPLY_MLN-type
 * functions without NSK_FLAG_HEAD_BY_VID) this is the derivative of the sum of the SAMPLER'S OWN conditionals, which is
 * then not the derivative of the pseudo-likelihood of one joint energy -- the limit nsk_icm states.
 * vids = the caller's variable ids in any order, NULL with nvids = 0 for all nvar variables; an id outside [0, nvar) is
 * NSK_E_INDEX, a repeated id NSK_E_INVALID (the selection is a set); a variable without a position contributes nothing
 * and is not counted in N below.  `which`, the chains and the handles refused (NSK_E_INVALID) follow nsk_conditionals /
 * nsk_log_potential rule for rule; the sequential scan is fine, several chains are served, a handle with a sample trace
 * is served and its rows and columns are untouched; a tally kept in the value bytes is first brought back to its array,
 * as in nsk_icm.
 * Range, decided before any launch from the graph and the selection alone: with B_w = the sum over the selected
 * variables' list entries naming weight w of m * vmax(f) -- m = 2 for an entry of a dataType-0 list, 1 for a dataType-1
 * one; vmax = arity for LINEAR, log(arity + 1) for RATIO, 1e6 for UFO, 1 otherwise -- the call is NSK_E_RANGE when
 * B_w * nchains >= 2^30 for some w.
 * nsk_pl_gradient: grad_q[i * nweight + w] = G_w of chain first_chain + i, in the caller's weight ids (slots are mapped
 * back as nsk_state_download maps the weights); grad = (double)grad_q * 2^-32; skipped[i] = the chain's skips.  Each of
 * the three may be NULL.  It changes nothing.
 * nsk_mple_steps: nsteps gradient-ascent steps on the mean log-pseudo-likelihood of the chains named, every chain one
 * training example.  N = (selected variables with a position) * nchains.  For t = 0 .. nsteps - 1, on the handle's
 * stream and without a host wait: zero G; the gradient launch above; then per weight slot, with S = the int64 sum of G
 * over the chains (exact) and step_0 = step, step_{t+1} = step_t * decay (the products formed on the host in t order):
 *   gbar = ((double)S * 2^-32) / N            one conversion, an exact scaling, one rounded division
 *   a = reg_param * w;  b = gbar - a;  c = step_t * b;  w = w + c      one rounded operation each
 * -- not for a fixed weight, which stays -- and gmax[t] = the largest |S| over the weights that are not fixed,
 * skipped[t] = the skips of step t summed over the chains (numbskull_amd.diagnostics.mple_step is the update in numpy).
 * The call synchronises once and downloads gmax and skipped (each may be NULL).  It leaves the new weights in the
 * device table, marked so that the next sweep call rebuilds what derives from them, and changes nothing else: values,
 * tallies, sweeps_done, the generator state and the trace stay.  nsteps outside [1, 65536], a step, decay or reg_param
 * that is not finite, or reg_param < 0: NSK_E_INVALID.  N == 0 is NSK_OK with nothing done.
 * Memory: the first call uploads what nsk_conditionals uploads, or finds it in place; the selection (4 bytes a
 * variable), chains x (nweight + 1) int64 and the per-step outputs (16 bytes a step) live for the call only, so
 * nsk_graph_info.device_bytes is afterwards what a nsk_conditionals call leaves.  NSK_E_NOMEM names the size of what
 * does not fit.  nsk_profile_* keeps counting sweep-kernel launches only.  A handle that never calls these allocates
 * and launches nothing for them. */
int nsk_pl_gradient(nsk_graph *g, int which, int64_t first_chain, int64_t nchains, const int64_t *vids, int64_t nvids,
                    int64_t *grad_q /* nchains x nweight, may be NULL */, double *grad /* same shape, may be NULL */,
                    int64_t *skipped /* nchains, may be NULL */);
int nsk_mple_steps(nsk_graph *g, int which, int64_t first_chain, int64_t nchains, const int64_t *vids, int64_t nvids,
                   int64_t nsteps, double step, double decay, double reg_param,
                   int64_t *gmax /* nsteps, may be NULL */, int64_t *skipped /* nsteps, may be NULL */);

/* Chain-summed moments and persistent contrastive divergence (FactorGraph.weight_moments / learn_pcd): full-batch
 * maximum-likelihood learning in which the handle's R chains (nsk_set_chains) are the persistent "fantasy particles".
 * Fixed-point moments: for a state x and a factor f, e_f = eval_factor(f, x) exactly as nsk_log_potential asks every
 * factor, as its first member sees it;
 *   q_f = e_f * 2^32 rounded to the nearest int64, ties to even (numpy: np.rint(e * 2.0**32).astype(np.int64))
 *   M_w = the sum over the chains named and over the factors f with weightId == w of q_f(x_chain)        int64
 * featureValue plays no part, as in potential(); a weight without a factor reads 0.  The sums are integers, so no order
 * of execution changes a bit (numbskull_amd.diagnostics.moment_counts is the rule in numpy), and ONE accumulator of
 * nweight x 8 bytes serves any number of chains: nothing is allocated as chains x nweight.  One lane per weight of at
 * most 16 factors, one wave per piece of at most 2048 factors of a longer one -- the cuts of nsk_weight_stats --, each
 * over its share of the chains; a wave adds its lanes' integers and issues at most one 64-bit global atomic per weight it
 * holds, a block's waves that end on the same weight one between them.
 * Range, decided before any launch from the graph alone: with B_w = the sum over the factors of w of vmax(f) -- vmax as
 * nsk_pl_gradient defines it: arity for LINEAR, log(arity + 1) for RATIO, 1e6 for UFO, 1 otherwise -- the call is
 * NSK_E_RANGE when B_w * nchains >= 2^30 for some w.
 * nsk_weight_moments: moments[w] = M_w over chains first_chain .. first_chain + nchains - 1, in the caller's weight ids.
 * `which`, the chains, the handles refused (NSK_E_INVALID) and reading without changing anything follow nsk_weight_stats
 * rule for rule; it is not a sweep, so the sequential scan is fine; a tally kept in the value bytes is first brought back
 * to its array, as in nsk_icm.
 * nsk_pcd_steps: nsteps steps over ALL chains of the handle, R = nsk_get_chains.  For t = 0 .. nsteps - 1, on the handle's
 * stream and without a host wait:
 *   1. what nsk_gibbs_sweeps(g, sweeps_per_step, sample_evidence, burnin = 1) enqueues -- it rebuilds what derives from
 *      the weights first, which every step leaves marked;
 *   2. zero M, then the moment launches over all R chains;
 *   3. one update launch, per weight slot that is not fixed, every line ONE rounded IEEE operation:
 *        m = ((double)M * 2^-32) / R              one conversion, an exact scaling, one division
 *        g = target_w - m
 *        if (normalize) g = g / n_w               n_w = the factors of w (a weight without a factor: n_w = 1)
 *        a = reg_param * w;  b = g - a;  c = step_t * b;  w = w + c
 *      with step_0 = step, step_{t+1} = step_t * decay (the products formed on the host in t order).
 * gmax[t] = the largest |g| over the weights that are not fixed, after the normalisation and before the penalty (0 when
 * every weight is fixed); moments[t * nweight + w] = that step's M_w in the caller's weight ids
 * (numbskull_amd.diagnostics.pcd_step is the update in numpy).  The fixed point of the iteration is where the model's
 * mean statistics equal the target: the maximum-likelihood estimate when the target is the data's mean statistics.
 * The call synchronises once and downloads gmax and moments (each may be NULL).  It leaves the new weights in the device
 * table, marked so that the next sweep call rebuilds what derives from them; the chains where the last sweep left them;
 * sweeps_done advanced by nsteps * sweeps_per_step.  Tallies are untouched (a tally kept in the value bytes is unpacked
 * first, as in nsk_tempered_sweeps), and a sample trace keeps its rows and columns: burn-in sweeps record nothing.
 * NSK_E_INVALID, before anything is enqueued and with the handle left as it was: a null graph or target; a target entry
 * that is not finite; nsteps outside [1, 65536]; sweeps_per_step < 1 or nsteps * sweeps_per_step > 2^31 - 1; a step,
 * decay or reg_param that is not finite, or reg_param < 0; normalize other than 0 or 1; the sequential scan; every
 * handle nsk_log_potential refuses.  NSK_E_RANGE: the rule above with nchains = R.  nweight == 0 is NSK_OK with nothing
 * done.
 * Memory: the first call uploads what nsk_weight_stats(scaled = 0) uploads short of its work list and result, or finds
 * it in place.  The accumulator (8 bytes a weight), the work list by weight slot (8 bytes a short weight, 16 a piece),
 * the target and the factor counts (16 bytes a weight) and the per-step outputs (8 bytes a step, and 8 x nsteps x nweight
 * only when moments is asked for) live for the call only, so nsk_graph_info.device_bytes is afterwards what a
 * nsk_weight_stats call leaves.  NSK_E_NOMEM names the size of what does not fit.  nsk_profile_* keeps counting
 * sweep-kernel launches only.  A handle that never calls these allocates and launches nothing for them. */
int nsk_weight_moments(nsk_graph *g, int which, int64_t first_chain, int64_t nchains,
                       int64_t *moments /* nweight, caller's weight ids */);
int nsk_pcd_steps(nsk_graph *g, const double *target /* nweight, caller's weight ids */,
                  int64_t nsteps, int64_t sweeps_per_step, int sample_evidence,
                  double step, double decay, double reg_param, int normalize,
                  double *gmax /* nsteps, may be NULL */,
                  int64_t *moments /* nsteps x nweight, may be NULL */);

/* PCD with latent variables (FactorGraph.learn_pcd(clamped = K)): a clamped and a free population of chains on one handle.
 * With latent variables the gradient of the log-likelihood of the evidence is E[S_w | evidence] - E[S_w], and BOTH
 * expectations move with the weights; nsk_pcd_steps' constant target is right for fully observed data only.  With
 * R = nsk_get_chains(g), K = nclamped and k = sweeps_per_step, chains [0, K) are the CLAMPED population -- they sample
 * the latent variables with the evidence held -- and chains [K, R) the FREE one.
 * clamp = 1: before the first step one launch writes initialValue into every variable with isEvidence 1, 2 or 3 of every
 * clamped chain (a list of {internal id, value} pairs uploaded for the call).  clamp = 0: the rows are trusted as they
 * are -- each clamped chain may hold the evidence of another training example.
 * With s0 the handle's sweep index at the call, for t = 0 .. nsteps - 1, on the handle's stream and without a host wait:
 *   1. clamped phase: what nsk_gibbs_sweeps(g, k, sample_evidence = 0, burnin = 1) enqueues on a handle that has the
 *      chains [0, K) and no other, at sweep indices s0 + 2kt .. s0 + 2kt + k - 1; the tables derived from the weights are
 *      rebuilt first, as every step leaves them marked;
 *   2. free phase: what nsk_gibbs_sweeps(g, k, free_sample_evidence, 1) enqueues on a handle that has the chains [K, R)
 *      and no other, at sweep indices s0 + 2kt + k .. s0 + 2k(t + 1) - 1;
 *   3. zero Mc and Mf, then the moment launches of nsk_weight_moments over the clamped chains into Mc and over the free
 *      chains into Mf: its rule, bit for bit, on two accumulators of nweight x 8 bytes;
 *   4. one update launch, per weight slot that is not fixed, every line ONE rounded IEEE operation:
 *        mc = ((double)Mc * 2^-32) / K
 *        mf = ((double)Mf * 2^-32) / (R - K)
 *        g  = mc - mf
 *        if (normalize) g = g / n_w
 *        a = reg_param * w;  b = g - a;  c = step_t * b;  w = w + c
 *      with step_0 = step, step_{t+1} = step_t * decay (the products formed on the host in t order): nsk_pcd_steps' update
 *      with target = mc and R - K chains (numbskull_amd.diagnostics.pcd_latent_step is the rule in numpy).
 * Generators: within a phase, local chain i of its population (global chain i, or K + i) draws what a one-chain handle
 * seeded seed ^ ((uint64_t)i << 32) draws at the phase's sweep indices -- what the sweep kernels make of the launch-local
 * chain index, so no sweep kernel and no kernel argument knows of the populations.  Clamped chain i and free chain i
 * share a key and never a sweep index, so they share no uniform.  Each phase takes the launches its population would
 * take as a handle of its own: the chain-batched table launches, chain after chain otherwise, the one-chain launches for
 * a population of one; never a captured sequence.  The phases plan their launches anew when their sample_evidence flags
 * differ (host work only), which drops the captured sequences of later plain calls; they are captured again on demand.
 * gmax[t] = the largest |g| over the weights that are not fixed, found as nsk_pcd_steps finds it; moments[(2 t) * nweight
 * + w] = that step's Mc_w and moments[(2 t + 1) * nweight + w] = its Mf_w, in the caller's weight ids.
 * The call synchronises once.  It leaves the new weights in the device table, marked so that the next sweep call rebuilds
 * what derives from them; the chains where the last sweeps left them; sweeps_done and the sweep index advanced by
 * 2 * k * nsteps.  Tallies are untouched (a tally kept in the value bytes is unpacked first), a sample trace keeps its
 * rows and columns, and nsk_graph_info.device_bytes is afterwards what a nsk_weight_stats call leaves.
 * NSK_E_INVALID, before anything is enqueued and with the handle left as it was: everything nsk_pcd_steps refuses (there
 * is no target); nclamped outside [1, R - 1], so R >= 2; clamp or normalize other than 0 or 1; 2 * nsteps * k > 2^31 - 1.
 * NSK_E_RANGE: the rule of nsk_weight_moments with nchains = max(K, R - K).  nweight == 0 is NSK_OK with nothing done. */
int nsk_pcd_latent_steps(nsk_graph *g, int64_t nclamped, int clamp,
                         int64_t nsteps, int64_t sweeps_per_step, int free_sample_evidence,
                         double step, double decay, double reg_param, int normalize,
                         double *gmax /* nsteps, may be NULL */,
                         int64_t *moments /* nsteps x 2 x nweight, may be NULL */);

/* Tempered sweep schedules (FactorGraph.tempered_sweeps / log_partition / log_evidence / anneal): sweeps at an inverse
 * temperature beta, driven by a schedule.  potential() is linear in the weights, so sampling from exp(beta U) / Z_beta,
 * U the log-potential above, IS sampling under the weight table beta * w: one beta per step, shared by every chain,
 * needs no other sweep kernel, draw table, plan or captured sequence.  The call acts on ALL chains of the handle (R =
 * nsk_get_chains).  With w_base the device weight table as it stands when the call begins, slot by slot, for
 * t = 0 .. nsteps - 1, in this order on the handle's stream and without a host wait between steps:
 *   1. scale  w[s] = betas[t] * w_base[s] for every slot, fixed weights included: one rounded float64 product;
 *   2. sweep  exactly what nsk_gibbs_sweeps(g, sweeps_per_step, sample_evidence, 1) enqueues under those weights -- the
 *             same sweep indices, generators, plans and captured sequences, the tables derived from the weights
 *             rebuilt first; nothing is tallied, no trace row is recorded or counted; sweeps_done and the sweep index
 *             advance by sweeps_per_step;
 *   3. score  U_t[r] = the log-potential of chain r's state under w_base (NOT the scaled table), with the very bits
 *             nsk_log_potential returns for that state and those weights; lp[t * R + r] = U_t[r];
 *   4. fold   if t + 1 < nsteps: log_weight[r] = log_weight[r] + (betas[t + 1] - betas[t]) * U_t[r] -- one rounded
 *             difference, one rounded product, one rounded addition, from 0.0, in t order, one lane per chain.  With a
 *             schedule from 0 to 1 these are the log importance weights of annealed importance sampling: log Z =
 *             log Z_0 + log mean_r exp(log_weight[r]), Z_0 the number of states of the variables the sweeps sample
 *             (numbskull_amd.diagnostics.ais_estimate);
 *   5. best   only when best_values or best_lp is asked for: at step 0 chain r's state and U_0[r] are kept
 *             unconditionally; afterwards the state replaces the kept one when U_t[r] > best strictly -- the earliest
 *             maximum wins, a NaN never wins.  The copy is device to device, decided on the device per chain.
 * Then w = w_base again, bit for bit (a copy, no division), the handle is marked so that a following sweep call rebuilds
 * the tables under the base weights, and the call synchronises ONCE and downloads what was asked for: log_weight
 * (R), lp (nsteps x R), best_lp (R), and best_values (R x nvar) through the gather of nsk_chains_download -- the
 * caller's variable ids, int64.  Each of the four may be NULL.  The values of the chains are left as the last step's
 * sweeps leave them; tallies, trace rows and columns, and the evidence chain are untouched (a handle with a sample trace
 * is served; a tally kept in the value bytes is first brought back to its array, as in nsk_icm).  If anything fails after
 * the first scale, the base weights are still restored before the error is returned.  While the call runs, a pointer
 * from nsk_device_buffer(NSK_BUF_WEIGHT) sees the SCALED table.
 * exp is unshifted, as in the sampler: a beta that overflows it is the sampler's own degenerate case.  With the literal
 * head lookup (IMPLY_MLN-type functions without NSK_FLAG_HEAD_BY_VID) potential() is not the gradient of one energy, the
 * sampler's stationary law is not exp(U) / Z, and the estimate has no meaning for such graphs (the limit nsk_icm states).
 * NSK_E_INVALID, before anything is enqueued and with values, weights, sweeps_done and the generator untouched: a null
 * graph or betas == NULL; nsteps outside [1, 65536]; sweeps_per_step < 1 or nsteps * sweeps_per_step > INT32_MAX; a beta
 * that is NaN, infinite or negative (the order is free: annealing goes past 1, a reverse run goes down); the
 * sequential scan; the handles nsk_log_potential refuses (own_range / NSK_FLAG_PARTITION, a boundary exchange).
 * Memory: the first call uploads what nsk_log_potential uploads, or finds it in place, and that stays; a call that asks
 * for best_values sets up the staging buffers of the state transfers where no transfer has yet, and they stay too.  The
 * copy of the base weights (8 bytes a weight), lp, log_weight, the flags and best log-potentials (12 bytes a chain) and
 * the best states (R x the bytes of a chain's values, rounded up to 16; only with best_values) live for the call only:
 * nsk_graph_info.device_bytes is afterwards what it was.  NSK_E_NOMEM names the size of what does not fit.
 * nsk_profile_* keeps counting sweep-kernel launches only. */
int nsk_tempered_sweeps(nsk_graph *g, const double *betas /* nsteps */, int64_t nsteps, int64_t sweeps_per_step,
                        int sample_evidence, double *log_weight /* chains, may be NULL */,
                        double *lp /* nsteps x chains, may be NULL */,
                        int64_t *best_values /* chains x nvar, the caller's ids, may be NULL */,
                        double *best_lp /* chains, may be NULL */);

/* Population annealing (FactorGraph.smc_sweeps / log_partition(resample=...) / log_evidence(resample=...)): the tempered
 * schedule above with the resampling step of sequential Monte Carlo between its steps.  Plain annealed importance
 * sampling anneals every chain on its own and averages the weights at the end; where a few chains carry almost all the
 * weight, the heavy chains are here duplicated over the light ones on the device and the run goes on with equal weights.
 * The call acts on ALL chains of the handle (R = nsk_get_chains, at most 1024).  For t = 0 .. nsteps - 1, on the handle's
 * stream and without a host wait, steps 1. - 4. of nsk_tempered_sweeps exactly as stated there -- scale, sweep, score under
 * w_base, fold: the same kernels, launches, sweep indices and bits -- and then, if t + 1 < nsteps:
 *   5. decide  logw_pre[t * R + r] = log_weight[r].  m = the maximum of the log_weight[r].  If a log_weight is NaN or m is
 *              not finite, step t does not resample.  Otherwise w_r = exp(log_weight[r] - m), exp the library's specified
 *              exponential (DESIGN.md "nsk_exp", the oracle's orc_exp_det bit for bit), and in chain order, sequentially,
 *                c_0 = w_0, c_r = c_(r-1) + w_r;   q_0 = w_0 * w_0, q_r = q_(r-1) + w_r * w_r;   S = c_(R-1), Q = q_(R-1)
 *              -- one rounded float64 operation each, the only arithmetic of the step whose order matters.  The step
 *              resamples iff S * S < (threshold * (double)R) * Q, the product in brackets formed once by the host: the
 *              effective sample size S^2 / Q of the population fell below threshold x R.  threshold = 0 never resamples,
 *              R = 1 never does, equal weights never do.
 *              A step that does not resample: resampled[t] = 0, ancestors[t * R + r] = r, log_weight stays.
 *              A step that does: systematic resampling with the caller's uniform offsets[t].  step = S / (double)R;
 *              target_i = ((double)i + offsets[t]) * step; a_i = the number of j with c_j <= target_i, at most R - 1;
 *              chain j has n_j = #{i : a_i = j} offspring (they sum to R; n_j is floor or ceil of R w_j / S up to the
 *              rounding of c and target).  The offspring are dealt to slots so that the copy is in place: a chain with
 *              n_j >= 1 keeps its slot, ancestors[t * R + j] = j; the dead slots (n_j = 0) in ascending order take the
 *              entries of the donor list in order, the list being j ascending with j repeated n_j - 1 times.
 *              resampled[t] = 1, and log_weight[r] = 0.0 for every r: the fold of the following steps starts afresh.
 *   6. copy    where ancestors[t * R + r] != r, the values of chain ancestors[t * R + r] replace those of chain r, device
 *              to device.  Every source kept its own slot, so nothing is read that the step writes.  The sweep generators
 *              are keyed by the slot r, so two copies of one state part ways at the next sweep.
 * With a schedule from 0 to 1: log Z = log Z_0 + the sum over the resampling steps t of log mean_r exp(logw_pre[t][r]) +
 * log mean_r exp(log_weight[r]) (numbskull_amd.diagnostics.smc_estimate; smc_resample is the rule of step 5 in numpy
 * and returns the device's ancestors integer for integer when fed logw_pre and that exp).  There is no best-state
 * tracking.  Then w = w_base again, bit for bit, the call synchronises ONCE and downloads what was asked for: log_weight
 * (R, the fold since the last resampling), lp (nsteps x R), logw_pre ((nsteps - 1) x R), ancestors ((nsteps - 1) x R,
 * int32), resampled (nsteps - 1, int32).  Each of the five may be NULL.  The values of the chains are left as the last
 * step leaves them; tallies, trace rows and columns and the evidence chain are untouched, a tally kept in the value bytes
 * is first brought back to its array, and an error after the first scale still restores the base weights -- all as in
 * nsk_tempered_sweeps, whose limits on what the estimate means hold here too.
 * NSK_E_INVALID, before anything is enqueued and with values, weights, sweeps_done and the generator untouched: what
 * nsk_tempered_sweeps refuses; a threshold outside [0, 1] or NaN; an offset outside [0, 1) or NaN (offsets, when given,
 * are nsteps - 1 doubles and all are checked); offsets == NULL while nsteps > 1 and threshold > 0.
 * Memory: what nsk_tempered_sweeps keeps, stays.  The copy of the base weights, lp, log_weight, logw_pre, the ancestors
 * and the flags live for the call only: nsk_graph_info.device_bytes is afterwards what it was.  NSK_E_NOMEM names the
 * size of what does not fit.  The offsets travel as kernel arguments.  A copy can carry a value from any slot into any
 * other, so after a call that may have copied the handle treats chain 0 and the chains behind it as lying in their domains
 * only if all of them did (the table kernels index with values: uploading one chain afresh does not clear the others).
 * nsk_profile_* keeps counting sweep-kernel launches only. */
int nsk_smc_sweeps(nsk_graph *g, const double *betas /* nsteps */, int64_t nsteps, int64_t sweeps_per_step,
                   int sample_evidence, double threshold, const double *offsets /* nsteps - 1, each in [0, 1) */,
                   double *log_weight /* chains, may be NULL */, double *lp /* nsteps x chains, may be NULL */,
                   double *logw_pre /* (nsteps - 1) x chains, may be NULL */,
                   int32_t *ancestors /* (nsteps - 1) x chains, may be NULL */,
                   int32_t *resampled /* nsteps - 1, may be NULL */);

/* Parallel tempering (FactorGraph.parallel_tempering): replica exchange between the chains of the handle.  The two calls
 * above are annealers -- beta changes over time and no chain samples the target along the way.  Here chain r stays at the
 * inverse temperature betas[r] for the whole call and STATES travel between the chains through Metropolis swaps, so a
 * chain at beta = 1 keeps sampling the target while the hot chains carry it across the barriers between its modes; its
 * tallies are marginals.  Temperatures do not move: chain r's tallies always belong to betas[r].
 * The call acts on ALL chains of the handle (R = nsk_get_chains).  With w_base the device weight table as it stands when
 * the call begins and s0 the sweep index at entry, for t = 0 .. nsteps - 1, in this order on the handle's stream and
 * without a host wait between steps:
 *   1. sweep   for r = 0 .. R - 1: w[s] = betas[r] * w_base[s] for every slot, fixed weights included (one rounded
 *              float64 product, the scale of nsk_tempered_sweeps), the tables derived from the weights are rebuilt, and
 *              chain r -- and no other -- runs sweeps_per_step sweeps by the one-chain launches, keyed seed ^ (r << 32),
 *              at the sweep indices s0 + t * sweeps_per_step + i: every replica of a step uses the same indices.  They
 *              are burn-in sweeps (nothing tallied), except those of chain tally_chain, which are tallied exactly as a
 *              one-chain inference call tallies them (tally_chain = -1: none).  No sweep kernel, kernel argument, plan or
 *              captured sequence differs from those of nsk_gibbs_sweeps;
 *   2. score   U[r] = the log-potential of chain r's state under w_base, for all chains in one walk, with the very bits
 *              nsk_log_potential returns; lp[t * R + r] = U[r] -- after the sweep, before the swap;
 *   3. decide  the pair of the chains r and r + 1 is proposed iff r and t have the same parity and r + 1 < R (the
 *              deterministic even-odd scheme: the pairs of a step are disjoint).  d = (betas[r] - betas[r + 1]) *
 *              (U[r + 1] - U[r]): two rounded differences, one rounded product.  The swap is accepted iff d >= 0.0, or
 *              d >= -745.0 and uniforms[t * (R - 1) + r] < exp(d), exp the library's specified exponential (DESIGN.md
 *              "nsk_exp", the oracle's orc_exp_det bit for bit); a NaN d rejects.  accepted[t * (R - 1) + r] is 1, 0, or
 *              -1 for a pair not proposed at step t (numbskull_amd.diagnostics.pt_swap_rule is this rule in numpy and
 *              returns the device's decisions integer for integer when fed the lp row and that exp);
 *   4. swap    the value bytes of the two chains of every accepted pair are exchanged in place, device to device.
 *              Tallies, trace storage and the evidence chain are not exchanged.  The sweep generators are keyed by the
 *              slot r, so a state goes on under the stream of the slot it moved to.
 * Then w = w_base again, bit for bit (a copy), the handle is marked so that a following sweep call rebuilds the tables
 * under the base weights, and the call synchronises ONCE and downloads lp (nsteps x R) and accepted (nsteps x (R - 1),
 * int32); each may be NULL.  sweeps_done and the sweep index have advanced by nsteps x sweeps_per_step, as after
 * nsk_tempered_sweeps.  An error after the first scale still restores the base weights.  A tally kept in the value bytes
 * is first brought back to its array; a pending uint8 position tally is folded into the masters at entry and again
 * before the call returns, so that only chain tally_chain's tallies have grown.  A swap can carry a value from a slot into
 * its neighbour, so after a call with R > 1 the handle treats chain 0 and the chains behind it as lying in their domains
 * only if all of them did, as after nsk_smc_sweeps.  R = 1 is served: it has no pairs and accepted has no columns.
 * NSK_E_INVALID, before anything is enqueued and with values, weights, counters and the generator untouched: what
 * nsk_tempered_sweeps refuses (the sequential scan, own_range / NSK_FLAG_PARTITION, a boundary exchange, nsteps outside
 * [1, 65536], sweeps_per_step < 1 or nsteps * sweeps_per_step > INT32_MAX); a beta that is negative, infinite or NaN;
 * uniforms == NULL while R > 1; a uniform outside [0, 1) or NaN (all nsteps x (R - 1) are checked); tally_chain outside
 * [-1, R); a handle that records a sample trace (tear it down first).
 * Memory: what nsk_log_potential uploads at its first use, stays.  The copy of the base weights, lp, the betas, the
 * uniforms, the decisions and the partner words live for the call only: nsk_graph_info.device_bytes is afterwards what
 * it was.  NSK_E_NOMEM names the size of what does not fit.
 * Cost: a step rebuilds the tables R times, once in front of every replica, where nsk_tempered_sweeps rebuilds them
 * once (DESIGN.md has the measurements).  nsk_profile_* keeps counting sweep-kernel launches only. */
int nsk_pt_sweeps(nsk_graph *g, const double *betas /* chains */, int64_t nsteps, int64_t sweeps_per_step,
                  int sample_evidence, const double *uniforms /* nsteps x (chains - 1), each in [0, 1) */,
                  int tally_chain /* -1: none */,
                  double *lp /* nsteps x chains, may be NULL */, int32_t *accepted /* nsteps x (chains - 1), may be NULL */);

/* Effective sample size from the trace, on the device (FactorGraph.mixing): per column of a BIT-PACKED trace, the
 * split-chain estimator of numbskull_amd.diagnostics.effective_sample_size with the lags cut at max_lag, in one
 * streaming pass over the packed rows -- no row is unpacked or leaves the device.  Rows first_row .. first_row +
 * nrows - 1 of the R chains are split as for split R-hat: n = nrows / 2, half-chains rows [0, n) and [nrows - n, nrows)
 * of every chain, H = 2 R of them (one chain is allowed: H = 2; the middle row of an odd nrows is unused).  For 0 / 1
 * columns every sum is a count over bit words; per column the device forms, in int64 and exactly, for k = 0 .. L,
 * L = min(max_lag, n - 1),
 *   A(k) = sum over half-chains h of  n^2 c_h(k) - n S_h (head_h(k) + tail_h(k)) + (n - k) S_h^2
 * (S_h the half-chain's sum, c_h(k) the sum of x(t) x(t + k) over t < n - k, head_h(k) and tail_h(k) the sums of its
 * first and last n - k rows: n^3 times the summed biased autocovariance at lag k), S1 = sum of S_h and S2 = sum of S_h^2.
 * The float64 epilogue, one rounded operation a step in the order DESIGN.md section 4 writes down: D = H n n (n - 1),
 * W = A(0) / D, B = (H S2 - S1^2) / (H (H - 1) n n), V = (n - 1) / n W + B, rho_k = 1 - ((A(0) - A(k)) / D) / V,
 * P_j = rho_2j + rho_2j+1 for j < (L + 1) / 2, tau = -1 + 2 x the sum of the initial run of P_j > 0.
 * nsk_trace_ess: per column mean = S1 / (H n); tau (NaN unless V > 0 and tau > 0); rhat2 = V / W (NaN unless V > 0;
 * split R-hat is its square root); truncated = 1 when every pair up to the last was positive and L < n - 1 (the
 * sequence did not end inside the window: tau is a lower bound, thin more).  The effective sample size is n H / tau.
 * The arrays are ncols long, in the caller's column order of nsk_trace_setup (repeats, and all nvar variables for
 * vids = NULL); any may be NULL.
 * nsk_trace_autocov_counts: the integers themselves for the trace columns cols[0 .. ncols_sel) (indices into the
 * caller's columns; any order, repeats allowed; outside [0, ncols): NSK_E_INDEX):
 * out[j (L + 3) ..] = A(0 .. L), S1, S2 of column cols[j].
 * Both synchronise with the handle's stream, read the trace and change nothing (rows, values, tallies, sweeps_done, the lp and
 * stats columns).  Their result buffers (25 bytes a device column; 8 (L + 3) a column of the words selected) are
 * allocated for the call and freed before it returns: nsk_graph_info.device_bytes shows them only meanwhile;
 * NSK_E_NOMEM names their size when they do not fit.  nsk_profile_* keeps counting sweep-kernel launches only.
 * Refused before any launch -- NSK_E_INVALID: no trace, plain (not bit-packed) rows, nrows < 4, max_lag outside
 * [1, 63]; NSK_E_RANGE: 4 H n^3 reaches 2^63 (decided from nrows and the chain count alone, before the rows recorded
 * are looked at); then NSK_E_INVALID: rows beyond those recorded. */
int nsk_trace_ess(nsk_graph *g, int64_t first_row, int64_t nrows, int64_t max_lag, double *mean /* ncols */,
                  double *tau, double *rhat2, uint8_t *truncated);
int nsk_trace_autocov_counts(nsk_graph *g, int64_t first_row, int64_t nrows, int64_t max_lag, const int64_t *cols,
                             int64_t ncols_sel, int64_t *out /* ncols_sel x (L + 3) */);

/* Pairwise joint marginals from the trace, on the device (FactorGraph.pairwise): for pairs (a, b) of columns of a
 * BIT-PACKED trace, how often both are 1 and how often each is, over rows first_row .. first_row + nrows - 1 of the R
 * chains (the window is not split) -- the 2 x 2 table of a pair is these three integers and the row count; no row is
 * unpacked or leaves the device.  pairs[2 j], pairs[2 j + 1] are indices into the caller's columns of nsk_trace_setup,
 * the numbering nsk_trace_autocov_counts takes for cols: any order, repeats allowed, a == b allowed.
 *   out[(j R + r) 3 + 0 .. 2] = n11, n1(a), n1(b) of chain r: the rows of the window where both columns are 1, where
 *   column a is, where column b is.
 * Two launches.  The 64-column words the pairs touch are each transposed once, 64 rows x 64 columns at a time, into a
 * scratch array T[word][bit][chain][block of 64 rows] whose words hold one column's rows along time (0 beyond the
 * window); then one wave per pair walks the R x ceil(nrows / 64) neighbouring words of both columns and sums
 * popcount(Ta & Tb), popcount(Ta), popcount(Tb) per chain in int64.  Integers throughout, no atomics: the counts are
 * those of numbskull_amd.diagnostics.pair_counts on the downloaded rows, exactly.
 * The call synchronises with the handle's stream, reads the trace and changes nothing (rows, values, tallies,
 * sweeps_done, the lp and stats columns).  Its buffers -- T, 512 bytes per touched word, chain and row block; the word
 * list, 4 bytes a word; the pairs as columns of T, 16 bytes a pair; the results, 24 bytes per pair and chain -- are
 * allocated for the call and freed before it returns: nsk_graph_info.device_bytes shows them only meanwhile;
 * NSK_E_NOMEM names their size when they do not fit.  nsk_profile_* keeps counting sweep-kernel launches only.
 * Refused before any launch -- NSK_E_INVALID: null graph, no trace, plain (not bit-packed) rows, nrows < 1,
 * first_row < 0, npairs < 0, pairs or out NULL with npairs > 0, rows beyond those recorded; NSK_E_INDEX: a column index
 * outside [0, ncols).  npairs == 0 is NSK_OK with nothing done. */
int nsk_trace_pair_counts(nsk_graph *g, int64_t first_row, int64_t nrows, const int64_t *pairs /* npairs x 2 */,
                          int64_t npairs, int64_t *out /* npairs x chains x 3 */);

/* The same statistics for CATEGORICAL variables (FactorGraph.mixing_values / contingency): a trace with one variable
 * of cardinality above 2 keeps PLAIN rows, one element of value_bytes per column, and the three calls above refuse it.
 * These serve it through INDICATORS: an indicator is a pair (column, value), and its series is the 0 / 1 sequence
 * x(t) == value of that column.  sel[2 i], sel[2 i + 1] = column and value of indicator i; quads[4 j .. 4 j + 3] =
 * column a, value a, column b, value b of pair j.  Columns are indices into the caller's columns of nsk_trace_setup (the
 * numbering nsk_trace_autocov_counts takes); any order, repeats allowed.
 * The outputs mean what those of nsk_trace_autocov_counts, nsk_trace_ess and nsk_trace_pair_counts mean with "column"
 * read as "the indicator's series": out[i (L + 3) ..] = A(0 .. L), S1, S2 of indicator i, L = min(max_lag, n - 1);
 * mean[i] is the marginal of the value, tau, rhat2 and truncated as above (nsel long each, any may be NULL);
 * out[(j R + r) 3 + 0 .. 2] = n11, n1(a), n1(b) of pair j in chain r.  A recorded value outside its variable's domain
 * (the handle allows that) matches no indicator.
 * The host sorts the indicators by (device column, value) and drops repeats -- two caller columns that name one variable
 * share a plane -- and scatters the results back in the caller's order.  k_trace_onehot writes the window's indicators
 * as time-major bit words (planes: bit i of a word is x(64 blk + i) == value, 0 beyond the segment), a 64-row x 64-column
 * tile of the trace at a time through LDS, every touched trace byte read once; for the counts and the summary the
 * segments are the H = 2 R half-chains and k_trace_autocov_planes, lane = indicator, forms the integers and the epilogue
 * of nsk_trace_ess word for word; for the pairs the segments are the R chains and k_trace_pair_counts runs unchanged on
 * pairs of planes.  Integers throughout, no atomics: the results are those of numbskull_amd.diagnostics (autocov_counts,
 * ess_from_counts, pair_counts) on diagnostics.indicators of the downloaded rows, exactly.
 * The calls synchronise with the handle's stream, read the trace and change nothing (rows, values, tallies,
 * sweeps_done, the lp and stats columns).  Their buffers -- the indicator list, 8 bytes an indicator, with 12 bytes a
 * touched column tile and 24 a segment; the planes, 8 bytes per distinct indicator, segment and block of 64 rows; the
 * pair list, 16 bytes a pair; the results -- are allocated for the call and freed before it returns:
 * nsk_graph_info.device_bytes shows them only meanwhile; NSK_E_NOMEM names their size when they do not fit.
 * nsk_profile_* keeps counting sweep-kernel launches only.
 * Refused before any launch, in this order -- NSK_E_INVALID: null graph, no trace, BIT-PACKED rows (the message names
 * the call above that serves them), nrows < 4 (pairs: < 1), max_lag outside [1, 63], first_row < 0, a negative count,
 * sel / quads / out NULL with a positive count; NSK_E_RANGE: 4 H n^3 reaches 2^63 (counts and summary; decided before
 * the rows recorded are looked at); NSK_E_INDEX: a column outside [0, ncols); NSK_E_RANGE: a value outside
 * [0, cardinality of the column's variable); NSK_E_INVALID: rows beyond those recorded.  A count of 0 is NSK_OK with
 * nothing done. */
int nsk_trace_value_autocov_counts(nsk_graph *g, int64_t first_row, int64_t nrows, int64_t max_lag,
                                   const int64_t *sel /* nsel x 2 */, int64_t nsel, int64_t *out /* nsel x (L + 3) */);
int nsk_trace_value_ess(nsk_graph *g, int64_t first_row, int64_t nrows, int64_t max_lag, const int64_t *sel /* nsel x 2 */,
                        int64_t nsel, double *mean /* nsel */, double *tau, double *rhat2, uint8_t *truncated);
int nsk_trace_value_pair_counts(nsk_graph *g, int64_t first_row, int64_t nrows, const int64_t *quads /* npairs x 4 */,
                                int64_t npairs, int64_t *out /* npairs x chains x 3 */);

/* RNG: the chromatic scan draws from Philox4x32-10 keyed by `seed`.  A variable's generator id is
 * its position in the compiled layout (nsk_graph_get_layout), so samples are a function of the seed
 * AND the layout the library chose (device, flags and diagnostic switches being equal, a graph
 * always compiles to the same layout).  Learning sweeps: counter (id, stream, sweep index);
 * inference sweeps: ids q and q + 64 with equal q >> 7 share one block, counter
 * ((q >> 7) * 64 + (q & 63), 0, sweep index), words 0-1 / 2-3 (pair scheme), except inside segments with
 * draw tables, where four ids share two blocks (quad and wide schemes, nsk_graph_get_generators).  The sweep index starts at `sweep0`
 * and advances by one per sweep of any kind; its high half (counter word 3) is XORed with the
 * handle's shard tag (nsk_set_rng_tag; 0 for a handle that owns the whole graph).  Sequential scan seeds MT19937 like
 * np.random.seed(seed); random.seed(seed). */
int nsk_set_seed(nsk_graph *g, uint64_t seed, uint64_t sweep0);
/* Shards of one graph must not share generator streams although their generator ids (layout
 * positions) coincide: Philox counter word 3 is the sweep index's high half XOR a shard tag.  The
 * tag defaults to own_begin (distinct for disjoint shards of one variable array); a handle built
 * from a shard-local graph (own variables + ghosts, renumbered) passes the GLOBAL id of its first
 * owned variable here, which also makes it sample exactly what the whole-graph handle with that
 * own_range samples. */
int nsk_set_rng_tag(nsk_graph *g, uint32_t tag);
int nsk_set_scan(nsk_graph *g, int scan);
/* Chromatic learning applies sample_and_sgd's update (learning.py:110-125) once per colour class:
 * a weight visited k times moves by step * (sum of its k gradients).  The reference updates per
 * visit, which is stable for any k * step; the batch is not, so a weight with k * step > cap uses
 * step = cap / k in that class (same fixed point).  Default 0.5; cap <= 0 switches clipping off.
 * nsk_graph_info.learn_clipped counts the clipped updates. */
int nsk_set_learn_cap(nsk_graph *g, double cap);
/* Chromatic learning, one-class lag (default on): the weight update of colour class c is applied beside
 * the sampling of class c + 1 (it rides in block 0 of that class's launch), which therefore sees the weights
 * as of the end of class c - 1 -- milder than the staleness of the reference's own Hogwild threads and of its distributed merge
 * (one epoch, salt/src/numbskull_master.py:223-224).  The pipeline is drained at the end of every
 * nsk_learn_sweeps call (the weights it leaves include every update).  It applies to handles with at most
 * 256 weights (they accumulate in LDS and the update rides in the next class's launch: the grids); with a
 * larger weight table the update is a launch of its own either way and every class waits for it
 * (nsk_graph_info.learn_lag says which).  lag = 0: every class waits for the previous class's update.  Same
 * fixed point either way; the oracle's device mode mirrors both. */
int nsk_set_learn_lag(nsk_graph *g, int lag);

/* Replaces run_pool(gibbsthread) at factorgraph.py:141 (burnin=1) and :163 (burnin=0):
 * `nsweeps` epochs of gibbsthread (inference.py:10-33) over the owned variables. */
int nsk_gibbs_sweeps(nsk_graph *g, int64_t nsweeps, int sample_evidence, int burnin);

/* Replaces the epoch loop around run_pool(learnthread) at factorgraph.py:194-206: `nsweeps`
 * epochs of learnthread/sample_and_sgd (learning.py:12-125), step *= decay after each. */
int nsk_learn_sweeps(nsk_graph *g, int64_t nsweeps, double step, double decay,
                     int regularization, double reg_param, int64_t truncation,
                     int learn_non_evidence);

/* Introspection used by tests, bench and the multi-GPU host code. */
typedef struct {
    int64_t nvar, nowned, ncolors, value_bytes, device_bytes;
    /* device_bytes: bytes the handle holds now; it drops when a later call frees arrays */
    int64_t nfast, ngeneric;          /* variables on the inlined / the generic kernel path       */
    double alg_bytes_inference;       /* algorithmic bytes per sweep       */
    double alg_bytes_learning;
    int64_t sweeps_done;
    double layout_bytes_inference;    /* bytes one sweep must move in the compiled device layout  */
    double layout_bytes_learning;     /*   (tile words, positions, distinct values, stores, tally) */
    int64_t ztab_entries;             /* draw-table entries (0: no tabulated program)              */
    double compile_seconds;           /* host time spent in the graph compiler                     */
    double learn_cap;                 /* nsk_set_learn_cap                                         */
    int64_t learn_clipped;            /* weight updates whose step was clipped so far              */
    int64_t grad_shift;               /* gradient sums are Q(31+s).(32-s) fixed point: s (0 unless one
                                         weight's sum in one colour class could reach 2^30)        */
    int64_t acc_copies;               /* copies of the global learning accumulators: 8 (one per XCD, after
                                         the device passed the self-test of nsk_graph_create), 1 for a
                                         graph that accumulates in LDS or a device that failed it; +16
                                         when the LDS path's bins are private to XCDs; 0 from
                                         nsk_graph_plan (no device)                                */
    int64_t learn_lag;                /* 1: learning sweeps of this handle run with the one-class lag
                                         (nsk_set_learn_lag on AND at most 256 weights: the update then
                                         rides in the next class's launch); 0: every class waits for the
                                         previous class's update                                    */
    int64_t direct_weights;           /* weights with a single factor that the learning kernels update in
                                         place at their one visit per class (no accumulator, no update
                                         launch for them); 0: none                                 */
    int64_t weight_slots;             /* 1: the device table keeps the single-factor weights in layout order
                                         (nsk_graph_get_weight_slots is not the identity); 0: caller's order */
    int64_t layout_hash;              /* with NSK_LAYOUT_HASH=1 in the environment: a 64-bit hash of every
                                         array of the compiled layout (colours, positions, tile and group
                                         streams, programs, weight slots ...) -- what a check that two builds /
                                         thread counts / library versions compile a graph alike compares;
                                         0 otherwise (hashing the layout of a 50M-variable graph takes seconds) */
    int64_t p2p_fused;                /* 1: after nsk_p2p_import(_local), the handle's inference sweeps exchange the
                                         boundary INSIDE their table launches (nsk_gibbs_sweeps_p2p: border tiles read
                                         the receive block, write into the readers' and raise the flags; no exchange
                                         kernels per sweep) -- a shard whose sampled variables all live in table
                                         segments and whose boundary values have one reader each; 0: exchange kernels */
    int64_t tab_quads;                /* position quads (256 consecutive positions) of the segments with draw tables */
    int64_t wide_quads;               /* ... of them the WIDE ones: one lane samples four consecutive positions from
                                         dword loads (nsk_graph_get_generators bit 41)                              */
    int64_t hubs;                     /* variables a whole wave or workgroup samples (positions of the wave-per-variable
                                         ranges that hold a variable): lists of 32 entries and more, and every generic-
                                         path variable of a colour with few of them                                  */
    int64_t hubs_ep;                  /* ... of them those with an entry-parallel stream (one lane per list entry; the
                                         others take the generic wave walk)                                          */
    int64_t hubs_block;               /* ... of those the ones a whole workgroup evaluates (more than 128 entries in a
                                         colour laid out as entry-parallel groups); the other hubs_ep - hubs_block
                                         take one wave each                                                          */
    /* tiles (64 consecutive positions of a colour's fast range that hold at least one variable) and groups by the
       kernel family that walks them -- see "Routes" below for the per-variable view */
    int64_t tiles_shape;              /* shape tiles: one word layout for the 64 lanes, per-lane functions and weights */
    int64_t tiles_shape_padded;       /* ... of them those whose stream holds at least one null member word (a lane's
                                         entry has fewer members than the tile's layout)                            */
    int64_t tiles_lane;               /* tiles with per-lane headers (every lane parses its own words)              */
    int64_t tiles_general;            /* general tiles walked one lane per variable (E entries of 2 + M words)      */
    int64_t tiles_general_roles;      /* ... of them those of member width M >= 4, walked by the role program
                                         (general_walk_roles) instead of the layouts specialised on M <= 3          */
    int64_t ep_groups;                /* entry-parallel groups: 256 positions of general-tile variables, one lane per
                                         list entry                                                                 */
    int64_t ep_groups_two_pass;       /* ... of them those with a variable of more than 8 entries: a second LDS pass */
} nsk_graph_info;
int nsk_graph_get_info(nsk_graph *g, nsk_graph_info *info);
int nsk_graph_get_colors(nsk_graph *g, int32_t *color /* nvar, -1 for ghosts */);
/* Internal numbering: the device keeps values in the order of its compiled layout (a sampled
 * variable at its position, the others after them).  iid[v] (nvar entries, may be NULL) = index of
 * variable v in the NSK_BUF_VALUE / NSK_BUF_VALUE_EVID buffers, *nid = their length in elements.
 * nsk_state_upload / nsk_state_download and the exchange lists take the caller's variable ids. */
int nsk_graph_get_layout(nsk_graph *g, int32_t *iid, int64_t *nid);
/* The chromatic scan's generator of every variable (nvar entries; -1: not sampled by this handle): bits
 * 0-39 the generator id (= the position in the compiled layout), bit 40 set when the variable's INFERENCE
 * draws come from the quad scheme -- positions inside segments with draw tables: ids q, q + 64, q + 128,
 * q + 192 with equal q >> 8 share two Philox blocks, counter ((q >> 8) * 64 + (q & 63), stream, sweep),
 * stream 2 word (q >> 6) & 3 = the draw's high word, stream 3 the same word its low word -- instead of
 * the pair scheme described at nsk_set_seed; bit 41 set instead when they come from the WIDE scheme -- positions
 * inside wide quads (nsk_graph_info.wide_quads: 256 consecutive positions of a table segment whose members are
 * consecutive positions too, so that one lane samples four of them from dword loads): ids 4 i .. 4 i + 3 with equal
 * q >> 2 share the two blocks, counter ((q >> 8) * 64 + ((q >> 2) & 63), stream, sweep), word q & 3 of stream 2 / 3 =
 * the draw's high / low word.  What a checker needs to reproduce the samples. */
int nsk_graph_get_generators(nsk_graph *g, int64_t *gen);

/* Weight slots: where the device table (NSK_BUF_WEIGHT) keeps each weight, slot[w] for the caller's id w
 * (nweight entries).  The identity except on whole-graph handles that update single-factor weights in place
 * (nsk_graph_info.direct_weights): there those weights are numbered among themselves in the order the layout
 * first meets them, so that the entries a workgroup walks read and update neighbouring slots.
 * nsk_state_upload / nsk_state_download always speak the caller's ids.  Returns 1 when some slot differs
 * from its id, 0 for the identity, < 0 on error. */
int nsk_graph_get_weight_slots(nsk_graph *g, int64_t *slot);

/* Host-only planning (no GPU touched): validate + colour the graph exactly as nsk_graph_create
 * would and report the colours / sizes.  `color` (nvar entries, may be NULL) gets -1 for variables
 * this handle does not sample. */
int nsk_graph_plan(const nsk_graph_desc *desc, int32_t *color, nsk_graph_info *info);
/* Host-only twin of nsk_ghost_needs (vids == NULL: query the count). */
int nsk_graph_plan_needs(const nsk_graph_desc *desc, int64_t *count, int32_t *vids);

/* Routes: which kernel family samples every variable, read back from the compiled layout -- one word per variable
 * (nvar entries), from a handle or host-only from a plan (both filled by the same function).  What tests and tools
 * use to see that a graph built for a routing edge landed on the side it was built for.
 *   bits 0-3   NSK_ROUTE_KIND: one of the NSK_ROUTE_* kinds below
 *   GENERAL and GROUP:
 *   bits 4-8   NSK_ROUTE_OWN_ENTRIES: list entries of the variable itself (a dataType-1 variable: over all its lists)
 *   bits 9-11  NSK_ROUTE_OWN_WIDTH: most other members of one of its entries
 *   GENERAL:
 *   bits 12-16 NSK_ROUTE_TILE_ENTRIES: entries E per lane of its tile -- the most any lane has, padded to a multiple
 *              of the walk's super-group (2, 4, 1, 4 entries for M = 0, 1, 2, 3; lanes with fewer carry padding entries)
 *   bits 17-19 NSK_ROUTE_TILE_WIDTH: member width M of its tile (M >= 4: the role-program walk)
 *   GROUP:
 *   bits 12-16 NSK_ROUTE_TILE_ENTRIES: most entries of a variable of its group
 *   bit  20    NSK_ROUTE_TWO_PASS: its group takes a second LDS pass (a variable of the group has more than 8 entries)
 *   SHAPE:
 *   bit  21    NSK_ROUTE_NULL_WORD: the lane's stream holds a null member word (its entry has fewer members than the
 *              tile's layout: padded shapes)
 *   HUB:
 *   bit  22    NSK_ROUTE_HUB_EP: the hub has an entry-parallel stream;  bit 23  NSK_ROUTE_HUB_BLOCK: ... evaluated by
 *              a whole workgroup (nsk_graph_info.hubs_ep / hubs_block count these) */
#define NSK_ROUTE_NONE 0        /* not sampled by this handle                                                   */
#define NSK_ROUTE_TABLE 1       /* uniform tile inside a segment with a draw table                              */
#define NSK_ROUTE_UNIFORM 2     /* uniform tile on the exp path (segment without a table, or a rest tile)       */
#define NSK_ROUTE_SHAPE 3       /* shape tile                                                                   */
#define NSK_ROUTE_LANE 4        /* tile with per-lane headers                                                   */
#define NSK_ROUTE_GENERAL 5     /* general tile, walked one lane per variable                                   */
#define NSK_ROUTE_GROUP 6       /* entry-parallel group                                                         */
#define NSK_ROUTE_HUB 7         /* a wave or a workgroup per variable                                           */
#define NSK_ROUTE_GENERIC 8     /* one-lane generic kernel                                                      */
#define NSK_ROUTE_KIND(r) ((r) & 15)
#define NSK_ROUTE_OWN_ENTRIES(r) (((r) >> 4) & 31)
#define NSK_ROUTE_OWN_WIDTH(r) (((r) >> 9) & 7)
#define NSK_ROUTE_TILE_ENTRIES(r) (((r) >> 12) & 31)
#define NSK_ROUTE_TILE_WIDTH(r) (((r) >> 17) & 7)
#define NSK_ROUTE_TWO_PASS(r) (((r) >> 20) & 1)
#define NSK_ROUTE_NULL_WORD(r) (((r) >> 21) & 1)
#define NSK_ROUTE_HUB_EP(r) (((r) >> 22) & 1)
#define NSK_ROUTE_HUB_BLOCK(r) (((r) >> 23) & 1)
int nsk_graph_plan_routes(const nsk_graph_desc *desc, int32_t *route /* nvar */);
int nsk_graph_get_routes(nsk_graph *g, int32_t *route /* nvar */);

/* Class plans: the launches a sweep would give every colour class, host-only from a plan -- one record of NSK_CLASS_REC
 * int32 per class, filled from the functions the sweep drivers launch from (csrc/nsk_class_plan.h) under the options
 * they would pass.  `learning` != 0: the learning sweep under `regularization`, else the inference sweep.  `grid_cap`
 * is what the drivers read from NSK_CLASS_GRID_CAP (NSK_DIAG=1): 0 none, else at most that many blocks (whole rounds of
 * XCDs where the launch has them) for every persistent grid whose waves walk their items in trips -- taken as an
 * argument, not from the environment; the other diagnostic switches (NSK_NO_OVERLAP, NSK_EP_PER_CU) count as in a sweep.
 * `rec` may be NULL (query): *nclass gets the number of classes either way.  A launch that is off leaves its fields 0.
 *   [NSK_CLS_SKIP]     learning: an empty class (no launch, no update)
 *   the general launch, k_gibbs_general / k_gibbs_ep* or k_learn_general / k_learn_ep*:
 *   [NSK_CLS_GEN_ON] [NSK_CLS_GEN_ITEMS] groups (entry-parallel) or general tiles  [NSK_CLS_GEN_GRID]
 *   [NSK_CLS_GEN_STREAM] -1 the handle's stream, 0 .. 2 a side stream  [NSK_CLS_GEN_EP] entry-parallel kernels
 *   [NSK_CLS_GEN_MAXC] 8 or 2 candidate values  [NSK_CLS_GEN_CAPPED] the register-capped twin
 *   [NSK_CLS_GEN_TILE0] [NSK_CLS_GEN_NTILES] its general tiles, relative to the class's first tile
 *   [NSK_CLS_GEN_HBLOCKS] hub blocks in front (long-list hubs first)  [NSK_CLS_GEN_GBLOCKS] tile / group blocks
 *   [NSK_CLS_GEN_RBLOCKS] blocks behind them for rest tiles only  [NSK_CLS_GEN_NREST] rest tiles the launch samples
 *   [NSK_CLS_GEN_BEHIND] enqueued behind the generic kernel's fork  [NSK_CLS_GEN_NBLOCKS] blocks the tiles need, 4 each
 *   the simple launches, four fields each -- on, items, grid, stream -- from:
 *   [NSK_CLS_GENERIC]  generic lanes: positions (inference), items of 64 positions (learning, k_learn_phase range mode)
 *   [NSK_CLS_HEAVY]    learning: hubs in a launch of their own (k_learn_heavy)
 *   [NSK_CLS_FAST]     rest tiles (k_gibbs_fast) / learn-rest tiles (k_learn_fast) no general launch took
 *   [NSK_CLS_DYN]      learning: tiles with per-lane headers (k_learn_phase list mode)
 *   the shape of the class:
 *   [NSK_CLS_NHUB] hubs  [NSK_CLS_NBH] of them long-list  [NSK_CLS_NGROUPS]  [NSK_CLS_NDYN]  [NSK_CLS_NLREST] learn-rest
 *   tiles  [NSK_CLS_NREST] rest tiles (inference)  [NSK_CLS_NGENERIC] generic positions  [NSK_CLS_NTILES] tiles
 *   [NSK_CLS_FB] [NSK_CLS_FE] [NSK_CLS_HE] [NSK_CLS_E] positions: tiles [fb, fe), hubs [fe, he), generic lanes [he, e)
 *   [NSK_CLS_KSTAT] learning: structural visit counts  [NSK_CLS_UPDATE] learning: a weight update follows
 *   [NSK_CLS_SEGMENTS] the class has segment launches  [NSK_CLS_SEG_TILES] learning: tiles in them */
#define NSK_CLASS_REC 48
#define NSK_CLS_SKIP 0
#define NSK_CLS_GEN_ON 1
#define NSK_CLS_GEN_ITEMS 2
#define NSK_CLS_GEN_GRID 3
#define NSK_CLS_GEN_STREAM 4
#define NSK_CLS_GEN_EP 5
#define NSK_CLS_GEN_MAXC 6
#define NSK_CLS_GEN_CAPPED 7
#define NSK_CLS_GEN_TILE0 8
#define NSK_CLS_GEN_NTILES 9
#define NSK_CLS_GEN_HBLOCKS 10
#define NSK_CLS_GEN_GBLOCKS 11
#define NSK_CLS_GEN_RBLOCKS 12
#define NSK_CLS_GEN_NREST 13
#define NSK_CLS_GEN_BEHIND 14
#define NSK_CLS_GEN_NBLOCKS 15
#define NSK_CLS_GENERIC 16
#define NSK_CLS_HEAVY 20
#define NSK_CLS_FAST 24
#define NSK_CLS_DYN 28
#define NSK_CLS_NHUB 32
#define NSK_CLS_NBH 33
#define NSK_CLS_NGROUPS 34
#define NSK_CLS_NDYN 35
#define NSK_CLS_NLREST 36
#define NSK_CLS_NREST 37
#define NSK_CLS_NGENERIC 38
#define NSK_CLS_NTILES 39
#define NSK_CLS_FB 40
#define NSK_CLS_FE 41
#define NSK_CLS_HE 42
#define NSK_CLS_E 43
#define NSK_CLS_KSTAT 44
#define NSK_CLS_UPDATE 45
#define NSK_CLS_SEGMENTS 46
#define NSK_CLS_SEG_TILES 47
int nsk_graph_plan_classes(const nsk_graph_desc *desc, int learning, int regularization, int grid_cap,
                           int32_t *rec /* NSK_CLASS_REC * classes */, int64_t *nclass);

/* HIP-event bracket on the library's stream: elapsed ms and number of sweep-kernel launches
 * between begin and end (bench.py's roofline leg). */
int nsk_profile_begin(nsk_graph *g);
int nsk_profile_end(nsk_graph *g, double *elapsed_ms, int64_t *kernel_launches);
/* the same bracket without blocking at its end: nsk_profile_mark records the closing event,
 * nsk_profile_read waits for it (handles whose streams wait for each other are marked first, read later) */
int nsk_profile_mark(nsk_graph *g);
int nsk_profile_read(nsk_graph *g, double *elapsed_ms, int64_t *kernel_launches);

/* Multi-GPU plumbing: raw device addresses of the value arrays (element size = value_bytes,
 * indexed by INTERNAL id, see nsk_graph_get_layout), of the weights (float64, indexed by weight SLOT: the
 * caller's id except where nsk_graph_get_weight_slots says otherwise -- never on a handle that samples a
 * range of a larger graph) and of the boundary staging buffers, and the stream the library launches on. */
#define NSK_BUF_VALUE 0
#define NSK_BUF_VALUE_EVID 1
#define NSK_BUF_WEIGHT 2
#define NSK_BUF_SEND 3         /* boundary exchange staging, after nsk_exchange_setup */
#define NSK_BUF_RECV 4
#define NSK_BUF_SEND_EVID 5
#define NSK_BUF_RECV_EVID 6
int nsk_device_buffer(nsk_graph *g, int which, void **ptr, int64_t *nbytes);
int nsk_set_stream(nsk_graph *g, void *hip_stream);

/* Boundary ("ghost") exchange for a range-partitioned graph: the reference copies owners' values to
 * the replicas once per epoch (salt/src/numbskull_master.py:165-224); here only the values another
 * partition actually reads travel.
 *   nsk_ghost_needs     sorted ids of the variables outside [own_begin, own_end) that this handle's
 *                       variables read (vids == NULL: query the count)
 *   nsk_exchange_setup  send_vids: the owned variables some other rank reads, in the order every
 *                       rank agreed on; recv_vids / recv_off: the same lists of all `world` ranks,
 *                       concatenated (-1: a variable this handle does not hold -- a shard-local graph
 *                       keeps only the ghosts it reads -- is skipped); slot: elements reserved per
 *                       rank in the gathered buffer.  May be repeated: the arrays of the previous
 *                       set-up are freed, so pointers obtained from nsk_device_buffer for the four
 *                       staging buffers (NSK_BUF_SEND .. NSK_BUF_RECV_EVID) are invalid afterwards
 *   nsk_exchange_pack   SEND[i] = value[send_vids[i]]          (which = NSK_BUF_VALUE[_EVID])
 *   nsk_exchange_unpack value[recv_vids[j]] = RECV[src*slot + j - recv_off[src]] for every src != rank
 * The all-gather of SEND into RECV is done by the caller (torch.distributed) or by the native loop
 * below. */
int nsk_ghost_needs(nsk_graph *g, int64_t *count, int32_t *vids);
int nsk_exchange_setup(nsk_graph *g, int world, int rank, const int32_t *send_vids, int64_t nsend,
                       const int32_t *recv_vids, const int64_t *recv_off, int64_t slot);
int nsk_exchange_pack(nsk_graph *g, int which);
int nsk_exchange_unpack(nsk_graph *g, int which);

/* Native RCCL loop: `nsweeps` x (sweep, pack, ncclAllGather over xGMI, unpack) enqueued on the
 * library's stream without returning to the host language.  unique_id: the 128-byte ncclUniqueId
 * created by nsk_comm_unique_id on rank 0 and broadcast by the caller; librccl_path: the RCCL
 * shared object to bind (the one torch has loaded). */
int nsk_comm_unique_id(const char *librccl_path, void *id128);
int nsk_comm_init(nsk_graph *g, int world, int rank, const void *id128, const char *librccl_path);
int nsk_gibbs_sweeps_exchange(nsk_graph *g, int64_t nsweeps, int sample_evidence, int burnin);
int nsk_learn_sweeps_exchange(nsk_graph *g, int64_t nsweeps, double step, double decay,
                              int regularization, double reg_param, int64_t truncation,
                              int learn_non_evidence);
int nsk_synchronize(nsk_graph *g);

/* Peer-to-peer boundary exchange on one node: instead of pack -> ncclAllGather -> unpack, a rank writes
 * the boundary values each peer reads straight into that peer's buffer (device memory the peer exposes
 * with hipIpc; over xGMI between GPUs) and raises a flag there; a rank waits for the flags of its peers
 * and scatters their values -- no collective, no host round trip per sweep (the reference's per-epoch
 * owner -> replica copy, salt/src/numbskull_master.py:165-224).  Learning epochs send both chains the same
 * way and merge the epoch's weight deltas as w = w_start + (d_0 + d_1 + ...) in rank order (the master's
 * rule, numbskull_master.py:223-224; minions' deltas numbskull_minion.py:260-280) by reduce-scatter +
 * all-gather over the same buffers: rank q owns slice [q nw / W, (q + 1) nw / W) of the weight vector, every
 * rank writes slice q of its deltas to rank q only, the owner adds them in rank order and writes the merged
 * slice to every rank -- one owner per weight, so all ranks end up with bit-identical weights.
 *   nsk_p2p_setup   PAIRWISE lists: send_vids[send_off[q] .. send_off[q+1]) = the owned variables rank q
 *                   reads, recv_vids[recv_off[q] ..) = the variables this handle reads from rank q, both in
 *                   the order the two sides agreed on (ascending global id); peer_base[q] = where this
 *                   rank's segment starts in q's receive list, peer_total[q] = length of q's receive list
 *   nsk_p2p_export  allocates this rank's buffer; handle64 (may be NULL) receives its hipIpc handle, *base
 *                   (may be NULL) its device address
 *   nsk_p2p_import  all_handles: world x 64 bytes, gathered by the caller (one process per rank)
 *   nsk_p2p_import_local  bases[q] = device address of rank q's buffer, for ranks that live in ONE process
 *                   (several handles on one device, or one process driving several GPUs with peer access)
 *   nsk_gibbs_sweeps_p2p / nsk_learn_sweeps_p2p  `nsweeps` x (sweep, push to peers, wait + unpack [+ weight
 *                   merge]) enqueued on the library's stream; asynchronous like nsk_gibbs_sweeps
 *   nsk_p2p_exchange  one exchange alone (learn != 0: both chains + weight deltas); part 0 = all of it,
 *                   1 = the pushes, 2 = wait + unpack (+ the owner's half of the weight merge), 3 = the closing
 *                   half of the weight merge (phase timings; several handles driven by one process issue the
 *                   parts breadth-first)
 *   nsk_p2p_selftest  the same kernels with a payload pattern that depends on sender, element, exchange and
 *                   chain instead of the state, compared on the receiving side instead of stored (state and
 *                   weights are left alone): checks that peer WRITES are visible, not only the flags; a
 *                   mismatch is reported by nsk_p2p_check.  Same `learn` / `part` arguments
 *   nsk_p2p_check   synchronises and returns NSK_E_DEVICE when a peer's flag did not arrive within
 *                   NSK_P2P_TIMEOUT_S seconds (default 30), or a self-test payload differed, since the last
 *                   check (nsk_state_download reports a time-out too) */
/* Partial factors (salt/src/messages.py:1333-1355 compute_pf_values / apply_pf_values): a reader shard that holds a
 * factor OR / AND / ISTRUE with several members owned by THIS shard takes ONE aggregate of them instead of every
 * member -- op 0: "some member is 1" (OR), op 1: "no member is 0" (AND, ISTRUE), a 1 / 0 value the reader keeps in a
 * boolean ghost variable that stands in the factor for those members (numbskull_amd/graphgen.py partial_factors does
 * the rewriting; the factor's value, hence every sample, is exactly what it is with the members themselves).
 * nsk_pf_setup registers the aggregates this handle computes: members of aggregate j = member_vids[member_off[j] ..
 * member_off[j+1]) (variables the handle holds).  A send list of nsk_p2p_setup (call it afterwards) names aggregate j
 * as variable id nvar + j; every peer-to-peer exchange recomputes them (both chains in learning) before it pushes. */
int nsk_pf_setup(nsk_graph *g, int64_t npf, const uint8_t *op, const int64_t *member_off, const int32_t *member_vids);
int nsk_p2p_setup(nsk_graph *g, int world, int rank, const int32_t *send_vids, const int64_t *send_off,
                  const int32_t *recv_vids, const int64_t *recv_off, const int64_t *peer_base,
                  const int64_t *peer_total);
int nsk_p2p_export(nsk_graph *g, void *handle64, void **base);
int nsk_p2p_import(nsk_graph *g, const void *all_handles);
int nsk_p2p_import_local(nsk_graph *g, void *const *bases);
int nsk_gibbs_sweeps_p2p(nsk_graph *g, int64_t nsweeps, int sample_evidence, int burnin);
int nsk_learn_sweeps_p2p(nsk_graph *g, int64_t nsweeps, double step, double decay, int regularization,
                         double reg_param, int64_t truncation, int learn_non_evidence);
int nsk_p2p_exchange(nsk_graph *g, int learn, int part);
int nsk_p2p_selftest(nsk_graph *g, int learn, int part);
/* The fused exchange (nsk_graph_info.p2p_fused) reads and writes peer memory with system-coherent loads / stores
 * and no fences.  nsk_p2p_selftest(g, 2, part) runs that protocol in isolation with a pattern payload (part 0: all
 * of it; 1 / 2: the writing / the reading half); nsk_p2p_fuse(g, 0) makes the handle keep the exchange kernels
 * (what PartitionedSampler does on every rank when any rank's test fails), nsk_p2p_fuse(g, 1) plans the fused
 * exchange again.  Returns 1 / 0 = fused or not afterwards, < 0 on error. */
int nsk_p2p_fuse(nsk_graph *g, int on);
int nsk_p2p_check(nsk_graph *g);
/* After a failed self-test the peers have advanced their exchange tags and written patterns into this rank's receive
 * blocks: nsk_p2p_reset zeroes this rank's exchange allocation (flags, both parities of the receive blocks, the
 * weight-delta slices), its error words and its tag.  EVERY rank calls it, with a barrier of the caller's before and
 * after (no peer may still be writing; none may start before all are clean): the mappings stay. */
int nsk_p2p_reset(nsk_graph *g);

/* ---- graph-aware partitioning (no GPU needed; salt/src/messages.py:542-670 find_connected_components /
 * find_metis_parts).  A partition is a VARIABLE ORDER in front of the samplers' range partition
 * (inference.py:17-18): nsk_graph_order keeps connected components together (method 0) and walks every component
 * breadth first from a pseudo-peripheral variable (method 1, Cuthill-McKee), so that the shard formula's cut runs
 * along a few BFS fronts; order[new id] = old id, cc_id[old id] = connected component (may be NULL), *ncc their
 * number.  nsk_comm_volume: the communication volume -- (variable, foreign part) pairs read across the cut, i.e.
 * the values one exchange moves, METIS' objtype = vol -- of the range partition into nparts <= 64 shards of the ids
 * new_id[old id] (NULL: the caller's ids). ---- */
int nsk_graph_order(int64_t nvar, int64_t nfactor, const nsk_factor *factor, int64_t nedge, const nsk_ftv *fmap,
                    int method, int64_t *order, int64_t *cc_id, int64_t *ncc);
int nsk_comm_volume(int64_t nvar, int64_t nfactor, const nsk_factor *factor, int64_t nedge, const nsk_ftv *fmap,
                    const int64_t *new_id, int nparts, int64_t *volume);
/* The multilevel partitioner (find_metis_parts, messages.py:593-670: nxmetis.partition with objtype = vol): heavy-edge
 * matching, a partition of the coarsest graph, greedy k-way boundary refinement on the way up and, at the finest
 * level, refinement of nsk_comm_volume itself with the parts held at exactly the shard formula's sizes.
 * order[new id] = old id: range g of the new ids is part g; part[old id] = g (may be NULL); stats (may be NULL)
 * receives 5 numbers: levels, coarsest vertices, edge cut after uncoarsening, communication volume before / after
 * the last refinement.  Deterministic in (graph, nparts, seed); nparts <= 64, nvar < 2^31. */
int nsk_graph_partition(int64_t nvar, int64_t nfactor, const nsk_factor *factor, int64_t nedge, const nsk_ftv *fmap,
                        int nparts, uint64_t seed, int64_t *order, int64_t *part, int64_t *stats);

/* ---- host-side index build and file parsing (no GPU needed) ---- */
/* dataloading.compute_var_map (dataloading.py:16-81), native and O(edges). */
int nsk_compute_var_map(int64_t nvar, const nsk_variable *variable, int64_t nfactor,
                        const nsk_factor *factor, int64_t nedge, const nsk_ftv *fmap,
                        int64_t nvtf, nsk_vtf *vmap, int64_t nfactor_index, int64_t *factor_index,
                        const uint8_t *domain_mask, const int64_t *factors_to_skip, int64_t nskip);
/* FactorGraph.__init__'s arrays (factorgraph.py:41-53) from the packed records, over the host threads: cstart[nvar + 1]
 * (cumulative tally slots: one for a binary variable, `cardinality` otherwise), init[nvar] (initialValue, dense),
 * *max_card, *longest (the longest factor_index_length of vmap; both may be NULL). */
int nsk_state_layout(int64_t nvar, const nsk_variable *variable, int64_t nvtf, const nsk_vtf *vmap,
                     int64_t *cstart, int64_t *init, int64_t *max_card, int64_t *longest);
/* dataloading.load_factors (dataloading.py:196-235) on the raw bytes of graph.factors. */
int nsk_parse_factors(const uint8_t *data, int64_t nbytes, int64_t nfactor, int64_t nedge,
                      nsk_factor *factor, nsk_ftv *fmap, const uint8_t *domain_mask,
                      const nsk_variable *variable, int64_t nvar, const nsk_vtf *vmap);

/* dataloading.load_domains (dataloading.py:159-187) on the raw bytes of graph.domains: marks
 * domain_mask, fills vmap[vtf_offset ..].value and re-maps initialValue exactly as the reference. */
int nsk_parse_domains(const uint8_t *data, int64_t nbytes, uint8_t *domain_mask, int64_t nvar,
                      nsk_variable *variable, nsk_vtf *vmap, int64_t nvtf);
/* FactorGraph.dump_probabilities (factorgraph.py:216-229): the "<vid> <value> <prob>" text file. */
int nsk_write_probabilities(const char *path, int64_t nvar, const nsk_variable *variable,
                            const nsk_vtf *vmap, int64_t nvtf, const int64_t *cstart,
                            const int64_t *count, int64_t ncount, double epochs);

/* Self-test hooks: run the device exp / Philox on caller data (parity tests vs the oracle). */
int nsk_selftest_exp(int device, const double *x, double *y, int64_t n);
int nsk_selftest_philox(int device, uint64_t seed, uint64_t sweep, uint32_t stream, int64_t n,
                        uint32_t *out /* 4*n words, counter c0 = 0..n-1 */);

/* Plain HBM stream-copy of `nbytes` (read + write) with `width`-byte accesses per lane (4 or 16;
 * 64 = four 16-byte non-temporal loads in flight per lane and non-temporal stores, the ceiling):
 * the achievable-bandwidth ceiling bench.py reports beside the sweep, and the calibration
 * workload for the rocprofv3 FETCH_SIZE / WRITE_SIZE counters. */
int nsk_selftest_stream(int device, int64_t nbytes, int width, int iters, double *gbytes_per_s);

int nsk_device_count(int *count);
const char *nsk_last_error(void);
const char *nsk_version(void);

#ifdef __cplusplus
}
#endif
#endif
