"""Call sequences on a handle that stays resident: a driver and the scripts of tests/test_resident_calls_gpu.py (the runs
against the oracle) and tests/test_resident_calls_cpu.py (what the oracle alone says about the same scripts), kept in one
place so that the two cannot drift apart.

The FactorGraph methods bracket every C-ABI call with a full nsk_state_upload and a full nsk_state_download, which resets
what a handle carries from one call to the next.  The driver uploads ONCE (``fg._push(0, 0)``) and from then on issues the
raw calls of include/numbskull_amd.h on ``fg._engine()``, the use INTEGRATION.md describes and bench.py times.  Every call
is mirrored in the oracle's device mode: ``gibbs_dev`` sweep by sweep under a 64-bit sweep counter of the driver's own,
``learn_call`` for a learning call, chain r by a run seeded ``seed ^ (r << 32)``.

What is compared, all of it for equality (weights as uint64 patterns): the values after every call, after a learning call
also the evidence chain and the weights.  Those downloads pass ``count = NULL``: nsk_state_download and
nsk_chains_download fold the tallies (fold_counts: the per-chain int32 tally, the uint8 position tally and a tally kept
in the value bytes) only inside ``if (count)``, so a download without a count array launches a gather and copies, and
leaves cnt_pos, pos_tally_sweeps and cnt_dirty as the call under test left them.  A count download IS a fold: tallies are
compared where a script says ``("counts",)`` and at the end of every script, nowhere else.

A script is a list of calls:
  ("gibbs", n, sample_evidence, burnin)        nsk_gibbs_sweeps
  ("learn", n, step, reg, trunc, lne)          nsk_learn_sweeps (decay 0.9, reg_param 0.05)
  ("weights", salt)                            nsk_state_upload(h, NULL, NULL, w, NULL): the current weights + seeded noise
  ("values", "bad" | "regular")                nsk_state_upload(h, v, NULL, NULL, NULL): a 2 in some binary variables / all back in domain
  ("seed", seed, sweep0)                       nsk_set_seed
  ("tag", tag)                                 nsk_set_rng_tag
  ("chains", n)                                nsk_set_chains
  ("counts",)                                  a count download in mid-script
  ("cond", n)                                  nsk_conditionals(what = 0) of n variables against og.potential, bit for bit
  ("lp",)                                      nsk_log_potential against the oracle's eval_factor within the header's bound
"""

import math
from collections import namedtuple

import numpy as np

from util import session, phases_from_colors
from numbskull_amd import _lib, graphgen
import tiles
import wide_trips

DECAY, REG_PARAM = 0.9, 0.05
M64 = (1 << 64) - 1


class Mirror(object):
    """The oracle's side of a script; with a handle (``fg``) also the device's, compared call by call."""

    def __init__(self, og, color, seed, fg=None, tally256=False):
        self.og, self.fg, self.seed, self.sweep = og, fg, int(seed), 0
        self.order, self.ps = phases_from_colors(color)
        vv, ve, wv, cnt = og.initial_state()
        self.vv, self.cnt, self.ve, self.wv = [vv], [cnt], ve, wv
        self.tallied = 0                # tallied sweeps since the start
        self.unfolded = 0               # ... since the last count download
        self.tally256 = tally256        # assert the precondition of the fold scripts at the 256th tallied sweep
        self.lively = []                # per call that samples: (call, values changed, weights changed or None)
        if fg is not None:
            self.L, self.h = _lib.lib(), fg._engine()
            fg._push(0, 0)              # the one full upload

    # ------------------------------------------------------------------ device helpers
    def _values(self):
        n, nv = len(self.vv), len(self.vv[0])
        out = np.empty((n, nv), np.int64)
        if n == 1:      # (count = NULL: nothing is folded, see the module docstring)
            _lib.check(self.L.nsk_state_download(self.h, _lib.ptr(out), None, None, None))
        else:
            _lib.check(self.L.nsk_chains_download(self.h, _lib.ptr(out), None))
        return out

    def _compare_values(self, what):
        got = self._values()
        for r, vv in enumerate(self.vv):
            bad = np.nonzero(got[r] != vv)[0]
            assert len(bad) == 0, (what, "chain", r, "differing variables", len(bad), bad[:12])

    def compare_counts(self, what):
        n, nc = len(self.cnt), len(self.cnt[0])
        got = np.empty((n, nc), np.int64)
        if n == 1:
            _lib.check(self.L.nsk_state_download(self.h, None, None, None, _lib.ptr(got)))
        else:
            _lib.check(self.L.nsk_chains_download(self.h, None, _lib.ptr(got)))
        self.unfolded = 0
        for r, cnt in enumerate(self.cnt):
            bad = np.nonzero(got[r] != cnt)[0]
            assert len(bad) == 0, (what, "chain", r, "differing tallies", len(bad), bad[:8], got[r][bad[:8]], cnt[bad[:8]])

    # ------------------------------------------------------------------ the calls
    def gibbs(self, n, se, burnin):
        moved = [False] * len(self.vv)          # per chain: did a sweep of this call change a value?
        for s in range(n):
            for r in range(len(self.vv)):
                last = self.vv[r].copy()
                assert self.og.gibbs_dev(self.order, self.ps, self.vv[r], self.wv, self.cnt[r], self.seed ^ (r << 32),
                                         (self.sweep + s) & M64, se, burnin=burnin) == 0
                moved[r] = moved[r] or bool((last != self.vv[r]).any())
            if not burnin:
                self.tallied += 1
                self.unfolded += 1
                if self.tally256 and self.tallied == 256:
                    # a slot that was 1 in all 256 sweeps (a byte that wraps if nothing folds in time) beside one that
                    # was not (the neighbour a carry out of that byte lands in)
                    for cnt in self.cnt:
                        assert cnt.max() == 256 and cnt.min() < 256, (int(cnt.max()), int(cnt.min()))
        self.sweep = (self.sweep + n) & M64
        self.lively.append((("gibbs", n), all(moved), None))
        if self.fg is not None:
            _lib.check(self.L.nsk_gibbs_sweeps(self.h, n, int(se), int(burnin)))
            self._compare_values(("gibbs", n, se, burnin, "ending at sweep", self.sweep))

    def learn(self, n, step, reg, trunc, lne):
        assert len(self.vv) == 1
        v0, e0, w0 = self.vv[0].copy(), self.ve.copy(), self.wv.copy()
        assert self.og.learn_call(self.order, self.ps, self.vv[0], self.ve, self.wv, n, step, DECAY, reg, REG_PARAM, trunc,
                                  lne, self.seed, self.sweep) == 0
        self.sweep = (self.sweep + n) & M64
        self.lively.append((("learn", n), bool((v0 != self.vv[0]).any() or (e0 != self.ve).any()), bool((w0 != self.wv).any())))
        if self.fg is not None:
            _lib.check(self.L.nsk_learn_sweeps(self.h, n, float(step), DECAY, int(reg), REG_PARAM, int(trunc), int(lne)))
            vv, ve, wv = np.empty_like(self.vv[0]), np.empty_like(self.ve), np.empty_like(self.wv)
            _lib.check(self.L.nsk_state_download(self.h, _lib.ptr(vv), _lib.ptr(ve), _lib.ptr(wv), None))
            what = ("learn", n, "ending at sweep", self.sweep)
            assert np.array_equal(vv, self.vv[0]), (what, np.nonzero(vv != self.vv[0])[0][:12])
            assert np.array_equal(ve, self.ve), (what, np.nonzero(ve != self.ve)[0][:12])
            bad = np.nonzero(wv.view(np.uint64) != self.wv.view(np.uint64))[0]
            assert len(bad) == 0, (what, "differing weights", len(bad), bad[:8], wv[bad[:8]], self.wv[bad[:8]])

    def weights(self, salt):
        """A weight upload alone.  It must not reset the tallies: every script calls it with a tally residue on the
        device (tallied sweeps and no count download since), which the comparison at the script's end still counts."""
        assert self.unfolded > 0, "the script uploads weights without a tally residue on the device"
        self.wv += np.random.default_rng(salt).normal(0, 0.2, len(self.wv))
        if self.fg is not None:
            w = np.ascontiguousarray(self.wv)
            _lib.check(self.L.nsk_state_upload(self.h, None, None, _lib.ptr(w), None))

    def values(self, kind):
        """A values upload alone.  "bad": a 2 in every 29th binary variable, evidence or not -- outside the domain, so
        the handle leaves its draw tables and captured sequences for the exp-per-update kernels.  "regular": the values as
        they are with every variable back inside its domain."""
        assert len(self.vv) == 1
        vv = self.vv[0]
        if kind == "bad":
            assert (self.og.variable["cardinality"] == 2).all()
            vv[::29] = 2
        else:
            assert kind == "regular"
            np.minimum(vv, self.og.variable["cardinality"] - 1, out=vv)
        if self.fg is not None:
            _lib.check(self.L.nsk_state_upload(self.h, _lib.ptr(np.ascontiguousarray(vv)), None, None, None))
            self._compare_values(("values", kind))

    def set_seed(self, seed, sweep0):
        self.seed, self.sweep = int(seed) & M64, int(sweep0) & M64
        if self.fg is not None:
            _lib.check(self.L.nsk_set_seed(self.h, self.seed, self.sweep))

    def tag(self, t):
        self.og.set_rng_tag(t)
        if self.fg is not None:
            _lib.check(self.L.nsk_set_rng_tag(self.h, int(t)))

    def chains(self, n):
        """New chains start from the initial values with empty tallies, as nsk_graph_create leaves a handle."""
        keep = min(n, len(self.vv))
        self.vv, self.cnt = self.vv[:keep], self.cnt[:keep]
        for _ in range(keep, n):
            vv, _, _, cnt = self.og.initial_state()
            self.vv.append(vv)
            self.cnt.append(cnt)
        if self.fg is not None:
            _lib.check(self.L.nsk_set_chains(self.h, n))
            self.unfolded = 0           # (nsk_set_chains folds: the tallies move with their chains)
            self._compare_values(("chains", n))

    def cond(self, n):
        """The potentials the next sweep would exponentiate, from the weights and values resident on the device."""
        nvar = len(self.vv[0])
        vids = np.ascontiguousarray(np.linspace(0, nvar - 1, n).astype(np.int64))
        card = self.og.variable["cardinality"][vids].astype(np.int64)
        off = np.concatenate([[0], np.cumsum(card)])
        want = np.zeros(int(off[-1]))
        for i, v in enumerate(vids):
            for k in range(card[i]):
                rc, want[off[i] + k] = self.og.potential(int(v), k, self.vv[0], self.wv)
                assert rc == 0
        if self.fg is not None:
            got = np.zeros_like(want)
            _lib.check(self.L.nsk_conditionals(self.h, _lib.BUF_VALUE, 0, 1, _lib.ptr(vids), len(vids), 0, _lib.ptr(got)))
            bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
            assert len(bad) == 0, ("potentials", len(bad), bad[:8], got[bad[:8]], want[bad[:8]])

    def lp(self):
        """include/numbskull_amd.h: the sum differs from the exactly rounded one by at most (nfactor + 1) 2^-53 sum |term|."""
        f, vid, x = self.og.factor, self.og.fmap["vid"], self.vv[0]
        e = np.zeros(len(f))
        for fid in range(len(f)):
            s, a = int(f[fid]["ftv_offset"]), int(f[fid]["arity"])
            vs = int(vid[s]) if a >= 1 and int(f[fid]["factorFunction"]) != -1 else -1
            rc, e[fid] = self.og.eval_factor(fid, vs, int(x[vs]) if vs >= 0 else 0, x)
            assert rc == 0
        t = self.wv[f["weightId"].astype(np.int64)] * e
        ref = math.fsum(t.tolist())
        bound = (len(t) + 1) * 2.0 ** -53 * math.fsum(np.abs(t).tolist())
        if self.fg is not None:
            out = np.zeros(1)
            _lib.check(self.L.nsk_log_potential(self.h, _lib.BUF_VALUE, 0, 1, _lib.ptr(out)))
            print("log-potential %.17g reference %.17g |diff| %.3g bound %.3g" % (out[0], ref, abs(out[0] - ref), bound))
            assert abs(out[0] - ref) <= bound, (out[0], ref, bound)

    def run(self, calls):
        ops = {"gibbs": self.gibbs, "learn": self.learn, "weights": self.weights, "values": self.values, "seed": self.set_seed,
               "tag": self.tag, "chains": self.chains, "cond": self.cond, "lp": self.lp}
        for call in calls:
            if call[0] == "counts":
                if self.fg is not None:
                    self.compare_counts(call)
            else:
                ops[call[0]](*call[1:])
        assert not self.tally256 or self.tallied >= 255         # ((14, 241) fills the bytes and stops there: no 256th sweep)
        if self.fg is not None:
            self.compare_counts("end of the script")
            self._compare_values("end of the script")       # (the fold left the values alone)


# ------------------------------------------------------------------------------------------------------- the graphs
def fold_grid():
    """48 x 40, weight 1.0, every cell starting at 1: EQUAL factors give +-1, so a cell whose four neighbours agree with
    it flips with probability 1 / (1 + e^8) and most slots are still 1 in every one of 256 sweeps (at the suite's usual
    0.3 no slot gets there).  Tables only: calls of 16 sweeps and more are captured."""
    return graphgen.ising_grid(48, 40, weight=1.0, initial=np.ones(48 * 40, np.int64))


def table_grid():
    """The suite's usual table grid, from seeded values: it moves in every sweep."""
    return graphgen.ising_grid(48, 40, weight=0.3, initial=np.random.default_rng(11).integers(0, 2, 48 * 40))


def wide_fold_grid():
    """The same on wide quads (under wide_trips.ENV): the 10M grid's kernel."""
    return graphgen.ising_grid(16, 1000, weight=1.0, initial=np.ones(16 * 1000, np.int64))


def learning_grid(rows=28, cols=80):
    """wide_trips.learning_grid shrunk: two free weights, every cell evidence with a seeded value."""
    rng = np.random.default_rng(1)
    return graphgen.ising_grid(rows, cols, weight=0.2, fixed=False, two_weights=True, evidence=rng.integers(0, 2, rows * cols))


def evidence_grid(rows=48, cols=40):
    """The table grid with a tenth of its cells evidence, seeded values everywhere."""
    n = rows * cols
    rng = np.random.default_rng(7)
    g = graphgen.ising_grid(rows, cols, weight=0.3, initial=rng.integers(0, 2, n))
    g[1]["isEvidence"][rng.choice(n, n // 10, replace=False)] = 1
    return g


def tile_case(name, nweight=None):
    return lambda: tiles.build_case(name, nweight=nweight, learn=True)[0]


# ------------------------------------------------------------------------------------------------------- the scripts
# graph: a builder; env: switches beyond those of `tile` (a tests/tiles.py case: its switches and head lookup);
# expect: what nsk_graph_info must say (a value, or ">0"); tally256: the fold precondition
Script = namedtuple("Script", "graph seed calls env tile expect tally256")


def _script(graph, seed, calls, env=(), tile=None, expect=(), tally256=False):
    return Script(graph, seed, tuple(calls), dict(env), tile, dict(expect), tally256)


def _tallied(*ns):
    return [("gibbs", n, 1, 0) for n in ns]


NO_GRAPH = {"NSK_DIAG": "1", "NSK_NO_GRAPH": "1"}
NO_PACK = dict(wide_trips.ENV, NSK_NO_PACK_TALLY="1")
SCRIPTS = {}

# ---- A: the tally residue a call leaves to the next.  Replays fold BEFORE a replay that would pass 255 sweeps, the eager
# loop folded AFTER the sweep that reached 255 exactly: 15 eager sweeps, then 3 x 64 + 3 x 16 captured ones leave 255 in
# the counter and the eager sweep behind them adds to full bytes.
FOLDS = {"15_241": _tallied(15, 241), "15_240_1": _tallied(15, 240, 1), "15_240_16": _tallied(15, 240, 16),
         "14_241": _tallied(14, 241), "1_254_1": _tallied(1, 254, 1), "15_burn5_241": [("gibbs", 15, 1, 0), ("gibbs", 5, 1, 1), ("gibbs", 241, 1, 0)]}
# (seed 5: this grid flips about one cell a sweep, and under seeds 1 .. 4 one of the 1-sweep calls moves nothing in the
#  oracle of tests/test_resident_calls_cpu.py)
for _n, _c in FOLDS.items():
    SCRIPTS["fold_" + _n] = _script(fold_grid, 5, _c, tally256=True)
    SCRIPTS["fold_eager_" + _n] = _script(fold_grid, 5, _c, env=NO_GRAPH, tally256=True)
SCRIPTS["fold_chains_15_241"] = _script(fold_grid, 5, [("chains", 3)] + _tallied(15, 241), tally256=True)
# ---- B: the same on wide quads: the packed tally unpacked into cnt_pos, and dword adds into cnt_pos
SCRIPTS["fold_wide_15_241"] = _script(wide_fold_grid, 3, _tallied(15, 241), env=wide_trips.ENV, expect={"wide_quads": ">0"}, tally256=True)
SCRIPTS["fold_wide_nopack_15_241"] = _script(wide_fold_grid, 3, _tallied(15, 241), env=NO_PACK, expect={"wide_quads": ">0"}, tally256=True)


# ---- C: weights across calls: learn, sweep, learn, sweep with no upload between (learn calls of 1 and 2 sweeps: a lagged
# handle with an odd number of colours ends on either weight set), then a weight upload alone with a tally residue on
# the device, eager and captured sweeps, and the potentials and the log-potential of the resident state
def _weights_calls(lne):
    return [("learn", 1, 0.02, 2, 1, lne), ("gibbs", 3, 1, 0), ("cond", 12), ("learn", 2, 0.02, 1, 3, lne), ("gibbs", 20, 1, 0), ("cond", 12),
            ("weights", 5), ("gibbs", 2, 1, 0), ("gibbs", 18, 1, 0), ("cond", 40), ("lp",),
            ("learn", 1, 0.01, 2, 1, lne), ("cond", 12), ("gibbs", 17, 1, 0), ("lp",)]


SCRIPTS["weights_grid"] = _script(learning_grid, 5, _weights_calls(0), expect={"learn_lag": 1, "direct_weights": 0})
SCRIPTS["weights_mixed_routes"] = _script(tile_case("mixed_routes"), 47, _weights_calls(1), tile="mixed_routes",
                                          expect={"learn_lag": 0, "direct_weights": ">0", "weight_slots": 1})
# more than 256 weights, one per factor: updated in place by the learning kernels, in slots of the layout's order
SCRIPTS["weights_per_factor"] = _script(tile_case("ep_rest_hubs"), 43, _weights_calls(1), tile="ep_rest_hubs",
                                        expect={"learn_lag": 0, "direct_weights": ">0", "weight_slots": 1})
# at most 256 weights and an odd number of colours: the lagged pipeline ends a 1-sweep call on the other weight set
SCRIPTS["weights_odd_colours"] = _script(tile_case("gen_m3_blocker"), 43, _weights_calls(1), tile="gen_m3_blocker",
                                         expect={"learn_lag": 1, "ncolors": 5})

# ---- D: what the plans and the captured graphs are keyed by: sample_evidence, burn-in, the packed tally, regular values
SCRIPTS["keys_evidence_grid"] = _script(evidence_grid, 21, [
    ("gibbs", 16, 1, 0), ("gibbs", 17, 0, 0), ("gibbs", 16, 1, 1), ("gibbs", 33, 1, 0), ("gibbs", 16, 0, 1), ("gibbs", 80, 0, 0),
    ("values", "bad"), ("gibbs", 16, 0, 0), ("gibbs", 19, 1, 0), ("values", "regular"), ("gibbs", 16, 0, 0), ("gibbs", 70, 1, 0),
    ("gibbs", 16, 1, 1), ("gibbs", 16, 0, 0)])

# the chain count changes under resident state: nsk_set_chains drops the plans and the captured graphs (they hold the
# arrays' addresses) and moves values and tallies; the chains both counts have keep theirs
SCRIPTS["keys_chain_count"] = _script(table_grid, 9, [
    ("gibbs", 20, 1, 0), ("chains", 3), ("gibbs", 36, 1, 0), ("gibbs", 16, 1, 1), ("chains", 2), ("gibbs", 17, 1, 0), ("chains", 1),
    ("gibbs", 33, 1, 0)])

# ---- E: the counter words: a seed with a high half, and the sweep index crossing 2^32 inside one call
SEED64 = 0x9E3779B97F4A7C15
SCRIPTS["counter_grid_16"] = _script(table_grid, 0, [("seed", SEED64, 2 ** 32 - 20), ("gibbs", 40, 1, 0)])
SCRIPTS["counter_grid_64"] = _script(table_grid, 0, [("seed", SEED64, 2 ** 32 - 70), ("gibbs", 100, 1, 0)])
SCRIPTS["counter_mixed_routes"] = _script(tile_case("mixed_routes"), 0, [("seed", SEED64, 2 ** 32 - 20), ("gibbs", 40, 1, 0)],
                                          tile="mixed_routes")
SCRIPTS["counter_chains"] = _script(table_grid, 0, [("chains", 3), ("seed", SEED64, 2 ** 32 - 20), ("gibbs", 40, 1, 0)])
SCRIPTS["counter_learning"] = _script(learning_grid, 0, [("seed", SEED64, 2 ** 32 - 2), ("learn", 4, 0.02, 2, 1, 0), ("tag", 12345),
                                                         ("gibbs", 20, 1, 0), ("learn", 2, 0.02, 1, 3, 0), ("gibbs", 3, 1, 0)])


def set_env(monkeypatch, script):
    if script.tile:
        tiles.set_switches(monkeypatch, script.tile)
    for k, v in script.env.items():
        monkeypatch.setenv(k, v)


def handle(monkeypatch, name):
    """(script, FactorGraph) under the script's switches; no device is touched yet."""
    sc = SCRIPTS[name]
    set_env(monkeypatch, sc)
    hbv = tiles.CASES[sc.tile].hbv if sc.tile else False
    _, fg = session(sc.graph(), seed=sc.seed, head_by_vid=hbv)
    return sc, fg, hbv


def check_info(sc, info):
    for k, want in sc.expect.items():
        assert (info[k] > 0) if want == ">0" else (info[k] == want), (k, want, info[k])
