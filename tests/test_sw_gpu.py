"""Swendsen-Wang on the device (nsk_sw_setup / nsk_sw_sweeps) against the numpy mirror diagnostics.sw_tables / sw_step with
the oracle's exp_det and the device's own Philox words (tests/sw.py), bit for bit and integer for integer.
tests/test_sw_cpu.py ties the mirror to the model."""

import ctypes as C

import numpy as np
import pytest

import bp
import sw
from numbskull_amd import _lib
from numbskull_amd.diagnostics import sw_tables, sw_step
from oracle import binding as orc
from util import session

pytestmark = pytest.mark.gpu


class Dev(object):
    """a resident handle of a case with its chains at distinct random states (clamped variables as the graph has them)"""

    def __init__(self, case, setup=True):
        build, hbv, self.sev, self.R = sw.CASES[case] if isinstance(case, str) else case
        _, self.fg = session(build(), seed=sw.SEED, head_by_vid=hbv)
        self.L, self.h, self.sweep = _lib.lib(), self.fg._engine(), 0
        self.fg._push(0, 0)
        var = self.fg.variable
        if self.R > 1:
            _lib.check(self.L.nsk_set_chains(self.h, self.R))
            x = np.tile(np.asarray(var["initialValue"], np.int64), (self.R, 1))
            x[:, var["isEvidence"] == 0] = np.random.default_rng(8).integers(0, 2, (self.R, int((var["isEvidence"] == 0).sum())))
            _lib.check(self.L.nsk_chains_upload(self.h, _lib.ptr(x), None))
        self.base, self.info = self.bytes(), _lib.SwInfo()
        if setup:
            _lib.check(self.setup())
            i = self.info
            self.order, self.ends = np.zeros(i.nvars, np.int64), np.zeros((i.nbonds, 2), np.int64)
            self.bond_factor = np.zeros(i.nbonds, np.int64)
            _lib.check(self.L.nsk_sw_layout(self.h, _lib.ptr(self.order), _lib.ptr(self.bond_factor), _lib.ptr(self.ends)))

    bytes = lambda self: self.fg.info()["device_bytes"]      # noqa: E731

    def setup(self):
        return self.L.nsk_sw_setup(self.h, _lib.BUF_VALUE, 0, self.sev, C.byref(self.info))

    def values(self, counts=False):
        out = np.empty((self.R, len(self.fg.count if counts else self.fg.variable)), np.int64)
        _lib.check(self.L.nsk_chains_download(self.h, None if counts else _lib.ptr(out), _lib.ptr(out) if counts else None))
        return out

    def tables(self):
        J, q, H = np.zeros(self.info.nbonds), np.zeros(self.info.nbonds), np.zeros(self.info.nvars, np.int64)
        for what, out in ((_lib.SW_J, J), (_lib.SW_Q, q), (_lib.SW_H, H)):
            _lib.check(self.L.nsk_sw_download(self.h, what, _lib.ptr(out)))
        return J, q, H

    def sweeps(self, nsteps, gibbs, burnin=0):
        out = np.full((3, nsteps, self.R), -1, np.int64)
        rc = self.L.nsk_sw_sweeps(self.h, nsteps, gibbs, burnin, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]))
        assert rc == _lib.OK, self.L.nsk_last_error().decode()
        return out

    def labels(self, r):
        out = np.full(self.info.nvars, -1, np.int32)
        _lib.check(self.L.nsk_sw_labels(self.h, r, _lib.ptr(out)))
        return out


def _steps_equal_the_mirror(d, nsteps=5):
    J, q, H = d.tables()
    total = np.zeros(3, np.int64)
    for _ in range(nsteps):
        x = d.values()
        got, after = d.sweeps(1, 0), d.values()
        for r in range(d.R):
            ub, uc = (sw.uniforms(sw.SEED, r, d.sweep, s, n, device=True) for s, n in ((4, d.info.nbonds), (5, d.info.nvars)))
            y, labels, clusters, largest, flipped = sw_step(x[r], d.order, d.ends, J, q, H, ub, uc, exp=orc.exp_det)
            assert np.array_equal(d.labels(r), labels) and np.array_equal(after[r], y), (d.sweep, r)
            assert tuple(got[:, 0, r]) == (clusters, largest, flipped), (d.sweep, r)
        d.sweep += 1
        total += got[:, 0].sum(axis=1)
    # lively: bonds were active, clusters of several variables, and some of them flipped
    assert 0 < total[2] and total[0] < nsteps * d.R * d.info.nvars and total[1] > nsteps * d.R
    return got


@pytest.mark.parametrize("name", sorted(sw.CASES))
def test_tables_equal_the_mirror(name):
    d = Dev(name)
    fg, bi = d.fg, _lib.BpInfo()
    _lib.check(d.L.nsk_bp_setup(d.h, _lib.BUF_VALUE, 0, d.sev, C.byref(bi)))
    theta = np.zeros(bi.ntable)
    _lib.check(d.L.nsk_bp_download(d.h, _lib.BP_THETA, _lib.ptr(theta)))
    t = sw_tables(theta, bp.bp_layout(fg.factor, fg.fmap, fg.variable, d.values()[0], bool(d.sev)), exp=orc.exp_det)
    J, q, H = d.tables()
    assert fg.info()["value_bytes"] == (4 if name == "grid_int32" else 1) and len(J) > 0 and np.abs(H).max() > 0
    assert np.array_equal(J.view(np.int64), t["J"].view(np.int64)) and np.array_equal(q.view(np.int64), t["q"].view(np.int64))
    assert np.array_equal(H, t["H"][d.order]) and np.array_equal(d.bond_factor, t["bond_factor"])
    assert np.array_equal(d.order[d.ends], t["bond_vars"])


@pytest.mark.parametrize("name", sorted(sw.CASES))
def test_steps_equal_the_mirror(name):
    d = Dev(name)
    _steps_equal_the_mirror(d)
    if name == "grid40":
        assert d.info.ntiles > 1 and d.info.ncross > 0


@pytest.mark.parametrize("name", ["grid40", "path3000"])
def test_small_tiles_and_later_trips(name, monkeypatch):
    monkeypatch.setenv("NSK_DIAG", "1")
    monkeypatch.setenv("NSK_SW_TILE", "64")
    monkeypatch.setenv("NSK_SW_GRID_CAP", "1")
    d = Dev(name)
    assert d.info.ntiles >= d.info.nvars // 64 and d.info.ncross > 0
    _steps_equal_the_mirror(d, 3)


def test_a_step_is_an_update_and_the_sweeps_of_gibbs():
    a, b = Dev("grid40"), Dev("grid40")
    a.sweeps(2, 1)
    for _ in range(2):
        b.sweeps(1, 0)
        _lib.check(b.L.nsk_gibbs_sweeps(b.h, 1, 0, 0))
    for d in (a, b):        # the sweep index too: one more sweep draws the same
        _lib.check(d.L.nsk_gibbs_sweeps(d.h, 1, 0, 0))
    assert np.array_equal(a.values(), b.values()) and np.array_equal(a.values(True), b.values(True)) and a.values(True).any()
    assert a.fg.info()["sweeps_done"] == b.fg.info()["sweeps_done"] == 3


def test_refusals_and_the_ledger():
    for cards, factor in (([2, 3, 2], (sw.EQUAL, [0, 1], [0, 0], 0.5)), ([2, 2, 2], (sw.AND, [0, 1, 2], [0, 0, 0], 0.5))):
        build = lambda: bp.spec_graph(cards, [0] * 3, [0] * 3, [(sw.ISTRUE, [0], [0], 0.3), factor])      # noqa: E731
        d = Dev((build, False, 0, 1), setup=False)
        assert d.setup() == _lib.E_INVALID and b"factor 1" in d.L.nsk_last_error() and d.bytes() == d.base
        assert d.L.nsk_sw_sweeps(d.h, 1, 0, 0, None, None, None) == _lib.E_INVALID       # nothing is set up
    d = Dev("grid5x7")
    assert d.L.nsk_sw_clear(d.h) == _lib.OK         # (the factor records the first set-up uploaded stay with the handle)
    base = d.bytes()
    assert d.setup() == _lib.OK
    held, tables = d.bytes(), d.tables()
    assert held == base + d.info.device_bytes > base
    for args in ((0, 0, 0), (65537, 0, 0), (1, -1, 0), (65536, 65536, 0)):
        assert d.L.nsk_sw_sweeps(d.h, *(args + (None, None, None))) == _lib.E_INVALID and d.bytes() == held, args
    assert d.L.nsk_sw_labels(d.h, 0, None) == _lib.E_INVALID and d.L.nsk_sw_download(d.h, 3, None) == _lib.E_INVALID
    d.fg.weight_value[0][0] = np.inf
    d.fg._push(0, 0)
    assert d.L.nsk_sw_refresh(d.h) == _lib.E_RANGE and all(np.array_equal(x, y) for x, y in zip(tables, d.tables()))
    assert d.setup() == _lib.E_RANGE and d.bytes() == held                      # the resident set-up stays
    assert d.L.nsk_sw_sweeps(d.h, 1, 0, 0, None, None, None) == _lib.OK         # every output may be NULL
    assert d.bytes() > held and d.L.nsk_sw_clear(d.h) == _lib.OK and d.bytes() == base
    assert d.L.nsk_sw_sweeps(d.h, 1, 0, 0, None, None, None) == _lib.E_INVALID


def test_python_api():
    build = sw.CASES["grid5x7"][0]
    d = Dev("grid5x7")
    want = _steps_equal_the_mirror(d, 1)
    _, fg = session(build(), seed=sw.SEED)
    res = fg.swendsen_wang(1, sweeps=0)
    assert np.array_equal(fg.var_value[0], d.values()[0]) and all(res[k][0, 0] == want[i, 0, 0] for i, k in enumerate(("clusters", "largest", "flipped")))
    _, fg = session(build(), seed=sw.SEED, chains=3)
    res = fg.swendsen_wang(4, sweeps=2, var_copy="all")
    assert res["clusters"].shape == (4, 3) and fg.var_value.shape[0] == 3 and res["info"]["nbonds"] == 58
    assert fg.count.sum() == fg.chain_count.sum() > 0 and fg.count.max() <= 3 * 4 * 2
    _, bad = session(bp.spec_graph([2, 3], [0, 0], [0, 0], [(sw.EQUAL, [0, 1], [0, 0], 0.5)]))
    with pytest.raises(ValueError, match="cardinality 3"):
        bad.swendsen_wang(1)
