"""Every point Gauss-Seidel kernel form on the designed dependency levels of tests/gs_cases.py, through the
device-pointer API (amg_mat_create, amg_mat_build_gs, amg_mat_gs_sweeps), bit for bit against the sequential oracle
(gs_cases.oracle, pinned to a plain Python restatement by tests/test_gs_cases_host.py).

A case first asserts, through amg_mat_gs_info, that the schedule took the forms it was designed for -- a case meant for
gs_chainl2_kernel cannot pass on gs_level_kernel -- and then sweeps every sequence in both flavours under the dataflow
form (look-ahead 0, 1 and 50), the chained sweeps of both generations, and a launch per level with and without the
entry-range hint.  x carries a guard region behind its halo; b, the halo and the guard must come back untouched.
One process; every switch is put back to its default."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import gs_cases as gc

pytestmark = pytest.mark.gpu

DEFAULTS = (("gs_flow", 1), ("gs_flow_lookahead", 0), ("gs_chain", 2), ("gs_level_hint", 1))
GUARD = 96
GUARD_FILL = -7.25
FLOW_SETTINGS = tuple(dict(gs_flow=2, gs_flow_lookahead=la) for la in (0, 1, 50))
OTHER_SETTINGS = (dict(gs_flow=0, gs_chain=2), dict(gs_flow=0, gs_chain=1), dict(gs_flow=0, gs_chain=0),
                  dict(gs_flow=0, gs_chain=0, gs_level_hint=0), dict(gs_flow=0, gs_chain=2, gs_level_hint=0))


def _lib():
    from pyamg_amd import _lib as lib
    return lib.lib()


def restore_defaults():
    L = _lib()
    for name, value in DEFAULTS:
        getattr(L, "amg_set_" + name)(value)


@pytest.fixture(scope="module", autouse=True)
def switch_defaults():
    try:
        yield
    finally:
        restore_defaults()


@contextlib.contextmanager
def switched(**kw):
    L = _lib()
    assert set(kw) <= set(dict(DEFAULTS))
    try:
        restore_defaults()
        for name, value in kw.items():
            getattr(L, "amg_set_" + name)(value)
        yield L
    finally:
        restore_defaults()


_ORACLE = {}


def oracle_result(case, seq, bsr1):
    """the model's x for one sequence, computed once per module and left unchanged"""
    key = (case.name, tuple(seq), bsr1)
    if key not in _ORACLE:
        r = gc.oracle(case, seq, bsr1, case.x, case.b)
        r.setflags(write=False)
        _ORACLE[key] = r
    return _ORACLE[key]


class Device(object):
    """one case on the device: the operator, pristine x and b, and working copies that end in a guard region"""

    def __init__(self, case):
        import torch
        from pyamg_amd import _lib
        self.torch, self.lib, self.case = torch, _lib, case
        self.L = _lib.lib()
        self.x0 = torch.from_numpy(np.concatenate((case.x, np.full(GUARD, GUARD_FILL)))).cuda()
        self.b0 = torch.from_numpy(np.concatenate((case.b, np.full(GUARD, GUARD_FILL)))).cuda()
        self.x, self.b = self.x0.clone(), self.b0.clone()
        self.mat = None

    def build(self):
        """(re)build the schedule under the switches in force; returns the amg_mat_gs_info fields by name"""
        c, L, lib = self.case, self.L, self.lib
        self.close()
        self.mat = L.amg_mat_create(0, c.n, c.ncols, lib.ip(c.Ap), lib.ip(c.Aj), lib.dp(c.Ax))
        assert self.mat
        out = np.full(len(gc.INFO_FIELDS) + 2, -99, dtype=np.intc)
        assert L.amg_mat_gs_info(self.mat, out.ctypes.data_as(C.c_void_p), len(gc.INFO_FIELDS)) < 0     # no schedule yet
        lib.check(L.amg_mat_build_gs(self.mat, None if c.order is None else lib.ip(c.order), 0 if c.order is None else len(c.order)))
        assert L.amg_mat_gs_info(self.mat, out.ctypes.data_as(C.c_void_p), len(out)) == len(gc.INFO_FIELDS)
        assert list(out[len(gc.INFO_FIELDS):]) == [-99, -99]
        assert L.amg_mat_gs_levels(self.mat) == out[0]
        return dict(zip(gc.INFO_FIELDS, (int(v) for v in out)))

    def sweep(self, seq, bsr1):
        torch = self.torch
        self.x.copy_(self.x0)
        sq = np.array(seq, dtype=np.uint8)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.lib.check(self.L.amg_mat_gs_sweeps(self.mat, C.c_void_p(self.x.data_ptr()), C.c_void_p(self.b.data_ptr()),
                                                sq.ctypes.data_as(C.c_void_p), len(seq), int(bsr1), st))
        return self.x.cpu().numpy()

    def inputs_untouched(self):
        return bool(self.torch.equal(self.b.view(self.torch.int64), self.b0.view(self.torch.int64)))

    def close(self):
        if self.mat:
            self.torch.cuda.synchronize()
            self.L.amg_mat_destroy(self.mat)
            self.mat = None


def check_sweep(dev, seq, bsr1, what, nan_rows_free=False):
    case = dev.case
    got = dev.sweep(seq, bsr1)
    want = oracle_result(case, seq, bsr1)
    tag = (case.name, "seq %s" % "".join(str(d) for d in seq), "bsr1" if bsr1 else "csr") + tuple(what)
    n, nc = case.n, case.ncols
    if nan_rows_free:                                       # rows the model makes NaN need only be NaN
        nan = np.isnan(want[:n])
        assert np.array_equal(np.isnan(got[:n]), nan), tag
        bad = gc.bit_mismatches(got[:n][~nan], want[:n][~nan])
    else:
        bad = gc.bit_mismatches(got[:n], want[:n])
    assert bad == 0, tag + ("%d of %d rows differ from the oracle" % (bad, n),)
    assert gc.bit_mismatches(got[n:nc], case.x[n:nc]) == 0, tag + ("the halo changed",)
    assert np.all(got[nc:] == GUARD_FILL), tag + ("the guard behind x changed",)


def expected_info(case, flow_mode):
    info = case.info(flow_mode)
    return {k: info[k] for k in gc.INFO_FIELDS}


def sweep_settings(dev, settings, seqs, L, **kw):
    for sw in settings:
        restore_defaults()
        for name, value in sw.items():
            getattr(L, "amg_set_" + name)(value)
        what = tuple("%s %d" % kv for kv in sorted(sw.items()))
        for seq in seqs:
            for bsr1 in (False, True):
                check_sweep(dev, seq, bsr1, what, **kw)
        assert dev.inputs_untouched(), (dev.case.name,) + what + ("b changed",)


@pytest.mark.parametrize("case", gc.all_cases(), ids=repr)
def test_designed_case(case, monkeypatch):
    if case.halo:
        monkeypatch.setenv("AMG_DIST_FLOW", "1")            # a rank's local operator: the dataflow form on request only
    dev = Device(case)
    try:
        with switched(gs_flow=2) as L:
            info = dev.build()
            assert {k: info[k] for k in case.expect} == case.expect, case.name
            assert info == expected_info(case, 2), case.name
            sweep_settings(dev, (FLOW_SETTINGS if info["flow"] else ()) + OTHER_SETTINGS, gc.SEQUENCES, L)
        # the default: where it picks the dataflow form, the level-ordered copies of the other paths are dropped
        short = (gc.SEQUENCES[4], gc.SEQUENCES[8])
        with switched() as L:
            info = dev.build()
            assert info == expected_info(case, 1), case.name
            assert info["level_copy"] == (0 if info["flow_auto"] else 1)
            sweep_settings(dev, ({},), short, L)
        # built without the form, swept with the form requested: the other paths serve it
        with switched(gs_flow=0) as L:
            info = dev.build()
            assert info == expected_info(case, 0) and not info["flow"], case.name
            sweep_settings(dev, (dict(gs_flow=2),), short, L)
        assert _lib().amg_gs_flow_status() == 0
    finally:
        dev.close()
        restore_defaults()


def test_info_needs_a_schedule_and_an_array():
    case = gc.all_cases()[1]
    dev = Device(case)
    try:
        with switched() as L:
            dev.build()
            few = np.full(4, -99, dtype=np.intc)
            assert L.amg_mat_gs_info(dev.mat, few.ctypes.data_as(C.c_void_p), 3) == 3
            assert list(few[:3]) == [case.info(1)[k] for k in gc.INFO_FIELDS[:3]] and few[3] == -99
            assert L.amg_mat_gs_info(dev.mat, None, 3) < 0
            assert L.amg_mat_gs_info(None, few.ctypes.data_as(C.c_void_p), 3) < 0
        assert _lib().amg_gs_flow_status() == 0
    finally:
        dev.close()


def test_sentinel_bits_in_x(monkeypatch):
    """x carries the dataflow sentinel 0x7FF4A5A55A5A0001 (a signalling NaN) at one owned and one halo position, each read
    by earlier rows: flow_gather_kernel quiets its copy -- what every arithmetic use would do -- instead of waiting for
    it.  Rows the model makes NaN need only be NaN; every other row matches bit for bit, and the halo keeps its bits.
    Kept last in the module."""
    case = gc.sentinel_case()
    monkeypatch.setenv("AMG_DIST_FLOW", "1")
    dev = Device(case)
    try:
        with switched(gs_flow=2) as L:
            info = dev.build()
            assert info["flow"] == 1 and info == expected_info(case, 2)
            sweep_settings(dev, FLOW_SETTINGS + OTHER_SETTINGS[:3], gc.SEQUENCES, L, nan_rows_free=True)
        assert _lib().amg_gs_flow_status() == 0
    finally:
        dev.close()
        restore_defaults()
