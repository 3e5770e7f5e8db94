"""Every block smoother kernel form on the designed block levels of tests/block_cases.py, bit for bit against the
sequential oracle (block_cases.oracle, pinned to a plain Python restatement by tests/test_block_cases_host.py).

The route is a one-level hierarchy whose coarse smoother is the smoother under test (amg_hier_create(1, 0),
amg_hier_set_matrix with the BSR blocks, amg_hier_set_coarse_smoother, amg_hier_finalize, amg_hier_relax): it needs no
P or R and issues real sweep sequences -- forward, backward and symmetric, one to three iterations; three symmetric
iterations are six sweeps, two dataflow launches.  A case first asserts, through amg_hier_block_info, that the schedule
took the form it was designed for -- a case meant for bgs_flow_kernel<3, 8, 16> cannot pass on bsr_stream_kernel -- and
then sweeps under the dataflow form (look-ahead 0, 1 and 50), the default, and the streamed levels (for the sliced
family also the level-cut slices).  Block Jacobi and the two point sweeps over the BSR level run the same way, and the
four flat amg_core entries over the whole range, sub-ranges and strides, every array argument compared.

One process; every switch is put back to its default.  Once a status word is non-zero or a call has failed, the remaining
cases skip: nothing more is launched after trouble."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import block_cases as bc
import flat_ranges
import oracle_lib

pytestmark = pytest.mark.gpu

DEFAULTS = (("gs_flow", 1), ("gs_flow_lookahead", 0), ("tile_target", 2048))
KIND = {"jacobi": 1, "gauss_seidel": 2, "block_jacobi": 5, "block_gauss_seidel": 6}
ORACLE_KIND = {"jacobi": "bsr_jacobi", "gauss_seidel": "bsr_gauss_seidel", "block_jacobi": "block_jacobi",
               "block_gauss_seidel": "block_gauss_seidel"}
SWEEPS = (("forward", 0, [0]), ("backward", 1, [1]), ("symmetric", 2, [0, 1]))
ALL_COMBOS = tuple((s, it) for s in SWEEPS for it in (1, 2, 3))
FEW_COMBOS = ((SWEEPS[2], 3), (SWEEPS[0], 1), (SWEEPS[1], 2))
CASES = bc.all_cases()
_TROUBLE = []                                               # set once: a non-zero status word or a failed call


def _lib():
    from pyamg_amd import _lib as lib
    return lib.lib()


def guard():
    if _TROUBLE:
        pytest.skip("an earlier case ended in trouble (%s): nothing more is launched" % _TROUBLE[0])


def call(rc, what):
    if rc != 0:
        _TROUBLE.append(what)
    from pyamg_amd import _lib as lib
    lib.check(rc)


def status_clean(what):
    st = _lib().amg_gs_flow_status()
    if st != 0:
        _TROUBLE.append("status word %d after %s" % (st, what))
    assert st == 0, what


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
    assert set(kw) <= set(dict(DEFAULTS))
    try:
        restore_defaults()
        for name, value in kw.items():
            getattr(_lib(), "amg_set_" + name)(value)
        yield
    finally:
        restore_defaults()


_ORACLE = {}


def oracle_result(case, kind, seq):
    """the oracle's x for one sequence, computed once per module and left unchanged"""
    key = (case.name, kind, tuple(seq))
    if key not in _ORACLE:
        r = bc.oracle(case, kind, seq, case.x, case.b)
        r.setflags(write=False)
        _ORACLE[key] = r
    return _ORACLE[key]


class Hier(object):
    """a one-level hierarchy over the case's blocks; the coarse smoother is the smoother under test"""

    def __init__(self, case):
        from pyamg_amd import _lib as lib
        self.lib, self.L, self.case = lib, lib.lib(), case
        self.h = self.L.amg_hier_create(1, 0)
        if not self.h:
            _TROUBLE.append("amg_hier_create")
        assert self.h
        n = case.nb * case.bs
        try:
            call(self.L.amg_hier_set_matrix(self.h, 0, 0, 1, n, n, case.bs, case.bs, case.Ap.ctypes.data, case.Aj.ctypes.data,
                                            case.Ax.ctypes.data, 0), "amg_hier_set_matrix")
        except Exception:
            self.close()
            raise

    def smoother(self, kind, sweep=0, iterations=1):
        d = self.lib.SmootherDesc()
        d.kind, d.iterations, d.sweep, d.omega = KIND[kind], iterations, sweep, bc.OMEGA
        if kind.startswith("block_"):
            d.blocksize, d.Dinv = self.case.bs, self.lib.dp(self.case.Dinv)
        call(self.L.amg_hier_set_coarse_smoother(self.h, C.byref(d)), "amg_hier_set_coarse_smoother")
        call(self.L.amg_hier_finalize(self.h), "amg_hier_finalize")

    def info(self, nout=len(bc.INFO_FIELDS) + 2):
        out = np.full(nout, -99, dtype=np.intc)
        k = self.L.amg_hier_block_info(self.h, 0, 2, out.ctypes.data_as(C.c_void_p), nout)
        assert k == len(bc.INFO_FIELDS) and list(out[k:]) == [-99] * (nout - k)
        return dict(zip(bc.INFO_FIELDS, (int(v) for v in out)))

    def relax(self):
        x, b = self.case.x.copy(), self.case.b.copy()
        call(self.L.amg_hier_relax(self.h, 0, 2, self.lib.dp(b), self.lib.dp(x)), "amg_hier_relax")
        assert bc.bit_mismatches(b, self.case.b) == 0
        return x

    def close(self):
        if self.h:
            self.L.amg_hier_destroy(self.h)
            self.h = None


def expected(case, smoother, flow_mode=2, sell_levels=False):
    info = case.info(smoother, flow_mode, sell_levels)
    return {k: info[k] for k in bc.INFO_FIELDS}


def sweep_combos(H, kind, combos, what):
    case = H.case
    for (sname, sweep, unit), its in combos:
        H.smoother(kind, sweep, its)
        got = H.relax()
        status_clean((case.name, kind, sname, its) + tuple(what))
        want = oracle_result(case, ORACLE_KIND[kind], unit * its)
        bad = bc.bit_mismatches(got, want)
        assert bad == 0, (case.name, kind, sname, "iterations %d" % its) + tuple(what) + ("%d of %d entries differ from the oracle" % (bad, len(want)),)


@contextlib.contextmanager
def hierarchy(case):
    H = Hier(case)
    try:
        yield H
    finally:
        H.close()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_block_gauss_seidel(case, monkeypatch):
    guard()
    kind = "block_gauss_seidel"
    monkeypatch.delenv("AMG_SELL_LEVELS", raising=False)
    try:
        # built wherever the form exists: the dataflow form under three look-aheads (else the streamed levels)
        with switched(gs_flow=2), hierarchy(case) as H:
            H.smoother(kind)
            info = H.info()
            assert {k: info[k] for k in case.expect} == case.expect, case.name
            assert info == expected(case, kind, 2), case.name
            for la in ((0, 1, 50) if info["flow"] else (0,)):
                _lib().amg_set_gs_flow_lookahead(la)
                sweep_combos(H, kind, ALL_COMBOS, ("flow 2", "look-ahead %d" % la))
        with switched(), hierarchy(case) as H:
            H.smoother(kind)
            assert H.info() == expected(case, kind, 1), case.name
            sweep_combos(H, kind, FEW_COMBOS, ("default",))
        # without the form: a streamed launch per level from the level-ordered copy
        with switched(gs_flow=0), hierarchy(case) as H:
            H.smoother(kind)
            info = H.info()
            assert info == expected(case, kind, 0) and not info["flow"] and info["level_copy"] and not info["slices"], case.name
            sweep_combos(H, kind, ALL_COMBOS, ("flow 0",))
        if case.family == "sliced":
            monkeypatch.setenv("AMG_SELL_LEVELS", "1")       # ... and from its level-cut slices
            with switched(gs_flow=0), hierarchy(case) as H:
                H.smoother(kind)
                info = H.info()
                assert info == expected(case, kind, 0, True) and info["slices"] > 0, case.name
                sweep_combos(H, kind, ALL_COMBOS, ("flow 0", "level slices"))
        status_clean(case.name)
    finally:
        restore_defaults()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_block_jacobi_and_the_point_sweeps(case):
    guard()
    try:
        with switched(), hierarchy(case) as H:
            # block Jacobi: the odd iteration count leaves the iterate in the other buffer
            H.smoother("block_jacobi")
            assert H.info() == expected(case, "block_jacobi"), case.name
            sweep_combos(H, "block_jacobi", ((SWEEPS[0], 1), (SWEEPS[0], 2)), ())
            # gauss_seidel on the BSR level: bsr_gauss_seidel, a backward sweep reverses the rows inside a block
            H.smoother("gauss_seidel")
            assert H.info() == expected(case, "gauss_seidel"), case.name
            sweep_combos(H, "gauss_seidel", tuple((s, it) for s in SWEEPS for it in (1, 2)), ())
            H.smoother("jacobi")
            assert H.info() == expected(case, "jacobi"), case.name
            sweep_combos(H, "jacobi", ((SWEEPS[0], 1), (SWEEPS[0], 2)), ())
        status_clean(case.name)
    finally:
        restore_defaults()


def flat_compare(case, names, what):
    from pyamg_amd import amg_core
    ref = flat_ranges.OracleTable(oracle_lib.load())
    ranges = bc.flat_ranges(case.nb)
    for nm in names:
        for fn, args in bc.flat_calls(case, ranges[nm]):
            want = flat_ranges.call_table(ref, fn, args)
            try:
                got = flat_ranges.call_table(amg_core, fn, args)
            except Exception:
                _TROUBLE.append("amg_core.%s" % fn)
                raise
            status_clean((case.name, fn, nm) + tuple(what))
            assert flat_ranges.bit_mismatches(want["x"], dict(args)["x"]) > 0, (case.name, fn, nm)      # the sweep did something
            flat_ranges.compare_all("%s: %s over %s %s" % (case.name, fn, nm, " ".join(what)), got, want)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_flat_entries(case):
    guard()
    try:
        names = ["all_fwd", "all_bwd"]
        if case.family == "oddities":
            names += ["sub_fwd", "stride2_fwd", "sub_bwd"]   # ntasks != nb: the dataflow form declines
        with switched():
            flat_compare(case, names, ())
        if case.family == "stream":
            # a lowered tile target: every level of the streamed sweeps takes several workgroups
            with switched(tile_target=256):
                flat_compare(case, ["all_fwd", "all_bwd"], ("tile target 256",))
            with switched(gs_flow=0, tile_target=256), hierarchy(case) as H:
                H.smoother("block_gauss_seidel")
                sweep_combos(H, "block_gauss_seidel", FEW_COMBOS, ("flow 0", "tile target 256"))
                H.smoother("block_jacobi")
                sweep_combos(H, "block_jacobi", ((SWEEPS[0], 1),), ("tile target 256",))
        status_clean(case.name)
    finally:
        restore_defaults()


def test_one_block_row_fewer_reports_no_slices(monkeypatch):
    guard()
    case = bc.sliced_minus_one()
    monkeypatch.setenv("AMG_SELL_LEVELS", "1")
    try:
        with switched(gs_flow=0), hierarchy(case) as H:
            H.smoother("block_gauss_seidel")
            info = H.info()
            assert info == expected(case, "block_gauss_seidel", 0, True) and info["slices"] == 0 and info["level_copy"] == 1
            sweep_combos(H, "block_gauss_seidel", ((SWEEPS[2], 1),), ("flow 0", "2^15 - 1 block rows"))
            H.smoother("block_jacobi")
            info = H.info()
            assert info == expected(case, "block_jacobi") and info["slices"] == 0
            sweep_combos(H, "block_jacobi", ((SWEEPS[0], 1),), ("2^15 - 1 block rows",))
        status_clean(case.name)
    finally:
        restore_defaults()


def test_every_kernel_form_was_selected():
    """what the per-case info assertions add up to: all twelve bgs_flow_kernel instantiations, the streamed kernel at
    every block size, both sliced block modes"""
    flow = {(c.bs, c.info()["seg"], c.info()["lpr"]) for c in CASES if c.info()["flow"]}
    assert flow == {(bs, seg, lpr) for bs in (2, 3) for seg, lpr in bc.FLOW_FORMS.values()}
    assert {c.bs for c in CASES if c.info(flow_mode=0)["level_copy"]} == {2, 3, 4, 5, 6, 7, 16}
    assert {c.bs for c in CASES if c.info(flow_mode=0, sell_levels=True)["slices"]} == {2, 3}
    assert {c.bs for c in CASES if c.info("block_jacobi")["slices"]} == {2, 3}


def test_info_needs_a_block_schedule_and_an_array():
    guard()
    case = next(c for c in CASES if c.name == "odd_short_plain")
    try:
        with switched(), hierarchy(case) as H:
            L = H.L
            few = np.full(4, -99, dtype=np.intc)
            d = H.lib.SmootherDesc()
            d.kind, d.iterations, d.blocksize, d.Dinv = KIND["block_gauss_seidel"], 1, case.bs, H.lib.dp(case.Dinv)
            call(L.amg_hier_set_coarse_smoother(H.h, C.byref(d)), "amg_hier_set_coarse_smoother")
            assert L.amg_hier_block_info(H.h, 0, 2, few.ctypes.data_as(C.c_void_p), 3) < 0          # not finalised: no schedule yet
            assert L.amg_hier_block_info(H.h, 0, 0, few.ctypes.data_as(C.c_void_p), 3) < 0          # no level smoother set
            call(L.amg_hier_finalize(H.h), "amg_hier_finalize")
            assert L.amg_hier_block_info(H.h, 0, 2, few.ctypes.data_as(C.c_void_p), 3) == 3
            want = expected(case, "block_gauss_seidel", 1)
            assert list(few[:3]) == [want[k] for k in bc.INFO_FIELDS[:3]] and few[3] == -99
            assert L.amg_hier_block_info(H.h, 0, 2, None, 3) < 0
            assert L.amg_hier_block_info(H.h, 1, 2, few.ctypes.data_as(C.c_void_p), 3) < 0
            assert L.amg_hier_block_info(None, 0, 2, few.ctypes.data_as(C.c_void_p), 3) < 0
        status_clean(case.name)
    finally:
        restore_defaults()
