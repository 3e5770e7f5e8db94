"""Every apply mode of every operator kernel form through the device-pointer API (amg_mat_apply, amg_mat_apply_rows),
on the irregular, multi-tile, empty, rectangular, coded and structured operators of tests/operator_cases.py, bit for
bit against the sequential oracle (cpu_backend.OracleBackend, pinned to a plain Python restatement by
tests/test_operator_cases_host.py).

Forms: csr_stream_kernel<MODE, 1> (default), csr_stream_kernel<MODE, 0> (amg_set_stream_variant(0)),
csr_stream_pipe_kernel (amg_set_stream_pipe(1)), the 16-bit column codes (amg_set_index16), csr_pattern_kernel,
stencil_kernel and stencil2_kernel.  Every output is pre-filled with a sentinel and ends with a NaN guard; x carries
a NaN at every column no entry references.  One process; every switch is put back to its default."""
import contextlib

import numpy as np
import pytest

import operator_cases as oc
from operator_cases import ALL_MODES, POLY_FIRST, SENTINEL, bit_mismatches

pytestmark = pytest.mark.gpu

DEFAULTS = (("stream_variant", 1), ("stream_pipe", 0), ("index16", 0), ("tile_target", 2048), ("xcd_chunk", 32),
            ("xcd_period", 1), ("stencil_form", 1), ("stencil_pairs", 1))
STREAM_FORMS = (("default", {}), ("scalar_loads", {"stream_variant": 0}), ("pipe", {"stream_pipe": 1}))


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
        for name, value in kw.items():
            getattr(L, "amg_set_" + name)(value)
        yield L
    finally:
        restore_defaults()


@contextlib.contextmanager
def device_backend():
    from pyamg_amd.distributed import HipBackend
    be = HipBackend(0)
    try:
        yield be
    finally:
        be.synchronize()
        be.close()


_ORACLE = {}


def oracle_result(case, mode, gscale, in_place, rows=None):
    """the model's arrays for one application, computed once per module"""
    key = (case.name, mode, gscale, in_place, rows)
    if key not in _ORACLE:
        if "be" not in _ORACLE:
            from cpu_backend import OracleBackend
            _ORACLE["be"] = OracleBackend()
        be = _ORACLE["be"]
        mkey = ("mat", id(case.csr[2]))
        if mkey not in _ORACLE:
            _ORACLE[mkey] = be.mat(*case.csr)
        _ORACLE[key] = oc.run_mode(be, _ORACLE[mkey], case, mode, gscale, in_place, rows)
    return _ORACLE[key]


def check(be, hm, case, mode, gscale, in_place, rows, what):
    """one launch against the model: the written rows, the sentinel everywhere else, the guards, the inputs"""
    got = oc.run_mode(be, hm, case, mode, gscale, in_place, rows)
    want = oracle_result(case, mode, gscale, in_place, rows)
    lo, hi = (0, case.n) if rows is None else rows
    tag = (case.name, "mode %d" % mode, "gscale %g" % gscale, "in place" if in_place else "", rows) + tuple(what)
    assert oc.check_untouched(case, got, mode, in_place, rows) == [], tag
    bad = bit_mismatches(got["out"][lo:hi], want["out"][lo:hi])
    assert bad == 0, tag + ("%d of %d rows differ from the oracle" % (bad, hi - lo),)
    assert not np.any(got["out"][lo:hi] == SENTINEL), tag + ("a row was never written",)
    if mode == POLY_FIRST:
        assert bit_mismatches(got["out2"][lo:hi], want["out2"][lo:hi]) == 0, tag + ("out2",)


def check_all_modes(be, hm, case, what, one_variant=False, ranges=True):
    for mode in case.modes:
        vs = oc.variants(mode)
        for label, gscale, in_place in (vs[-1:] if one_variant else vs):
            check(be, hm, case, mode, gscale, in_place, None, what)
        if ranges:
            label, gscale, in_place = vs[-1]
            for rows in case.row_ranges():
                check(be, hm, case, mode, gscale, in_place, rows, what)


def create(be, L, case):
    """the operator on the device, created under the case's tile target; the library's row blocking is the case's"""
    L.amg_set_tile_target(case.tile_target)
    try:
        hm = be.mat(*case.csr)
    finally:
        L.amg_set_tile_target(2048)
    assert L.amg_mat_rows_per_block(hm) == case.rpb, case.name
    return hm


# ------------------------------------------------------------------------------------------------ irregular rows
@pytest.mark.parametrize("form", STREAM_FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("case", oc.irregular_cases(), ids=repr)
def test_irregular_rows(case, form):
    """short / medium / skewed / long / empty / rectangular families: every mode (plain, gscale 0.375, POLY_LAST in
    place, Jacobi on the gathered iterate) and the row ranges, in each stream form"""
    with device_backend() as be, switched(**form[1]) as L:
        hm = create(be, L, case)
        assert L.amg_mat_form(hm) == 0
        check_all_modes(be, hm, case, (form[0],))


@pytest.mark.parametrize("form", STREAM_FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("case", oc.many_blocks_cases(), ids=repr)
def test_many_blocks(case, form):
    """3003 rows under rows-per-workgroup 1 (more row blocks than the persistent grid: a workgroup of the pipe kernel
    walks several), 2, 32 and 256"""
    with device_backend() as be, switched(**form[1]) as L:
        hm = create(be, L, case)
        assert L.amg_mat_form(hm) == 0
        check_all_modes(be, hm, case, (form[0],))


@pytest.mark.parametrize("pipe", (0, 1), ids=("plain", "pipe"))
@pytest.mark.parametrize("chunk", (0, 5, 32))
def test_xcd_block_map_writes_every_row_once(chunk, pipe):
    """3003 and 1502 row blocks under amg_set_xcd_chunk: a block the map skips keeps the sentinel, a block it visits
    twice shows in MATVEC_ACC (accumulated twice) -- either fails the comparison"""
    with device_backend() as be, switched(xcd_chunk=chunk, stream_pipe=pipe) as L:
        for case in oc.many_blocks_cases()[:2]:
            hm = create(be, L, case)
            check_all_modes(be, hm, case, ("chunk %d" % chunk, "pipe %d" % pipe), one_variant=True)


# ------------------------------------------------------------------------------------------------ 16-bit column codes
def test_coded_columns():
    """the smallest matrix the 16-bit column coding accepts, half of its row blocks coded: all modes with the switch on
    and off after creation, in every stream form, and row ranges that start on / off a coded block boundary"""
    case = oc.coded_case()
    flags = oc.coded_block_flags(case)
    coded_entries = sum(case.block_entries(k) for k in range(case.blocks()) if flags[k])
    with device_backend() as be, switched(index16=1) as L:
        hm = create(be, L, case)
        assert L.amg_mat_form(hm) == 0
        assert abs(L.amg_mat_index16_fraction(hm) - coded_entries / float(case.nnz)) < 1e-12
        assert flags[2] and not flags[3]
        ranges = case.row_ranges() + [(2 * case.rpb, 5 * case.rpb + 17), (2 * case.rpb + 1, 5 * case.rpb + 17)]
        for on in (1, 0):
            L.amg_set_index16(on)
            for name, sw in STREAM_FORMS:
                for k, v in sw.items():
                    getattr(L, "amg_set_" + k)(v)
                what = ("index16 %d" % on, name)
                check_all_modes(be, hm, case, what, one_variant=(name != "default"), ranges=False)
                for mode in ALL_MODES:
                    label, gscale, in_place = oc.variants(mode)[-1]
                    for rows in (ranges if name == "default" else ranges[-2:]):
                        check(be, hm, case, mode, gscale, in_place, rows, what)
                L.amg_set_stream_variant(1)
                L.amg_set_stream_pipe(0)
    # without the switch at creation no codes are kept
    with device_backend() as be:
        hm = create(be, _lib(), oc.irregular_cases()[0])
        assert _lib().amg_mat_index16_fraction(hm) == 0.0


# ------------------------------------------------------------------------------------------------ structured grids
@pytest.mark.parametrize("case", oc.structured_cases(), ids=repr)
def test_structured_forms(case):
    """27-point, 7-point and 1-D 5-point grid operators with dropped entries, planted zero diagonals and an optional
    [owned | halo] extension, through the stencil kernels (one and two rows per lane), the offset-pattern kernel and
    -- POLY_FIRST, which neither supports -- the stream kernel.  stencil_pairs 2 forces the two-rows-per-lane kernel,
    which the default (1) takes only from 30 M rows up.  The 27-point operator stays in the offset-pattern form
    whatever the stencil switch says (operator_cases.structured_cases); the 7-point and 5-point ones take the stencil
    form.  The plane-periodic block map behind amg_set_xcd_period needs 64 row blocks per grid plane and does not
    engage at these sizes: both settings must simply give the same bits."""
    with device_backend() as be, switched() as L:
        hm = create(be, L, case)
        assert L.amg_mat_form(hm) == case.form
        L.amg_set_stencil_form(0)
        assert L.amg_mat_form(hm) == 1
        L.amg_set_stencil_form(1)
        n = case.n
        odd = [(1, n), (257, n - 1), (255, 513), (n - 3, n)]          # starts at odd rows, inside and at the end of a block
        first = True
        for stencil in (1, 0):
            for pairs in (1, 0, 2):
                if stencil == 0 and pairs == 2:
                    continue
                for period in (1, 0):
                    L.amg_set_stencil_form(stencil)
                    L.amg_set_stencil_pairs(pairs)
                    L.amg_set_xcd_period(period)
                    what = ("stencil %d" % stencil, "pairs %d" % pairs, "period %d" % period)
                    check_all_modes(be, hm, case, what, one_variant=not first, ranges=False)
                    if period == 1:
                        for mode in case.modes:
                            label, gscale, in_place = oc.variants(mode)[-1]
                            for rows in case.row_ranges() + odd:
                                check(be, hm, case, mode, gscale, in_place, rows, what)
                    first = False


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_are_refused():
    """mode -1 and 8, row_lo > row_hi and row_hi > nrows: an error code, and nothing written"""
    case = [c for c in oc.irregular_cases() if c.name == "medium"][0]
    with device_backend() as be, switched() as L:
        hm = create(be, L, case)

        def full(mode_sent):
            def call(hm_, mode, a):
                return L.amg_mat_apply(hm_, mode_sent, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(),
                                       a[4].data_ptr(), float(a[5]), float(a[6]), be.stream())
            return call

        def rows(mode_sent, lo, hi):
            def call(hm_, mode, a):
                return L.amg_mat_apply_rows(hm_, mode_sent, lo, hi, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(),
                                            a[3].data_ptr(), a[4].data_ptr(), float(a[5]), float(a[6]), be.stream())
            return call

        n = case.n
        for call in (full(-1), full(8), rows(-1, 0, n), rows(8, 0, n), rows(0, 5, 4), rows(0, 0, n + 1), rows(0, -1, n),
                     rows(0, n + 1, n + 2)):
            # operands laid out as for POLY_FIRST (both outputs pre-filled); an empty range: nothing may change
            got = oc.run_mode(be, hm, case, POLY_FIRST, call=call)
            assert got["rc"] != 0
            assert oc.check_untouched(case, got, POLY_FIRST, rows=(0, 0)) == []
        assert L.amg_last_error()
        # the handle still works
        check(be, hm, case, 0, 1.0, False, None, ("after the refused calls",))
