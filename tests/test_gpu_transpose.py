"""GPU: the device transpose (csrc/transpose.hip) -- the flat entry amg_csr_transpose_device and
classical.transpose(device=True) against scipy's P.T.tocsr() on every designed operand of transpose_cases and on the
prolongators of real hierarchies, each with the form its rows of R took; the argument errors of the C entry; and the
device allocations, which every call leaves where they were.  Everything is compared on the raw bytes."""
import ctypes as C

import numpy as np
import pytest

import classical_io as cio
import transpose_cases as tc
from pyamg_amd import _lib, classical

pytestmark = pytest.mark.gpu

POISON_I = -77


def flat(P, fetch=True):
    """amg_csr_transpose_device on P's arrays -> (rc, Rp, Rj, Rx)"""
    n_row, n_col = P.shape
    Pp, Pj, Px = (np.ascontiguousarray(a, dtype=t) for a, t in ((P.indptr, np.intc), (P.indices, np.intc), (P.data, np.float64)))
    Rp = np.full(n_col + 1, POISON_I, dtype=np.intc)
    handle = C.c_void_p()
    rc = _lib.lib().amg_csr_transpose_device(n_row, n_col, Pp.ctypes.data, Pj.ctypes.data, Px.ctypes.data, Rp.ctypes.data,
                                             C.byref(handle))
    if rc != 0:
        assert not handle.value
        return rc, Rp, None, None
    assert handle.value
    if not fetch:
        assert _lib.lib().amg_csr_transpose_fetch(handle, None, None) == (_lib.AMG_EINVAL if Rp[-1] else 0)
        return rc, Rp, None, None
    Rj, Rx = np.full(Rp[-1], POISON_I, dtype=np.intc), np.full(Rp[-1], np.nan)
    assert _lib.lib().amg_csr_transpose_fetch(handle, Rj.ctypes.data, Rx.ctypes.data) == 0
    return rc, Rp, Rj, Rx


def check_against_scipy(P, forms=None):
    want = P.T.tocsr()
    before = _lib.live_buffers()
    rc, Rp, Rj, Rx = flat(P)
    route = _lib.transpose_last_route()
    assert rc == 0 and _lib.live_buffers() == before
    assert cio.same_bits(Rp, want.indptr.astype(np.intc)) and cio.same_bits(Rj, want.indices.astype(np.intc))
    assert cio.same_bits(Rx, want.data)
    if P.nnz == 0:
        assert route == dict(launched=0, lane_rows=0, lds_rows=0, hbm_rows=0)
    else:
        assert (route["launched"], (route["lane_rows"], route["lds_rows"], route["hbm_rows"])) == (1, tc.forms_of(P))
    if forms is not None:
        assert {f for f in ("lane", "lds", "hbm") if route[f + "_rows"] > 0} == forms
    R = classical.transpose(P, device=True)
    assert _lib.live_buffers() == before
    assert R.shape == want.shape and R.dtype == want.dtype and R.indices.dtype == want.indices.dtype
    assert R.indptr.dtype == want.indptr.dtype and cio.same_csr(R, want)
    assert R.has_sorted_indices == want.has_sorted_indices
    return Rp, Rj, Rx


@pytest.mark.parametrize("name", sorted(tc.cases()))
def test_designed_case_equals_scipy_and_takes_its_form(name):
    P, forms = tc.cases()[name]
    check_against_scipy(P, forms)


def test_interleaved_columns_twice_give_identical_bytes():
    P, _ = tc.cases()["interleaved"]
    first, second = flat(P), flat(P)
    for a, b in zip(first[1:], second[1:]):
        assert cio.same_bits(a, b)


@pytest.mark.parametrize("name", ["poisson_pmis", "poisson_pmis_ext"])
def test_prolongators_of_real_hierarchies(name):
    ml = tc.host_hierarchy(name)
    assert len(ml.levels) == len(tc.HIERARCHIES[name][2])
    for lvl in ml.levels[:-1]:
        Rp, Rj, Rx = check_against_scipy(lvl.P)
        assert cio.same_bits(Rj, lvl.R.indices.astype(np.intc)) and cio.same_bits(Rx, lvl.R.data)


def test_bad_arrays_are_refused_before_any_launch():
    P, _ = tc.cases()["shuffled"]
    before = _lib.live_buffers()

    def edited(what, at, value):
        Q = P.copy()
        getattr(Q, what)[at] = value
        return Q

    for Q, what in ((edited("indptr", 2, P.indptr[1] - 1), "decrease"), (edited("indices", 3, P.shape[1]), "outside"),
                    (edited("indices", 3, -1), "outside"), (edited("indptr", 0, 1), "do not start at 0")):
        rc, Rp, _, _ = flat(Q)
        assert rc == _lib.AMG_EINVAL and np.all(Rp == POISON_I), what
        with pytest.raises(ValueError, match=what):
            _lib.check(rc)
        assert _lib.live_buffers() == before
    handle = C.c_void_p()
    assert _lib.lib().amg_csr_transpose_device(1, 1, None, None, None, None, C.byref(handle)) == _lib.AMG_EINVAL
    assert _lib.lib().amg_csr_transpose_fetch(None, None, None) == _lib.AMG_EINVAL
    assert _lib.live_buffers() == before


def test_unfetched_handles_are_released():
    before = _lib.live_buffers()
    for name in ("shuffled", "no_entries", "hub_%d_last" % (tc.LDS_MAX + 1)):
        rc, Rp, _, _ = flat(tc.cases()[name][0], fetch=False)
        assert rc == 0 and _lib.live_buffers() == before


def test_python_route_refuses_what_the_entry_does_not_take():
    P, _ = tc.cases()["shuffled"]
    with pytest.raises(NotImplementedError, match="float64"):
        classical.transpose(P.astype(np.float32), device=True)
    with pytest.raises(TypeError):
        classical.transpose(P.tocsc(), device=True)
