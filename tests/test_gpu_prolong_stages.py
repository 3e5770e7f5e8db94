"""Symmetric strength, fit_candidates and Jacobi prolongation smoothing on the device (csrc/prolong.hip, DESIGN.md section
8m) against their host routes, which tests/test_prolong_cases_host.py pins to the plain-Python models, on every designed
case of tests/prolong_cases.py; then the solver option that sends every level through them.  Every comparison is exact
equality of arrays, dtypes and format included.

Every route gives a row -- or an aggregate -- one lane whatever its length: the 700-entry star row and the aggregate of
700 members run in the same kernels as everything else."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import prolong_cases as pc
from pyamg_amd import _lib, aggregation, smoothed_aggregation_solver
from pyamg_amd.aggregation import fit_candidates, jacobi_prolongation_smoother, symmetric_strength_of_connection
from pyamg_amd.gallery import poisson

pytestmark = pytest.mark.gpu


def _good_times(times):
    return len(times) == 3 and min(times) >= 0.0


@pytest.mark.parametrize("name", pc.strength_names())
def test_device_strength_equals_the_host_route(name):
    A, theta = pc.strength_cases()[name]
    live, times = _lib.live_buffers(), []
    dev = symmetric_strength_of_connection(A.copy(), theta, device=True, times=times)
    assert pc.same_matrix(dev, symmetric_strength_of_connection(A.copy(), theta, device=False))
    assert _good_times(times) and _lib.live_buffers() == live


def test_device_strength_of_bsr_blocks_equals_the_host_route():
    A = sps.kron(poisson((6, 6), format="csr"), np.array([[2.0, 1.0], [1.0, 2.0]])).tobsr(blocksize=(2, 2))
    for theta in (0, 0.25, 0.5):
        times = []
        dev = symmetric_strength_of_connection(A, theta, device=True, times=times)
        assert pc.same_matrix(dev, symmetric_strength_of_connection(A, theta, device=False))
        assert _good_times(times) == (theta != 0)       # theta == 0 reads the pattern only and stays on the host


@pytest.mark.parametrize("name", pc.fit_names())
def test_device_fit_candidates_equals_the_host_route(name):
    AggOp, B = pc.fit_cases()[name]
    live, times = _lib.live_buffers(), []
    T, Bc = fit_candidates(AggOp.copy(), B.copy(), device=True, times=times)
    Th, Bh = fit_candidates(AggOp.copy(), B.copy(), device=False)
    assert pc.same_matrix(T, Th)
    assert Bc.dtype == Bh.dtype and Bc.shape == Bh.shape and np.array_equal(Bc, Bh)
    assert np.array_equal(np.signbit(T.data), np.signbit(Th.data))
    assert _good_times(times) and _lib.live_buffers() == live


@pytest.mark.parametrize("name", pc.jacobi_names())
def test_device_jacobi_equals_the_host_route(name):
    c = pc.jacobi_cases()[name]

    def run(device, times=None):
        np.random.seed(7)
        S = c["S"].copy()
        P = jacobi_prolongation_smoother(S, c["T"].copy(), None, None, omega=c["omega"], degree=c["degree"],
                                         weighting=c["weighting"], device=device, times=times)
        return P, S, np.random.rand()
    live, times = _lib.live_buffers(), []
    dev, host = run(True, times), run(False)
    assert pc.same_matrix(dev[0], host[0]) and dev[0].format == c["T"].format
    assert pc.same_matrix(dev[1], host[1]) and dev[2] == host[2]        # the same sort of S, the same draws
    assert (_good_times(times) if c["degree"] else times == []) and _lib.live_buffers() == live


# The degenerate sizes: no rows, no stored entries, one row.  An upload of no bytes, an allocation of no size and the
# branches that launch nothing must give what the host route gives.
@pytest.mark.parametrize("name", pc.degenerate_strength_names())
def test_device_strength_equals_the_host_route_on_degenerate_sizes(name):
    A, theta = pc.degenerate_strength_cases()[name]
    live, times = _lib.live_buffers(), []
    dev = symmetric_strength_of_connection(A.copy(), theta, device=True, times=times)
    assert pc.same_matrix(dev, symmetric_strength_of_connection(A.copy(), theta, device=False))
    assert _good_times(times) and _lib.live_buffers() == live


@pytest.mark.parametrize("name", pc.degenerate_fit_names())
def test_device_fit_candidates_equals_the_host_route_on_degenerate_sizes(name):
    AggOp, B = pc.degenerate_fit_cases()[name]
    live, times = _lib.live_buffers(), []
    T, Bc = fit_candidates(AggOp.copy(), B.copy(), device=True, times=times)
    Th, Bh = fit_candidates(AggOp.copy(), B.copy(), device=False)
    assert pc.same_matrix(T, Th)
    assert Bc.dtype == Bh.dtype and Bc.shape == Bh.shape and np.array_equal(Bc, Bh)
    assert _good_times(times) and _lib.live_buffers() == live


@pytest.mark.parametrize("name", pc.degenerate_jacobi_names())
def test_device_jacobi_equals_the_host_route_on_degenerate_sizes(name):
    c = pc.degenerate_jacobi_cases()[name]

    def run(device, times=None):
        S = c["S"].copy()
        P = jacobi_prolongation_smoother(S, c["T"].copy(), None, None, omega=c["omega"], degree=c["degree"],
                                         weighting=c["weighting"], device=device, times=times)
        return P, S
    live, times = _lib.live_buffers(), []
    dev, host = run(True, times), run(False)
    assert pc.same_matrix(dev[0], host[0]) and pc.same_matrix(dev[1], host[1])
    assert _good_times(times) and _lib.live_buffers() == live


def test_failed_and_refused_calls_leave_no_buffers():
    L, live = _lib.lib(), _lib.live_buffers()
    A, theta = pc.strength_cases()["designed_theta_0.25"]
    AggOp, B = pc.fit_cases()["random_2x3"]
    c = pc.jacobi_cases()[pc.find_jacobi_case("poisson_12x12", degree=1)]
    S, T = sps.csr_matrix(c["S"]), c["T"]
    n = A.shape[0]
    handle, out = C.c_void_p(), np.empty(n + 1, dtype=np.intc)
    outside = A.indices.copy()
    outside[5] = n
    assert L.amg_symmetric_strength_device(n, A.indptr.ctypes.data, outside.ctypes.data, A.data.ctypes.data, 0.25, out.ctypes.data,
                                           C.byref(handle), None) == _lib.AMG_EINVAL and not handle.value
    assert L.amg_symmetric_strength_device(n, A.indptr.ctypes.data, A.indices.ctypes.data, A.data.ctypes.data, -1.0, out.ctypes.data,
                                           C.byref(handle), None) == _lib.AMG_EINVAL and not handle.value
    two = np.array([0, 2, 2], dtype=np.intc), np.array([0, 1], dtype=np.intc)
    Tx, R = np.empty(2), np.empty(2)
    assert L.amg_fit_candidates_device(2, 2, 1, 1, two[0].ctypes.data, two[1].ctypes.data, np.ones(2).ctypes.data, 1e-10, Tx.ctypes.data,
                                       R.ctypes.data, None) == _lib.AMG_EINVAL
    twice = np.zeros(len(T.indices), dtype=np.intc), np.arange(0, 2 * (T.shape[0] // 2) + 1, 2, dtype=np.intc)
    half = T.shape[0] // 2
    m = S[:half, :half].tocsr()
    out = np.empty(half + 1, dtype=np.intc)
    assert L.amg_jacobi_prolongation_device(half, T.shape[1], m.indptr.ctypes.data, m.indices.ctypes.data, m.data.ctypes.data,
                                            np.ones(half).ctypes.data, 1.0, 1, twice[1].ctypes.data, twice[0].ctypes.data,
                                            np.ones(2 * half).ctypes.data, out.ctypes.data, C.byref(handle),
                                            None) == _lib.AMG_EINVAL and not handle.value
    bad = A.copy()
    bad.data[17] = np.nan
    with pytest.raises(NotImplementedError):
        symmetric_strength_of_connection(bad, theta, device=True)
    with pytest.raises(NotImplementedError):
        fit_candidates(AggOp, np.where(B == B[5, 1], np.inf, B), device=True)
    with pytest.raises(NotImplementedError):
        jacobi_prolongation_smoother(c["S"].copy(), T, None, None, filter=True, device=True)
    assert _lib.live_buffers() == live


def test_device_auto_takes_the_device_route_and_answers_refusals_on_the_host(monkeypatch):
    A, theta = pc.strength_cases()["designed_theta_0.25"]
    AggOp, B = pc.fit_cases()["random_2x3"]
    c = pc.jacobi_cases()[pc.find_jacobi_case("poisson_12x12", degree=1)]
    kw = dict(omega=c["omega"], degree=c["degree"], weighting=c["weighting"])
    wide = np.ones((c["S"].shape[0], 2))                # two candidates: outside the device route of the smoothing

    def smoothed(B=None, **more):
        np.random.seed(7)
        return jacobi_prolongation_smoother(c["S"].copy(), c["T"].copy(), None, B, **kw, **more)
    bad = A.copy()
    bad.data[17] = np.nan
    bad_B = np.where(B == B[5, 1], np.inf, B)
    with np.errstate(invalid="ignore"):
        host = (symmetric_strength_of_connection(A.copy(), theta), fit_candidates(AggOp, B), smoothed(),
                symmetric_strength_of_connection(bad.copy(), theta), fit_candidates(AggOp, bad_B), smoothed(wide))
    flags = ("SYMMETRIC_STRENGTH_DEVICE_AUTO", "FIT_CANDIDATES_DEVICE_AUTO", "JACOBI_DEVICE_AUTO")
    assert [getattr(aggregation, flag) for flag in flags] == [False] * 3
    times = []
    symmetric_strength_of_connection(A.copy(), theta, times=times)
    fit_candidates(AggOp, B, times=times)
    smoothed(times=times)
    assert times == []                                  # device=None is the host route while the flags are False
    for flag in flags:
        monkeypatch.setattr(aggregation, flag, True)
    t1, t2, t3 = [], [], []
    assert pc.same_matrix(symmetric_strength_of_connection(A.copy(), theta, times=t1), host[0]) and _good_times(t1)
    got = fit_candidates(AggOp, B, times=t2)
    assert pc.same_matrix(got[0], host[1][0]) and np.array_equal(got[1], host[1][1]) and _good_times(t2)
    assert pc.same_matrix(smoothed(times=t3), host[2]) and _good_times(t3)
    t1, t2, t3 = [], [], []
    with np.errstate(invalid="ignore"):
        assert pc.same_matrix(symmetric_strength_of_connection(bad.copy(), theta, times=t1), host[3])
        got = fit_candidates(AggOp, bad_B, times=t2)
    assert np.array_equal(got[0].data, host[4][0].data, equal_nan=True) and np.array_equal(got[1], host[4][1], equal_nan=True)
    assert pc.same_matrix(smoothed(wide, times=t3), host[5])
    assert t1 == t2 == t3 == []                         # refused: answered by the host route, silently


@pytest.mark.parametrize("aggregate", ["standard", "mis"])
@pytest.mark.parametrize("grid", [(30, 30), (12, 12, 12)], ids=["poisson_30x30", "poisson_12x12x12"])
def test_solver_on_the_device_stages_equals_the_host_hierarchy(grid, aggregate):
    A = poisson(grid, format="csr")
    b = np.random.RandomState(2).rand(A.shape[0])

    def build(**kw):
        np.random.seed(5)
        ml = smoothed_aggregation_solver(A.copy(), aggregate=aggregate, max_coarse=20, **kw)
        res = []
        ml.solve(b, tol=1e-10, residuals=res)
        return ml, res
    (dev, res_d), (host, res_h) = build(device=True), build(device=False, fast=False)
    assert len(dev.levels) == len(host.levels) > 2
    for ld, lh in zip(dev.levels, host.levels):
        for what in ("A", "P", "R"):
            assert hasattr(ld, what) == hasattr(lh, what)
            if hasattr(ld, what):
                assert pc.same_matrix(getattr(ld, what), getattr(lh, what)), what
        assert ld.B.dtype == lh.B.dtype and np.array_equal(ld.B, lh.B)
    assert res_d == res_h and len(res_d) > 2
