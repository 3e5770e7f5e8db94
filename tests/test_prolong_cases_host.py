"""The host routes of symmetric strength, fit_candidates and Jacobi prolongation smoothing against the plain-Python models
of tests/prolong_cases.py on every designed case, the `device` keyword on a machine without a GPU, and the refusals of
the device routes, which come before the library is touched.  Every comparison is exact equality
of arrays, dtypes and format included."""
import os

import numpy as np
import pytest
import scipy.sparse as sps

import prolong_cases as pc
from pyamg_amd import _host, aggregation, rootnode_solver, smoothed_aggregation_solver, strength
from pyamg_amd.aggregation import fit_candidates, jacobi_prolongation_smoother, symmetric_strength_of_connection
from pyamg_amd.gallery import poisson

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _touched(*a, **k):
    raise AssertionError("the library was touched")


def _untouchable(monkeypatch):
    from pyamg_amd import _lib
    monkeypatch.setattr(_lib, "lib", _touched)
    monkeypatch.setattr(_lib, "device_count", _touched)


# ------------------------------------------------------------------------------------------------------- strength
@pytest.mark.parametrize("name", pc.strength_names())
def test_strength_host_route_equals_the_model(name, monkeypatch):
    A, theta = pc.strength_cases()[name]
    Sp, Sj, Sx = pc.model_strength(A, theta)
    want = sps.csr_matrix((Sx, Sj, Sp), shape=A.shape)
    plain = symmetric_strength_of_connection(A.copy(), theta)
    assert pc.same_matrix(plain, want)
    _untouchable(monkeypatch)
    for device in (False, None):
        assert pc.same_matrix(symmetric_strength_of_connection(A.copy(), theta, device=device), plain)


def test_strength_cases_hold_what_they_are_designed_for():
    A = pc.designed_operator()
    rows = [A.indices[A.indptr[i]:A.indptr[i + 1]] for i in range(A.shape[0])]
    assert len(rows[0]) == pc.STAR and 5 not in rows[5] and list(rows[6]).count(6) == 2 and len(rows[7]) == 0
    assert not np.any(A.data[A.indptr[9]:A.indptr[10]]) and list(rows[11]).count(40) == 2
    assert any(np.any(np.diff(r) < 0) for r in rows) and np.any(A.data < 0) and np.any(A.data > 0)
    S = symmetric_strength_of_connection(A.copy(), 0.5)
    assert S.indptr[9] - S.indptr[8] == 1 and S.indptr[10] - S.indptr[9] == 3       # row 8 keeps its diagonal only
    assert np.array_equal(S.data[S.indptr[9]:S.indptr[10]], np.zeros(3))            # stored zeros: divided by 1
    P = poisson((9, 9), format="csr")
    assert symmetric_strength_of_connection(P, 0.25).nnz == P.nnz                   # exactly on the threshold: kept
    assert symmetric_strength_of_connection(P, 0.5).nnz == P.shape[0]
    assert strength.symmetric_strength_of_connection is symmetric_strength_of_connection


def test_strength_of_bsr_blocks_goes_through_the_same_route(monkeypatch):
    A = sps.kron(poisson((6, 6), format="csr"), np.array([[2.0, 1.0], [1.0, 2.0]])).tobsr(blocksize=(2, 2))
    _untouchable(monkeypatch)
    for theta in (0, 0.25):
        plain = symmetric_strength_of_connection(A, theta)
        for device in (False, None):
            assert pc.same_matrix(symmetric_strength_of_connection(A, theta, device=device), plain)
    assert pc.same_matrix(symmetric_strength_of_connection(A, 0, device=True), symmetric_strength_of_connection(A, 0))


# --------------------------------------------------------------------------------------------- tentative prolongator
@pytest.mark.parametrize("name", pc.fit_names())
def test_fit_candidates_host_route_equals_the_model(name, monkeypatch):
    AggOp, B = pc.fit_cases()[name]
    K1, K2 = B.shape[0] // AggOp.shape[0], B.shape[1]
    Tp, Tj, Tx, R = pc.model_fit(AggOp, B)
    want = sps.bsr_matrix((Tx, Tj, Tp), shape=(K1 * AggOp.shape[0], K2 * AggOp.shape[1]), blocksize=(K1, K2))
    T, Bc = fit_candidates(AggOp.copy(), B.copy())
    assert pc.same_matrix(T, want)
    assert Bc.dtype == R.dtype and Bc.shape == R.shape and np.array_equal(Bc, R)
    assert np.array_equal(T.indptr, AggOp.indptr) and np.array_equal(T.indices, AggOp.indices)
    if name.startswith("equal_columns"):
        assert not np.any(T.data[:, :, 1]) and not np.any(R.reshape(-1, K2, K2)[:, 1, 1])
        assert not np.any(R.reshape(-1, K2, K2)[3, :, 2])
    _untouchable(monkeypatch)
    for device in (False, None):
        T2, Bc2 = fit_candidates(AggOp.copy(), B.copy(), device=device)
        assert pc.same_matrix(T2, T) and np.array_equal(Bc2, Bc)


def test_the_names_are_the_cases():
    assert pc.strength_names() == list(pc.strength_cases()) and pc.fit_names() == list(pc.fit_cases())
    assert pc.jacobi_names() == list(pc.jacobi_cases())


def test_fit_cases_hold_what_they_are_designed_for():
    AggOp = pc.designed_aggregates()
    assert tuple(np.bincount(AggOp.indices, minlength=AggOp.shape[1])) == pc.SIZES
    assert np.count_nonzero(np.diff(AggOp.indptr) == 0) == 10
    B = pc.fit_cases()["random_1x1"][1]
    assert B[3, 0] == 0.0 and np.signbit(B[3, 0])


# ------------------------------------------------------------------------------------------------- Jacobi smoothing
@pytest.mark.parametrize("name", pc.jacobi_names())
def test_jacobi_host_route_equals_the_model(name, monkeypatch):
    c = pc.jacobi_cases()[name]
    np.random.seed(7)
    S = c["S"].copy()
    plain = jacobi_prolongation_smoother(S, c["T"].copy(), None, None, omega=c["omega"], degree=c["degree"], weighting=c["weighting"])
    drawn = np.random.rand()
    np.random.seed(7)
    Sm = c["S"].copy()
    dinv, w = pc.jacobi_weights(Sm, c["omega"], c["weighting"])
    assert pc.same_matrix(Sm, S)                # the same in-place sort on both sides
    want = pc.model_jacobi(Sm, c["T"], dinv, w, c["degree"])
    assert pc.same_matrix(plain, want)
    assert plain.format == c["T"].format
    _untouchable(monkeypatch)
    for device in (False, None):
        np.random.seed(7)
        got = jacobi_prolongation_smoother(c["S"].copy(), c["T"].copy(), None, None, omega=c["omega"], degree=c["degree"],
                                           weighting=c["weighting"], device=device)
        assert pc.same_matrix(got, plain) and np.random.rand() == drawn


def _steps(name):
    """what the subtractions of a case do: (routine, longest row of P, longest row of X) per step"""
    c = pc.jacobi_cases()[name]
    np.random.seed(7)
    S, steps = c["S"].copy(), []
    dinv, w = pc.jacobi_weights(S, c["omega"], c["weighting"])
    return pc.model_jacobi(S, c["T"], dinv, w, c["degree"], steps), steps


def test_jacobi_cases_hold_what_they_are_designed_for():
    S, T, T_rev = pc.designed_smoothing_operands()
    rows = lambda M, i: list(M.indices[M.indptr[i]:M.indptr[i + 1]])
    for M in (T, T_rev):
        assert M.shape[1] == 95 and all(M.indptr[i + 1] == M.indptr[i] for i in (7, 15, 16)) and M.indptr[21] - M.indptr[20] == 1
    assert rows(S, 20) == [20] and S[30, 30] == 0.0 and 30 in rows(S, 30) and len(rows(S, 0)) == pc.STAR
    assert any(np.any(np.diff(rows(S, i)) < 0) and np.any(np.diff(rows(S, i)) > 0) for i in range(S.shape[0]))
    find = pc.find_jacobi_case
    # the general order, with rows of several entries on both sides from the second step on; the star row meets 88 aggregates
    for weighting in ("diagonal", "local", "block"):
        P, steps = _steps(find("designed", degree=2, weighting=weighting))
        assert [s[0] for s in steps] == ["general", "general"] and steps[0][1:] == (1, 88)
        assert steps[1][1] > 1 and steps[1][2] > 1
        assert P.indptr[17] > P.indptr[15] and P.indptr[1] - P.indptr[0] >= 88     # empty rows of T get entries from X
    # the merge: rows of up to 88 entries of X against T's rows of one entry and against its empty rows
    for weighting in ("diagonal", "local"):
        P, steps = _steps(find("reversed", degree=1, weighting=weighting))
        assert steps == [("merge", 1, 88)] and P.indptr[17] > P.indptr[15] and P.indptr[1] - P.indptr[0] >= 88
        assert _steps(find("reversed", degree=2, weighting=weighting))[1][0][0] == "merge"
    # T - T is an exact zero and is dropped by the merge and by the general order
    for prefix, routine in (("reversed", "merge"), ("designed", "general")):
        P, steps = _steps(find(prefix, degree=1, weighting="local", omega=1.0))
        assert steps[0][0] == routine and P.indptr[21] == P.indptr[20]
        P, steps = _steps(find(prefix, degree=1, weighting="local", omega=4.0 / 3.0))
        assert steps[0][0] == routine and P.indptr[21] - P.indptr[20] == 1
    # every Poisson level takes the general order
    assert all(s[0] == "general" for name in pc.jacobi_cases() if name.startswith("poisson") for s in _steps(name)[1])
    cases = pc.jacobi_cases().values()
    assert {c["degree"] for c in cases} == {0, 1, 2, 3} and {c["weighting"] for c in cases} == {"diagonal", "local", "block"}
    assert {(c["S"].format, c["T"].format) for c in cases} == {(a, b) for a in ("csr", "bsr") for b in ("csr", "bsr")}
    for prefix in ("designed", "reversed", "poisson"):
        assert {c["T"].format for n, c in pc.jacobi_cases().items() if n.startswith(prefix)} == {"csr", "bsr"}


# ------------------------------------------------------------------------------------------------- degenerate sizes
@pytest.mark.parametrize("name", pc.degenerate_strength_names())
def test_strength_host_route_equals_the_model_on_degenerate_sizes(name):
    A, theta = pc.degenerate_strength_cases()[name]
    Sp, Sj, Sx = pc.model_strength(A, theta)
    got = symmetric_strength_of_connection(A.copy(), theta)
    assert pc.same_matrix(got, sps.csr_matrix((Sx, Sj, Sp), shape=A.shape))
    assert got.nnz == (1 if A.shape[0] == 1 else 0) and np.array_equal(got.data, np.ones(got.nnz))


@pytest.mark.parametrize("name", pc.degenerate_fit_names())
def test_fit_candidates_host_route_equals_the_model_on_degenerate_sizes(name):
    AggOp, B = pc.degenerate_fit_cases()[name]
    Tp, Tj, Tx, R = pc.model_fit(AggOp, B)
    T, Bc = fit_candidates(AggOp.copy(), B.copy())
    assert pc.same_matrix(T, sps.bsr_matrix((Tx, Tj, Tp), shape=AggOp.shape, blocksize=(1, 1)))
    assert Bc.dtype == R.dtype and Bc.shape == R.shape and np.array_equal(Bc, R)
    assert Bc[-1, 0] == 0.0 and T.nnz == AggOp.nnz      # the aggregate without members: a zero in R, no block in T


@pytest.mark.parametrize("name", pc.degenerate_jacobi_names())
def test_jacobi_host_route_equals_the_model_on_degenerate_sizes(name):
    c = pc.degenerate_jacobi_cases()[name]
    S, Sm = c["S"].copy(), c["S"].copy()
    got = jacobi_prolongation_smoother(S, c["T"].copy(), None, None, omega=c["omega"], degree=c["degree"], weighting=c["weighting"])
    dinv, w = pc.jacobi_weights(Sm, c["omega"], c["weighting"])
    assert pc.same_matrix(Sm, S) and pc.same_matrix(got, pc.model_jacobi(Sm, c["T"], dinv, w, c["degree"]))
    if name.startswith("no_entries"):
        assert pc.same_matrix(got, c["T"])              # nothing to subtract: T itself


def test_degenerate_names_are_the_cases():
    assert pc.degenerate_strength_names() == list(pc.degenerate_strength_cases())
    assert pc.degenerate_fit_names() == list(pc.degenerate_fit_cases())
    assert pc.degenerate_jacobi_names() == list(pc.degenerate_jacobi_cases())
    assert pc.degenerate_graph_names() == list(pc.degenerate_graphs())


# ------------------------------------------------------------------------------------------------------- refusals
def test_device_refusals_come_before_the_library(monkeypatch):
    A, _ = pc.strength_cases()["designed_theta_0.25"]
    AggOp, B = pc.fit_cases()["random_2x3"]
    c = pc.jacobi_cases()[pc.find_jacobi_case("poisson_12x12", S="csr", T="csr")]
    S, T = c["S"], c["T"]
    nan_A = A.copy()
    nan_A.data[17] = np.nan
    nan_B = B.copy()
    nan_B[5, 1] = np.inf
    blocks = sps.kron(S, np.eye(3)).tobsr(blocksize=(3, 3))
    want_nan = symmetric_strength_of_connection(nan_A.copy(), 0.25)
    with np.errstate(invalid="ignore"):
        want_fit = fit_candidates(AggOp, nan_B)
    _untouchable(monkeypatch)
    outside = "outside the restated setup"

    def refused(call):
        with pytest.raises(NotImplementedError, match=outside):
            call()
    refused(lambda: symmetric_strength_of_connection(A.astype(np.complex128), 0.25, device=True))
    refused(lambda: symmetric_strength_of_connection(nan_A.copy(), 0.25, device=True))
    refused(lambda: symmetric_strength_of_connection(A.astype(np.float32), 0.25, device=True))
    refused(lambda: fit_candidates(AggOp, B.astype(np.complex128), device=True))
    refused(lambda: fit_candidates(AggOp, B.astype(np.float32), device=True))
    refused(lambda: fit_candidates(AggOp, nan_B, device=True))
    wide_index = AggOp.copy()
    wide_index.indices, wide_index.indptr = AggOp.indices.astype(np.int64), AggOp.indptr.astype(np.int64)
    assert wide_index.indices.dtype == np.int64
    refused(lambda: fit_candidates(wide_index, B, device=True))
    refused(lambda: jacobi_prolongation_smoother(S.astype(np.complex128), T, None, None, device=True))
    refused(lambda: jacobi_prolongation_smoother(S, T, None, np.ones((S.shape[0], 2)), device=True))
    refused(lambda: jacobi_prolongation_smoother(blocks, sps.kron(T, np.eye(3)).tobsr(blocksize=(3, 3)), None, None, device=True))
    refused(lambda: jacobi_prolongation_smoother(S, T, None, None, filter=True, device=True))
    twice = sps.csr_matrix((np.ones(2 * T.shape[0]), np.zeros(2 * T.shape[0], dtype=np.intc),
                            np.arange(0, 2 * T.shape[0] + 1, 2, dtype=np.intc)), shape=T.shape)
    refused(lambda: jacobi_prolongation_smoother(S, twice, None, None, device=True))
    refused(lambda: smoothed_aggregation_solver(S.astype(np.complex128), device=True))
    refused(lambda: smoothed_aggregation_solver(S, B=np.ones((S.shape[0], 2)), device=True))
    refused(lambda: smoothed_aggregation_solver(blocks, device=True))
    refused(lambda: smoothed_aggregation_solver(S, smooth=("jacobi", {"filter": True}), device=True))
    with pytest.raises(AssertionError, match="the library was touched"):        # the keyword reaches rootnode_solver's strength
        rootnode_solver(S, strength=("symmetric", {"theta": 0.25, "device": True}), max_coarse=10)
    # device=None: the host route; with a stage's DEVICE_AUTO and a GPU "present" a refusal is answered by the host route
    for flag in ("SYMMETRIC_STRENGTH_DEVICE_AUTO", "FIT_CANDIDATES_DEVICE_AUTO", "JACOBI_DEVICE_AUTO"):
        assert getattr(aggregation, flag) is False
        monkeypatch.setattr(aggregation, flag, True)
    monkeypatch.setattr(_host, "device_present", lambda: True)
    assert pc.same_matrix(symmetric_strength_of_connection(nan_A.copy(), 0.25), want_nan)
    with np.errstate(invalid="ignore"):
        got = fit_candidates(AggOp, nan_B)
    assert np.array_equal(got[0].data, want_fit[0].data, equal_nan=True) and np.array_equal(got[0].indices, want_fit[0].indices)
    assert np.array_equal(got[1], want_fit[1], equal_nan=True)
    with pytest.raises(NotImplementedError, match=outside):
        jacobi_prolongation_smoother(S, T, None, None, filter=True)
    for call in (lambda: symmetric_strength_of_connection(A.copy(), 0.25), lambda: fit_candidates(AggOp, B),
                 lambda: jacobi_prolongation_smoother(S.copy(), T, None, None, weighting="local")):
        with pytest.raises(AssertionError, match="the library was touched"):        # the routes are live
            call()


# ------------------------------------------------------------------------------------------------------- the solver
def _same_hierarchy(a, b):
    if len(a.levels) != len(b.levels):
        return False
    for la, lb in zip(a.levels, b.levels):
        for what in ("A", "P", "R"):
            if hasattr(la, what) != hasattr(lb, what) or (hasattr(la, what) and not pc.same_matrix(getattr(la, what), getattr(lb, what))):
                return False
        if not np.array_equal(la.B, lb.B):
            return False
    return True


@pytest.mark.parametrize("options", [{}, {"aggregate": "mis"}, {"strength": ("symmetric", {"theta": 0.25}), "max_coarse": 20}],
                         ids=["defaults", "mis", "theta"])
def test_solver_device_option_leaves_the_host_hierarchies_alone(options, monkeypatch):
    A = poisson((30, 30), format="csr")
    options = dict({"max_coarse": 50}, **options)

    def build(**kw):
        np.random.seed(3)
        return smoothed_aggregation_solver(A.copy(), **dict(options, **kw))
    today = build()
    generic = build(fast=False)
    assert len(today.levels) > 2
    _untouchable(monkeypatch)
    assert _same_hierarchy(build(device=None), today)
    assert _same_hierarchy(build(device=False), today)
    assert _same_hierarchy(build(device=False, fast=False), generic)
    with pytest.raises(AssertionError, match="the library was touched"):        # device=True is live on every stage
        build(device=True)


def test_header_declares_the_new_entries():
    with open(os.path.join(ROOT, "include", "amgcore_hip.h")) as f:
        text = f.read()
    for name in ("amg_symmetric_strength_device", "amg_symmetric_strength_fetch", "amg_fit_candidates_device",
                 "amg_jacobi_prolongation_device", "amg_jacobi_prolongation_fetch"):
        assert ("int %s(" % name) in text, name
