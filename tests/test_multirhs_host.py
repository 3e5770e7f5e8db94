"""solve_many without a GPU: the amg_hierm_* symbols and their bindings, the validation errors and the refusals
(all of which happen before any device work), the preconditioner's fall-back to the column loop, and the grouping
of k right-hand sides into layouts of 1, 2, 4 and 8 columns."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pyamg_amd", "lib", "libamgcore_hip.so")
SYMBOLS = ["amg_hierm_create", "amg_hierm_destroy", "amg_hierm_set_matrix", "amg_hierm_set_smoother",
           "amg_hierm_set_coarse_dense", "amg_hierm_set_coarse_smoother", "amg_hierm_finalize", "amg_hierm_solve",
           "amg_hierm_cycle", "amg_hierm_device_bytes", "amg_hierm_last_solve_ms"]
N = 64


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(LIB)
    for s in SYMBOLS:
        assert hasattr(raw, s), s
    from pyamg_amd import _lib
    L = _lib.lib()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes is not None, "%s has no argtypes" % s
    assert L.amg_hierm_device_bytes.restype is ctypes.c_long
    assert L.amg_hierm_last_solve_ms.restype is ctypes.c_double
    assert len(L.amg_hierm_solve.argtypes) == 10
    assert len(L.amg_hierm_create.argtypes) == 4


def _ml(A=None, smoother="gauss_seidel", coarse="pinv", P=None):
    """a small float64 two-level hierarchy built on the host (nothing touches a device)"""
    import pyamg_amd
    if A is None:
        A = sps.diags([-np.ones(N - 1), 2 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1], format="csr")
    if P is None:
        P = sps.csr_matrix(np.kron(np.eye(A.shape[0] // 2), np.ones((2, 1))))
    l0, l1 = pyamg_amd.multilevel_solver.level(), pyamg_amd.multilevel_solver.level()
    l0.A, l0.P, l0.R = A, P, P.T.asformat(P.format)
    l1.A = sps.csr_matrix(P.T @ A @ P)
    ml = pyamg_amd.multilevel_solver([l0, l1], coarse_solver=coarse)
    pyamg_amd.change_smoothers(ml, smoother, smoother)
    return ml


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to build a device mirror fails the test"""
    from pyamg_amd import multilevel

    def boom(*a, **k):
        raise AssertionError("device work started")
    monkeypatch.setattr(multilevel._DeviceHierarchyC128, "__init__", boom)
    monkeypatch.setattr(multilevel._DeviceHierarchy, "__init__", boom)
    monkeypatch.setattr(multilevel._DeviceHierarchyMulti, "__init__", boom)


B8 = np.ones((N, 8))


# ---------------------------------------------------------------------------------------------- validation
@pytest.mark.parametrize("B, X0", [
    (np.ones((N + 1, 2)), None),                 # wrong first dimension
    (np.ones(N), None),                          # one vector is solve()'s business
    (np.ones((N, 2, 1)), None),
    (np.ones((N, 2)), np.zeros((N, 3))),         # X0 of another shape
    (np.ones((N, 2)), np.zeros(N)),
    (np.ones((N, 0)), None),                     # no column
])
def test_validation_errors(no_device, B, X0):
    with pytest.raises(ValueError):
        _ml().solve_many(B, X0=X0)


def test_unknown_cycle_is_a_type_error(no_device):
    with pytest.raises(TypeError):
        _ml().solve_many(B8, cycle="Q")


def test_solve_still_refuses_two_columns(no_device):
    with pytest.raises(ValueError):
        _ml().solve(np.ones((N, 2)))


# ---------------------------------------------------------------------------------------------- refusals
def test_refuses_amli(no_device):
    with pytest.raises(NotImplementedError):
        _ml().solve_many(B8, cycle="AMLI")


def test_refuses_accel(no_device):
    with pytest.raises(NotImplementedError):
        _ml().solve_many(B8, accel="cg")


def test_refuses_complex_hierarchy(no_device):
    A = sps.diags([-np.ones(N - 1), (2 + 0.5j) * np.ones(N), -np.ones(N - 1)], [-1, 0, 1], format="csr",
                  dtype=np.complex128)
    with pytest.raises(NotImplementedError):
        _ml(A=A).solve_many(B8)


def test_refuses_complex_right_hand_sides(no_device):
    with pytest.raises(NotImplementedError):
        _ml().solve_many(B8.astype(np.complex128))


@pytest.mark.parametrize("which", ["A", "P"])
def test_refuses_bsr_blocks(no_device, which):
    A = sps.diags([-np.ones(N - 1), 2 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1], format="csr")
    P = sps.csr_matrix(np.kron(np.eye(N // 2), np.ones((2, 1))))
    if which == "A":
        ml = _ml(A=A.tobsr(blocksize=(2, 2)))
    else:
        ml = _ml(A=A, P=P.tobsr(blocksize=(2, 1)))
    with pytest.raises(NotImplementedError):
        ml.solve_many(B8)


def test_accepts_bsr_1x1_up_to_the_device(monkeypatch):
    """BSR(1,1) operators pass the checks: the first thing that fails is the (patched) device construction"""
    from pyamg_amd import multilevel

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(multilevel._DeviceHierarchyMulti, "__init__", reached)
    A = sps.diags([-np.ones(N - 1), 2 * np.ones(N), -np.ones(N - 1)], [-1, 0, 1], format="csr")
    with pytest.raises(Reached):
        _ml(A=A.tobsr(blocksize=(1, 1))).solve_many(B8)


@pytest.mark.parametrize("spec", [("block_jacobi", {"blocksize": 2}), ("block_gauss_seidel", {"blocksize": 2}), ("gauss_seidel_indexed", {"indices": np.arange(N)}),
                                  "multicolor_gauss_seidel", "gauss_seidel_ne", "gauss_seidel_nr", "jacobi_ne", "schwarz",
                                  "cg", "gmres", "cgnr"])
@pytest.mark.parametrize("side", ["pre", "post"])
def test_refuses_out_of_scope_smoothers(no_device, spec, side):
    import pyamg_amd
    ml = _ml()
    pre, post = (spec, "gauss_seidel") if side == "pre" else ("gauss_seidel", spec)
    pyamg_amd.change_smoothers(ml, pre, post)
    with pytest.raises(NotImplementedError):
        ml.solve_many(B8)


@pytest.mark.parametrize("coarse", ["cg", "gmres", "bicgstab", "cgs", "minres", "schwarz", "jacobi_ne", "gauss_seidel_nr",
                                    ("block_jacobi", {"blocksize": 2}), ("block_gauss_seidel", {"blocksize": 2})])
def test_refuses_out_of_scope_coarse_solvers(no_device, coarse):
    with pytest.raises(NotImplementedError):
        _ml(coarse=coarse).solve_many(B8)


def test_refuses_callable_coarse_solver(no_device):
    with pytest.raises(NotImplementedError):
        _ml(coarse=lambda A, b: np.zeros_like(b)).solve_many(B8)


def test_refuses_device_tensors(no_device):
    class FakeTensor(object):
        is_cuda = True

        def data_ptr(self):
            return 0
    with pytest.raises(NotImplementedError):
        _ml().solve_many(FakeTensor())
    with pytest.raises(NotImplementedError):
        _ml().solve_many(B8, X0=FakeTensor())


def test_refuses_partitioned_hierarchies():
    from pyamg_amd import distributed
    with pytest.raises(NotImplementedError):
        distributed.DistributedSolver.solve_many(object(), B8)


@pytest.mark.parametrize("smoother", ["jacobi", "gauss_seidel", "sor", "chebyshev", "richardson",
                                      ("polynomial", {"coefficients": [0.3, 0.2]}), None])
@pytest.mark.parametrize("coarse", ["pinv", "lu", "splu", "jacobi", "gauss_seidel", "sor", "chebyshev", None])
def test_scope_passes_the_checks(smoother, coarse):
    """everything section 5 of the contract takes gets through the refusals (no device needed for that)"""
    from pyamg_amd import multilevel
    ml = _ml(smoother=smoother, coarse=coarse)
    kind, _ = multilevel._DeviceHierarchyMulti.check_levels(ml)
    assert kind in ("dense", "smoother", "none")
    assert ml._check_many("w") == "W"


# ---------------------------------------------------------------------------------------------- preconditioner
def test_matmat_of_a_refused_hierarchy_loops_over_columns(no_device, monkeypatch):
    ml = _ml(smoother=("block_gauss_seidel", {"blocksize": 2}))
    calls = []

    def stub(b, **kw):
        calls.append((np.array(b), kw))
        return 2.0 * np.asarray(b)
    monkeypatch.setattr(ml, "solve", stub)
    M = ml.aspreconditioner(cycle="W")
    X = np.arange(N * 3, dtype=np.float64).reshape(N, 3)
    Y = M.matmat(X)
    assert Y.shape == (N, 3) and np.array_equal(Y, 2.0 * X)
    assert len(calls) == 3
    for j, (b, kw) in enumerate(calls):
        assert np.array_equal(np.ravel(b), X[:, j])
        assert kw == {"maxiter": 1, "cycle": "W", "tol": 1e-12}
    # matvec and M * b are what they were
    assert np.array_equal(M.matvec(X[:, 0]), 2.0 * X[:, 0])
    assert np.array_equal(M * X[:, 1], 2.0 * X[:, 1])


def test_matmat_of_a_taken_hierarchy_is_one_solve_many(monkeypatch):
    ml = _ml()
    calls = []

    def stub(B, **kw):
        calls.append((np.array(B), kw))
        return 3.0 * np.asarray(B)
    monkeypatch.setattr(ml, "solve_many", stub)
    M = ml.aspreconditioner(batched=True)
    X = np.arange(N * 5, dtype=np.float64).reshape(N, 5)
    assert np.array_equal(M.matmat(X), 3.0 * X)
    assert len(calls) == 1 and calls[0][1] == {"maxiter": 1, "cycle": "V", "tol": 1e-12}


def test_matmat_default_follows_the_measured_crossover(no_device, monkeypatch):
    """batched=None: the batched cycle only where it was measured faster than the column loop"""
    from pyamg_amd import multilevel
    pays = multilevel._batched_cycle_pays
    small = _ml(smoother="jacobi")                       # 64 unknowns, no Gauss-Seidel sweeps
    assert [pays(small, k) for k in (1, 2, 3, 4, 5, 8, 11)] == [False, False, True, True, True, True, True]
    assert not any(pays(_ml(smoother=sm), k) for sm in ("gauss_seidel", "sor") for k in (4, 8))

    class Big(object):                                    # the gate reads the level-0 size and the descriptors only
        def __init__(self, n):
            lvl = type("L", (), {})()
            lvl.A = sps.csr_matrix((n, n))
            self.levels = [lvl, lvl]
    assert [pays(Big(32768), k) for k in (3, 4, 5, 8)] == [False, False, True, True]
    assert [pays(Big(1000000), k) for k in (4, 5, 6, 7, 8)] == [False, False, False, True, True]
    assert not any(pays(Big(4096000), k) for k in range(1, 9))       # 1.06 at 8 columns: inside the margin
    assert not any(pays(Big(125000000), k) for k in range(1, 9))
    # and matmat obeys it: two columns of the small hierarchy go through solve, four through solve_many
    seen = []
    monkeypatch.setattr(small, "solve", lambda b, **kw: seen.append("solve") or np.asarray(b))
    monkeypatch.setattr(small, "solve_many", lambda B, **kw: seen.append("many") or np.asarray(B))
    M = small.aspreconditioner()
    M.matmat(np.ones((N, 2)))
    M.matmat(np.ones((N, 4)))
    assert seen == ["solve", "solve", "many"]
    seen[:] = []
    small.aspreconditioner(batched=False).matmat(np.ones((N, 4)))
    assert seen == ["solve"] * 4


# ---------------------------------------------------------------------------------------------- mirror lifetime
def test_change_smoothers_drops_the_mirror():
    import pyamg_amd

    class Mirror(object):
        closed = False

        def close(self):
            self.closed = True
    ml = _ml()
    m = Mirror()
    ml._devm = m
    pyamg_amd.change_smoothers(ml, "jacobi", "jacobi")
    assert m.closed and ml._devm is None


# ---------------------------------------------------------------------------------------------- grouping
@pytest.mark.parametrize("k, expect", [
    (1, [(0, 1, 1)]),
    (2, [(0, 2, 2)]),
    (3, [(0, 3, 4)]),
    (5, [(0, 5, 8)]),
    (8, [(0, 8, 8)]),
    (9, [(0, 8, 8), (8, 1, 1)]),
    (17, [(0, 8, 8), (8, 8, 8), (16, 1, 1)]),
])
def test_column_groups(k, expect):
    from pyamg_amd.multilevel import _rhs_groups
    assert _rhs_groups(k) == expect
    assert sum(c for _, c, _ in _rhs_groups(k)) == k


def test_column_groups_reject_no_column():
    from pyamg_amd.multilevel import _rhs_groups
    with pytest.raises(ValueError):
        _rhs_groups(0)
