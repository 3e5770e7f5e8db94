"""pyamg_amd.krylov_c128 without a device: the accelerated-solve fixtures are well formed, every refusal is raised
before the device mirror is built, the refusal of the string names is unchanged, and the numpy restatements of
tests/krylov_host_c128.py reproduce the reference's histories with the host cycle as preconditioner."""
import os

import numpy as np
import pytest
import scipy.sparse as sps
from scipy.sparse.linalg import LinearOperator

import accel_c128
import c128_cycle
import krylov_host_c128

NAMES = accel_c128.names()
EXPECTED = {
    "cheb2_magnetic3d": ["bicgstab", "cg", "fgmres", "gmres"],
    "sa_default_magnetic2d": ["cg", "gmres"],
    "gs_sym_V_shifted2d": ["bicgstab", "fgmres", "gmres"],
    "sor_W_shifted2d": ["fgmres"],
    "jacobi_F_x0_magnetic2d": ["bicgstab", "gmres"],
    "bsr_bjac_gs": ["bicgstab", "gmres"],
    "one_level": ["gmres"],
}


def test_fixture_listing():
    assert NAMES == sorted("%s__%s" % (c, m) for c, ms in EXPECTED.items() for m in ms)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_well_formed(name):
    assert os.path.getsize(accel_c128.path(name)) < 1000000
    z = np.load(accel_c128.path(name), allow_pickle=False)
    assert sorted(z.files) == ["b", "case", "meta_json", "residuals", "x", "x0"]
    f = accel_c128.load(name)
    m = f["meta"]
    assert name == "%s__%s" % (f["case"], m["method"]) and m["case"] == f["case"]
    assert f["case"] in c128_cycle.cases()
    n = c128_cycle.load(f["case"])["levels"][0]["A"].shape[0]
    for k in ("b", "x0", "x"):
        assert f[k].dtype == np.complex128 and f[k].shape == (n,)
    res = f["residuals"]
    assert res.dtype == np.float64 and res.ndim == 1 and np.all(np.isfinite(res))
    assert m["iterations"] == len(res) - 1
    assert m["iterations"] >= 3 or f["case"] == "one_level"
    assert m["cycle"] in ("V", "W", "F") and m["method"] in krylov_host_c128.METHODS
    thr = m["tol"] * res[0]                    # what every stopping test compares with
    assert np.all(np.abs(res - thr) > 1e-6 * thr)
    assert res[-1] < thr


def test_restart_case_present():
    m = accel_c128.load("gs_sym_V_shifted2d__gmres")["meta"]
    assert (m["restrt"], m["maxiter"]) == (3, 4) and m["iterations"] > 3


# --------------------------------------------------------------------------- refusals, before any device work
def _ml(A=None, smoother="gauss_seidel", coarse="pinv", dtype=np.complex128):
    """a small two-level hierarchy built on the host (nothing touches a device)"""
    import pyamg_amd
    if A is None:
        n = 64
        d = (2 + 0.5j) if dtype == np.complex128 else 2.0
        A = sps.diags([-np.ones(n - 1), d * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr", dtype=dtype)
    P = sps.csr_matrix(np.kron(np.eye(A.shape[0] // 2), np.ones((2, 1))))
    l0, l1 = pyamg_amd.multilevel_solver.level(), pyamg_amd.multilevel_solver.level()
    l0.A, l0.P, l0.R = A, P, P.T.tocsr()
    l1.A = sps.csr_matrix(P.T @ A @ P)
    ml = pyamg_amd.multilevel_solver([l0, l1], coarse_solver=coarse)
    pyamg_amd.change_smoothers(ml, smoother, smoother)
    return ml


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to build the device mirror fails the test"""
    from pyamg_amd import multilevel

    def boom(*a, **k):
        raise AssertionError("device work started")
    monkeypatch.setattr(multilevel._DeviceHierarchyC128, "__init__", boom)
    monkeypatch.setattr(multilevel._DeviceHierarchy, "__init__", boom)


METHODS = ["cg", "bicgstab", "gmres", "fgmres"]
B = np.ones(64, dtype=np.complex128)


def test_module_surface():
    import pyamg_amd
    from pyamg_amd import krylov_c128
    assert pyamg_amd.krylov_c128 is krylov_c128
    assert sorted(krylov_c128.METHODS) == sorted(METHODS)
    for name in ("cr", "cgne", "cgnr", "steepest_descent", "minimal_residual"):
        assert not hasattr(krylov_c128, name)


def test_preconditioner_carries_hierarchy_and_cycle():
    ml = _ml()
    M = ml.aspreconditioner(cycle="W")
    assert M.hierarchy is ml and M.cycle == "W"
    assert isinstance(M, LinearOperator) and M.shape == (64, 64) and M.dtype == np.complex128


@pytest.mark.parametrize("method", METHODS)
def test_refuses_no_preconditioner(no_device, method):
    from pyamg_amd import krylov_c128
    ml = _ml()
    with pytest.raises(NotImplementedError, match="scipy"):
        krylov_c128.METHODS[method](ml.levels[0].A, B)


@pytest.mark.parametrize("method", METHODS)
def test_refuses_float64_hierarchy(no_device, method):
    from pyamg_amd import krylov_c128
    ml = _ml(dtype=np.float64)
    with pytest.raises(NotImplementedError, match="scipy"):
        krylov_c128.METHODS[method](ml.levels[0].A, np.ones(64), M=ml.aspreconditioner())


@pytest.mark.parametrize("method", METHODS)
def test_refuses_foreign_operator(no_device, method):
    from pyamg_amd import krylov_c128
    ml = _ml()
    M = LinearOperator((64, 64), matvec=lambda v: v, dtype=np.complex128)
    with pytest.raises(NotImplementedError, match="scipy"):
        krylov_c128.METHODS[method](ml.levels[0].A, B, M=M)


@pytest.mark.parametrize("method", METHODS)
def test_refuses_another_operator(no_device, method):
    from pyamg_amd import krylov_c128
    ml = _ml()
    A = ml.levels[0].A
    for other in (sps.csr_matrix(A * 2.0), A[:32, :32], A.toarray()):
        with pytest.raises(NotImplementedError, match="scipy"):
            krylov_c128.METHODS[method](other, B[:other.shape[0]], M=ml.aspreconditioner())


@pytest.mark.parametrize("method", METHODS)
def test_refuses_amli(no_device, method):
    from pyamg_amd import krylov_c128
    ml = _ml()
    with pytest.raises(NotImplementedError, match="scipy"):
        krylov_c128.METHODS[method](ml.levels[0].A, B, M=ml.aspreconditioner(cycle="AMLI"))
    with pytest.raises(NotImplementedError):
        ml.solve(B, cycle="AMLI", accel=krylov_c128.METHODS[method])


@pytest.mark.parametrize("method", METHODS)
def test_refuses_bad_maxiter(no_device, method):
    from pyamg_amd import krylov_c128
    ml = _ml()
    with pytest.raises(ValueError):
        krylov_c128.METHODS[method](ml.levels[0].A, B, maxiter=0, M=ml.aspreconditioner())


def test_refuses_out_of_scope_smoother(no_device):
    from pyamg_amd import krylov_c128
    ml = _ml(smoother="gauss_seidel_ne")
    with pytest.raises(NotImplementedError):
        krylov_c128.gmres(ml.levels[0].A, B, M=ml.aspreconditioner())
    with pytest.raises(NotImplementedError):
        ml.solve(B, accel=krylov_c128.gmres)


@pytest.mark.parametrize("accel", METHODS)
def test_name_refusal_unchanged(no_device, accel):
    ml = _ml()
    with pytest.raises(NotImplementedError, match="the device Krylov methods are float64 only; for a complex128 "
                                                  "hierarchy pass a scipy.sparse.linalg callable as accel, or use "
                                                  r"aspreconditioner\(\) as M"):
        ml.solve(B, accel=accel)


# --------------------------------------------------------------------------- the numpy restatements
@pytest.fixture(scope="module")
def core():
    core = c128_cycle.reference_core()
    if core is None:
        pytest.skip("oracle/_ref (the reference's compiled kernels) is absent: the host cycle needs them")
    return core


@pytest.mark.parametrize("name", NAMES)
def test_host_restatement_reproduces_reference(core, name):
    f = accel_c128.load(name)
    m = f["meta"]
    g = c128_cycle.load(f["case"])
    A = g["levels"][0]["A"]
    host = c128_cycle.HostCycle(g, core)
    kw = {"maxiter": m["maxiter"]}
    if m["method"] in ("gmres", "fgmres"):
        kw["restrt"] = m["restrt"]
    x, res, _ = krylov_host_c128.METHODS[m["method"]](
        lambda v: A @ v, lambda v: host.iterates(v, np.zeros_like(v), 1, m["cycle"])[0], f["b"], f["x0"], m["tol"], **kw)
    assert all(type(r) is float for r in res)
    accel_c128.assert_matches(res, x, f["residuals"], f["x"], name)
