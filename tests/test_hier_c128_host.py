"""complex128 resident hierarchies without a GPU: the new symbols, the refusals (which happen before any device
work), complex descriptors from change_smoothers, the fixtures, and the host restatement of the cycle
(tests/c128_cycle.py) against the reference's recorded iterates."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sps

import c128_cycle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pyamg_amd", "lib", "libamgcore_hip.so")
SYMBOLS = ["amg_hierx_create", "amg_hierx_destroy", "amg_hierx_set_matrix", "amg_hierx_set_smoother",
           "amg_hierx_set_block_matrix", "amg_hierx_set_coarse_dense", "amg_hierx_set_coarse_callback",
           "amg_hierx_finalize", "amg_hierx_solve", "amg_hierx_cycle", "amg_hierx_device_bytes",
           "amg_hierx_last_solve_ms"]
CASES = c128_cycle.cases()


def test_symbols_exported():
    L = ctypes.CDLL(LIB)
    for s in SYMBOLS:
        assert hasattr(L, s), s


def test_other_value_types_not_implemented():
    from pyamg_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p(123)
    for vt in (_lib.AMG_VALUE_F64, _lib.AMG_VALUE_F32, _lib.AMG_VALUE_C64):
        assert L.amg_hierx_create(vt, 2, 0, ctypes.byref(h)) == _lib.AMG_ENOTIMPL
        assert h.value is None


def _ml(A=None, smoother="gauss_seidel", coarse="pinv"):
    """a small complex128 two-level hierarchy built on the host (nothing touches a device)"""
    import pyamg_amd
    if A is None:
        n = 64
        A = sps.diags([-np.ones(n - 1), (2 + 0.5j) * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr",
                      dtype=np.complex128)
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


def test_refuses_amli(no_device):
    ml = _ml()
    with pytest.raises(NotImplementedError):
        ml.solve(np.ones(64, dtype=np.complex128), cycle="AMLI")


@pytest.mark.parametrize("spec", ["gauss_seidel_ne", "gauss_seidel_nr", "jacobi_ne", "schwarz",
                                  ("gauss_seidel_indexed", {"indices": np.arange(64)}), "multicolor_gauss_seidel",
                                  "cg", "gmres", "cgnr"])
@pytest.mark.parametrize("side", ["pre", "post"])
def test_refuses_out_of_scope_smoothers(no_device, spec, side):
    import pyamg_amd
    ml = _ml()
    pre, post = (spec, "gauss_seidel") if side == "pre" else ("gauss_seidel", spec)
    pyamg_amd.change_smoothers(ml, pre, post)
    with pytest.raises(NotImplementedError):
        ml.solve(np.ones(64, dtype=np.complex128))


@pytest.mark.parametrize("coarse", ["cg", "gmres", "bicgstab", "schwarz", "jacobi_ne", "gauss_seidel_nr"])
def test_refuses_device_krylov_and_other_coarse_solvers(no_device, coarse):
    ml = _ml(coarse=coarse)
    with pytest.raises(NotImplementedError):
        ml.solve(np.ones(64, dtype=np.complex128))


def test_refuses_device_krylov_coarse_callable(no_device):
    from pyamg_amd import krylov
    ml = _ml(coarse=krylov.METHODS["cg"])
    with pytest.raises(NotImplementedError):
        ml.solve(np.ones(64, dtype=np.complex128))


def test_save_load_refuse_complex(tmp_path):
    ml = _ml()
    with pytest.raises(NotImplementedError):
        ml.save(str(tmp_path / "h"))
    assert not (tmp_path / "h").exists()
    # a directory holding complex operators (written by hand) is refused on load
    import pyamg_amd
    mlr = _ml(A=sps.diags([-np.ones(63), 2 * np.ones(64), -np.ones(63)], [-1, 0, 1], format="csr"))
    mlr.save(str(tmp_path / "r"))
    f = str(tmp_path / "r" / "A0_data.npy")
    np.save(f, np.load(f).astype(np.complex128))
    with pytest.raises(NotImplementedError):
        pyamg_amd.multilevel_solver.load(str(tmp_path / "r"))


def test_partitioned_path_refuses_complex():
    from pyamg_amd import distributed
    ml = _ml()
    with pytest.raises(NotImplementedError):
        distributed.levels_from_ml(ml)
    levels = [{"A": ml.levels[0].A, "P": ml.levels[0].P, "R": ml.levels[0].R, "pre": None, "post": None},
              {"A": ml.levels[1].A}]
    with pytest.raises(NotImplementedError):
        distributed.DistributedSolver(levels, None, None, 0, 1)


@pytest.mark.parametrize("accel", ["cg", "gmres", "fgmres", "bicgstab"])
def test_refuses_device_krylov(no_device, accel):
    ml = _ml()
    with pytest.raises(NotImplementedError, match="aspreconditioner"):
        ml.solve(np.ones(64, dtype=np.complex128), accel=accel)
    from pyamg_amd import krylov
    with pytest.raises(NotImplementedError):
        ml.solve(np.ones(64, dtype=np.complex128), accel=krylov.METHODS[accel])


def test_refuses_torch_tensors(no_device):
    torch = pytest.importorskip("torch")
    ml = _ml()

    class FakeCuda(object):           # what solve() sees of a CUDA tensor; no device is touched
        is_cuda = True
        dtype = torch.complex128

        def data_ptr(self):
            return 0
    with pytest.raises(NotImplementedError):
        ml.solve(FakeCuda())


def test_real_A_complex_b_refused(no_device):
    ml = _ml(A=sps.diags([-np.ones(63), 2 * np.ones(64), -np.ones(63)], [-1, 0, 1], format="csr"))
    with pytest.raises(NotImplementedError):
        ml.solve(np.ones(64, dtype=np.complex128))


def _fake_cuda_vector():
    torch = pytest.importorskip("torch")

    class FakeCuda(object):           # what solve() sees of a CUDA tensor; no device is touched
        is_cuda = True
        dtype = torch.float64

        def data_ptr(self):
            return 0
    return FakeCuda()


@pytest.mark.parametrize("call", ["solve_f64", "solve_c128", "solve_accel", "solve_many", "cycle_complexity",
                                  "device_tensor"])
def test_unknown_cycle_name_is_one_message(no_device, monkeypatch, call):
    """every entry that takes a cycle name upper-cases it and refuses an unknown one with the same TypeError, before
    any device work"""
    from pyamg_amd import multilevel
    monkeypatch.setattr(multilevel._DeviceHierarchyMulti, "__init__", multilevel._DeviceHierarchy.__init__)
    real = _ml(A=sps.diags([-np.ones(63), 2 * np.ones(64), -np.ones(63)], [-1, 0, 1], format="csr"))
    calls = {"solve_f64": lambda: real.solve(np.ones(64), cycle="z"),
             "solve_c128": lambda: _ml().solve(np.ones(64, dtype=np.complex128), cycle="z"),
             "solve_accel": lambda: real.solve(np.ones(64), cycle="z", accel="cg"),
             "solve_many": lambda: real.solve_many(np.ones((64, 2)), cycle="z"),
             "cycle_complexity": lambda: real.cycle_complexity("z"),
             "device_tensor": lambda: real.solve(_fake_cuda_vector(), cycle="z")}
    with pytest.raises(TypeError) as err:
        calls[call]()
    assert str(err.value) == "Unrecognized cycle type (Z)"


def test_change_smoothers_keeps_complex_descriptors():
    import pyamg_amd
    ml = _ml()
    A = sps.kron(ml.levels[0].A, np.array([[2.0, 1.0], [1.0, 3.0]])).tobsr(blocksize=(2, 2))
    mlb = _ml(A=sps.csr_matrix(A))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pyamg_amd.change_smoothers(ml, ("jacobi", {"omega": 4.0 / 3.0}), "richardson")
        pyamg_amd.change_smoothers(mlb, ("block_jacobi", {"blocksize": 2}), ("block_gauss_seidel", {"blocksize": 2}))
        d = ml.levels[0].presmoother.desc
        assert np.isfinite(d["omega"]) and d["omega"] > 0
        for side in ("presmoother", "postsmoother"):
            Dinv = getattr(mlb.levels[0], side).desc["Dinv"]
            assert Dinv.dtype == np.complex128 and np.any(Dinv.imag != 0)
        from pyamg_amd import smoothing
        name, kw = smoothing.spec_from_descriptor(mlb.levels[0].presmoother.desc)
        assert kw["Dinv"].dtype == np.complex128


def test_float32_complex64_hierarchies_keep_refusal():
    ml = _ml()
    for lvl in ml.levels:
        lvl.A = lvl.A.astype(np.complex64)
    with pytest.raises(NotImplementedError):
        ml.solve(np.ones(64, dtype=np.complex64))


@pytest.mark.parametrize("case", CASES)
def test_fixture_well_formed(case):
    path = os.path.join(c128_cycle.GOLDEN, case + ".npz")
    assert os.path.getsize(path) < 1 << 20
    g = c128_cycle.load(case)
    for k in ("b", "x0", "x", "x_iter1", "x_iter2", "Mb"):
        assert g[k].dtype == np.complex128 and g[k].shape == (g["levels"][0]["A"].shape[0],), k
    assert g["residuals"].dtype == np.float64
    for L in g["levels"]:
        assert L["A"].dtype == np.complex128
    tol = g["meta"]["tol"] * np.linalg.norm(g["b"])
    assert np.all(np.abs(g["residuals"] - tol) > 1e-6 * tol), "a stop decision lies within 1e-6 of tol"


def test_fixture_cases_present():
    assert len(CASES) >= 10 and "sor_negzero" in CASES


@pytest.mark.parametrize("case", CASES)
def test_host_restatement_matches_reference(case):
    core = c128_cycle.reference_core()
    if core is None:
        pytest.skip("oracle/_ref (the reference's compiled kernels) is absent: development container only")
    g = c128_cycle.load(case)
    H = c128_cycle.HostCycle(g, core)
    its = H.iterates(g["b"], g["x0"], 2, g["meta"]["cycle"])
    assert c128_cycle.bit_mismatches(its[0], g["x_iter1"]) == 0
    if len(g["residuals"]) > 2:
        assert c128_cycle.bit_mismatches(its[1], g["x_iter2"]) == 0
    Mb = H.iterates(g["b"], np.zeros_like(g["b"]), 1, g["meta"]["cycle"])[0]
    assert c128_cycle.bit_mismatches(Mb, g["Mb"]) == 0


def test_sor_fixture_pins_numpy_scaling():
    """sor_negzero: decoupled rows with b_i = (-0, -v); SOR's blend gives +0 there under numpy's promoted product and
    -0 under component-wise scaling, so a device that scaled component-wise would fail the GPU tests"""
    core = c128_cycle.reference_core()
    if core is None:
        pytest.skip("oracle/_ref (the reference's compiled kernels) is absent: development container only")
    g = c128_cycle.load("sor_negzero")
    its = c128_cycle.HostCycle(g, core).iterates(g["b"], g["x0"], 1)
    bad = c128_cycle.HostCycle(g, core, scale=c128_cycle.componentwise).iterates(g["b"], g["x0"], 1)
    assert c128_cycle.bit_mismatches(its[0], g["x_iter1"]) == 0
    assert c128_cycle.bit_mismatches(bad[0], g["x_iter1"]) > 0


def test_sor_fixture_has_signed_zeros():
    g = c128_cycle.load("sor_negzero")
    A = g["levels"][0]["A"]
    rows = [i for i in range(A.shape[0]) if A.indptr[i + 1] - A.indptr[i] == 1]
    assert len(rows) >= 5
    assert np.all(np.signbit(g["b"].real[rows])) and np.all(g["b"].imag[rows] < 0)
    assert np.all(g["x_iter1"].real[rows] == 0) and not np.any(np.signbit(g["x_iter1"].real[rows]))
