"""complex128 resident hierarchies on the MI355X: every fixture of tests/golden/hier_c128/ solved on the device
gives the reference's iterates bit for bit, its iteration count, and its residual history within the float64
rule of golden_io.history_tolerance; plus a live ~1M-unknown magnetic Laplacian against the host restatement."""
import numpy as np
import pytest
import scipy.sparse as sps

import c128_cycle
import golden_io

pytestmark = pytest.mark.gpu
CASES = c128_cycle.cases()


def same(a, b):
    return c128_cycle.bit_mismatches(np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)) == 0


@pytest.mark.parametrize("case", CASES)
def test_solve_matches_reference(case):
    g = c128_cycle.load(case)
    m = g["meta"]
    ml = c128_cycle.build_ml(g)
    its, res = [], []
    x0 = None if not np.any(g["x0"]) else g["x0"]
    x = ml.solve(g["b"], x0=x0, tol=m["tol"], maxiter=m["maxiter"], cycle=m["cycle"], residuals=res,
                 callback=lambda xk: its.append(np.array(xk, copy=True)))
    assert x.dtype == np.complex128 and x.shape == g["b"].shape
    assert len(res) == len(g["residuals"]), "iterations %d, reference %d" % (len(res) - 1, len(g["residuals"]) - 1)
    assert all(type(r) is float for r in res)
    assert len(its) == len(res) - 1
    assert same(its[0], g["x_iter1"])
    assert same(its[1] if len(its) > 1 else its[0], g["x_iter2"])
    assert same(x, g["x"])
    A = g["levels"][0]["A"]
    golden_io.assert_history(res, g["residuals"], A, g["x"], g["b"])


@pytest.mark.parametrize("case", CASES)
def test_solve_without_callback_and_preconditioner(case):
    g = c128_cycle.load(case)
    m = g["meta"]
    ml = c128_cycle.build_ml(g)
    res = []
    x0 = None if not np.any(g["x0"]) else g["x0"]
    x = ml.solve(g["b"], x0=x0, tol=m["tol"], maxiter=m["maxiter"], cycle=m["cycle"], residuals=res)
    assert same(x, g["x"]) and len(res) == len(g["residuals"])
    golden_io.assert_history(res, g["residuals"], g["levels"][0]["A"], g["x"], g["b"])
    M = ml.aspreconditioner(cycle=m["cycle"])
    assert M.dtype == np.complex128
    assert same(M * g["b"], g["Mb"])
    assert ml.device_hierarchy().device_bytes() > 0
    assert ml.device_hierarchy().last_solve_ms() >= 0.0


def test_scipy_accel_runs_with_device_cycle():
    import scipy.sparse.linalg as spla
    g = c128_cycle.load("cheb2_magnetic3d")
    ml = c128_cycle.build_ml(g)
    res = []
    x = ml.solve(g["b"], tol=1e-8, maxiter=30, accel=spla.gmres, residuals=res)
    A = g["levels"][0]["A"]
    assert x.dtype == np.complex128
    assert np.linalg.norm(g["b"] - A @ x) <= 1e-6 * np.linalg.norm(g["b"])
    assert len(res) >= 2


def _magnetic3d(n, shift, seed):
    rng = np.random.RandomState(seed)
    T = sps.diags([np.ones(n - 1), np.ones(n - 1)], [-1, 1], format="csr")
    I = sps.identity(n, format="csr")
    G = (sps.kron(sps.kron(T, I), I) + sps.kron(sps.kron(I, T), I) + sps.kron(sps.kron(I, I), T)).tocoo()
    up = G.row < G.col
    r, c = G.row[up], G.col[up]
    ph = np.exp(1j * rng.uniform(-np.pi, np.pi, size=r.size))
    N = n ** 3
    W = sps.coo_matrix((np.concatenate([ph, ph.conj()]), (np.concatenate([r, c]), np.concatenate([c, r]))),
                       shape=(N, N)).tocsr()
    deg = np.asarray(abs(W).sum(axis=1)).ravel()
    A = (sps.diags(deg + shift) - W).tocsr().astype(np.complex128)
    A.sort_indices()
    return A


def test_live_magnetic_1m_two_cycles_match_host():
    core = c128_cycle.reference_core()
    if core is None:
        pytest.skip("oracle/_ref (the reference's compiled kernels) is absent: the host restatement needs them")
    import pyamg_amd
    n = 100
    A = _magnetic3d(n, 0.05, seed=3)
    # real SA aggregates from the project's float64 setup on |A|'s pattern; complex Galerkin products by scipy
    Ar = sps.csr_matrix((np.abs(A.data), A.indices, A.indptr), shape=A.shape)
    mlr = pyamg_amd.smoothed_aggregation_solver(Ar, max_coarse=500, max_levels=4)
    levels, Ak = [], A
    for i, lr in enumerate(mlr.levels):
        lvl = pyamg_amd.multilevel_solver.level()
        lvl.A = Ak
        if i < len(mlr.levels) - 1:
            lvl.P = sps.csr_matrix(lr.P)
            lvl.R = lvl.P.T.tocsr()
            Ak = sps.csr_matrix(lvl.R @ Ak @ lvl.P)
        levels.append(lvl)
    import scipy.linalg
    M = np.ascontiguousarray(scipy.linalg.pinv(levels[-1].A.toarray()), dtype=np.complex128)
    ml = pyamg_amd.multilevel_solver(levels, coarse_solver=("dense", {"M": M}))
    nl = len(levels) - 1
    cheb = ("polynomial", {"coefficients": [-0.1, 0.9, 1.4]})
    pre = [("gauss_seidel", {"sweep": "symmetric"})] + [cheb] * (nl - 1)
    post = [cheb] * nl
    pyamg_amd.change_smoothers(ml, pre, post)
    rng = np.random.RandomState(5)
    b = rng.rand(A.shape[0]) + 1j * rng.rand(A.shape[0])
    its = []
    ml.solve(b, tol=1e-30, maxiter=2, callback=lambda xk: its.append(np.array(xk, copy=True)))
    g = {"levels": [], "coarse": ("dense", {"M": M})}
    for i, lvl in enumerate(levels):
        L = {"A": lvl.A}
        if i < nl:
            L.update(P=lvl.P, R=lvl.R, pre=golden_io.canonical({"name": pre[i][0], **pre[i][1]}),
                     post=golden_io.canonical({"name": post[i][0], **post[i][1]}))
        g["levels"].append(L)
    host = c128_cycle.HostCycle(g, core).iterates(b, np.zeros_like(b), 2, "V")
    assert len(its) == 2
    assert same(its[0], host[0]) and same(its[1], host[1])


def test_scipy_only_coarse_krylov_runs_on_complex_vectors():
    """a coarse Krylov name only scipy has runs as a host callback on complex128 vectors"""
    g = c128_cycle.load("cheb2_magnetic3d")
    g = dict(g, coarse=("bicg", {"tol": 1e-12, "maxiter": 500}))
    ml = c128_cycle.build_ml(g)
    res = []
    x = ml.solve(g["b"], tol=1e-8, maxiter=60, residuals=res)
    A = g["levels"][0]["A"]
    assert x.dtype == np.complex128
    assert np.linalg.norm(g["b"] - A @ x) <= 2e-8 * np.linalg.norm(g["b"])


def test_handle_is_sealed_after_finalize():
    """setters after amg_hierx_finalize are refused; a second finalize is a no-op"""
    from pyamg_amd import _lib
    g = c128_cycle.load("gs_sym_V_shifted2d")
    ml = c128_cycle.build_ml(g)
    dev = ml.device_hierarchy()
    M = np.zeros((2, 2), dtype=np.complex128)
    assert dev.L.amg_hierx_set_coarse_dense(dev.h, M.ctypes.data, 2) == _lib.AMG_ESTATE
    d = _lib.SmootherDescX()
    assert dev.L.amg_hierx_set_smoother(dev.h, 0, 0, d) == _lib.AMG_ESTATE
    assert dev.L.amg_hierx_finalize(dev.h) == 0
    x = ml.solve(g["b"], tol=g["meta"]["tol"], maxiter=g["meta"]["maxiter"])
    assert same(x, g["x"])


def test_history_reservation_and_timing():
    """the device history holds maxiter + 2 doubles, is counted in device_bytes and only grows; a history left by a
    longer solve changes nothing in a shorter one; solve and cycle both time themselves"""
    g = c128_cycle.load("gs_sym_V_shifted2d")
    cyc = str(g["meta"]["cycle"]).upper()
    ml = c128_cycle.build_ml(g)
    ml.solve(g["b"], tol=0, maxiter=2, cycle=cyc)
    dev = ml.device_hierarchy()
    assert dev.last_solve_ms() > 0.0
    small = dev.device_bytes()
    ml.solve(g["b"], tol=0, maxiter=20, cycle=cyc)
    grown = dev.device_bytes()
    assert grown - small == 8 * (22 - 4)
    res = []
    x = ml.solve(g["b"], tol=0, maxiter=5, cycle=cyc, residuals=res)
    assert dev.device_bytes() == grown
    fresh = c128_cycle.build_ml(g)
    res_fresh = []
    x_fresh = fresh.solve(g["b"], tol=0, maxiter=5, cycle=cyc, residuals=res_fresh)
    assert fresh.device_hierarchy().device_bytes() == small + 8 * (7 - 4)
    assert same(x, x_fresh)
    assert len(res) == len(res_fresh) == 6
    assert np.array_equal(np.array(res).view(np.int64), np.array(res_fresh).view(np.int64))
    # the cycle entry, as the first timed call of a handle (no solve has set the time before it); it gives what the
    # preconditioner gives (one cycle of solve), which leaves the history as it was
    Mb = ml.aspreconditioner(cycle=cyc) * g["b"]
    assert dev.device_bytes() == grown
    cold_ml = c128_cycle.build_ml(g)
    cold = cold_ml.device_hierarchy()
    assert cold.last_solve_ms() == 0.0
    b1 = np.ascontiguousarray(g["b"], dtype=np.complex128)
    x1 = np.zeros_like(b1)
    cold.cycle(b1, x1, cyc, x0_zero=True)
    assert cold.last_solve_ms() > 0.0
    assert same(x1, Mb)
