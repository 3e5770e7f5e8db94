"""pyamg_amd.krylov's shared method bodies without a device, on tests/krylov_numpy.py's host vectors: in complex128
against the restatements of tests/krylov_host_c128.py (which are pinned to the reference's own histories), the
breakdown and 1 x 1 branches in complex128, and the three edges on which the float64 methods follow the reference."""
import numpy as np
import pytest
import scipy.sparse as sps

import accel_c128
import krylov_host_c128
from krylov_numpy import NumpyVectors
from pyamg_amd import krylov

METHODS = ["cg", "bicgstab", "gmres", "fgmres"]


def shifted_laplacian(n):
    return sps.diags([-np.ones(n - 1), (2 + 0.5j) * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr",
                     dtype=np.complex128)


def solve(method, A, M, b, x0, dtype=np.complex128, **kw):
    """-> (x, residuals, info, callback arguments) of krylov.<method> on host vectors"""
    V = NumpyVectors(A, M, dtype=dtype)
    bd, xd = V.upload(b), V.upload(x0)
    res, seen = [], []
    info = krylov.METHODS[method](V, bd, xd, residuals=res, callback=seen.append, **kw)
    return V.download(xd), res, info, seen


# n = 6, maxiter = 6: the last inner iteration of the GMRES pair has inner == n - 1 (no reflector, no rotation);
# n = 40, restrt = 3: restart cycles and the exit by tolerance
SYSTEMS = {"n6_maxiter6": (6, dict(tol=1e-30, maxiter=6), None), "n40_restrt3": (40, dict(tol=1e-8, maxiter=30), 3)}


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("system", sorted(SYSTEMS))
def test_complex_methods_match_the_restatements(system, method):
    """the fixtures' rule (accel_c128.assert_matches): the same iteration count, histories within rtol 1e-9 /
    atol 1e-13 res[0], x within 1e-10 relative"""
    n, kw, restrt = SYSTEMS[system]
    if method in ("gmres", "fgmres"):
        kw = dict(kw, restrt=restrt)
    A = shifted_laplacian(n)
    d = A.diagonal()

    def jacobi(v):
        return (2.0 / 3.0) * v / d
    rng = np.random.RandomState(2)
    b = rng.rand(n) + 1j * rng.rand(n)
    x0 = rng.rand(n) - 1j * rng.rand(n)
    xr, ref, info_ref = krylov_host_c128.METHODS[method](lambda v: A @ v, jacobi, b, x0, **kw)
    x, res, info, _ = solve(method, A, jacobi, b, x0, **kw)
    assert info == info_ref and all(type(r) is float for r in res)
    if system == "n6_maxiter6":
        assert len(ref) == 7
    else:                                # the operator is not Hermitian: cg runs its 30 iterations, the others converge
        assert len(ref) > 4 and (info == 0 or method == "cg")
    accel_c128.assert_matches(res, x, ref, xr, "%s %s" % (system, method))


@pytest.mark.parametrize("method", ["gmres", "fgmres"])
def test_complex_breakdown_and_1x1(method):
    """test_host_api's float64 cases in complex128: a Krylov space exhausted inside a restart cycle with tol = 0 leaves
    the exact solution alone in the following cycles; a 1 x 1 system is solved directly"""
    rng = np.random.RandomState(0)
    n = 40
    b = rng.rand(n) + 1j * rng.rand(n)
    u, w = rng.rand(n) + 1j * rng.rand(n), rng.rand(n) - 1j * rng.rand(n)
    B = np.eye(n) + np.outer(u, u.conj()) + np.outer(w, w.conj())
    x, _, _, _ = solve(method, B, None, b, np.zeros(n), tol=0.0, restrt=6, maxiter=3)
    assert np.all(np.isfinite(x)) and np.allclose(B @ x, b, rtol=1e-8, atol=1e-10)
    a, rhs = np.complex128(4 + 2j), np.complex128(2 - 3j)
    x, _, info, _ = solve(method, np.array([[a]]), None, [rhs], [0.0], tol=1e-8, restrt=3, maxiter=2)
    assert info == 0 and x[0] == rhs / a


@pytest.mark.parametrize("method", ["gmres", "fgmres"])
def test_float64_callback_on_immediate_convergence(method):
    """krylov/_gmres_householder.py:186-188, _fgmres.py:179-181: the callback sees the first residual norm once"""
    n = 12
    A = sps.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(n, n)).tocsr()
    xs = np.arange(1.0, n + 1)
    x, res, info, seen = solve(method, A, None, A @ xs, xs, dtype=np.float64, tol=1e-8)
    assert info == 0 and len(res) == 1 and seen == res and np.array_equal(x, xs)


@pytest.mark.parametrize("method", ["bicgstab", "gmres", "fgmres"])
def test_float64_1x1_is_a_division(method):
    """krylov/_bicgstab.py:111-114, _fgmres.py:163-166: x = b / a, which b * (1 / a) does not give for these values"""
    a, b = 3.0, 5.0
    assert b / a != b * (1.0 / a)
    x, _, info, _ = solve(method, np.array([[a]]), None, [b], [0.0], dtype=np.float64, tol=1e-8, maxiter=2)
    assert info == 0 and x[0] == b / a
