"""Krylov methods around the device-resident cycle of a complex128 hierarchy: cg, bicgstab, gmres (Householder, left
preconditioning) and fgmres (right preconditioning) of the reference's pyamg/krylov, with its signature

    (A, b, x0=None, tol=1e-5, restrt=None, maxiter=None, M=None, callback=None, residuals=None) -> (x, info)

(restrt: the two GMRES variants only).  M must be the aspreconditioner() of a complex128 pyamg_amd hierarchy and A that
hierarchy's level-0 operator; the functions are also what `ml.solve(b, accel=pyamg_amd.krylov_c128.gmres)` takes.
Anything else -- no M, a foreign operator, an AMLI cycle, another A -- raises NotImplementedError before any device
work: scipy.sparse.linalg's methods run those, with host vectors.

Every vector lives in HBM (include/amgcore_hip.h section 5: amg_hierx_apply, amg_hierx_cycle with device vectors,
amg_devx_*); what crosses PCIe per iteration is a handful of scalars.  The Householder sequences of the GMRES pair
(amg_core/krylov.h apply_householders, householder_hornerscheme) run as one chain of launches whose inner products
never leave the device, so an inner iteration costs a fixed number of host reads whatever its index
(DeviceSpaceC128.host_reads counts them).  The method bodies are krylov.py's, shared with the float64 hierarchies:
this module holds the complex128 vector space they run on and the public functions with the reference's signature.
Inner products are fixed-order device reductions where the reference calls BLAS, so histories agree to rounding
(pinned against the reference's own histories in tests/golden/accel_c128/).
"""
import ctypes as C

import numpy as np
from scipy import sparse

from . import _lib, krylov

__all__ = ["cg", "bicgstab", "gmres", "fgmres", "DeviceSpaceC128"]

_H2D, _D2H, _D2D = 0, 1, 2
_SZ = 16          # bytes of a complex128


class DeviceSpaceC128(krylov.VectorSpace):
    """complex128 vectors of level 0 of a device hierarchy plus the two operators a Krylov method needs: A (the level
    operator) and M (one multigrid cycle from a zero guess).  A krylov.VectorSpace whose dot (the conjugated inner
    product sum conj(x_i) y_i) and peek return np.complex128, whose reflect_range / horner run the Householder
    sequences without leaving the device, and whose reflectors are allocated as a restart cycle reaches them.
    host_reads counts the calls that brought a value to the host."""
    dtype = np.complex128

    def __init__(self, dev, cycle):
        self.L = _lib.lib()
        self.dev = dev
        self.h = dev.h
        self.n = int(self.L.amg_hierx_level_size(self.h, 0))
        self.stream = self.L.amg_hierx_stream(self.h)
        self.scratch = self.L.amg_hierx_scratch(self.h)
        if not self.scratch:
            raise _lib.AmgError(self.L.amg_last_error().decode())
        self.cycle = cycle
        self.host_reads = 0
        self._owned = []

    # -- storage
    def new(self, count=None):
        count = int(self.n if count is None else count)
        p = self.L.amg_hierx_vec_alloc(self.h, count)
        if not p:
            raise MemoryError(self.L.amg_last_error().decode())
        self._owned.append((p, count))
        return p

    def _free(self, owned):
        self.L.amg_hierx_vec_free(self.h, *owned)

    def reflectors(self, limit):
        return _Reflectors(self, limit)

    def upload(self, host, dst=None):
        host = np.ascontiguousarray(np.ravel(host), dtype=np.complex128)
        dst = self.new(len(host)) if dst is None else dst
        _lib.check(self.L.amg_devx_copy(dst, host.ctypes.data, len(host), _H2D, self.stream))
        return dst

    def download(self, src, count=None, offset=0):
        count = self.n if count is None else count
        out = np.empty(count, dtype=np.complex128)
        if count:
            _lib.check(self.L.amg_devx_copy(out.ctypes.data, src + _SZ * offset, count, _D2H, self.stream))
        self.host_reads += 1
        return out

    def poke(self, dst, offset, values):
        values = np.ascontiguousarray(np.atleast_1d(values), dtype=np.complex128)
        _lib.check(self.L.amg_devx_copy(dst + _SZ * offset, values.ctypes.data, len(values), _H2D, self.stream))

    def peek(self, src, offset):
        return self.download(src, 1, offset)[0]

    # -- BLAS-1 on (sub)vectors: `off` skips leading entries
    def copy(self, dst, src, off=0):
        if self.n - off > 0:
            _lib.check(self.L.amg_devx_copy(dst + _SZ * off, src + _SZ * off, self.n - off, _D2D, self.stream))

    def fill(self, x, value, off=0):
        if self.n - off > 0:
            value = complex(value)
            _lib.check(self.L.amg_devx_fill(x + _SZ * off, value.real, value.imag, self.n - off, self.stream))

    def scale(self, out, x, c):                       # out = c * x
        c = complex(c)
        _lib.check(self.L.amg_devx_scale(out, x, c.real, c.imag, self.n, self.stream))

    def axpy(self, y, a, x):                          # y += a * x
        a = complex(a)
        _lib.check(self.L.amg_devx_axpy(y, x, a.real, a.imag, self.n, self.stream))

    def xpby(self, p, beta, z):                       # p = beta * p + z
        beta = complex(beta)
        _lib.check(self.L.amg_devx_xpby(p, beta.real, beta.imag, z, self.n, self.stream))

    def sub(self, out, a, b):                         # out = a - b
        _lib.check(self.L.amg_devx_sub(out, a, b, self.n, self.stream))

    def dot(self, x, y):                              # sum conj(x_i) y_i
        r = (C.c_double * 2)()
        _lib.check(self.L.amg_devx_zdotc(x, y, self.n, self.scratch, 1, r, self.stream))
        self.host_reads += 1
        return np.complex128(complex(r[0], r[1]))

    def norm(self, x, off=0):
        if self.n - off <= 0:
            return 0.0
        r = C.c_double(0.0)
        _lib.check(self.L.amg_hierx_norm(self.h, x + _SZ * off, self.n - off, C.byref(r)))
        self.host_reads += 1
        return r.value

    # -- Householder sequences (amg_core/krylov.h:34-53, 97-120): no host synchronisation between reflectors
    def _vectors(self, W):
        return (C.c_void_p * max(1, len(W)))(*W), len(W)

    def reflect_range(self, v, W, start, stop, step):
        """for j in range(start, stop, step): v <- v - 2 <W[j], v> W[j]"""
        arr, nW = self._vectors(W)
        _lib.check(self.L.amg_devx_householders(v, arr, nW, self.n, int(start), int(stop), int(step), self.scratch,
                                                self.stream))

    def horner(self, v, W, y, inner):
        """for j = inner .. 0: v[j] += y[j]; v <- v - 2 <W[j], v> W[j]; y (host) is uploaded once"""
        y = np.ascontiguousarray(np.ravel(y), dtype=np.complex128)
        yd = self.upload(y)
        arr, nW = self._vectors(W)
        _lib.check(self.L.amg_devx_horner(v, arr, nW, yd, self.n, int(inner), -1, -1, self.scratch, self.stream))

    # -- operators
    def A(self, x, out):
        _lib.check(self.L.amg_hierx_apply(self.h, 0, x, out))

    def M(self, r, out):
        self.dev.cycle_device(r, out, self.cycle)


class _Reflectors(object):
    """the Householder vectors of a restart cycle, allocated as the cycle reaches them"""

    def __init__(self, V, limit):
        self.V, self.limit, self.vecs = V, limit, []

    def __getitem__(self, j):
        while len(self.vecs) <= j < self.limit:
            self.vecs.append(self.V.new())
        return self.vecs[j]

    def __len__(self):
        return len(self.vecs)

    def __iter__(self):
        return iter(self.vecs)


# --------------------------------------------------------------------------- the public functions: host vectors in and out
_SCIPY = ("this device Krylov method runs with M = ml.aspreconditioner() of a complex128 pyamg_amd hierarchy and "
          "A = ml.levels[0].A only (%s); use a scipy.sparse.linalg method for anything else")


def _resolve(A, M):
    """-> (hierarchy, cycle) of the preconditioner M, or NotImplementedError; no device work"""
    from . import multilevel
    ml, cycle = getattr(M, "hierarchy", None), getattr(M, "cycle", None)
    if M is None:
        raise NotImplementedError(_SCIPY % "M is None: unpreconditioned operation is not implemented")
    if not isinstance(ml, multilevel.multilevel_solver) or cycle is None:
        raise NotImplementedError(_SCIPY % "M is not the aspreconditioner() of a pyamg_amd hierarchy")
    if not multilevel._is_c128(ml):
        raise NotImplementedError(_SCIPY % "M belongs to a hierarchy that is not complex128")
    cycle = str(cycle).upper()
    if cycle not in ("V", "W", "F"):
        raise NotImplementedError(_SCIPY % ("%s cycles are not implemented for complex128 hierarchies" % cycle))
    A0 = ml.levels[0].A
    if A is not A0:
        same = sparse.issparse(A) and A.shape == A0.shape and A.dtype == A0.dtype and (A != A0).nnz == 0
        if not same:
            raise NotImplementedError(_SCIPY % "A is not the hierarchy's level-0 operator")
    if ml._dev is None:
        multilevel._DeviceHierarchyC128.check_levels(ml)
    return ml, cycle


def _run(method, A, b, x0, M, callback, **kw):
    krylov._maxiter(kw.get("maxiter"), None)
    ml, cycle = _resolve(A, M)
    b = np.asarray(b)
    n = ml.levels[0].A.shape[0]
    if b.size != n or (x0 is not None and np.size(x0) != n):
        raise ValueError("b and x0 must have %d entries" % n)
    b1 = np.ascontiguousarray(np.ravel(b), dtype=np.complex128)
    x1 = np.zeros(n, dtype=np.complex128) if x0 is None else np.ascontiguousarray(np.ravel(x0), dtype=np.complex128)
    with DeviceSpaceC128(ml.device_hierarchy(), cycle) as V:
        bd, xd = V.upload(b1), V.upload(x1)
        info = krylov.METHODS[method](V, bd, xd, callback=callback, **kw)
        x = V.download(xd)
    return x.reshape(b.shape), info


def cg(A, b, x0=None, tol=1e-5, restrt=None, maxiter=None, M=None, callback=None, residuals=None):
    """Preconditioned conjugate gradients (krylov/_cg.py); callback(x) after every iteration; info -1: indefinite
    operator or preconditioner (Re <Ap, p> < 0 or Re <r, z> < 0).  restrt is ignored."""
    return _run("cg", A, b, x0, M, callback, tol=tol, maxiter=maxiter, residuals=residuals)


def bicgstab(A, b, x0=None, tol=1e-5, restrt=None, maxiter=None, M=None, callback=None, residuals=None):
    """Right-preconditioned BiCGStab (krylov/_bicgstab.py); callback(x) after every iteration.  restrt is ignored."""
    return _run("bicgstab", A, b, x0, M, callback, tol=tol, maxiter=maxiter, residuals=residuals)


def gmres(A, b, x0=None, tol=1e-5, restrt=None, maxiter=None, M=None, callback=None, residuals=None):
    """Left-preconditioned Householder GMRES (krylov/_gmres_householder.py); callback(normr) per inner iteration."""
    return _run("gmres", A, b, x0, M, callback, tol=tol, restrt=restrt, maxiter=maxiter, residuals=residuals)


def fgmres(A, b, x0=None, tol=1e-5, restrt=None, maxiter=None, M=None, callback=None, residuals=None):
    """Right-preconditioned flexible Householder GMRES (krylov/_fgmres.py); callback(normr) per inner iteration."""
    return _run("fgmres", A, b, x0, M, callback, tol=tol, restrt=restrt, maxiter=maxiter, residuals=residuals)


METHODS = {"cg": cg, "bicgstab": bicgstab, "gmres": gmres, "fgmres": fgmres}
