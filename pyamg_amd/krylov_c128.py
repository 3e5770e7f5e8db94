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
(DeviceSpaceC128.host_reads counts them).  Each method follows the reference line by line -- conjugated inner
products, mysign(x) = x / |x|, the BLAS rotg Givens block [[c, s], [-conj(s), c]], complex H, g and Q on the host;
inner products are fixed-order device reductions where the reference calls BLAS, so histories agree to rounding
(pinned against the reference's own histories in tests/golden/accel_c128/).
"""
import ctypes as C

import numpy as np
import scipy.linalg
from scipy import sparse

from . import _lib
from .krylov import _inner_limits

__all__ = ["cg", "bicgstab", "gmres", "fgmres", "DeviceSpaceC128"]

_H2D, _D2H, _D2D = 0, 1, 2
_SZ = 16          # bytes of a complex128


def _c(v):
    return np.complex128(v)


class DeviceSpaceC128(object):
    """complex128 vectors of level 0 of a device hierarchy plus the two operators a Krylov method needs: A (the level
    operator) and M (one multigrid cycle from a zero guess).  The method surface of krylov.DeviceSpace; dot returns a
    Python complex (the conjugated inner product sum conj(x_i) y_i), and reflect_range / horner run the Householder
    sequences without leaving the device.  host_reads counts the calls that brought a value to the host."""

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

    def release(self):
        for p, count in self._owned:
            self.L.amg_hierx_vec_free(self.h, p, count)
        self._owned = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

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
        return _c(self.download(src, 1, offset)[0])

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
        return complex(r[0], r[1])

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

    def residual(self, out, b, x, tmp):               # out = b - A x
        self.A(x, tmp)
        self.sub(out, b, tmp)


def _mysign(x):
    """the complex sign x / |x| (krylov/_fgmres.py:16, _gmres_householder.py:16)"""
    return 1.0 if x == 0.0 else x / abs(x)


def _check_maxiter(maxiter):
    if maxiter is not None and maxiter < 1:
        raise ValueError("Number of iterations must be positive")


# --------------------------------------------------------------------------- the methods on device vectors
def _cg(V, b, x, tol=1e-5, maxiter=None, residuals=None, callback=None):
    """Preconditioned conjugate gradients (krylov/_cg.py:84-183) with conjugated inner products.  The history is
    sqrt(<r, M r>); the reference stores that complex scalar, whose imaginary part is zero for a Hermitian positive
    definite M -- here its real part is stored, and the curvature tests look at real parts.
    -> info (0 converged, -1 indefinite operator / preconditioner, else the iteration count)"""
    if maxiter is None:
        maxiter = int(1.3 * V.n) + 2
    r, z, p, Ap = V.new(), V.new(), V.new(), V.new()
    V.residual(r, b, x, Ap)
    V.M(r, z)
    V.copy(p, z)
    rz = _c(V.dot(r, z))
    normr = float(np.sqrt(rz).real)
    if residuals is not None:
        residuals[:] = [normr]
    normb = V.norm(b) or 1.0
    if normr < tol * normb:
        return 0
    if normr != 0.0:
        tol = tol * normr
    it = 0
    while True:
        V.A(p, Ap)
        rz_old = rz
        pAp = _c(V.dot(Ap, p))
        if pAp.real < 0.0:
            return -1
        alpha = rz / pAp
        V.axpy(x, alpha, p)
        if (it % 8) and it > 0:
            V.axpy(r, -alpha, Ap)
        else:
            V.residual(r, b, x, z)
        V.M(r, z)
        rz = _c(V.dot(r, z))
        if rz.real < 0.0:
            return -1
        V.xpby(p, rz / rz_old, z)
        it += 1
        normr = float(np.sqrt(rz).real)
        if residuals is not None:
            residuals.append(normr)
        if callback is not None:
            callback(V.download(x))
        if normr < tol:
            return 0
        if rz == 0.0:
            return -1
        if it == maxiter:
            return it


def _bicgstab(V, b, x, tol=1e-5, maxiter=None, residuals=None, callback=None):
    """Right-preconditioned BiCGStab (krylov/_bicgstab.py:80-167): 2-norm history, conjugated inner products."""
    if maxiter is None:
        maxiter = V.n + 5
    r, rstar, p, Mp, AMp, s_, Ms, AMs = (V.new() for _ in range(8))
    V.residual(r, b, x, Mp)
    normr = V.norm(r)
    if residuals is not None:
        residuals[:] = [normr]
    normb = V.norm(b) or 1.0
    if normr < tol * normb:
        return 0
    if normr != 0.0:
        tol = tol * normr
    if V.n == 1:
        return _solve_1x1(V, b, x)
    V.copy(rstar, r)
    V.copy(p, r)
    rr_old = _c(V.dot(rstar, r))
    it = 0
    while True:
        V.M(p, Mp)
        V.A(Mp, AMp)
        alpha = rr_old / _c(V.dot(rstar, AMp))
        V.copy(s_, r)
        V.axpy(s_, -alpha, AMp)                       # s = r - alpha A M p
        V.M(s_, Ms)
        V.A(Ms, AMs)
        omega = _c(V.dot(AMs, s_)) / _c(V.dot(AMs, AMs))
        V.axpy(x, alpha, Mp)
        V.axpy(x, omega, Ms)
        V.copy(r, s_)
        V.axpy(r, -omega, AMs)                        # r = s - omega A M s
        rr_new = _c(V.dot(rstar, r))
        beta = (rr_new / rr_old) * (alpha / omega)
        rr_old = rr_new
        V.axpy(p, -omega, AMp)                        # p = r + beta (p - omega A M p)
        V.xpby(p, beta, r)
        it += 1
        normr = V.norm(r)
        if residuals is not None:
            residuals.append(normr)
        if callback is not None:
            callback(V.download(x))
        if normr < tol:
            return 0
        if it == maxiter:
            return it


def _solve_1x1(V, b, x):
    """a 1 x 1 system is solved directly: x = b / A[0, 0] (krylov/_fgmres.py:163-166, _gmres_householder.py:163-166)"""
    e, a = V.new(), V.new()
    V.fill(e, 1.0)
    V.A(e, a)
    V.poke(x, 0, V.peek(b, 0) / V.peek(a, 0))
    return 0


def _first_reflector(V, w, r, normr):
    """w = r + mysign(r[0]) ||r|| e_0, normalised (krylov/_fgmres.py:200-203); -> beta"""
    V.copy(w, r)
    w0 = V.peek(w, 0)
    beta = _mysign(w0) * normr
    V.poke(w, 0, w0 + beta)
    V.scale(w, w, 1.0 / V.norm(w))
    return beta


def _krylov_vector(V, v, W, inner):
    """v = P_0 ... P_inner e_inner (krylov/_fgmres.py:226-231)"""
    w = W[inner]
    V.scale(v, w, -2.0 * np.conjugate(V.peek(w, inner)))
    V.poke(v, inner, V.peek(v, inner) + 1.0)
    V.reflect_range(v, W, inner - 1, -1, -1)


def _hessenberg_step(V, v, W, inner, max_inner, Q, g, H):
    """The part of one (F)GMRES inner iteration after v holds P_inner ... P_0 (A ...) (krylov/_fgmres.py:250-303): the
    next reflector, then -- on the host, v has at most inner + 2 non-zero leading entries now -- the accumulated
    Givens rotations, the new rotation, the Hessenberg column."""
    n = V.n
    if inner != n - 1:
        if inner < max_inner - 1:
            # the reference starts every restart cycle from zeroed reflectors (W = zeros(...), _fgmres.py:212): after
            # a breakdown (alpha == 0) the next step must not find the previous cycle's vector here
            V.fill(W[inner + 1], 0.0)
        alpha = V.norm(v, off=inner + 1)
        if alpha != 0:
            alpha = _mysign(V.peek(v, inner + 1)) * alpha
            if inner < max_inner - 1:
                w = W[inner + 1]
                V.copy(w, v, off=inner + 1)
                V.poke(w, inner + 1, V.peek(w, inner + 1) + alpha)
                V.scale(w, w, 1.0 / V.norm(w))
            V.poke(v, inner + 1, -alpha)
            V.fill(v, 0.0, off=inner + 2)
    head = V.download(v, min(n, inner + 2))
    for j in range(inner):                            # amg_core/krylov.h apply_givens: rotations 0 .. inner-1 in order
        q0, q1, q2, q3 = Q[4 * j:4 * j + 4]
        a, bb = head[j], head[j + 1]
        head[j] = q0 * a + q1 * bb
        head[j + 1] = q2 * a + q3 * bb
    if inner != n - 1 and head[inner + 1] != 0:
        c, s = scipy.linalg.blas.zrotg(head[inner], head[inner + 1])
        Qblock = np.array([[c, s], [-np.conjugate(s), c]], dtype=np.complex128)
        Q[4 * inner:4 * inner + 4] = np.ravel(Qblock)
        g[inner:inner + 2] = np.dot(Qblock, g[inner:inner + 2])
        head[inner] = np.dot(Qblock[0, :], head[inner:inner + 2])
        head[inner + 1] = 0.0
    m = min(max_inner, len(head))
    H[:m, inner] = head[:m]


def _stagnated(V, update, x):
    """max |update_i / x_i| over x_i != 0 below 1e-12 (krylov/_fgmres.py:343-349): checked on the host copy of the two
    vectors only when the update is tiny in norm to begin with, which is the only way the entrywise test can hold"""
    nu, nx = V.norm(update), V.norm(x)
    if nx == 0.0 or nu > 1e-10 * nx:
        return False
    u, xx = V.download(update), V.download(x)
    idx = xx != 0
    return bool(idx.any() and np.max(np.abs(u[idx] / xx[idx])) < 1e-12)


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


def _fgmres(V, b, x, tol=1e-5, restrt=None, maxiter=None, residuals=None, callback=None):
    """Flexible GMRES, right preconditioning, Householder orthogonalisation (krylov/_fgmres.py:114-357); history:
    the 2-norm of the (true) residual, estimated through the rotated right-hand side inside a restart cycle."""
    n = V.n
    if n == 1:
        return _solve_1x1(V, b, x)
    max_outer, max_inner = _inner_limits(n, restrt, maxiter)
    r, v, t = V.new(), V.new(), V.new()
    V.residual(r, b, x, t)
    normr = V.norm(r)
    keep = residuals is not None
    if keep:
        residuals[:] = [normr]
    normb = V.norm(b) or 1.0
    if normr < tol * normb:
        if callback is not None:
            callback(normr)
        return 0
    if normr != 0.0:
        tol = tol * normr
    W = _Reflectors(V, max_inner)
    Z = _Reflectors(V, max_inner)
    niter = 0
    for outer in range(max_outer):
        beta = _first_reflector(V, W[0], r, normr)
        Q = np.zeros(4 * max_inner, dtype=np.complex128)
        H = np.zeros((max_inner, max_inner), dtype=np.complex128)
        g = np.zeros(max_inner + 2, dtype=np.complex128)
        g[0] = -beta
        inner = 0
        for inner in range(max_inner):
            _krylov_vector(V, v, W, inner)
            V.M(v, Z[inner])
            V.A(Z[inner], v)
            V.reflect_range(v, W, 0, inner + 1, 1)
            _hessenberg_step(V, v, W, inner, max_inner, Q, g, H)
            if inner < max_inner - 1:
                normr = float(abs(g[inner + 1]))
                if normr < tol:
                    break
                if callback is not None:
                    callback(normr)
                if keep:
                    residuals.append(normr)
            niter += 1
        y = scipy.linalg.solve(H[:inner + 1, :inner + 1], g[:inner + 1])
        V.fill(t, 0.0)                                             # update = Z[:, :inner+1] y
        for k in range(inner + 1):
            V.axpy(t, y[k], Z[k])
        V.axpy(x, 1.0, t)
        V.residual(r, b, x, v)
        normr = V.norm(r)
        if callback is not None:
            callback(normr)
        if keep:
            residuals.append(normr)
        if _stagnated(V, t, x):
            return -1
        if normr < tol:
            return 0
    return niter


def _gmres(V, b, x, tol=1e-5, restrt=None, maxiter=None, residuals=None, callback=None):
    """GMRES with LEFT preconditioning and Householder orthogonalisation (krylov/_gmres_householder.py:108-375, the
    reference's default `orthog`); history: the norm of the preconditioned residual M (b - A x)."""
    n = V.n
    if n == 1:
        return _solve_1x1(V, b, x)
    max_outer, max_inner = _inner_limits(n, restrt, maxiter)
    r, v, t = V.new(), V.new(), V.new()
    V.residual(t, b, x, v)
    V.M(t, r)
    normr = V.norm(r)
    keep = residuals is not None
    if keep:
        residuals[:] = [normr]
    normb = V.norm(b) or 1.0
    if normr < tol * normb:
        if callback is not None:
            callback(normr)
        return 0
    if normr != 0.0:
        tol = tol * normr
    W = _Reflectors(V, max_inner + 1)
    niter = 0
    for outer in range(max_outer):
        beta = _first_reflector(V, W[0], r, normr)
        Q = np.zeros(4 * max_inner, dtype=np.complex128)
        H = np.zeros((max_inner, max_inner), dtype=np.complex128)
        g = np.zeros(max_inner + 2, dtype=np.complex128)
        g[0] = -beta
        inner = 0
        for inner in range(max_inner):
            _krylov_vector(V, v, W, inner)
            V.A(v, t)
            V.M(t, v)
            V.reflect_range(v, W, 0, inner + 1, 1)
            _hessenberg_step(V, v, W, inner, max_inner, Q, g, H)
            niter += 1
            if inner < max_inner - 1:
                normr = float(abs(g[inner + 1]))
                if normr < tol:
                    break
                if callback is not None:
                    callback(normr)
                if keep:
                    residuals.append(normr)
        y = scipy.linalg.solve(H[:inner + 1, :inner + 1], g[:inner + 1])
        V.fill(t, 0.0)
        V.horner(t, W, y, inner)                                   # amg_core/krylov.h householder_hornerscheme
        V.axpy(x, 1.0, t)
        V.residual(v, b, x, r)
        V.M(v, r)
        normr = V.norm(r)
        if callback is not None:
            callback(normr)
        if keep:
            residuals.append(normr)
        if _stagnated(V, t, x):
            return -1
        if normr < tol:
            return 0
    return niter


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
    _check_maxiter(kw.get("maxiter"))
    ml, cycle = _resolve(A, M)
    b = np.asarray(b)
    n = ml.levels[0].A.shape[0]
    if b.size != n or (x0 is not None and np.size(x0) != n):
        raise ValueError("b and x0 must have %d entries" % n)
    b1 = np.ascontiguousarray(np.ravel(b), dtype=np.complex128)
    x1 = np.zeros(n, dtype=np.complex128) if x0 is None else np.ascontiguousarray(np.ravel(x0), dtype=np.complex128)
    with DeviceSpaceC128(ml.device_hierarchy(), cycle) as V:
        bd, xd = V.upload(b1), V.upload(x1)
        info = method(V, bd, xd, callback=callback, **kw)
        x = V.download(xd)
    return x.reshape(b.shape), info


def cg(A, b, x0=None, tol=1e-5, restrt=None, maxiter=None, M=None, callback=None, residuals=None):
    """Preconditioned conjugate gradients (krylov/_cg.py); callback(x) after every iteration; info -1: indefinite
    operator or preconditioner (Re <Ap, p> < 0 or Re <r, z> < 0).  restrt is ignored."""
    return _run(_cg, A, b, x0, M, callback, tol=tol, maxiter=maxiter, residuals=residuals)


def bicgstab(A, b, x0=None, tol=1e-5, restrt=None, maxiter=None, M=None, callback=None, residuals=None):
    """Right-preconditioned BiCGStab (krylov/_bicgstab.py); callback(x) after every iteration.  restrt is ignored."""
    return _run(_bicgstab, A, b, x0, M, callback, tol=tol, maxiter=maxiter, residuals=residuals)


def gmres(A, b, x0=None, tol=1e-5, restrt=None, maxiter=None, M=None, callback=None, residuals=None):
    """Left-preconditioned Householder GMRES (krylov/_gmres_householder.py); callback(normr) per inner iteration."""
    return _run(_gmres, A, b, x0, M, callback, tol=tol, restrt=restrt, maxiter=maxiter, residuals=residuals)


def fgmres(A, b, x0=None, tol=1e-5, restrt=None, maxiter=None, M=None, callback=None, residuals=None):
    """Right-preconditioned flexible Householder GMRES (krylov/_fgmres.py); callback(normr) per inner iteration."""
    return _run(_fgmres, A, b, x0, M, callback, tol=tol, restrt=restrt, maxiter=maxiter, residuals=residuals)


METHODS = {"cg": cg, "bicgstab": bicgstab, "gmres": gmres, "fgmres": fgmres}
