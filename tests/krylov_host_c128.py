"""TEST INFRASTRUCTURE: host restatements of the reference's Krylov methods (pyamg/krylov) on complex128 vectors, each
citing the lines it follows, written against two callables -- `A(v)` (operator) and `M(v)` (preconditioner) -- as
tests/krylov_host.py is for float64.  They are pinned by the histories the reference itself produced
(tests/golden/accel_c128/*.npz, with c128_cycle.HostCycle as M) and then serve as the order-of-operations oracle
for the device implementations on systems no fixture covers.

Every function takes `dot` (the conjugated inner product sum conj(x_i) y_i, numpy's vdot by default) and `norm`, so
that a test can run the same method with another summation order.  -> (x, residuals, info)"""
import numpy as np
import scipy.linalg


def _norm(v):
    return float(np.sqrt(np.sum(v.real * v.real + v.imag * v.imag)))


def mysign(x):
    """krylov/_fgmres.py:16-21"""
    return 1.0 if x == 0.0 else x / abs(x)


def cg(A, M, b, x0, tol, maxiter=None, dot=np.vdot, norm=_norm):
    """krylov/_cg.py:84-183; the history holds the real part of sqrt(<r, M r>)"""
    x = np.array(x0, dtype=np.complex128)
    if maxiter is None:
        maxiter = int(1.3 * len(b)) + 2
    r = b - A(x)
    z = M(r)
    p = z.copy()
    rz = np.complex128(dot(r, z))
    res = [float(np.sqrt(rz).real)]
    normb = norm(b) or 1.0
    if res[0] < tol * normb:
        return x, res, 0
    if res[0] != 0.0:
        tol = tol * res[0]
    it = 0
    while True:
        Ap = A(p)
        rz_old = rz
        pAp = np.complex128(dot(Ap, p))
        if pAp.real < 0.0:
            return x, res, -1
        alpha = rz / pAp
        x += alpha * p
        if (it % 8) and it > 0:
            r -= alpha * Ap
        else:
            r = b - A(x)
        z = M(r)
        rz = np.complex128(dot(r, z))
        if rz.real < 0.0:
            return x, res, -1
        p *= rz / rz_old
        p += z
        it += 1
        res.append(float(np.sqrt(rz).real))
        if res[-1] < tol:
            return x, res, 0
        if rz == 0.0:
            return x, res, -1
        if it == maxiter:
            return x, res, it


def bicgstab(A, M, b, x0, tol, maxiter=None, dot=np.vdot, norm=_norm):
    """krylov/_bicgstab.py:80-167"""
    x = np.array(x0, dtype=np.complex128)
    if maxiter is None:
        maxiter = len(x) + 5
    r = b - A(x)
    res = [norm(r)]
    normb = norm(b) or 1.0
    if res[0] < tol * normb:
        return x, res, 0
    if res[0] != 0.0:
        tol = tol * res[0]
    rstar = r.copy()
    p = r.copy()
    rr_old = np.complex128(dot(rstar, r))
    it = 0
    while True:
        Mp = M(p)
        AMp = A(Mp)
        alpha = rr_old / np.complex128(dot(rstar, AMp))
        s = r - alpha * AMp
        Ms = M(s)
        AMs = A(Ms)
        omega = np.complex128(dot(AMs, s)) / np.complex128(dot(AMs, AMs))
        x = x + alpha * Mp + omega * Ms
        r = s - omega * AMs
        rr_new = np.complex128(dot(rstar, r))
        beta = (rr_new / rr_old) * (alpha / omega)
        rr_old = rr_new
        p = r + beta * (p - omega * AMp)
        it += 1
        res.append(norm(r))
        if res[-1] < tol:
            return x, res, 0
        if it == maxiter:
            return x, res, it


def _limits(n, restrt, maxiter):
    """krylov/_fgmres.py:139-158"""
    if restrt:
        return (maxiter if maxiter else 1), min(int(restrt), n)
    if maxiter is None:
        maxiter = min(n, 40)
    return 1, min(int(maxiter), n)


def _reflect(v, W, js, dot):
    """amg_core/krylov.h:34-53: alpha = <w_j, v>; alpha *= -2; v += alpha w_j"""
    for j in js:
        alpha = np.complex128(dot(W[j], v)) * -2
        v += alpha * W[j]


def _inner_step(v, W, inner, max_inner, n, Q, g, H, norm):
    """krylov/_fgmres.py:250-303 = _gmres_householder.py:254-307: next reflector, Givens rotations, Hessenberg column"""
    if inner != n - 1:
        w = W[inner + 1] if inner < max_inner - 1 else None
        vslice = v[inner + 1:]
        alpha = norm(vslice)
        if alpha != 0:
            alpha = mysign(vslice[0]) * alpha
            if w is not None:
                w[inner + 1:] = vslice
                w[inner + 1] += alpha
                w[:] = w / norm(w)
            v[inner + 1] = -alpha
            v[inner + 2:] = 0.0
    for rot in range(inner):                          # amg_core/krylov.h apply_givens
        t = v[rot]
        v[rot] = Q[4 * rot] * t + Q[4 * rot + 1] * v[rot + 1]
        v[rot + 1] = Q[4 * rot + 2] * t + Q[4 * rot + 3] * v[rot + 1]
    if inner != n - 1 and v[inner + 1] != 0:
        c, s = scipy.linalg.blas.zrotg(v[inner], v[inner + 1])
        Qblock = np.array([[c, s], [-np.conjugate(s), c]], dtype=np.complex128)
        Q[4 * inner:4 * inner + 4] = np.ravel(Qblock)
        g[inner:inner + 2] = np.dot(Qblock, g[inner:inner + 2])
        v[inner] = np.dot(Qblock[0, :], v[inner:inner + 2])
        v[inner + 1] = 0.0
    H[:, inner] = v[0:max_inner]


def _stagnated(update, x):
    idx = x != 0
    return bool(idx.any() and np.max(np.abs(update[idx] / x[idx])) < 1e-12)


def fgmres(A, M, b, x0, tol, restrt=None, maxiter=None, dot=np.vdot, norm=_norm):
    """krylov/_fgmres.py:114-357: right-preconditioned flexible GMRES with Householder reflections"""
    x = np.array(x0, dtype=np.complex128)
    n = len(b)
    max_outer, max_inner = _limits(n, restrt, maxiter)
    r = b - A(x)
    normr = norm(r)
    res = [normr]
    normb = norm(b) or 1.0
    if normr < tol * normb:
        return x, res, 0
    if normr != 0.0:
        tol = tol * normr
    niter = 0
    for outer in range(max_outer):
        w = r
        beta = mysign(w[0]) * normr
        w[0] += beta
        w /= norm(w)
        Q = np.zeros(4 * max_inner, dtype=np.complex128)
        H = np.zeros((max_inner, max_inner), dtype=np.complex128)
        W = np.zeros((max_inner, n), dtype=np.complex128)
        Z = np.zeros((n, max_inner), dtype=np.complex128)
        W[0, :] = w
        g = np.zeros(n, dtype=np.complex128)
        g[0] = -beta
        for inner in range(max_inner):
            v = -2.0 * np.conjugate(W[inner, inner]) * W[inner]
            v[inner] += 1.0
            _reflect(v, W, range(inner - 1, -1, -1), dot)
            v = M(v)
            Z[:, inner] = v
            v = A(v)
            _reflect(v, W, range(0, inner + 1), dot)
            _inner_step(v, W, inner, max_inner, n, Q, g, H, norm)
            if inner < max_inner - 1:
                normr = float(abs(g[inner + 1]))
                if normr < tol:
                    break
                res.append(normr)
            niter += 1
        y = scipy.linalg.solve(H[:inner + 1, :inner + 1], g[:inner + 1])
        update = np.dot(Z[:, :inner + 1], y)
        x = x + update
        r = b - A(x)
        normr = norm(r)
        res.append(normr)
        if _stagnated(update, x):
            return x, res, -1
        if normr < tol:
            return x, res, 0
    return x, res, niter


def gmres(A, M, b, x0, tol, restrt=None, maxiter=None, dot=np.vdot, norm=_norm):
    """krylov/_gmres_householder.py:108-375: left-preconditioned GMRES with Householder reflections"""
    x = np.array(x0, dtype=np.complex128)
    n = len(b)
    max_outer, max_inner = _limits(n, restrt, maxiter)
    r = M(b - A(x))
    normr = norm(r)
    res = [normr]
    normb = norm(b) or 1.0
    if normr < tol * normb:
        return x, res, 0
    if normr != 0.0:
        tol = tol * normr
    niter = 0
    for outer in range(max_outer):
        w = r
        beta = mysign(w[0]) * normr
        w[0] = w[0] + beta
        w[:] = w / norm(w)
        Q = np.zeros(4 * max_inner, dtype=np.complex128)
        H = np.zeros((max_inner, max_inner), dtype=np.complex128)
        W = np.zeros((max_inner + 1, n), dtype=np.complex128)
        W[0, :] = w
        g = np.zeros(n, dtype=np.complex128)
        g[0] = -beta
        for inner in range(max_inner):
            v = -2.0 * np.conjugate(W[inner, inner]) * W[inner]
            v[inner] = v[inner] + 1.0
            _reflect(v, W, range(inner - 1, -1, -1), dot)
            v = M(A(v))
            _reflect(v, W, range(0, inner + 1), dot)
            _inner_step(v, W, inner, max_inner, n, Q, g, H, norm)
            niter += 1
            if inner < max_inner - 1:
                normr = float(abs(g[inner + 1]))
                if normr < tol:
                    break
                res.append(normr)
        y = scipy.linalg.solve(H[:inner + 1, :inner + 1], g[:inner + 1])
        update = np.zeros(n, dtype=np.complex128)
        for j in range(inner, -1, -1):                # amg_core/krylov.h householder_hornerscheme
            update[j] += y[j]
            _reflect(update, W, [j], dot)
        x = x + update
        r = M(b - A(x))
        normr = norm(r)
        res.append(normr)
        if _stagnated(update, x):
            return x, res, -1
        if normr < tol:
            return x, res, 0
    return x, res, niter


METHODS = {"cg": cg, "bicgstab": bicgstab, "gmres": gmres, "fgmres": fgmres}
