"""Smoothed-aggregation setup on the CPU -- the part of
/root/reference/pyamg/aggregation/aggregation.py the BASELINE configurations
use, restated so that a hierarchy can be built where the reference cannot
travel (the GPU box).  The hierarchy is built ONCE on the host and shipped to
HBM by ``multilevel_solver``; nothing here runs inside the cycle.

Supported subset (anything else raises NotImplementedError):
  strength   'symmetric' / ('symmetric', {'theta', 'device'}) | 'evolution' / 'ode' (one candidate, strength.py) | None |
             ('predefined', {'C': csr})
  aggregate  'standard' | 'mis' / ('mis', {'device'}) (MIS(2) aggregation) |
             ('predefined', {'AggOp': csr})
  smooth     ('jacobi', {'omega', 'degree', 'weighting', 'device'}) | ('energy', {'krylov': 'cg', 'maxiter', 'tol',
             'degree', 'weighting': 'local' | 'diagonal', 'device'}) (smooth.py) | None
  device     True | False | None: the device routes of strength, MIS(2) aggregation, fit_candidates and Jacobi
             smoothing on every level
  symmetry   'hermitian' | 'symmetric'
  improve_candidates  relaxation descriptors (run on the device) | None

Arithmetic follows the reference step by step (same scipy sparse products,
same RNG consumption in the spectral-radius estimates), so for a seeded run the
operators match the reference's to rounding -- tests/test_setup_golden.py pins
that against the captured hierarchies.
"""
import ctypes as C
import os
import time

import numpy as np
import scipy.sparse as sparse
from scipy.sparse import bsr_matrix, csr_matrix, isspmatrix_bsr, isspmatrix_csr

from ._host import attempt, dp as _dp, f64 as _f64, host_lib, i32 as _i32, ip as _ip, lp as _lp, outside, route
from .multilevel import multilevel_solver
from .smooth import energy_prolongation_smoother
from .smoothing import change_smoothers
from .util import (approximate_spectral_radius, approximate_spectral_radius_device, get_diagonal,
                   release_device_operator, scale_rows, use_device_for)

__all__ = ["smoothed_aggregation_solver", "standard_aggregation", "mis_aggregation", "fit_candidates",
           "symmetric_strength_of_connection", "jacobi_prolongation_smoother", "energy_prolongation_smoother"]


def greedy_colouring(A):
    """colour of every row of the (symmetrised) pattern of A, first-fit in natural order"""
    M = A if (isspmatrix_csr(A) or isspmatrix_bsr(A)) else csr_matrix(A)
    if isspmatrix_bsr(M) and M.blocksize != (1, 1):
        M = M.tocsr()
    Ap = np.ascontiguousarray(M.indptr, dtype=np.intc)
    Aj = np.ascontiguousarray(M.indices, dtype=np.intc)
    if not host_lib().amgsetup_pattern_symmetric(M.shape[0], _ip(Ap), _ip(Aj)):
        # a colouring must respect both a_ij and a_ji (a structurally symmetric pattern -- the usual case -- needs no
        # symmetrised copy: first-fit only looks at neighbour SETS)
        S = csr_matrix((np.ones(len(M.indices), dtype=np.int8), M.indices, M.indptr), shape=M.shape)
        S = (S + S.T).tocsr()
        Ap = np.ascontiguousarray(S.indptr, dtype=np.intc)
        Aj = np.ascontiguousarray(S.indices, dtype=np.intc)
    colour = np.empty(M.shape[0], dtype=np.intc)
    ncol = host_lib().amgsetup_greedy_coloring(M.shape[0], _ip(Ap), _ip(Aj), _ip(colour))
    return colour, ncol


def unpack_arg(v):
    if isinstance(v, tuple):
        return v[0], v[1]
    return v, {}


def blocksize(A):
    return A.blocksize[0] if isspmatrix_bsr(A) else 1


# --------------------------------------------------------------------------- strength
# What device=None does for each of the three stages of DESIGN.md section 8m when a GPU is present: the host route,
# whatever profiles/r22_sa_stages.txt shows.
SYMMETRIC_STRENGTH_DEVICE_AUTO = False
FIT_CANDIDATES_DEVICE_AUTO = False
JACOBI_DEVICE_AUTO = False


def _finite_f64(what, values):
    """the refusals every float64 device route of section 8m shares, raised before the library is touched"""
    if values.dtype.kind == "c":
        raise outside("%s of complex values on the device" % what)
    if values.dtype != np.float64:
        raise outside("%s of %s values on the device" % (what, values.dtype))
    if not np.isfinite(values).all():
        raise outside("%s of values that are not finite on the device" % what)


def _symmetric_strength_device(A, theta, times=None):
    """amg_symmetric_strength_device and its fetch on a CSR float64 operator.  times: a list that receives (upload, in
    HBM, fetch) in milliseconds."""
    n = A.shape[0]
    if A.shape[0] != A.shape[1]:
        raise outside("symmetric strength of a matrix that is not square on the device")
    nnz = int(A.indptr[-1]) if n else 0
    _finite_f64("symmetric strength", A.data[:nnz])
    if nnz >= 2 ** 31:
        raise outside("symmetric strength of 2^31 entries or more on the device")
    from . import _lib
    L = _lib.lib()
    Ap, Aj, Ax = _i32(A.indptr), _i32(A.indices), _f64(A.data)
    Sp = np.empty(n + 1, dtype=np.intc)
    handle = C.c_void_p()
    ms = (C.c_double * 3)()
    _lib.check(L.amg_symmetric_strength_device(n, Ap.ctypes.data, Aj.ctypes.data, Ax.ctypes.data, float(theta), Sp.ctypes.data,
                                               C.byref(handle), ms))
    kept = int(Sp[-1])
    (Sj, Sx), _ = _lib.fetch_result(handle, L.amg_symmetric_strength_fetch, [(kept, np.intc), (kept, np.float64)], ms)
    if times is not None:
        times.extend([ms[0], ms[1], ms[2]])
    return csr_matrix((Sx, Sj.astype(A.indices.dtype, copy=False), Sp.astype(A.indptr.dtype, copy=False)), shape=A.shape)


def _symmetric_strength_host(A, theta):
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    isdiag = rows == A.indices
    if A.dtype.kind == "c":
        d = np.zeros(n, dtype=A.dtype)
        np.add.at(d, rows[isdiag], A.data[isdiag])
        diags = np.sqrt(d.real * d.real + d.imag * d.imag)
        normsq = A.data.real * A.data.real + A.data.imag * A.data.imag
    else:
        d = np.zeros(n)
        np.add.at(d, rows[isdiag], A.data[isdiag])
        diags = np.abs(d)
        normsq = A.data * A.data
    eps = (theta * theta) * diags
    keep = isdiag | (normsq >= eps[rows] * diags[A.indices])
    Sp = np.concatenate(([0], np.cumsum(np.bincount(rows[keep], minlength=n)))).astype(A.indptr.dtype)
    return _magnitudes_by_largest(csr_matrix((A.data[keep], A.indices[keep], Sp), shape=A.shape))


def _magnitudes_by_largest(S):
    S.data = np.abs(S.data)
    # scale_rows_by_largest_entry (util/utils.py)
    largest = np.maximum.reduceat(S.data, S.indptr[:-1][np.diff(S.indptr) > 0]) if S.nnz else np.array([])
    scale = np.ones(S.shape[0])
    scale[np.diff(S.indptr) > 0] = largest
    scale[scale == 0] = 1.0
    S.data = S.data / np.repeat(scale, np.diff(S.indptr))
    return S


def symmetric_strength_of_connection(A, theta=0, device=None, times=None):
    """pyamg/strength.py:213-318, amg_core/smoothed_aggregation.h:49-99:
    keep a_ij with |a_ij|^2 >= theta^2 |a_ii| |a_jj| (the diagonal always), take
    magnitudes and scale each row by its largest entry.  Complex operators: the
    diagonal is summed as a complex number, |d| = sqrt(re^2 + im^2) (linalg.h mynorm)
    and |a_ij|^2 = re^2 + im^2 (mynormsq).

    device : True = the device route (CSR, real float64, finite values), False or None = the host
    route (None: the device route where SYMMETRIC_STRENGTH_DEVICE_AUTO and a GPU).  A BSR operator with theta != 0
    is reduced to its block norms on the host and handed on as CSR; with theta == 0 it stays on the host.
    times : a list that receives the device route's (upload, in HBM, fetch) milliseconds."""
    if theta < 0:
        raise ValueError("expected a positive theta")
    if isspmatrix_csr(A):
        A = csr_matrix(A)
        return attempt(route(device, SYMMETRIC_STRENGTH_DEVICE_AUTO), lambda: _symmetric_strength_device(A, theta, times),
                       lambda: _symmetric_strength_host(A, theta))
    if isspmatrix_bsr(A):
        M, N = A.shape
        R, Cb = A.blocksize
        if R != Cb:
            raise ValueError("matrix must have square blocks")
        if theta == 0:
            data = np.ones(len(A.indices), dtype=A.dtype)
            return _magnitudes_by_largest(csr_matrix((data, A.indices.copy(), A.indptr.copy()), shape=(int(M / R), int(N / Cb))))
        data = (np.conjugate(A.data) * A.data).reshape(-1, R * Cb).sum(axis=1)
        Ab = csr_matrix((data, A.indices, A.indptr), shape=(int(M / R), int(N / Cb)))
        return symmetric_strength_of_connection(Ab, theta, device, times)
    raise TypeError("expected csr_matrix or bsr_matrix")


# --------------------------------------------------------------------------- aggregation
def standard_aggregation(Cm):
    """pyamg/aggregation/aggregate.py:20-105 -> (AggOp, Cpts)"""
    if not isspmatrix_csr(Cm):
        raise TypeError("expected csr_matrix")
    if Cm.shape[0] != Cm.shape[1]:
        raise ValueError("expected square matrix")
    num_rows = Cm.shape[0]
    Ap = np.ascontiguousarray(Cm.indptr, dtype=np.intc)
    Aj = np.ascontiguousarray(Cm.indices, dtype=np.intc)
    Tj = np.empty(num_rows, dtype=np.intc)
    Cpts = np.empty(num_rows, dtype=np.intc)
    num_aggregates = host_lib().amgsetup_standard_aggregation(num_rows, _ip(Ap), _ip(Aj), _ip(Tj), _ip(Cpts))
    Cpts = Cpts[:num_aggregates]
    if num_aggregates == 0:
        return csr_matrix((num_rows, 1), dtype="int8"), np.array([], dtype=np.intc)
    shape = (num_rows, num_aggregates)
    if Tj.min() == -1:
        mask = Tj != -1
        row = np.arange(num_rows, dtype=np.intc)[mask]
        col = Tj[mask]
        data = np.ones(len(col), dtype="int8")
        return sparse.coo_matrix((data, (row, col)), shape=shape).tocsr(), Cpts
    Tp = np.arange(num_rows + 1, dtype=np.intc)
    Tx = np.ones(len(Tj), dtype="int8")
    return csr_matrix((Tx, Tj, Tp), shape=shape), Cpts


# What device=None does for mis_aggregation when a GPU is present: the host route, whatever the measurement in
# profiles/r21_mis_aggregation.txt shows.
MIS_DEVICE_AUTO = False


def _mis_aggregation_device(n, Ap, Aj, y, agg, cpts, times=None):
    """amg_mis_aggregation_device; agg and cpts (int32, n each) are written.  Returns (aggregates, rounds of the set).
    times: a list that receives (upload, rounds, fetch) in milliseconds."""
    from . import _lib
    from .graph import _finite_weights
    _finite_weights(y)
    n_agg, rounds = C.c_int(0), C.c_int(0)
    ms = (C.c_double * 3)()
    _lib.check(_lib.lib().amg_mis_aggregation_device(n, Ap.ctypes.data, Aj.ctypes.data, y.ctypes.data, agg.ctypes.data,
                                                     cpts.ctypes.data, C.byref(n_agg), C.byref(rounds), ms))
    if times is not None:
        times.extend([ms[0], ms[1], ms[2]])
    return n_agg.value, rounds.value


def _mis_aggregation_host(n, Ap, Aj, y, agg, cpts):
    from .graph import _no_end
    rounds = C.c_int(0)
    n_agg = _no_end(host_lib().amgsetup_mis_aggregation(n, _ip(Ap), _ip(Aj), _dp(y), _ip(agg), _ip(cpts), C.byref(rounds)))
    return n_agg, rounds.value


def mis_aggregation(Cm, y=None, device=None, times=None, rounds=None):
    """MIS(2) aggregation -> (AggOp, Cpts), shaped and typed as standard_aggregation's.

    Cm : square csr_matrix with a structurally symmetric pattern (ValueError otherwise); only the pattern is read.
    y : one weight per vertex, None draws np.random.rand(n).  The roots are the members of the distance-2 independent
    set on y that have an off-diagonal entry; a vertex next to a root joins it, and a vertex still unassigned joins,
    among the aggregates of its neighbours, the one whose root has the largest (y[root], root).  Vertices without
    off-diagonal entries get a zero row.
    device : True = the device route (finite weights only), False or None = the host route (None: the device route
    where MIS_DEVICE_AUTO and a GPU).
    times, rounds : lists that receive the device route's (upload, rounds, fetch) milliseconds and the rounds of the
    set."""
    if not isspmatrix_csr(Cm):
        raise TypeError("expected csr_matrix")
    if Cm.shape[0] != Cm.shape[1]:
        raise ValueError("expected square matrix")
    n = Cm.shape[0]
    Ap, Aj = _i32(Cm.indptr), _i32(Cm.indices)
    if n and not host_lib().amgsetup_pattern_symmetric(n, _ip(Ap), _ip(Aj)):
        raise ValueError("expected a structurally symmetric pattern")
    y = _f64(np.random.rand(n) if y is None else y)
    if y.shape != (n,):
        raise ValueError("expected one weight per vertex")
    agg = np.empty(n, dtype=np.intc)
    Cpts = np.empty(n, dtype=np.intc)
    n_agg, ran = 0, 0
    if n:
        n_agg, ran = attempt(route(device, MIS_DEVICE_AUTO), lambda: _mis_aggregation_device(n, Ap, Aj, y, agg, Cpts, times),
                             lambda: _mis_aggregation_host(n, Ap, Aj, y, agg, Cpts))
    if rounds is not None:
        rounds.append(ran)
    Cpts = Cpts[:n_agg].copy()
    if n_agg == 0:
        return csr_matrix((n, 1), dtype="int8"), Cpts
    mask = agg != -1
    Tp = np.concatenate(([0], np.cumsum(mask))).astype(np.intc)
    return csr_matrix((np.ones(Tp[-1], dtype="int8"), agg[mask], Tp), shape=(n, n_agg)), Cpts


# --------------------------------------------------------------------------- tentative prolongator
def _fit_candidates_device(AggOp, B, tol, times=None):
    """amg_fit_candidates_device: T in the layout Q.T.tobsr() has on the host route (the offsets and columns of AggOp, node
    i's K1 x K2 block) and B_coarse.  times: a list that receives (upload, in HBM, fetch) in milliseconds."""
    _finite_f64("fit_candidates", B)
    N_fine, N_coarse = AggOp.shape
    K1, K2 = int(B.shape[0] / N_fine), B.shape[1]
    if K2 < 1:
        raise outside("fit_candidates without candidates on the device")
    if N_fine and np.diff(AggOp.indptr).max() > 1:
        raise outside("fit_candidates with a node in more than one aggregate on the device")
    if AggOp.indptr.dtype != np.intc or AggOp.indices.dtype != np.intc:
        raise outside("fit_candidates of an AggOp without 32-bit indices on the device")     # (T carries AggOp's arrays)
    Tp, Tj = np.array(AggOp.indptr, dtype=np.intc), np.array(AggOp.indices[:AggOp.indptr[-1]], dtype=np.intc)
    if len(Tj) and (Tj.min() < 0 or Tj.max() >= N_coarse):
        raise ValueError("AggOp holds a column outside the matrix")
    from . import _lib
    Bc = _f64(B)
    Tx = np.empty((len(Tj), K1, K2), dtype=np.float64)
    R = np.zeros((N_coarse, K2, K2), dtype=np.float64)
    ms = (C.c_double * 3)()
    _lib.check(_lib.lib().amg_fit_candidates_device(N_fine, N_coarse, K1, K2, Tp.ctypes.data, Tj.ctypes.data, Bc.ctypes.data,
                                                    float(tol), Tx.ctypes.data, R.ctypes.data, ms))
    if times is not None:
        times.extend([ms[0], ms[1], ms[2]])
    return bsr_matrix((Tx, Tj, Tp), shape=(K1 * N_fine, K2 * N_coarse), blocksize=(K1, K2)), R.reshape(-1, K2)


def fit_candidates(AggOp, B, tol=1e-10, device=None, times=None):
    """pyamg/aggregation/tentative.py:19-166 / amg_core/smoothed_aggregation.h:323-500:
    per aggregate, modified Gram-Schmidt QR of the candidates restricted to it.

    device : True = the device route (float64 candidates with finite values, any K1 and K2, at most
    one aggregate per node), False or None = the host route (None: the device route where FIT_CANDIDATES_DEVICE_AUTO and
    a GPU).  times : a list that receives the device route's (upload, in HBM, fetch) milliseconds."""
    if not isspmatrix_csr(AggOp):
        raise TypeError("expected csr_matrix for argument AggOp")
    B = np.asarray(B)
    if B.dtype.kind == "c":
        B = np.asarray(B, dtype=np.complex128)
    elif B.dtype not in ["float32", "float64"]:
        B = np.asarray(B, dtype="float64")
    if len(B.shape) != 2:
        raise ValueError("expected 2d array for argument B")
    if B.shape[0] % AggOp.shape[0] != 0:
        raise ValueError("dimensions of AggOp %s and B %s are incompatible" % (AggOp.shape, B.shape))
    return attempt(route(device, FIT_CANDIDATES_DEVICE_AUTO), lambda: _fit_candidates_device(AggOp, B, tol, times),
                   lambda: _fit_candidates_host(AggOp, B, tol))


def _fit_candidates_host(AggOp, B, tol):
    N_fine, N_coarse = AggOp.shape
    K1 = int(B.shape[0] / N_fine)
    K2 = B.shape[1]
    AggOp_csc = AggOp.tocsc()
    Ap, Ai = AggOp_csc.indptr, AggOp_csc.indices
    nnz = AggOp.nnz
    BS = K1 * K2
    Bb = B.reshape(-1, K1, K2)
    # copy blocks: Qx[ii] = B block of fine node Ai[ii]   (smoothed_aggregation.h:341-351)
    Qx, R = _aggregate_qr(Bb[Ai], Ap, N_coarse, K1, K2, tol)
    Q = bsr_matrix((Qx.swapaxes(1, 2).copy(), Ai, Ap), shape=(K2 * N_coarse, K1 * N_fine))
    Q = Q.T.tobsr()
    R = R.reshape(-1, K2)
    return Q, R


def _aggregate_qr(Qx, Ap, N_coarse, K1, K2, tol):
    """Per-aggregate modified Gram-Schmidt of the candidate blocks Qx (one K1 x K2 block per member, members of
    aggregate j at Ap[j]:Ap[j+1]) -> (Q blocks, R (N_coarse, K2, K2)); smoothed_aggregation.h:341-452."""
    if np.asarray(Qx).dtype.kind == "c":
        return _aggregate_qr_c128(Qx, Ap, N_coarse, K1, K2, tol)
    Qx = np.array(Qx, dtype=np.float64)
    nnz = Qx.shape[0]
    R = np.zeros((N_coarse, K2, K2), dtype=np.float64)
    if K1 == 1 and K2 == 1:
        # scalar fast path (one candidate, scalar unknowns)
        q = np.empty(nnz, dtype=np.float64)
        Rv = np.zeros(N_coarse, dtype=np.float64)
        Bv = np.ascontiguousarray(Qx.ravel(), dtype=np.float64)
        Ap32 = np.ascontiguousarray(Ap, dtype=np.intc)
        Ai32 = np.arange(nnz, dtype=np.intc)
        host_lib().amgsetup_fit_candidates_scalar(N_coarse, _ip(Ap32), _ip(Ai32), _dp(Bv), _dp(q), _dp(Rv),
                                                  float(tol))
        R[:, 0, 0] = Rv
        return q.reshape(-1, 1, 1), R
    # general case: modified Gram-Schmidt per aggregate, batched over the aggregates that have the
    # same number of members; every sum runs over the rows in storage order, one row at a time,
    # exactly as the reference's scalar loops do (smoothed_aggregation.h:367-452)
    counts = np.diff(Ap)
    for m in np.unique(counts):
        if m == 0:
            continue
        aggs = np.nonzero(counts == m)[0]
        pos = (np.asarray(Ap)[aggs][:, None] + np.arange(m)[None, :]).astype(np.int64)      # (ng, m)
        blk = Qx[pos].reshape(len(aggs), m * K1, K2).copy()
        nrow = m * K1
        for bj in range(K2):
            norm_j = np.zeros(len(aggs))
            for rr in range(nrow):
                norm_j = norm_j + blk[:, rr, bj] * blk[:, rr, bj]
            norm_j = np.sqrt(norm_j)
            threshold_j = tol * norm_j
            for bi in range(bj):
                dot_prod = np.zeros(len(aggs))
                for rr in range(nrow):
                    dot_prod = dot_prod + blk[:, rr, bi] * blk[:, rr, bj]
                blk[:, :, bj] = blk[:, :, bj] - dot_prod[:, None] * blk[:, :, bi]
                R[aggs, bi, bj] = dot_prod
            norm_j = np.zeros(len(aggs))
            for rr in range(nrow):
                norm_j = norm_j + blk[:, rr, bj] * blk[:, rr, bj]
            norm_j = np.sqrt(norm_j)
            ok = norm_j > threshold_j
            scale = np.zeros(len(aggs))
            scale[ok] = 1.0 / norm_j[ok]
            R[aggs, bj, bj] = np.where(ok, norm_j, 0.0)
            blk[:, :, bj] = blk[:, :, bj] * scale[:, None]
        Qx[pos] = blk.reshape(len(aggs), m, K1, K2)
    return Qx, R


def _aggregate_qr_c128(Qx, Ap, N_coarse, K1, K2, tol):
    """_aggregate_qr for complex128 candidates (fit_candidates_complex, smoothed_aggregation.h:322-470), batched over
    the aggregates of equal size, real and imaginary parts in arrays of their own so that every operation is one
    correctly rounded real ufunc call:
      norm      sum over the rows of re*re + im*im (complex_norm), a real sum from zero
      dot       sum over the rows of conj(q_bi) * q_bj (complex_dot conjugates its SECOND argument, the column bi
                that is already orthonormal), a complex sum from zero
      update    q_bj -= dot * q_bi, then q_bj *= (1/norm + 0i), both full complex products."""
    Qx = np.array(Qx, dtype=np.complex128)
    R = np.zeros((N_coarse, K2, K2), dtype=np.complex128)
    counts = np.diff(Ap)

    def cmul(ar, ai, br, bi):
        return ar * br - ai * bi, ar * bi + ai * br

    for m in np.unique(counts):
        if m == 0:
            continue
        aggs = np.nonzero(counts == m)[0]
        pos = (np.asarray(Ap)[aggs][:, None] + np.arange(m)[None, :]).astype(np.int64)      # (ng, m)
        blk = Qx[pos].reshape(len(aggs), m * K1, K2)
        br, bi_ = np.ascontiguousarray(blk.real), np.ascontiguousarray(blk.imag)
        nrow = m * K1

        def colnorm(bj):
            acc = np.zeros(len(aggs))
            for rr in range(nrow):
                acc = acc + (br[:, rr, bj] * br[:, rr, bj] + bi_[:, rr, bj] * bi_[:, rr, bj])
            return np.sqrt(acc)

        for bj in range(K2):
            threshold_j = tol * colnorm(bj)
            for b2 in range(bj):
                dr, di = np.zeros(len(aggs)), np.zeros(len(aggs))
                for rr in range(nrow):
                    pr, pi = cmul(br[:, rr, b2], -bi_[:, rr, b2], br[:, rr, bj], bi_[:, rr, bj])
                    dr = dr + pr
                    di = di + pi
                pr, pi = cmul(dr[:, None], di[:, None], br[:, :, b2], bi_[:, :, b2])
                br[:, :, bj] = br[:, :, bj] - pr
                bi_[:, :, bj] = bi_[:, :, bj] - pi
                R.real[aggs, b2, bj] = dr
                R.imag[aggs, b2, bj] = di
            norm_j = colnorm(bj)
            ok = norm_j > threshold_j
            scale = np.zeros(len(aggs))
            scale[ok] = 1.0 / norm_j[ok]
            R[aggs, bj, bj] = np.where(ok, norm_j, 0.0)
            pr, pi = cmul(br[:, :, bj], bi_[:, :, bj], scale[:, None], np.zeros((len(aggs), 1)))
            br[:, :, bj] = pr
            bi_[:, :, bj] = pi
        out = np.empty(blk.shape, dtype=np.complex128)
        out.real, out.imag = br, bi_
        Qx[pos] = out.reshape(len(aggs), m, K1, K2)
    return Qx, R


# --------------------------------------------------------------------------- prolongation smoothing
def _jacobi_weights(S, omega, weighting):
    """(D^-1 S, w) of the smoothing step P - (w * D^-1 S) P, and D^-1 as the vector that scaled the rows: everything
    that both routes share, the in-place sort of S by get_diagonal and the one np.random draw of the spectral radius
    included"""
    if weighting == "diagonal":
        D_inv = get_diagonal(S, inv=True)
        D_inv_S = scale_rows(S, D_inv, copy=True)
        return D_inv_S, omega / approximate_spectral_radius(D_inv_S), D_inv
    D = np.abs(S) * np.ones((S.shape[0], 1), dtype=S.dtype)
    D_inv = np.zeros_like(D)
    D_inv[D != 0] = 1.0 / np.abs(D[D != 0])
    return scale_rows(S, D_inv, copy=True), omega, D_inv


def _scalar_blocks(M):
    return isspmatrix_csr(M) or (isspmatrix_bsr(M) and M.blocksize == (1, 1))


def _jacobi_device_refusals(S, T, B, filter, weighting):
    """what puts a call outside the device route of jacobi_prolongation_smoother, raised before the library is touched
    and before anything is drawn or sorted"""
    what = "Jacobi prolongation smoothing"
    if filter:
        raise outside("filtered prolongation smoothing")
    if weighting not in ("diagonal", "local", "block"):
        raise outside("weighting=%r" % (weighting,))
    for M in (S, T):
        if not (isspmatrix_csr(M) or isspmatrix_bsr(M)):
            raise outside("%s of operands that are neither CSR nor BSR on the device" % what)
        if np.dtype(M.dtype).kind == "c":
            raise outside("%s of complex operators on the device" % what)
        if not _scalar_blocks(M):
            raise outside("%s with blocks larger than 1 x 1 on the device" % what)
        if M.dtype != np.float64 or M.indptr.dtype != np.intc or M.indices.dtype != np.intc:
            raise outside("%s of operands other than float64 with 32-bit indices on the device" % what)
    if B is not None and np.ndim(B) == 2 and np.shape(B)[1] > 1:
        raise outside("%s with more than one candidate on the device" % what)
    if S.shape[0] != S.shape[1] or S.shape[1] != T.shape[0]:
        raise ValueError("dimensions of S %s and T %s are incompatible" % (S.shape, T.shape))
    if not _columns_once(T):
        raise outside("%s of a prolongator with a column twice in a row on the device" % what)


def _jacobi_device(S, T, D_inv, w, degree, times=None):
    """amg_jacobi_prolongation_device and its fetch: the smoothed prolongator in T's format.  times: a list that receives
    (upload, in HBM, fetch) in milliseconds."""
    from . import _lib
    L = _lib.lib()
    n, nc = T.shape
    Sp, Sj, Sx = _i32(S.indptr), _i32(S.indices), _f64(np.ravel(S.data))
    Tp, Tj, Tx = _i32(T.indptr), _i32(T.indices), _f64(np.ravel(T.data))
    dinv = _f64(np.ravel(D_inv))
    Pp = np.empty(n + 1, dtype=np.intc)
    handle = C.c_void_p()
    ms = (C.c_double * 3)()
    _lib.check(L.amg_jacobi_prolongation_device(n, nc, Sp.ctypes.data, Sj.ctypes.data, Sx.ctypes.data, dinv.ctypes.data, float(w),
                                                int(degree), Tp.ctypes.data, Tj.ctypes.data, Tx.ctypes.data, Pp.ctypes.data,
                                                C.byref(handle), ms))
    nnz = int(Pp[-1])
    (Pj, Px), _ = _lib.fetch_result(handle, L.amg_jacobi_prolongation_fetch, [(nnz, np.intc), (nnz, np.float64)], ms)
    if times is not None:
        times.extend([ms[0], ms[1], ms[2]])
    if isspmatrix_bsr(T):
        return bsr_matrix((Px.reshape(-1, 1, 1), Pj, Pp), shape=T.shape)
    return csr_matrix((Px, Pj, Pp), shape=T.shape)


def jacobi_prolongation_smoother(S, T, Cm, B, omega=4.0 / 3.0, degree=1, filter=False,
                                 weighting="diagonal", device=None, times=None, weights=None):
    """pyamg/aggregation/smooth.py:67-210 (weighting 'diagonal' / 'local', no filtering).

    device : True = the device route (real float64 S and T with 1 x 1 blocks, one candidate, no
    filtering; the diagonal, the spectral radius and the row sums of 'local' stay on the host, the weights, the products
    and the differences run in HBM), False or None = the host route (None: the device route where JACOBI_DEVICE_AUTO
    and a GPU).  times : a list that receives the device route's (upload, in HBM, fetch) milliseconds.
    weights : what _jacobi_weights(S, omega, weighting) returned to a caller that has already sorted S and drawn for
    it (the resident chain, which hands a level it could not finish on); nothing is sorted or drawn again."""
    way = route(device, JACOBI_DEVICE_AUTO)
    if way is not False:
        try:
            _jacobi_device_refusals(S, T, B, filter, weighting)
        except NotImplementedError:
            if way is True:
                raise
            way = False
    if filter:
        raise NotImplementedError("filtered prolongation smoothing is outside the restated setup")
    if weighting == "block":
        if isspmatrix_csr(S) or (isspmatrix_bsr(S) and S.blocksize[0] == 1):
            weighting = "diagonal"
    if weighting not in ("diagonal", "local"):
        raise NotImplementedError("weighting=%r" % weighting)
    D_inv_S, w, D_inv = _jacobi_weights(S, omega, weighting) if weights is None else weights
    if degree <= 0:
        return T                        # (after the weights, as ever: S is sorted and the estimate has drawn)

    def on_host():
        W = w * D_inv_S
        P = T
        for i in range(degree):
            P = P - (W * P)
        return P
    # (a refusal of the library comes after the weights, so the host route that answers it draws nothing again)
    return attempt(way, lambda: _jacobi_device(S, T, D_inv, w, degree, times), on_host)


# --------------------------------------------------------------------------- driver
def _levelize_sa(to_levelize, max_levels, max_coarse):
    """util/utils.py:1872-1953"""
    if isinstance(to_levelize, tuple):
        if to_levelize[0] == "predefined":
            to_levelize = [to_levelize]
            max_levels = 2
            max_coarse = 0
        else:
            to_levelize = [to_levelize for i in range(max_levels - 1)]
    elif isinstance(to_levelize, str):
        if to_levelize == "predefined":
            raise ValueError("predefined to_levelize requires a user-provided CSR matrix")
        to_levelize = [to_levelize for i in range(max_levels - 1)]
    elif isinstance(to_levelize, list):
        if isinstance(to_levelize[-1], tuple) and (to_levelize[-1][0] == "predefined"):
            max_levels = len(to_levelize) + 1
            max_coarse = 0
        elif len(to_levelize) < max_levels - 1:
            to_levelize = to_levelize + [to_levelize[-1]] * (max_levels - 1 - len(to_levelize))
    elif to_levelize is None:
        to_levelize = [(None, {}) for i in range(max_levels - 1)]
    else:
        raise ValueError("invalid to_levelize")
    return max_levels, max_coarse, to_levelize


def _levelize_smooth(to_levelize, max_levels):
    """util/utils.py:1956-2006"""
    if isinstance(to_levelize, tuple) or isinstance(to_levelize, str):
        return [to_levelize for i in range(max_levels)]
    if isinstance(to_levelize, list):
        if len(to_levelize) < max_levels:
            return to_levelize + [to_levelize[-1]] * (max_levels - len(to_levelize))
        return list(to_levelize)
    if to_levelize is None:
        return [(None, {}) for i in range(max_levels)]
    return to_levelize


def _improve(method, A, B):
    """relaxation_as_linear_operator(method, A, 0) * B  (util/utils.py:1129-1204,
    aggregation.py:313-320): relax A x = 0 from each candidate column.  Setup runs on
    the CPU: Gauss-Seidel sweeps use the host restatement of relaxation.h:34-62."""
    if A.dtype.kind == "c":
        return _improve_c128(method, A, B)
    from . import smoothing
    fn, kwargs = unpack_arg(method)
    lvl = multilevel_solver.level()
    lvl.A = A
    desc = getattr(smoothing, "setup_" + str(fn))(lvl, **kwargs).desc
    n = A.shape[0]
    b = np.zeros(n)
    out = np.empty_like(B)
    L = host_lib()
    its = int(desc.get("iterations", 1))
    sw = desc.get("sweep", "forward")
    if desc["name"] == "gauss_seidel" and (isspmatrix_csr(A) or A.blocksize == (1, 1)):
        if isspmatrix_bsr(A):
            raise NotImplementedError("candidate improvement on BSR(1,1) levels")
        Ap = np.ascontiguousarray(A.indptr, dtype=np.intc)
        Aj = np.ascontiguousarray(A.indices, dtype=np.intc)
        Ax = np.ascontiguousarray(A.data, dtype=np.float64)

        def sweep(x, reverse):
            if reverse:
                L.amgsetup_gauss_seidel(_ip(Ap), _ip(Aj), _dp(Ax), _dp(x), _dp(b), n - 1, -1, -1)
            else:
                L.amgsetup_gauss_seidel(_ip(Ap), _ip(Aj), _dp(Ax), _dp(x), _dp(b), 0, n, 1)
    elif desc["name"] == "block_gauss_seidel":
        bs = int(desc["blocksize"])
        Ab = A.tobsr(blocksize=(bs, bs))                      # relaxation.py:563
        Ap = np.ascontiguousarray(Ab.indptr, dtype=np.intc)
        Aj = np.ascontiguousarray(Ab.indices, dtype=np.intc)
        Ax = np.ascontiguousarray(np.ravel(Ab.data), dtype=np.float64)
        Dinv = np.ascontiguousarray(np.ravel(desc["Dinv"]), dtype=np.float64)
        nb = n // bs

        def sweep(x, reverse):
            if reverse:
                L.amgsetup_block_gauss_seidel(_ip(Ap), _ip(Aj), _dp(Ax), _dp(x), _dp(b), _dp(Dinv), nb - 1, -1, -1, bs)
            else:
                L.amgsetup_block_gauss_seidel(_ip(Ap), _ip(Aj), _dp(Ax), _dp(x), _dp(b), _dp(Dinv), 0, nb, 1, bs)
    else:
        raise NotImplementedError("improve_candidates=%r on this matrix is outside the restated setup" % (fn,))
    sweep_code = {"forward": 0, "backward": 1, "symmetric": 2}.get(sw)

    def relax_column(j, pipelined_ok=False):
        x = np.array(B[:, j], dtype=np.float64, order="C")
        ran = 0
        if pipelined_ok and sweep_code is not None:
            # all sweeps of this column by several host threads that trail each other chunk by chunk
            # (setup_host.cpp: pipelined_sweep) -- the sequential result; 0 = the operator does not qualify
            if desc["name"] == "gauss_seidel":
                ran = L.amgsetup_gauss_seidel_pipelined(_ip(Ap), _ip(Aj), _dp(Ax), _dp(x), _dp(b), n, sweep_code, its)
            else:
                ran = L.amgsetup_block_gauss_seidel_pipelined(_ip(Ap), _ip(Aj), _dp(Ax), _dp(x), _dp(b), _dp(Dinv),
                                                              nb, bs, sweep_code, its)
        if not ran:
            for it in range(its):
                if sw in ("forward", "symmetric"):
                    sweep(x, False)
                if sw in ("backward", "symmetric"):
                    sweep(x, True)
        out[:, j] = x
        return ran

    if desc["name"] == "gauss_seidel" and sweep_code is not None and use_device_for(A) \
            and os.environ.get("AMG_SETUP_DEVICE_GS", "1") != "0":
        # r3: the sweeps on the GPU, in the operator's own row order from its CSR arrays (csrc/gsflow.hip: gs_natural_kernel;
        # the operator is in HBM for the spectral-radius estimate anyway) -- the sequential result bit for bit.  Operators
        # with rows of more than 8 entries (coarse levels) keep the host sweeps below.
        from . import _lib
        from .util import device_operator
        dirs = bytes(({0: [0], 1: [1], 2: [0, 1]}[sweep_code]) * its)
        op = device_operator(A)
        cols = []
        for j in range(B.shape[1]):
            x = np.array(B[:, j], dtype=np.float64, order="C")
            rc = _lib.lib().amg_hier_gs_natural(op.h, 0, x.ctypes.data, None, dirs, len(dirs))
            if rc != 0:
                cols = None
                if rc != _lib.AMG_ENOTIMPL:
                    # e.g. the persistent kernel gave up waiting because another process holds part of the GPU: the host
                    # sweeps below produce the same numbers (x is only written on success)
                    import warnings
                    warnings.warn("candidate improvement on the GPU failed (%s); using the host sweeps"
                                  % _lib.lib().amg_last_error().decode(), RuntimeWarning)
                break
            cols.append(x)
        if cols is not None:
            for j, x in enumerate(cols):
                out[:, j] = x
            return out
    if n > 100000 and os.environ.get("AMG_SETUP_PIPELINED_GS", "1") != "0":
        # first column through the pipelined sweep; if the operator qualifies, so do the others
        if relax_column(0, True):
            for j in range(1, B.shape[1]):
                relax_column(j, True)
            return out
        first = 1
    else:
        first = 0
    if first >= B.shape[1]:
        return out
    if B.shape[1] - first > 1 and n > 100000:
        # the candidates are relaxed independently (each sweep is sequential): one host thread per column
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(B.shape[1], 8)) as pool:
            list(pool.map(relax_column, range(first, B.shape[1])))
    else:
        for j in range(first, B.shape[1]):
            relax_column(j)
    return out


def _improve_c128(method, A, B):
    """_improve for a complex128 operator: the sequential sweeps of csrc/setup_host.cpp on scalar.hpp arithmetic
    (amgsetup_gauss_seidel_c128 / amgsetup_block_gauss_seidel_c128); at or above util.DEVICE_RHO_MIN_ROWS with a
    device present, the complex128 entries of the flat table (pyamg_amd.relaxation), which give the same bits."""
    from . import smoothing, util
    fn, kwargs = unpack_arg(method)
    lvl = multilevel_solver.level()
    lvl.A = A
    desc = getattr(smoothing, "setup_" + str(fn))(lvl, **kwargs).desc
    n = A.shape[0]
    its = int(desc.get("iterations", 1))
    sw = desc.get("sweep", "forward")
    if sw not in ("forward", "backward", "symmetric"):
        raise ValueError("valid sweep directions are 'forward', 'backward', and 'symmetric'")
    b = np.zeros(n, dtype=np.complex128)
    out = np.empty((n, B.shape[1]), dtype=np.complex128)
    L = host_lib()
    if desc["name"] == "gauss_seidel" and isspmatrix_csr(A):
        bs, Dinv, M = 1, None, A
    elif desc["name"] == "block_gauss_seidel":
        bs = int(desc["blocksize"])
        M = A.tobsr(blocksize=(bs, bs))                       # relaxation.py:563
        Dinv = np.ascontiguousarray(np.ravel(desc["Dinv"]), dtype=np.complex128)
    else:
        raise NotImplementedError("improve_candidates=%r on this matrix is outside the restated setup" % (fn,))
    from . import _lib
    on_device = n >= util.DEVICE_RHO_MIN_ROWS and os.environ.get("AMG_SETUP_DEVICE_GS", "1") != "0" \
        and _lib.device_count() > 0
    Ap = np.ascontiguousarray(M.indptr, dtype=np.intc)
    Aj = np.ascontiguousarray(M.indices, dtype=np.intc)
    Ax = np.ascontiguousarray(np.ravel(M.data), dtype=np.complex128)
    nb = n // bs
    for j in range(B.shape[1]):
        x = np.array(B[:, j], dtype=np.complex128, order="C")
        if on_device:
            from . import relaxation
            if Dinv is None:
                relaxation.gauss_seidel(M, x, b, iterations=its, sweep=sw)
            else:
                relaxation.block_gauss_seidel(M, x, b, iterations=its, sweep=sw, blocksize=bs,
                                              Dinv=np.asarray(desc["Dinv"], dtype=np.complex128).reshape(-1, bs, bs))
        else:
            for it in range(its):
                for rng in ([(0, nb, 1)] if sw == "forward" else [(nb - 1, -1, -1)] if sw == "backward"
                            else [(0, nb, 1), (nb - 1, -1, -1)]):
                    if Dinv is None:
                        L.amgsetup_gauss_seidel_c128(_ip(Ap), _ip(Aj), Ax.ctypes.data, x.ctypes.data, b.ctypes.data, *rng)
                    else:
                        L.amgsetup_block_gauss_seidel_c128(_ip(Ap), _ip(Aj), Ax.ctypes.data, x.ctypes.data, b.ctypes.data,
                                                           Dinv.ctypes.data, rng[0], rng[1], rng[2], bs)
        out[:, j] = x
    return out


def smoothed_aggregation_solver(A, B=None, BH=None, symmetry="hermitian", strength="symmetric",
                                aggregate="standard", smooth=("jacobi", {"omega": 4.0 / 3.0}),
                                presmoother=("block_gauss_seidel", {"sweep": "symmetric"}),
                                postsmoother=("block_gauss_seidel", {"sweep": "symmetric"}),
                                improve_candidates=[("block_gauss_seidel", {"sweep": "symmetric",
                                                                            "iterations": 4}), None],
                                max_levels=10, max_coarse=500, diagonal_dominance=False, keep=False,
                                fast=True, device=None, **kwargs):
    """Create a multilevel solver using Smoothed Aggregation (SA)
    (pyamg/aggregation/aggregation.py:30-290); returns a pyamg_amd.multilevel_solver.

    device : None = every stage as its own options say.  True or False = the `device` option of symmetric strength,
    MIS(2) aggregation, fit_candidates and Jacobi smoothing on every level that does not set its own; with True every
    level takes the generic path of extend_hierarchy, and options that put one of these stages outside its device route
     raise NotImplementedError before any level is built.  Where all four stages of a level run
    on the device and _chain_options takes it ('symmetric' strength, 'mis' aggregation, Jacobi smoothing, real float64,
    one candidate), the levels are chained in HBM from one upload of A and B; the hierarchy is
    the same, bit for bit.  LAST_BUILD records the route of the last build."""
    if not (isspmatrix_csr(A) or isspmatrix_bsr(A)):
        try:
            A = csr_matrix(A)
        except Exception:
            raise TypeError("Argument A must have type csr_matrix or bsr_matrix, or be convertible to csr_matrix")
    if A.dtype.kind == "c":
        A = A.astype(np.complex128) if A.dtype != np.complex128 else A      # complex64 is raised, as float32 is
    else:
        A = A.astype(np.float64) if A.dtype != np.float64 else A
    if symmetry not in ("symmetric", "hermitian"):
        raise NotImplementedError("symmetry=%r is outside the restated setup" % (symmetry,))
    if diagonal_dominance:
        raise NotImplementedError("diagonal_dominance is outside the restated setup")
    A.symmetry = symmetry
    if A.shape[0] != A.shape[1]:
        raise ValueError("expected square matrix")
    if B is None:
        if blocksize(A) == 1:
            B = np.ones((A.shape[0], 1), dtype=A.dtype)         # = the kron below for 1x1 blocks, without its temporaries
        else:
            B = np.kron(np.ones((int(A.shape[0] / blocksize(A)), 1), dtype=A.dtype), np.eye(blocksize(A)))
    else:
        B = np.asarray(B, dtype=A.dtype)
        if len(B.shape) == 1:
            B = B.reshape(-1, 1)
        if B.shape[0] != A.shape[0]:
            raise ValueError("The near null-space modes B have incorrect dimensions for matrix A")

    max_levels, max_coarse, strength = _levelize_sa(strength, max_levels, max_coarse)
    max_levels, max_coarse, aggregate = _levelize_sa(aggregate, max_levels, max_coarse)
    improve_candidates = _levelize_smooth(list(improve_candidates) if isinstance(improve_candidates, list)
                                          else improve_candidates, max_levels)
    smooth = _levelize_smooth(smooth, max_levels)
    if device is not None:
        device = bool(device)
        strength = _with_device(strength, ("symmetric",), device)
        aggregate = _with_device(aggregate, ("mis",), device)
        smooth = _with_device(smooth, ("jacobi",), device)
        if device:
            _device_setup_refusals(A, B, smooth)

    verbose = os.environ.get("AMG_SETUP_VERBOSE", "0") != "0"
    t0 = time.perf_counter()
    levels = [multilevel_solver.level()]
    levels[-1].A = A
    levels[-1].B = B
    LAST_BUILD["uploads"] = 0
    LAST_BUILD["levels"] = []
    chain = _Chain()
    try:
        while len(levels) < max_levels and int(levels[-1].A.shape[0] / blocksize(levels[-1].A)) > max_coarse:
            extend_hierarchy(levels, strength, aggregate, smooth, improve_candidates, keep or not fast, device=device, chain=chain)
    finally:
        chain.close()
    t1 = time.perf_counter()
    ml = multilevel_solver(levels, **kwargs)
    t2 = time.perf_counter()
    change_smoothers(ml, presmoother, postsmoother)
    if verbose:
        print("[setup] levels %.2fs, multilevel_solver (coarse solver) %.2fs, smoothers %.2fs"
              % (t1 - t0, t2 - t1, time.perf_counter() - t2), flush=True)
    return ml


def _with_device(levelized, stages, device):
    """the per-level options with device=`device` added to every stage of `stages` that does not set its own"""
    out = []
    for entry in levelized:
        fn, kw = unpack_arg(entry)
        if fn in stages and "device" not in kw:
            entry = (fn, dict(kw, device=device))
        out.append(entry)
    return out


def _device_setup_refusals(A, B, smooth):
    """smoothed_aggregation_solver(device=True): what puts a stage outside its device route on every level, raised
    before any level is built"""
    if A.dtype.kind == "c":
        raise outside("smoothed aggregation of a complex operator on the device")
    for entry in smooth:
        fn, kw = unpack_arg(entry)
        if fn != "jacobi" or not kw.get("device", False):
            continue
        if blocksize(A) != 1:
            raise outside("Jacobi prolongation smoothing with blocks larger than 1 x 1 on the device")
        if B.shape[1] > 1:
            raise outside("Jacobi prolongation smoothing with more than one candidate on the device")
        if kw.get("filter", False):
            raise outside("filtered prolongation smoothing")
        if kw.get("weighting", "diagonal") not in ("diagonal", "local", "block"):
            raise outside("weighting=%r" % (kw.get("weighting"),))


def poisson(grid, format="csr"):
    """gallery.poisson(grid) (pyamg/gallery/laplacian.py:14-69) for 1-3 dimensions, generated
    natively: 2d on the diagonal, -1 off it, last axis fastest, sorted int32 indices."""
    grid = tuple(int(g) for g in grid)
    if not 1 <= len(grid) <= 3 or min(grid) < 1:
        raise ValueError("invalid grid shape: %s" % str(grid))
    g3 = (1,) * (3 - len(grid)) + grid
    L = host_lib()
    n = g3[0] * g3[1] * g3[2]
    nnz = L.amgsetup_poisson_nnz(*g3)
    if nnz >= 2 ** 31:
        raise ValueError("matrix exceeds int32 indices")
    Ap = np.empty(n + 1, dtype=np.int64)
    Aj = np.empty(nnz, dtype=np.intc)
    Ax = np.empty(nnz, dtype=np.float64)
    L.amgsetup_poisson(g3[0], g3[1], g3[2], 2.0 * len(grid), _lp(Ap), _ip(Aj), _dp(Ax))
    A = csr_matrix((Ax, Aj, Ap.astype(np.intc)), shape=(n, n))
    A.has_sorted_indices = True
    A._amg_columns_once = True              # a stencil's offsets are distinct (_columns_once)
    return A.asformat(format)


def _csr_arrays64(M):
    """(indptr int64, indices int32, data f64) of a CSR / BSR(1,1) matrix, without copies when possible"""
    data = M.data.reshape(-1) if isspmatrix_bsr(M) else M.data
    return (np.ascontiguousarray(M.indptr, dtype=np.int64), np.ascontiguousarray(M.indices, dtype=np.intc),
            np.ascontiguousarray(data, dtype=np.float64))


def _columns_once(M):
    """No row of the CSR / BSR(1,1) matrix M holds a column twice: what the device products require of their right-hand
    operands (csrc/spgemm.hip: the lanes of a group take a right-hand row's entries side by side).  scipy and the host
    products take such rows as they are, so an operator that fails this stays with them.  Operators this package
    formed as a product hold each column once by construction and say so (_amg_columns_once)."""
    if getattr(M, "_amg_columns_once", False):
        return True
    if not M.has_sorted_indices:
        # the pattern alone, sorted in a copy: duplicates are then neighbours, which is what scipy's check looks for
        M = csr_matrix((np.ones(len(M.indices), dtype=np.int8), M.indices.copy(), M.indptr), shape=M.shape)
        M.sort_indices()
    return bool(M.has_canonical_format)


def _matmat(Aa, Ba, shape):
    """C = A*B with scipy's csr_matmat arithmetic and output order, row-parallel on the host."""
    (Ap, Aj, Ax), (Bp, Bj, Bx) = Aa, Ba
    L = host_lib()
    n_row, n_col = shape
    Cp = np.empty(n_row + 1, dtype=np.int64)
    nnz = L.amgsetup_csr_matmat_count(n_row, n_col, _lp(Ap), _ip(Aj), _lp(Bp), _ip(Bj), _lp(Cp))
    Cj = np.empty(nnz, dtype=np.intc)
    Cx = np.empty(nnz, dtype=np.float64)
    nnz2 = L.amgsetup_csr_matmat_fill(n_row, n_col, _lp(Ap), _ip(Aj), _dp(Ax), _lp(Bp), _ip(Bj), _dp(Bx),
                                      _lp(Cp), _ip(Cj), _dp(Cx))
    if nnz2 != nnz:
        Cj = Cj[:nnz2].copy()
        Cx = Cx[:nnz2].copy()
    return Cp, Cj, Cx


def _as_bsr11(arrs, shape):
    Cp, Cj, Cx = arrs
    if Cp[-1] >= 2 ** 31:
        raise ValueError("operator exceeds int32 indices")
    M = bsr_matrix((Cx.reshape(-1, 1, 1), Cj, Cp.astype(np.intc)), shape=shape, copy=False)
    return M


def _scalar_fast_path_ok(A, B, strength_l, aggregate_l, smooth_l):
    if A.dtype.kind == "c":
        return False                    # the flat-array fast paths are float64: complex operators take the generic path
    if not (isspmatrix_csr(A) or (isspmatrix_bsr(A) and A.blocksize == (1, 1))):
        return False
    return _default_options(B, strength_l, aggregate_l, smooth_l)


def _default_options(B, strength_l, aggregate_l, smooth_l):
    """one candidate, symmetric strength with theta = 0, standard aggregation, one Jacobi smoothing step"""
    if B.shape[1] != 1:
        return False
    fn, kw = unpack_arg(strength_l)
    if fn != "symmetric" or kw.get("theta", 0) != 0 or kw.get("device"):
        return False
    fn, kw = unpack_arg(aggregate_l)
    if fn != "standard" or kw:
        return False
    fn, kw = unpack_arg(smooth_l)
    if fn != "jacobi" or kw.get("degree", 1) != 1 or kw.get("filter", False) or kw.get("device") or \
            kw.get("weighting", "diagonal") not in ("diagonal", "block"):
        return False
    return True


def _extend_scalar(levels, smooth_l, keep, rho_fn):
    """extend_hierarchy for scalar problems with one candidate (the BASELINE Poisson
    configurations), on flat arrays with the host helpers: same arithmetic as the generic
    path below, sized for 10^8 unknowns."""
    A = levels[-1].A
    B = levels[-1].B
    L = host_lib()
    n = A.shape[0]
    verbose = os.environ.get("AMG_SETUP_VERBOSE", "0") != "0"
    _t = [time.perf_counter()]

    def lap(what):
        if verbose:
            now = time.perf_counter()
            print("[setup] level %d (%d rows) %-22s %6.2fs" % (len(levels) - 1, n, what, now - _t[0]), flush=True)
            _t[0] = now
    Ap, Aj, Ax = _csr_arrays64(A)
    Ap32 = np.ascontiguousarray(A.indptr, dtype=np.intc)
    # rho(D^-1 A) does not depend on the aggregation: when the rows are already sorted (level 0 of the gallery
    # operators; get_diagonal's in-place sort below is then a no-op and the aggregation reads the same order either
    # way) the estimate -- upload of A, Arnoldi on the GPU -- runs in a thread of its own beside aggregation and
    # tentative prolongator.  Neither of those draws random numbers, so the estimate's single np.random.rand draw is the
    # same draw.
    early = None
    if n >= 1000000 and rho_fn is _rho_D_inv_A_host and use_device_for(A) and getattr(A, "has_sorted_indices", False) \
            and os.environ.get("AMG_SETUP_OVERLAP_RHO", "1") != "0":
        import threading
        box = {}

        def estimate():
            try:
                d = np.empty(n, dtype=np.float64)
                L.amgsetup_csr_diagonal_inv(n, _lp(Ap), _ip(Aj), _dp(Ax), _dp(d))
                box["D_inv"] = d
                box["rho"] = rho_fn(A, d)
            except BaseException as e:      # noqa: BLE001 -- re-raised in the main thread
                box["error"] = e
        early = (threading.Thread(target=estimate), box)
        early[0].start()
    # strength with theta = 0 keeps every entry: the aggregation only reads the pattern
    agg = np.empty(n, dtype=np.intc)
    cpts = np.empty(n, dtype=np.intc)
    n_agg = L.amgsetup_standard_aggregation(n, _ip(Ap32), _ip(Aj), _ip(agg), _ip(cpts))
    del cpts
    lap("aggregation")
    if n_agg == 0:
        raise ValueError("aggregation produced no aggregates")
    # tentative prolongator
    Bv = np.ascontiguousarray(B.ravel(), dtype=np.float64)
    Tp = np.empty(n + 1, dtype=np.int64)
    Tj = np.empty(n, dtype=np.intc)
    Tx = np.empty(n, dtype=np.float64)
    Bc = np.empty(n_agg, dtype=np.float64)
    tnnz = L.amgsetup_tentative_scalar(n, n_agg, _ip(agg), _dp(Bv), 1e-10, _lp(Tp), _ip(Tj), _dp(Tx), _dp(Bc))
    Tj, Tx = Tj[:tnnz], Tx[:tnnz]
    # Jacobi prolongation smoothing: rho(D^-1 A), then P = T - (omega/rho) D^-1 A T
    fn, kw = unpack_arg(smooth_l)
    omega = kw.get("omega", 4.0 / 3.0)
    lap("tentative prolongator")
    # get_diagonal(A, inv=True), row-parallel on the flat arrays -- including its side effect: the reference sorts
    # A's rows in place here (util/utils.py:566), so everything from here on sees the sorted order
    if early is not None:
        early[0].join()
        if "error" in early[1]:
            raise early[1]["error"]
        D_inv, rho = early[1]["D_inv"], early[1]["rho"]
        lap("rho(D^-1 A) (overlapped)")
    else:
        if Aj.ctypes.data == A.indices.ctypes.data and Ax.ctypes.data == A.data.ctypes.data and Ax.size == A.data.size \
                and Aj.flags.writeable and Ax.flags.writeable:
            L.amgsetup_csr_sort_indices(n, _lp(Ap), _ip(Aj), _dp(Ax))
            A.has_sorted_indices = True
        else:
            A.sort_indices()
            Ap, Aj, Ax = _csr_arrays64(A)
        D_inv = np.empty(n, dtype=np.float64)
        L.amgsetup_csr_diagonal_inv(n, _lp(Ap), _ip(Aj), _dp(Ax), _dp(D_inv))
        lap("diagonal")
        rho = rho_fn(A, D_inv)
        lap("rho(D^-1 A)")
    w = omega / rho
    Pp = np.empty(n + 1, dtype=np.int64)
    dnull = C.POINTER(C.c_double)()
    inull = C.POINTER(C.c_int)()
    pnnz = L.amgsetup_smooth_prolongator(n, n_agg, _lp(Ap), _ip(Aj), _dp(Ax), _dp(D_inv), float(w), _lp(Tp),
                                         _ip(Tj), _dp(Tx), _lp(Pp), inull, dnull)
    Pj = np.empty(pnnz, dtype=np.intc)
    Px = np.empty(pnnz, dtype=np.float64)
    L.amgsetup_smooth_prolongator(n, n_agg, _lp(Ap), _ip(Aj), _dp(Ax), _dp(D_inv), float(w), _lp(Tp),
                                  _ip(Tj), _dp(Tx), _lp(Pp), _ip(Pj), _dp(Px))
    # R = P^H (real: transpose)
    Rp = np.empty(n_agg + 1, dtype=np.int64)
    Rj = np.empty(pnnz, dtype=np.intc)
    Rx = np.empty(pnnz, dtype=np.float64)
    lap("smoothed prolongator")
    L.amgsetup_csr_transpose(n, n_agg, _lp(Pp), _ip(Pj), _dp(Px), _lp(Rp), _ip(Rj), _dp(Rx))
    lap("R = P^T")
    # Galerkin product (R*A)*P: on the GPU when A already sits in HBM (the spectral-radius estimate uploaded it),
    # else row-parallel on the host -- the same products in the same order either way
    # (A is the right-hand operand of R*A: an operator with a column twice in a row stays with the host products, which
    # take it as scipy does; its rows are sorted by now, so this is scipy's own cached check)
    Ac = None
    if os.environ.get("AMG_SETUP_DEVICE_GALERKIN", "1") != "0" and _columns_once(A):
        from .util import galerkin_device
        Ac = galerkin_device(A, (Rp, Rj, Rx), (Pp, Pj, Px), n_agg)
        if Ac is not None:
            lap("(R*A)*P on the device")
    if Ac is None:
        RA = _matmat((Rp, Rj, Rx), (Ap, Aj, Ax), (n_agg, n))
        lap("R*A")
        Ac = _matmat(RA, (Pp, Pj, Px), (n_agg, n_agg))
        del RA
        lap("(R*A)*P")
    P = _as_bsr11((Pp, Pj, Px), (n, n_agg))
    R = _as_bsr11((Rp, Rj, Rx), (n_agg, n))
    Anew = _as_bsr11(Ac, (n_agg, n_agg))
    Anew._amg_columns_once = True           # a csr_matmat result, from either path
    if keep:
        levels[-1].AggOp = agg
    levels[-1].P = P
    levels[-1].R = R
    levels.append(multilevel_solver.level())
    Anew.symmetry = A.symmetry
    levels[-1].A = Anew
    levels[-1].B = Bc.reshape(-1, 1)
    lap("wrap as BSR(1,1)")


def _block_fast_path_ok(A, B, strength_l, aggregate_l, smooth_l):
    """square-block BSR operator (any number of candidates), default strength / aggregation / smoothing"""
    if A.dtype.kind == "c":
        return False
    if not (isspmatrix_bsr(A) and A.blocksize[0] == A.blocksize[1] and 1 < A.blocksize[0] <= 16):
        return False
    return _default_options(np.empty((1, 1)), strength_l, aggregate_l, smooth_l)


def _bsr_matmat(Aa, Ba, n_brow, R, N, Cc):
    """C = A*B for BSR arrays with R x N and N x Cc blocks: scipy's bsr_matmat arithmetic and block order"""
    (Ap, Aj, Ax), (Bp, Bj, Bx) = Aa, Ba
    L = host_lib()
    Cp = np.empty(n_brow + 1, dtype=np.int64)
    nb = L.amgsetup_bsr_matmat_count(n_brow, _lp(Ap), _ip(Aj), _lp(Bp), _ip(Bj), _lp(Cp))
    Cj = np.empty(nb, dtype=np.intc)
    Cx = np.empty(nb * R * Cc, dtype=np.float64)
    L.amgsetup_bsr_matmat_fill(n_brow, R, N, Cc, _lp(Ap), _ip(Aj), _dp(Ax), _lp(Bp), _ip(Bj), _dp(Bx), _lp(Cp), _ip(Cj), _dp(Cx))
    return Cp, Cj, Cx


def _extend_block(levels, smooth_l, keep, rho_fn):
    """extend_hierarchy for a BSR(bs, bs) operator (BASELINE configuration C5: 3x3 blocks, the default bs
    candidates) on flat arrays with the host helpers -- the arithmetic and the stored block order of the generic
    scipy path (bsr_matmat, bsr_minus_bsr, bsr_transpose), row-parallel and sized for 5*10^7 unknowns."""
    A = levels[-1].A
    B = np.asarray(levels[-1].B, dtype=np.float64)
    L = host_lib()
    bs = A.blocksize[0]
    K = B.shape[1]
    n = A.shape[0]
    nb = n // bs
    verbose = os.environ.get("AMG_SETUP_VERBOSE", "0") != "0"
    _t = [time.perf_counter()]

    def lap(what):
        if verbose:
            now = time.perf_counter()
            print("[setup] level %d (%d rows, bs %d) %-22s %6.2fs" % (len(levels) - 1, n, bs, what, now - _t[0]), flush=True)
            _t[0] = now
    Ap = np.ascontiguousarray(A.indptr, dtype=np.int64)
    Ap32 = np.ascontiguousarray(A.indptr, dtype=np.intc)
    Aj = np.ascontiguousarray(A.indices, dtype=np.intc)
    Ax = np.ascontiguousarray(A.data.reshape(-1), dtype=np.float64)
    # strength with theta = 0 keeps every block (strength.py:283-287); the aggregation reads the block pattern
    agg = np.empty(nb, dtype=np.intc)
    cpts = np.empty(nb, dtype=np.intc)
    n_agg = L.amgsetup_standard_aggregation(nb, _ip(Ap32), _ip(Aj), _ip(agg), _ip(cpts))
    del cpts
    lap("aggregation")
    if n_agg == 0:
        raise ValueError("aggregation produced no aggregates")
    # tentative prolongator: per-aggregate QR of the candidates (fit_candidates' arithmetic), as one
    # bs x K block per aggregated node
    Tx, Bc = _fit_candidates_flat(agg, n_agg, B, bs)
    lap("tentative prolongator")
    fn, kw = unpack_arg(smooth_l)
    omega = kw.get("omega", 4.0 / 3.0)
    D_inv = get_diagonal(A, inv=True)
    rho = rho_fn(A, D_inv)
    lap("rho(D^-1 A)")
    w = omega / rho
    Pp = np.empty(nb + 1, dtype=np.int64)
    xs = C.c_int(0)
    inull, dnull = C.POINTER(C.c_int)(), C.POINTER(C.c_double)()
    pb = L.amgsetup_smooth_prolongator_block(nb, bs, K, _lp(Ap), _ip(Aj), _dp(Ax), _dp(D_inv), float(w), _ip(agg), _dp(Tx),
                                             _lp(Pp), inull, dnull, C.byref(xs))
    Pj = np.empty(pb, dtype=np.intc)
    Px = np.empty(pb * bs * K, dtype=np.float64)
    L.amgsetup_smooth_prolongator_block(nb, bs, K, _lp(Ap), _ip(Aj), _dp(Ax), _dp(D_inv), float(w), _ip(agg), _dp(Tx),
                                        _lp(Pp), _ip(Pj), _dp(Px), C.byref(xs))
    del Tx
    lap("smoothed prolongator")
    Rp = np.empty(n_agg + 1, dtype=np.int64)
    Rj = np.empty(pb, dtype=np.intc)
    Rx = np.empty(pb * bs * K, dtype=np.float64)
    L.amgsetup_bsr_transpose(nb, n_agg, bs, K, _lp(Pp), _ip(Pj), _dp(Px), _lp(Rp), _ip(Rj), _dp(Rx))
    lap("R = P^T")
    RA = _bsr_matmat((Rp, Rj, Rx), (Ap, Aj, Ax), n_agg, K, bs, bs)
    lap("R*A")
    Ac = _bsr_matmat(RA, (Pp, Pj, Px), n_agg, K, bs, K)
    del RA
    lap("(R*A)*P")
    if max(Pp[-1], Ac[0][-1]) >= 2 ** 31:
        raise ValueError("operator exceeds int32 indices")
    P = bsr_matrix((Px.reshape(-1, bs, K), Pj, Pp.astype(np.intc)), shape=(n, n_agg * K), copy=False)
    R = bsr_matrix((Rx.reshape(-1, K, bs), Rj, Rp.astype(np.intc)), shape=(n_agg * K, n), copy=False)
    Anew = bsr_matrix((Ac[2].reshape(-1, K, K), Ac[1], Ac[0].astype(np.intc)), shape=(n_agg * K, n_agg * K), copy=False)
    if keep:
        levels[-1].AggOp = agg
    levels[-1].P = P
    levels[-1].R = R
    levels.append(multilevel_solver.level())
    Anew.symmetry = A.symmetry
    levels[-1].A = Anew
    levels[-1].B = Bc


def _fit_candidates_flat(agg, n_agg, B, K1, tol=1e-10):
    """fit_candidates (tentative.py:19-166) on the aggregate id of every node instead of AggOp:
    -> (Tx: (n_nodes, K1, K2) blocks of the tentative prolongator, zero for unaggregated nodes; R: (n_agg*K2, K2))."""
    n_nodes = len(agg)
    K2 = B.shape[1]
    member = np.nonzero(agg >= 0)[0]
    order = member[np.argsort(agg[member], kind="stable")]          # CSC order of AggOp: by aggregate, ascending node
    counts = np.bincount(agg[member], minlength=n_agg)
    Ap = np.concatenate(([0], np.cumsum(counts)))
    Qx, R = _aggregate_qr(B.reshape(-1, K1, K2)[order], Ap, n_agg, K1, K2, tol)
    Tx = np.zeros((n_nodes, K1, K2), dtype=np.float64)
    Tx[order] = Qx
    return np.ascontiguousarray(Tx.reshape(-1)), R.reshape(-1, K2)


def _rho_D_inv_A_host(A, D_inv):
    """approximate_spectral_radius(scale_rows(A, D_inv)) as the reference does it (smooth.py:169-171);
    operators beyond util.DEVICE_RHO_MIN_ROWS run the Arnoldi iterations on the GPU."""
    if use_device_for(A):
        return approximate_spectral_radius_device(A, D_inv)
    return approximate_spectral_radius(scale_rows(A, D_inv, copy=True))


def _galerkin_c128_device(R, A, P):
    """(R*A)*P of a complex128 level on the GPU (util.galerkin_device, csrc/spgemm.hip) as the BSR(1,1) matrix scipy's
    R * A * P gives, or None: no device, AMG_SETUP_DEVICE_GALERKIN=0, a level below the gates
    (util.DEVICE_GALERKIN_C128_MIN_ROWS, None = never, and util.DEVICE_RHO_MIN_ROWS), operands with blocks larger
    than 1 x 1, an operator A with a column twice in a row, or a row too long for the device tables --
    the caller then uses scipy's products."""
    from . import util
    gate = util.DEVICE_GALERKIN_C128_MIN_ROWS
    if os.environ.get("AMG_SETUP_DEVICE_GALERKIN", "1") == "0" or gate is None \
            or A.shape[0] < max(gate, util.DEVICE_RHO_MIN_ROWS):
        return None
    for M in (R, A, P):
        if not (isspmatrix_csr(M) or (isspmatrix_bsr(M) and M.blocksize == (1, 1))):
            return None
    from . import _lib
    if _lib.device_count() <= 0:
        return None
    if not _columns_once(A):                # (P and R*A are this package's own: each column once by construction)
        return None
    def arrays(M):
        return (np.ascontiguousarray(M.indptr, dtype=np.int64), np.ascontiguousarray(M.indices, dtype=np.intc),
                np.ascontiguousarray(np.ravel(M.data), dtype=np.complex128))
    Ac = util.galerkin_device(arrays(A), arrays(R), arrays(P), P.shape[1])
    if Ac is None:
        return None
    return _as_bsr11(Ac, (P.shape[1], P.shape[1]))


# --------------------------------------------------------------------------- the resident chain
# The route of the last smoothed_aggregation_solver build, for the tests and tools/bench_sa_hierarchy.py.  uploads:
# operators sent to HBM by the chain (one per chain; the stage routes' own uploads are not counted).  levels: one record
# per level built: chained (the whole level, its transpose and its Galerkin product ran in HBM on the chain's resident
# operator), resident (the chain built the prolongator, whoever formed the product), strength_mode (what the chain was
# told about the host's format of A_l; None off the chain), stopped (why the chain handed the level on: 'no aggregate',
# 'smoothing refused' or None), times (milliseconds by CHAIN_STAGES), products (the tables of R * A and (R * A) * P,
# _lib.SPGEMM_TABLES) and transpose (_lib.TRANSPOSE_ROUTE_FIELDS).
LAST_BUILD = {"uploads": 0, "levels": []}
CHAIN_STAGES = ("upload", "strength", "aggregation", "tentative", "sort", "smoothing", "transpose", "galerkin", "fetch")
# What tools/bench_sa_hierarchy.py turns off to time the per-stage device route (every stage uploads its operands and
# fetches its result, transpose and Galerkin product on the host); not an option of the setup.
_RESIDENT_CHAIN = True
# a coarse operator of this many entries or more does not fit the host's 32-bit index arrays: the level's product is
# treated as refused, as the device library itself refuses it
_PRODUCT_ENTRIES_LIMIT = 2 ** 31
_STOPPED = {1: "no aggregate", 2: "smoothing refused"}


def _record_level(chained=False, resident=False, strength_mode=None, stopped=None, times=None, products=None, transpose=None):
    LAST_BUILD["levels"].append({"chained": chained, "resident": resident, "strength_mode": strength_mode, "stopped": stopped,
                                 "times": times or {}, "products": products, "transpose": transpose})


class _Chain:
    """the resident chain of one smoothed_aggregation_solver call: the handle of amg_sa_chain_begin and what the last
    level's flags said about the operator it left in HBM: its rows and whether its values are finite"""

    def __init__(self):
        self.handle = None
        self.finite = True
        self.n = 0

    def close(self):
        if self.handle is not None:
            from . import _lib
            handle, self.handle = self.handle, None
            _lib.lib().amg_sa_chain_free(handle)


def _chain_options(A, B, strength_l, aggregate_l, smooth_l, device):
    """(theta, omega, degree, weighting) where the whole level runs in HBM, None otherwise: a real float64 operator
    with scalar unknowns and one candidate; 'symmetric' strength with theta alone, 'mis' aggregation without weights of
    its own and 'jacobi' smoothing without filtering, of one step or more, with weighting 'diagonal', 'local' or
    'block'; none of the four stages sent to the host (`device` is fit_candidates' option, the others carry theirs)."""
    if not (isspmatrix_csr(A) or (isspmatrix_bsr(A) and A.blocksize == (1, 1))) or A.dtype != np.float64:
        return None
    if np.ndim(B) != 2 or B.shape[1] != 1 or B.dtype != np.float64:
        return None
    if route(device, FIT_CANDIDATES_DEVICE_AUTO) is False:
        return None
    fn, kw = unpack_arg(strength_l)
    if fn != "symmetric" or set(kw) - {"theta", "device"} or route(kw.get("device"), SYMMETRIC_STRENGTH_DEVICE_AUTO) is False:
        return None
    theta = kw.get("theta", 0)
    if not theta >= 0:
        return None
    fn, kw = unpack_arg(aggregate_l)
    if fn != "mis" or set(kw) - {"device"} or route(kw.get("device"), MIS_DEVICE_AUTO) is False:
        return None
    fn, kw = unpack_arg(smooth_l)
    if fn != "jacobi" or set(kw) - {"omega", "degree", "weighting", "filter", "device"} \
            or route(kw.get("device"), JACOBI_DEVICE_AUTO) is False:
        return None
    weighting = kw.get("weighting", "diagonal")
    if kw.get("filter", False) or weighting not in ("diagonal", "local", "block") or kw.get("degree", 1) < 1:
        return None
    # ('block' on scalar unknowns is 'diagonal', as jacobi_prolongation_smoother has it)
    return theta, kw.get("omega", 4.0 / 3.0), int(kw.get("degree", 1)), "diagonal" if weighting == "block" else weighting


def _chain_strength_mode(A, theta):
    """What symmetric_strength_of_connection makes of the host's A_l: a CSR operator's values as they are; of a BSR
    operator with 1 x 1 blocks (every level that scipy's bsr * csr * bsr left) the squared values, and with theta == 0
    the whole pattern with every value 1.0"""
    from . import _lib
    if isspmatrix_csr(A):
        return _lib.SA_STRENGTH_CSR
    return _lib.SA_STRENGTH_ONES if theta == 0 else _lib.SA_STRENGTH_SQUARED


def _chain_level_call(handle, n, theta, mode, y, D_inv, w, degree, B, sizes, flags, ms):
    """amg_sa_chain_level -> 0 or _lib.CHAIN_PRODUCT_REFUSED (the tests wrap it to see the calls).  n: the rows of the
    host's A_l, which the entry compares with its resident operator's before it reads y, D_inv and B."""
    from . import _lib
    rc = _lib.lib().amg_sa_chain_level(handle, n, float(theta), mode, y.ctypes.data, D_inv.ctypes.data, float(w), degree,
                                       None if B is None else B.ctypes.data, 1e-10, sizes, flags, None, ms)
    if rc != _lib.CHAIN_PRODUCT_REFUSED:
        _lib.check(rc)
    return rc


def _chain_level(levels, chain, options, keep, improved):
    """One level on the chain's resident operator and candidate (amg_sa_chain_level / _fetch): strength, MIS(2)
    aggregation, the tentative prolongator, Jacobi smoothing, R = P^T and R A P in HBM; the host hierarchy receives what
    it keeps.  The first level of a chain vets and uploads A and B.  improved: B is new on the host (candidate
    improvement) and replaces the resident one.  The host draws the weights of the set and then takes the diagonal and
    the spectral radius, in the order of the stage route, before the call.

    Returns None where the level is built, or what the stage route needs to finish a level that stopped (no aggregate,
    or a refused product of the smoothing) without sorting or drawing again: {'C', 'y', 'weights'}.  Whatever is
    outside the chain raises NotImplementedError before anything is drawn; one from the level entry, after the draws,
    becomes a RuntimeError.  Where a Galerkin product is refused the
    level is finished on the host from the fetched P, and the chain ends."""
    from . import _lib
    A, B = levels[-1].A, levels[-1].B
    theta, omega, degree, weighting = options
    n = A.shape[0]
    what = "a chained smoothed-aggregation level"
    if chain.handle is not None and chain.n != n:
        chain.close()                       # not the operator the chain left: this level begins another
    if chain.handle is None:
        if A.indptr.dtype != np.intc or A.indices.dtype != np.intc:
            raise outside("%s of an operator without 32-bit indices" % what)
        if n == 0 or A.shape[0] != A.shape[1] or int(A.indptr[-1]) >= 2 ** 31:
            raise outside("%s of an operator that is empty, not square or of 2^31 entries or more" % what)
        if not _columns_once(A):
            raise outside("%s of an operator with a column twice in a row" % what)
    elif not chain.finite:
        raise outside("%s of an operator with values that are not finite" % what)
    _finite_f64(what, B)
    Bv = _f64(np.ravel(B))
    if chain.handle is None:
        # (in the order its product left it: the host's copy is sorted only below; a value that is not finite is
        # AMG_ENOTIMPL from the pass over the uploaded operator)
        Ap, Aj, Ax = _i32(A.indptr), _i32(A.indices), _f64(np.ravel(A.data))
        handle = C.c_void_p()
        _lib.check(_lib.lib().amg_sa_chain_begin(n, Ap.ctypes.data, Aj.ctypes.data, Ax.ctypes.data, Bv.ctypes.data, C.byref(handle)))
        chain.handle, chain.finite, chain.n = handle, True, n
        LAST_BUILD["uploads"] += 1
        improved = False
    mode = _chain_strength_mode(A, theta)
    y = _f64(np.random.rand(n))
    weights = _jacobi_weights(A, omega, weighting)
    D_inv = _f64(np.ravel(weights[2]))
    sizes = (C.c_long * 5)()
    flags = (C.c_int * _lib.SA_CHAIN_FLAG_FIELDS)()
    ms = (C.c_double * len(CHAIN_STAGES))()
    try:
        rc = _chain_level_call(chain.handle, n, theta, mode, y, D_inv, weights[1], degree, Bv if improved else None, sizes, flags, ms)
    except NotImplementedError as e:
        # the weights are drawn and the host's A_l is sorted: a refusal now must not reach the stage route, which would
        # draw and sort again (the entry reports what it cannot finish in its flags instead)
        raise RuntimeError("a chained smoothed-aggregation level was refused after its draws: %s" % e) from e
    s_nnz, t_nnz, p_nnz, c_nnz, n_coarse = (int(v) for v in sizes)
    stopped = int(flags[3])
    refused = rc == _lib.CHAIN_PRODUCT_REFUSED or c_nnz >= _PRODUCT_ENTRIES_LIMIT
    # the handle is the chain, which _Chain.close frees: nothing to release where an allocation fails
    built, whole = not stopped, not stopped and not refused
    arrays = _lib.allocate(_csr_specs(n, p_nnz, built) + _csr_specs(n_coarse, p_nnz, whole) + _csr_specs(n_coarse, c_nnz, whole)
                           + [(n_coarse, np.float64) if built else None] + _csr_specs(n, s_nnz, keep or stopped)
                           + ([(n, np.intc), (t_nnz, np.float64)] if keep and built else [None, None]))
    Pp, Pj, Px, Rp, Rj, Rx, Cp, Cj, Cx, Bc, Sp, Sj, Sx, agg, Tx = arrays
    _lib.check(_lib.lib().amg_sa_chain_fetch(chain.handle, *(None if a is None else a.ctypes.data for a in arrays), ms))
    _record_level(chained=whole, resident=built, strength_mode=mode, stopped=_STOPPED.get(stopped),
                  times=dict(zip(CHAIN_STAGES, ms)), products=(_lib.SPGEMM_TABLES[flags[4]], _lib.SPGEMM_TABLES[flags[5]]),
                  transpose=dict(zip(_lib.TRANSPOSE_ROUTE_FIELDS, (int(v) for v in flags[6:10]))))
    Cm = None
    if Sp is not None:
        Cm = csr_matrix((Sx, Sj.astype(A.indices.dtype, copy=False), Sp.astype(A.indptr.dtype, copy=False)), shape=A.shape)
    if stopped:
        chain.close()
        return {"C": Cm, "y": y, "weights": weights}
    P = bsr_matrix((Px.reshape(-1, 1, 1), Pj, Pp), shape=(n, n_coarse))
    symmetry = A.symmetry
    if refused:
        chain.close()
        R = P.conj().T.asformat(P.format) if symmetry == "hermitian" else P.T.asformat(P.format)
        Ac = R * A * P
    else:
        chain.finite, chain.n = bool(flags[1]), n_coarse
        R = bsr_matrix((Rx.reshape(-1, 1, 1), Rj, Rp), shape=(n_coarse, n))
        Ac = bsr_matrix((Cx.reshape(-1, 1, 1), Cj, Cp), shape=(n_coarse, n_coarse))
    if keep:
        mask = agg != -1
        Tp = np.concatenate(([0], np.cumsum(mask))).astype(np.intc)
        Tj = agg[mask]
        levels[-1].C = Cm
        levels[-1].AggOp = csr_matrix((np.ones(Tp[-1], dtype="int8"), Tj, Tp), shape=(n, n_coarse))
        levels[-1].T = bsr_matrix((Tx.reshape(-1, 1, 1), Tj.copy(), Tp.copy()), shape=(n, n_coarse), blocksize=(1, 1))
    levels[-1].P = P
    levels[-1].R = R
    levels.append(multilevel_solver.level())
    Ac._amg_columns_once = True             # a csr_matmat result, from either path
    Ac.symmetry = symmetry
    levels[-1].A = Ac
    levels[-1].B = Bc.reshape(-1, 1)
    return None


def _csr_specs(n_row, nnz, wanted=True):
    """the (count, dtype) of the three arrays of a CSR matrix for _lib.allocate, None each where it is not wanted"""
    return [(n_row + 1, np.intc), (nnz, np.intc), (nnz, np.float64)] if wanted else [None, None, None]


def extend_hierarchy(levels, strength, aggregate, smooth, improve_candidates, keep=True, rho_fn=None, device=None, chain=None):
    """aggregation.py:293-435.  device: fit_candidates' option (the other stages carry theirs in their keywords); True
    also keeps the level on the generic path.  chain: the resident chain of the calling smoothed_aggregation_solver
    (_Chain); with it, a level that _chain_options takes is built, transposed and multiplied in HBM."""
    A = levels[-1].A
    B = levels[-1].B

    li = len(levels) - 1
    # stage lines for complex operators only: the generic path of a real operator prints what it printed before
    verbose = os.environ.get("AMG_SETUP_VERBOSE", "0") != "0" and np.iscomplexobj(A)
    n_rows, dtype = A.shape[0], A.dtype
    _t = [time.perf_counter()]

    def lap(what):
        if verbose:
            now = time.perf_counter()
            print("[setup] level %d (%d rows, %s, generic) %-22s %6.2fs" % (li, n_rows, dtype, what, now - _t[0]),
                  flush=True)
            _t[0] = now
    fn, kwargs = unpack_arg(improve_candidates[li])
    # (running the candidate improvement beside the aggregation was tried: both are bound by host memory bandwidth and
    # the pair took longer than one after the other)
    if fn is not None:
        B = _improve((fn, kwargs), A, B)
        levels[-1].B = B
        lap("candidate improvement")

    # what the chain hands on where it stopped a level after its draws: C, the weights of the set, the Jacobi weights
    handed = None
    options = _chain_options(A, B, strength[li], aggregate[li], smooth[li], device) if chain is not None and _RESIDENT_CHAIN else None
    if options is not None:
        try:
            handed = _chain_level(levels, chain, options, keep, fn is not None)
            if handed is None:
                return
        except NotImplementedError:
            # a refusal from before the level's draws (_chain_level turns a later one into an error): the stage routes
            # answer, as they did
            chain.close()
        except BaseException:
            chain.close()
            raise
    elif chain is not None:
        # a level that is built elsewhere ends the chain: its resident operator is A_l, and the next level that the
        # chain takes has to begin another one from the A_{l+1} this level leaves on the host
        chain.close()
    if chain is not None and handed is None:
        _record_level()

    if not keep and not device and _scalar_fast_path_ok(A, B, strength[li], aggregate[li], smooth[li]):
        return _extend_scalar(levels, smooth[li], keep, rho_fn or _rho_D_inv_A_host)
    if not keep and not device and _block_fast_path_ok(A, B, strength[li], aggregate[li], smooth[li]):
        return _extend_block(levels, smooth[li], keep, rho_fn or _rho_D_inv_A_host)

    fn, kwargs = unpack_arg(strength[len(levels) - 1])
    if handed is not None:
        Cm = handed["C"]
    elif fn == "symmetric":
        Cm = symmetric_strength_of_connection(A, **kwargs)
    elif fn in ("ode", "evolution"):
        from .strength import evolution_strength_of_connection
        if "B" in kwargs:
            Cm = evolution_strength_of_connection(A, **kwargs)
        else:
            Cm = evolution_strength_of_connection(A, B, **kwargs)
    elif fn == "predefined":
        Cm = kwargs["C"].tocsr()
    elif fn is None:
        Cm = A.tocsr()
    else:
        raise NotImplementedError("strength=%r is outside the restated setup" % (fn,))

    fn, kwargs = unpack_arg(aggregate[len(levels) - 1])
    if fn == "standard":
        AggOp = standard_aggregation(Cm, **kwargs)[0]
    elif fn == "mis" and handed is not None:
        AggOp = mis_aggregation(Cm, y=handed["y"], **kwargs)[0]
    elif fn == "mis":
        AggOp = mis_aggregation(Cm, **kwargs)[0]        # draws the level's rand(n) here, before the spectral radius does
    elif fn == "predefined":
        AggOp = kwargs["AggOp"].tocsr()
    else:
        raise NotImplementedError("aggregate=%r is outside the restated setup" % (fn,))
    lap("strength, aggregation")

    T, B = fit_candidates(AggOp, B, device=device)
    lap("tentative prolongator")

    fn, kwargs = unpack_arg(smooth[len(levels) - 1])
    if fn == "jacobi":
        P = jacobi_prolongation_smoother(A, T, Cm, B, weights=None if handed is None else handed["weights"], **kwargs)
    elif fn == "energy":
        P = energy_prolongation_smoother(A, T, Cm, B, None, (False, {}), **kwargs)
    elif fn is None:
        P = T
    else:
        raise NotImplementedError("smooth=%r is outside the restated setup" % (fn,))

    lap("smoothed prolongator")
    symmetry = A.symmetry
    R = P.conj().T.asformat(P.format) if symmetry == "hermitian" else P.T.asformat(P.format)
    lap("R = P^H" if symmetry == "hermitian" else "R = P^T")

    if keep:
        levels[-1].C = Cm
        levels[-1].AggOp = AggOp
        levels[-1].T = T
    levels[-1].P = P
    levels[-1].R = R

    levels.append(multilevel_solver.level())
    Ac = _galerkin_c128_device(R, A, P) if A.dtype.kind == "c" else None
    what = "(R*A)*P by scipy" if Ac is None else "(R*A)*P on the device"
    A = R * A * P if Ac is None else Ac
    A._amg_columns_once = True              # a csr_matmat result, from either path
    lap(what)
    A.symmetry = symmetry
    levels[-1].A = A
    levels[-1].B = B
