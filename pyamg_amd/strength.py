"""Strength of connection measures of the smoothed-aggregation setup (pyamg/strength.py of the reference).

``symmetric_strength_of_connection`` is the one ``aggregation.py`` always had.  ``evolution_strength_of_connection``
(alias ``ode_strength_of_connection``) is strength.py:433-816 for a real float64 operator and ONE candidate vector,
by one of two routes that return the same bits in the same stored order when they are given the same spectral-radius
estimate ``rho``:

  host    the reference's statements restated with numpy / scipy, its two native steps (the incomplete product and
          the distance filter) in csrc/setup_host.cpp;
  device  every stage in HBM (csrc/strength.hip, amg_evolution_strength_device), for k = 1, 2, 4, 8, ...

Both draw the global RNG exactly where the reference does: one approximate_spectral_radius(Dinv A) per call.
Unlike the reference, neither changes its arguments: the reference sorts A and removes its stored zeros in place and
overwrites the zeros of B with 1.0; here that happens on copies.

Outside the restated setup (NotImplementedError): complex operators, more than one candidate, BSR blocks larger
than 1 x 1, block_flag=True, value types other than float64.
"""
import ctypes as C
from warnings import warn

import numpy as np
import scipy.sparse as sparse
from scipy.sparse import csr_matrix, isspmatrix_bsr, isspmatrix_csr

from . import util
from ._host import dp as _dp, host_lib, ip as _ip, outside as _outside, route
from .aggregation import symmetric_strength_of_connection
from .util import approximate_spectral_radius, scale_rows

__all__ = ["symmetric_strength_of_connection", "evolution_strength_of_connection", "ode_strength_of_connection"]

# What device=None does on operators of at least util.DEVICE_RHO_MIN_ROWS rows when a GPU is present: decided by the
# measurement in profiles/r13_evolution_strength.txt.
DEVICE_AUTO = False

_DBL_MAX = np.finfo(np.float64).max
_DBL_MIN = np.finfo(np.float64).tiny


def _power_of_two(k):
    return k >= 1 and (k & (k - 1)) == 0


def _canonical_csr(A):
    """A as CSR with sorted rows and no stored zeros (strength.py:559, 570-571), never the caller's own arrays changed"""
    M = A.tocsr() if not isspmatrix_csr(A) else A
    if M is A and (not M.has_sorted_indices or np.any(M.data == 0)):
        M = M.copy()
    M.eliminate_zeros()
    M.sort_indices()
    return M


def evolution_strength_of_connection(A, B=None, epsilon=4.0, k=2, proj_type="l2", block_flag=False,
                                     symmetrize_measure=True, device=None, rho=None):
    """Evolution strength of connection (pyamg/strength.py:433-816), the NullDim == 1 branch.

    A : csr_matrix or bsr_matrix with 1 x 1 blocks, float64.  B : one candidate vector (default: ones).
    epsilon >= 1 : drop tolerance, an entry stays when its distance is < epsilon times the row's smallest;
    np.inf keeps all.  k : time steps.  symmetrize_measure : 0.5 (S + S^T).
    device : True = the device pipeline (k a power of two), False = the host path, None = the host path unless
    DEVICE_AUTO, a GPU and util.DEVICE_RHO_MIN_ROWS rows.
    rho : the spectral radius of Dinv A when it is known already; None draws the reference's estimate.
    Returns the strength matrix as csr_matrix, rows scaled by their largest entry."""
    if epsilon < 1.0:
        raise ValueError("expected epsilon > 1.0")
    if k <= 0:
        raise ValueError("number of time steps must be > 0")
    if proj_type not in ["l2", "D_A"]:
        raise ValueError("proj_type must be 'l2' or 'D_A'")
    if (not isspmatrix_csr(A)) and (not isspmatrix_bsr(A)):
        raise TypeError("expected csr_matrix or bsr_matrix")
    if A.dtype.kind == "c" or (B is not None and np.iscomplexobj(B)):
        raise _outside("evolution strength of a complex operator")
    if A.dtype != np.float64:
        raise _outside("evolution strength of a %s operator" % A.dtype)
    if isspmatrix_bsr(A) and A.blocksize != (1, 1):
        raise _outside("evolution strength of BSR blocks larger than 1 x 1")
    if block_flag:
        raise _outside("evolution strength with block_flag=True")
    if int(k) != k:
        raise TypeError("number of time steps must be an integer")
    k = int(k)
    n = A.shape[0]
    if B is None:
        b = np.ones(n, dtype=np.float64)
    else:
        Bm = np.asarray(B, dtype=np.float64)
        if Bm.ndim == 1:
            Bm = Bm.reshape(-1, 1)
        if Bm.ndim != 2 or Bm.shape[1] != 1:
            raise _outside("evolution strength with more than one candidate")
        if Bm.shape[0] != n:
            raise ValueError("candidate vector has incompatible shape")
        b = np.array(Bm[:, 0], dtype=np.float64)            # a copy: zeros become 1.0 below
    if device is True and not _power_of_two(k):
        raise _outside("the device pipeline with k=%d (not a power of two)" % k)

    # strength.py:542-568: Dinv A for the time step's scaling, from A as handed in
    D = A.diagonal()
    Dinv = np.zeros_like(D)
    mask = (D != 0.0)
    Dinv[mask] = 1.0 / D[mask]
    Dinv[D == 0] = 1.0
    Dinv_A = scale_rows(A, Dinv, copy=True)
    csrflag = isspmatrix_csr(A)
    A = _canonical_csr(A)
    if rho is None:
        rho = approximate_spectral_radius(Dinv_A)
    rho = float(rho)

    if route(device, DEVICE_AUTO and n >= util.DEVICE_RHO_MIN_ROWS and _power_of_two(k)) is not False:
        Cm = _device_measure(A, b, rho, epsilon, k, symmetrize_measure)
        if Cm is None:
            if device is True:
                raise _outside("the device pipeline for an operator with duplicate entries")
        else:
            return Cm
    return _host_measure(A, Dinv_A, b, rho, epsilon, k, symmetrize_measure, csrflag)


ode_strength_of_connection = evolution_strength_of_connection


def _host_measure(A, Dinv_A, b, rho, epsilon, k, symmetrize_measure, csrflag):
    """strength.py:573-816 statement by statement (A: sorted CSR without stored zeros)"""
    dimen = A.shape[1]
    nsquare = int(np.log2(k))
    ninc = k - 2 ** nsquare

    # one time step, transposed so that columns are rows (strength.py:595-598)
    I = sparse.eye(dimen, dimen, format="csr", dtype=A.dtype)
    Atilde = (I - (1.0 / rho) * Dinv_A)
    Atilde = Atilde.T.tocsr()
    mask = A.copy()

    if ninc > 0:
        warn("The most efficient time stepping for the Evolution Strength Method is done in powers of two.\n"
             "You have chosen " + str(k) + " time steps.")
        for i in range(nsquare):
            Atilde = Atilde * Atilde
        JacobiStep = (I - (1.0 / rho) * Dinv_A).T.tocsr()
        for i in range(ninc):
            Atilde = Atilde * JacobiStep
        del JacobiStep
        mask.data[:] = 1.0
        Atilde = Atilde.multiply(mask).tocsr()
        Atilde.eliminate_zeros()
        Atilde.sort_indices()
    elif nsquare == 0:
        pass
    else:
        for i in range(nsquare - 1):
            Atilde = Atilde * Atilde
        AtildeCSC = Atilde.tocsc()
        AtildeCSC.sort_indices()
        mask.sort_indices()
        Atilde.sort_indices()
        ic = lambda a: np.ascontiguousarray(a, dtype=np.intc)
        Ap, Aj, Ax = ic(Atilde.indptr), ic(Atilde.indices), np.ascontiguousarray(Atilde.data, dtype=np.float64)
        Bp, Bj, Bx = ic(AtildeCSC.indptr), ic(AtildeCSC.indices), np.ascontiguousarray(AtildeCSC.data, dtype=np.float64)
        Sp, Sj = ic(mask.indptr), ic(mask.indices)
        Sx = np.ascontiguousarray(mask.data, dtype=np.float64)
        host_lib().amgsetup_incomplete_mat_mult_csr(_ip(Ap), _ip(Aj), _dp(Ax), _ip(Bp), _ip(Bj), _dp(Bx), _ip(Sp), _ip(Sj),
                                                    _dp(Sx), int(dimen))
        mask.data = Sx
        del AtildeCSC, Atilde
        Atilde = mask
        Atilde.eliminate_zeros()
        Atilde.sort_indices()
    del Dinv_A, mask

    # the one-candidate shortcut (strength.py:690-737): Strength(i, j) = |1 - (z(i) / b(j)) / (z(j) / b(i))|
    b = b.copy()
    b[b == 0] = 1.0
    DAtilde = Atilde.diagonal()
    DAtildeDivB = np.ravel(DAtilde) / b
    data = Atilde.data.copy()
    counts = np.diff(Atilde.indptr)
    zt = np.ones_like(data) * np.repeat(DAtildeDivB, counts)        # csr_scale_rows on a matrix of ones
    zt = zt * b[Atilde.indices]                                     # csr_scale_columns
    angle = (zt * data + 0.0 * 0.0) < 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = zt / data
    weak_ratio = (np.abs(ratio) < 1e-4)
    val = np.abs(1.0 - ratio)
    val[weak_ratio] = 0.0
    val[angle] = 0.0
    Atilde.data = val
    Atilde.eliminate_zeros()
    Atilde.data[Atilde.data < np.sqrt(np.finfo(float).eps)] = 1e-4
    del data, weak_ratio, angle
    Atilde.data = np.array(np.real(Atilde.data), dtype=float)

    # drop tolerance (strength.py:779-783)
    if epsilon != np.inf:
        Sp, Sj = np.ascontiguousarray(Atilde.indptr, dtype=np.intc), np.ascontiguousarray(Atilde.indices, dtype=np.intc)
        Sx = np.ascontiguousarray(Atilde.data, dtype=np.float64)
        host_lib().amgsetup_apply_distance_filter(int(dimen), float(epsilon), _ip(Sp), _ip(Sj), _dp(Sx), 0)
        Atilde.data = Sx
        Atilde.eliminate_zeros()

    if symmetrize_measure:
        Atilde = 0.5 * (Atilde + Atilde.T)

    # every point is strongly connected to itself (strength.py:789-792)
    I = sparse.eye(dimen, dimen, format="csr")
    I.data -= Atilde.diagonal()
    Atilde = Atilde + I

    if not csrflag:
        # strength.py:796-807 for 1 x 1 blocks: the block's smallest non-zero value, DBL_MAX when it has none (min_blocks)
        Atilde = Atilde.tobsr(blocksize=(1, 1))
        blocks = np.ravel(np.asarray(Atilde.data))
        CSRdata = np.where(blocks != 0.0, blocks, _DBL_MAX)
        Atilde = csr_matrix((CSRdata, Atilde.indices, Atilde.indptr), shape=Atilde.shape)

    Atilde.data = 1.0 / Atilde.data

    # scale_rows_by_largest_entry (util/utils.py:1830-1869; maximum_row_value counts up from DBL_MIN)
    counts = np.diff(Atilde.indptr)
    largest = np.full(Atilde.shape[0], _DBL_MIN)
    rows = np.repeat(np.arange(Atilde.shape[0]), counts)
    np.maximum.at(largest, rows, np.abs(Atilde.data))
    largest[largest != 0] = 1.0 / largest[largest != 0]
    Atilde = csr_matrix((Atilde.data * np.repeat(largest, counts), Atilde.indices, Atilde.indptr), shape=Atilde.shape)
    return Atilde


def _device_measure(A, b, rho, epsilon, k, symmetrize_measure, times=None):
    """the pipeline of csrc/strength.hip on a sorted CSR operator without stored zeros; None when the operator holds
    duplicate entries (the host path then does what scipy does with them).  times: a list that receives
    (upload, stages, fetch) in milliseconds."""
    from . import _lib
    if not A.has_canonical_format:
        return None
    L = _lib.lib()
    n = A.shape[0]
    Ap = np.ascontiguousarray(A.indptr, dtype=np.int64)
    Aj = np.ascontiguousarray(A.indices, dtype=np.intc)
    Ax = np.ascontiguousarray(A.data, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    Cp = np.empty(n + 1, dtype=np.int64)
    handle = C.c_void_p()
    ms = (C.c_double * 2)()
    _lib.check(L.amg_evolution_strength_device(n, Ap.ctypes.data, Aj.ctypes.data, Ax.ctypes.data, b.ctypes.data,
                                               float(rho), float(epsilon), int(k), int(bool(symmetrize_measure)),
                                               Cp.ctypes.data, C.byref(handle), ms))
    nnz = int(Cp[n])
    (Cj, Cx), fetch_ms = _lib.fetch_result(handle, L.amg_strength_fetch, [(nnz, np.intc), (nnz, np.float64)])
    if times is not None:
        times.extend([ms[0], ms[1], fetch_ms])
    if nnz >= 2 ** 31:
        raise ValueError("strength matrix exceeds int32 indices")
    return csr_matrix((Cx, Cj, Cp.astype(np.intc)), shape=A.shape)
