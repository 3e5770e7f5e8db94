"""Energy-minimisation prolongation smoothing (pyamg/aggregation/smooth.py:904-1177 with krylov='cg', :283-457).

``energy_prolongation_smoother`` takes a real float64 operator, CSR or BSR of any block size, and any number of
candidates, by one of two routes that return the same bits in the same stored order:

  host    the reference's statements restated with numpy / scipy; its three native steps (the incomplete block product,
          the constraint projection, B_i^T B_i), the block-row product U B_c and the inner product in
          csrc/setup_host.cpp;
  device  the sparsity pattern, BtBinv and the row weights are computed on the host and uploaded once with A, T and
          B_c; the whole CG iteration runs in HBM (csrc/energy.hip, amg_energy_smooth_device) and two small reads per
          iteration come back.

Both iterate on ONE fixed pattern, Atilde^degree T un-amalgamated and sorted: where the reference lets scipy's sparse
sums drop zero results, a stored 0.0 stays here; it contributes what a missing entry contributes, and the final
eliminate_zeros() removes all-zero blocks either way.  The result has sorted rows.  Unlike the
reference, neither route changes its arguments (the reference sorts T and removes its zero blocks in place).

Root-node smoothing (Cpt_params = (True, {'P_I', 'I_F', ...}) from util.get_Cpt_params) is the
same iteration with the root-node rules on that fixed pattern: the pattern is I_F * pattern + P_I (every root row holds
its one block), T is fitted to T B_c = B_f first when B has more columns than A's blocks have rows, and the root block
of every column is set back to the identity after the fit and after every T += alpha P -- the reference's
T = I_F * T + P_I; R, Z, P and AP are not masked.  prefilter ({'k'}, {'theta'} or both) cuts the pattern before the
iteration, postfilter cuts the smoothed T and re-fits it in one second pass; both need root-node parameters.

Outside the restated setup (NotImplementedError): krylov 'cgnr' and 'gmres', weighting='block', prefilter / postfilter
without root-node parameters, a true Cpt_params[0] without P_I and I_F, complex or non-float64 operators.
"""
import ctypes as C

import numpy as np
from scipy.sparse import bsr_matrix, csr_matrix, isspmatrix_bsr, isspmatrix_csr

from . import _lib
from ._host import attempt, dp as _dp, f64 as _dc, host_lib, i32 as _ic, ip as _ip, outside as _outside, route

__all__ = ["energy_prolongation_smoother"]

# What device=None does when a GPU is present: decided by the measurement in profiles/r14_energy_smoothing.txt
# (DESIGN.md section 8f).
DEVICE_AUTO = False


def _prefiltered(S, prefilter):
    """smooth.py:1093-1124: the rows of S cut to their k largest entries, to the entries at or above theta times the
    row's largest, or (both keys) to the union of the two"""
    from .util import filter_matrix_rows, truncate_rows
    if "theta" in prefilter and "k" in prefilter:
        return truncate_rows(S, prefilter["k"]) + filter_matrix_rows(S, prefilter["theta"])
    if "k" in prefilter:
        return truncate_rows(S, prefilter["k"])
    return filter_matrix_rows(S, prefilter["theta"])


def sparsity_pattern(T, Atilde, degree, prefilter=None, root=None):
    """smooth.py:1078-1132: the block pattern of Atilde^degree T (T itself for degree 0) as sorted (indptr, indices)
    over T's block grid.  T: bsr_matrix.
    prefilter ({'k'}, {'theta'} or both): applied to the amalgamated product as scipy returns it, its entries being the
    path counts, BEFORE the rows are sorted -- equal counts tie all the time and the stored order decides which
    survive (util.truncate_rows); with degree 0 it filters the scalar rows of T's own values.
    root (I_F, P_I as block-level csr patterns): I_F * pattern + P_I, i.e. every root row holds its one block."""
    R, Cc = T.blocksize
    shape = (T.shape[0] // R, T.shape[1] // Cc)
    S = csr_matrix((np.ones(T.indices.shape), T.indices.copy(), T.indptr.copy()), shape=shape)
    if degree > 0:
        S.sort_indices()
        At = csr_matrix((np.ones(Atilde.indices.shape), Atilde.indices, Atilde.indptr), shape=Atilde.shape)
        for _ in range(degree):
            S = At * S
        if prefilter:
            S = csr_matrix(_prefiltered(S, prefilter))
    elif prefilter:
        F = bsr_matrix(_prefiltered(T, prefilter), blocksize=(R, Cc))
        S = csr_matrix((np.ones(F.indices.shape), F.indices, F.indptr), shape=shape)
        S.sum_duplicates()
    else:
        S.sum_duplicates()
    if root is not None:
        S.data[:] = 1.0
        S = csr_matrix(root[0] * S + root[1])
    S.sort_indices()
    return _ic(S.indptr), _ic(S.indices)


def _root_structure(P_I, I_F, n_brow, n_bcol, R, Cc):
    """-> (root_row: the block row of every coarse block column's root node; I_F and P_I as block-level csr patterns)"""
    if not (isspmatrix_bsr(P_I) and isspmatrix_bsr(I_F)):
        raise TypeError("Cpt_params: P_I and I_F must be bsr_matrix")
    if R != Cc or P_I.blocksize != (R, Cc) or I_F.blocksize != (R, R) or P_I.shape != (n_brow * R, n_bcol * Cc) \
            or I_F.shape != (n_brow * R, n_brow * R):
        raise ValueError("Cpt_params: P_I and I_F must have the shapes and the square blocks of T and A")
    PI = csr_matrix((np.ones(len(P_I.indices)), P_I.indices.copy(), P_I.indptr.copy()), shape=(n_brow, n_bcol))
    IF = csr_matrix((np.ones(len(I_F.indices)), I_F.indices.copy(), I_F.indptr.copy()), shape=(n_brow, n_brow))
    rows = np.repeat(np.arange(n_brow), np.diff(PI.indptr))
    if len(rows) == 0:
        return None, IF, PI                 # the trivial coarse grid: no root node
    if len(rows) != n_bcol or np.diff(PI.indptr).max() > 1 or len(np.unique(PI.indices)) != n_bcol:
        raise ValueError("Cpt_params: P_I must hold one block per coarse node, each in a row of its own")
    if not np.array_equal(P_I.data, np.broadcast_to(np.eye(R), P_I.data.shape)):
        raise ValueError("Cpt_params: the blocks of P_I must be identities")
    if np.intersect1d(rows, IF.indices).size:
        raise ValueError("Cpt_params: I_F must be empty at the root nodes")
    root_row = np.empty(n_bcol, dtype=np.intc)
    root_row[PI.indices] = rows
    return root_row, IF, PI


def pinv_array(a, cond=None):
    """util/linalg.py:583-649: every m x m block of a (n, m, m) replaced by its pseudo-inverse.  1 x 1: 1 / a, and 0
    where a is 0; otherwise LAPACK gelss against the identity with the reference's cond (eps * 1e6 for float64)."""
    n, m = a.shape[0], a.shape[1]
    if m == 1:
        zero = (a == 0.0).nonzero()[0]
        a[zero] = 1.0
        a[:] = 1.0 / a
        a[zero] = 0.0
        return
    from scipy.linalg.lapack import _compute_lwork, get_lapack_funcs
    gelss, gelss_lwork = get_lapack_funcs(("gelss", "gelss_lwork"), (np.ones((1,), dtype=a.dtype),))
    RHS = np.eye(m, dtype=a.dtype)
    lwork = _compute_lwork(gelss_lwork, m, m, m)
    if cond is None:
        cond = np.finfo(np.float64).eps * 1e6
    for kk in range(n):
        a[kk] = gelss(a[kk], RHS, cond=cond, lwork=lwork, overwrite_a=True, overwrite_b=False)[1]


def calc_BtB(B, Sp, Sj, n_brow, Cc):
    """the first half of compute_BtBinv (util/utils.py:1684-1698): B_i^T B_i per block row of the pattern, (n_brow, k, k)"""
    ND = B.shape[1]
    BsqCols = ND * (ND + 1) // 2
    Bsq = np.zeros((B.shape[0], BsqCols), dtype=np.float64)
    counter = 0
    for i in range(ND):
        for j in range(i, ND):
            Bsq[:, counter] = B[:, i] * B[:, j]
            counter += 1
    BtB = np.zeros((n_brow, ND, ND), dtype=np.float64)
    host_lib().amgsetup_calc_BtB(ND, n_brow, Cc, _dp(Bsq), BsqCols, _dp(BtB), _ip(Sp), _ip(Sj))
    return BtB


def compute_BtBinv(B, Sp, Sj, n_brow, Cc):
    """util/utils.py:1617-1707 on the pattern's arrays"""
    BtBinv = calc_BtB(B, Sp, Sj, n_brow, Cc).transpose((0, 2, 1)).copy()
    pinv_array(BtBinv)
    return BtBinv


def _weights(A, weighting):
    """the diagonal preconditioner of smooth.py:346-360, one weight per scalar row"""
    if weighting == "diagonal":
        D = np.asarray(A.diagonal(), dtype=np.float64).ravel()
        Dinv = np.zeros_like(D)
        mask = (D != 0.0)
        Dinv[mask] = 1.0 / D[mask]
        return Dinv
    D = np.ravel(abs(A) * np.ones((A.shape[0], 1), dtype=A.dtype))          # Gershgorin
    Dinv = np.zeros_like(D)
    Dinv[D != 0] = 1.0 / np.abs(D[D != 0])
    return Dinv


def _scatter(T, Sp, Sj):
    """-> (T's blocks on the pattern, zero blocks elsewhere, raveled; per stored block of T whether the pattern holds it)"""
    R, Cc = T.blocksize
    n_brow, n_bcol = T.shape[0] // R, T.shape[1] // Cc
    rows = np.repeat(np.arange(n_brow, dtype=np.int64), np.diff(T.indptr))
    keys = rows * n_bcol + T.indices
    pat = np.repeat(np.arange(n_brow, dtype=np.int64), np.diff(Sp)) * n_bcol + Sj        # ascending: rows sorted and unique
    at = np.minimum(np.searchsorted(pat, keys), len(pat) - 1)
    inside = pat[at] == keys
    Tx = np.zeros((len(Sj), R, Cc), dtype=np.float64)
    np.add.at(Tx, at[inside], T.data[inside])       # a block T stores twice is summed, as scipy reads such a matrix
    return Tx.ravel(), inside


def fit_on_pattern(L, n_brow, R, Cc, ND, Sp, Sj, Tx, Bc, Bf, BtBinv):
    """the arithmetic of util.filter_operator on values Tx of the pattern: diff = T B_c - B_f (the block-row product,
    then one subtraction per scalar), then T_i <- T_i - diff_i BtBinv_i B_i^T.  Returns the fitted values."""
    Tx = Tx.copy()
    diff = np.empty(n_brow * R * ND, dtype=np.float64)
    L.amgsetup_energy_block_row_product(n_brow, R, Cc, ND, _ip(Sp), _ip(Sj), _dp(Tx), _dp(Bc), _dp(diff))
    diff = diff - Bf
    L.amgsetup_satisfy_constraints_helper(R, Cc, n_brow, ND, _dp(Bc), _dp(diff), _dp(BtBinv), _ip(Sp), _ip(Sj), _dp(Tx))
    return Tx


class _Plan(object):
    """everything both routes share: A's arrays, the pattern, T on it, B_c, BtBinv and the row weights; for root-node
    smoothing root_row (the block row of every column's root) and root_at (that row's single block on the pattern);
    Bf (raveled) when the initial fit T B_c = B_f runs"""
    root_row = None
    root_at = None
    Bf = None


def _set_identity(p, Tx):
    """the single block of every root row becomes the identity: the reference's T = I_F * T + P_I on the fixed pattern"""
    Tx.reshape(-1, p.R, p.Cc)[p.root_at] = np.eye(p.R)


def _cg_host(p, maxiter, tol, trace=None):
    """smooth.py:362-457 on the fixed pattern; returns T's values on the pattern"""
    L = host_lib()
    n_brow, n_bcol, R, Cc, ND = p.n_brow, p.n_bcol, p.R, p.Cc, p.ND
    Sp, Sj = p.Sp, p.Sj
    UB = np.empty(n_brow * R * ND, dtype=np.float64)
    out = np.empty(2, dtype=np.float64)
    row_weight = np.repeat(np.repeat(p.Dinv.reshape(-1, R), np.diff(Sp), axis=0), Cc, axis=1).ravel()

    def product(X, S):                      # X on the pattern is its own right operand
        L.amgsetup_incomplete_mat_mult_bsr(_ip(p.Ap), _ip(p.Aj), _dp(p.Ax), _ip(Sp), _ip(Sj), _dp(X), _ip(Sp), _ip(Sj),
                                           _dp(S), n_brow, n_bcol, R, R, Cc)

    def project(U):
        L.amgsetup_energy_block_row_product(n_brow, R, Cc, ND, _ip(Sp), _ip(Sj), _dp(U), _dp(p.Bc), _dp(UB))
        L.amgsetup_satisfy_constraints_helper(R, Cc, n_brow, ND, _dp(p.Bc), _dp(UB), _dp(p.BtBinv), _ip(Sp), _ip(Sj), _dp(U))

    def inner(X, Y):
        L.amgsetup_energy_inner_product(n_brow, R * Cc, _ip(Sp), _dp(X), _dp(Y), _dp(out))
        return np.float64(out[0]), out[1]

    Tx = p.Tx.copy()
    Rx = np.zeros_like(Tx)
    if p.Bf is not None:
        # the initial fit (smooth.py:1142-1146): T lives on the pattern from here on
        Tx = fit_on_pattern(L, n_brow, R, Cc, ND, Sp, Sj, Tx, p.Bc, p.Bf, p.BtBinv)
        if p.root_at is not None:
            _set_identity(p, Tx)
        product(Tx, Rx)
    else:
        # the first residual from T as it is stored: blocks of T outside the pattern enter here and nowhere else
        L.amgsetup_incomplete_mat_mult_bsr(_ip(p.Ap), _ip(p.Aj), _dp(p.Ax), _ip(p.Tp), _ip(p.Tj), _dp(p.Tdata), _ip(Sp), _ip(Sj),
                                           _dp(Rx), n_brow, n_bcol, R, R, Cc)
    Rx *= -1.0
    project(Rx)
    Px = None
    APx = np.empty_like(Tx)
    oldsum = np.float64(0.0)
    i = 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        while i < maxiter:
            Zx = Rx * row_weight
            newsum, nonzero = inner(Rx, Zx)
            if trace is not None:
                trace.append([float(newsum), 0.0])
            if nonzero == 0.0 or newsum < tol:
                break
            if i == 0:
                Px = Zx
            else:
                beta = newsum / oldsum
                Px = Zx + beta * Px
            oldsum = newsum
            APx[:] = 0.0
            product(Px, APx)
            project(APx)
            pAp, _ = inner(Px, APx)
            if trace is not None:
                trace[-1][1] = float(pAp)
            alpha = newsum / pAp
            Tx = Tx + alpha * Px
            if p.root_at is not None:       # nothing else is masked: R, Z, P and AP keep what the arithmetic leaves
                _set_identity(p, Tx)
            Rx = Rx - alpha * APx
            i += 1
    return Tx, i


def _cg_device(p, maxiter, tol, trace=None, times=None):
    """the same iteration by csrc/energy.hip; times: a list that receives (upload, iterations, fetch) in milliseconds"""
    L = _lib.lib()
    handle = C.c_void_p()
    ms = (C.c_double * 2)()
    its = C.c_int(0)
    tr = np.zeros(2 * max(maxiter, 1), dtype=np.float64)
    if p.root_row is None and p.Bf is None:
        _lib.check(L.amg_energy_smooth_device(p.n_brow, p.n_bcol, p.R, p.Cc, p.ND, p.Ap.ctypes.data, p.Aj.ctypes.data,
                                              p.Ax.ctypes.data, p.Sp.ctypes.data, p.Sj.ctypes.data, p.Tx.ctypes.data,
                                              p.Bc.ctypes.data, p.BtBinv.ctypes.data, p.Dinv.ctypes.data, int(maxiter), float(tol),
                                              C.byref(handle), C.byref(its), tr.ctypes.data, ms))
    else:
        if p.root_row is None:
            raise _outside("the device route for an initial fit without root nodes")
        _lib.check(L.amg_energy_smooth_rootnode_device(p.n_brow, p.n_bcol, p.R, p.Cc, p.ND, p.Ap.ctypes.data, p.Aj.ctypes.data,
                                                       p.Ax.ctypes.data, p.Sp.ctypes.data, p.Sj.ctypes.data, p.Tx.ctypes.data,
                                                       p.Bc.ctypes.data, p.BtBinv.ctypes.data, p.Dinv.ctypes.data,
                                                       p.root_row.ctypes.data, None if p.Bf is None else p.Bf.ctypes.data,
                                                       int(maxiter), float(tol), C.byref(handle), C.byref(its),
                                                       tr.ctypes.data, ms))
    (Tx,), fetch_ms = _lib.fetch_result(handle, L.amg_energy_fetch, [(p.Tx.shape, p.Tx.dtype)])
    if times is not None:
        times.extend([ms[0], ms[1], fetch_ms])
    if trace is not None:
        started = min(maxiter, its.value + 1)
        trace.extend([float(tr[2 * q]), float(tr[2 * q + 1])] for q in range(started))
    return Tx, its.value


def energy_prolongation_smoother(A, T, Atilde, B, Bf, Cpt_params, krylov="cg", maxiter=4, tol=1e-8, degree=1,
                                 weighting="local", prefilter={}, postfilter={}, device=None, _trace=None, _times=None):
    """Minimise the energy of the columns of T under the constraints T B_c = B_f and a sparsity pattern
    (smooth.py:904-1177), by CG.

    A : csr_matrix or bsr_matrix, float64, symmetric positive definite.  T : the tentative prolongator, csr or bsr
    with T.blocksize[0] == A.blocksize[0].  Atilde : csr strength matrix on A's block grid (None: A's own pattern).
    B : the coarse candidates, (T.shape[1], k).  Bf, Cpt_params : None and (False, {}), or for root-node smoothing the
    fine candidates (T.shape[0], k) and (True, the dictionary of util.get_Cpt_params).  prefilter, postfilter : {'k': the
    entries kept per row} and / or {'theta': the fraction of the row's largest magnitude below which an entry is
    dropped}, root-node smoothing only.  maxiter, tol : CG stops after maxiter iterations, when <R, Z> < tol or
    when the residual holds no non-zero.  degree : the pattern is Atilde^degree T.  weighting : 'local' (Gershgorin
    row sums) or 'diagonal'.
    device : True = the initial fit and the iteration in HBM, False = the host route, None = the host route unless DEVICE_AUTO and a
    GPU; under None, whatever the device route refuses goes to the host route.
    Returns the smoothed prolongator as bsr_matrix with sorted rows and no all-zero blocks."""
    if maxiter < 0:
        raise ValueError("maxiter must be > 0")
    if tol > 1:
        raise ValueError("tol must be <= 1")
    if krylov != "cg":
        raise _outside("energy smoothing with krylov=%r" % (krylov,))
    if weighting == "block":
        raise _outside("energy smoothing with weighting='block'")
    if weighting not in ("local", "diagonal"):
        raise ValueError("weighting value is invalid")
    root = bool(Cpt_params[0])
    if root and not ("P_I" in Cpt_params[1] and "I_F" in Cpt_params[1]):
        raise _outside("root-node energy smoothing without the operators P_I and I_F in Cpt_params[1]")
    if (len(prefilter) > 0 or len(postfilter) > 0) and not root:
        raise _outside("energy smoothing with a prefilter or postfilter but without root-node parameters")
    if not set(prefilter) <= {"k", "theta"}:
        raise ValueError("Unrecognized prefilter option")
    if not (set(postfilter) <= {"k", "theta"} or set(postfilter) == {"secondpass"}):
        raise ValueError("Unrecognized postfilter option")
    if not (isspmatrix_csr(A) or isspmatrix_bsr(A)):
        raise TypeError("A must be csr_matrix or bsr_matrix")
    if not (isspmatrix_csr(T) or isspmatrix_bsr(T)):
        raise TypeError("T must be csr_matrix or bsr_matrix")
    if A.dtype.kind == "c" or T.dtype.kind == "c" or np.iscomplexobj(B):
        raise _outside("energy smoothing of a complex operator")
    if A.dtype != np.float64 or T.dtype != np.float64:
        raise _outside("energy smoothing of a %s operator" % (A.dtype if A.dtype != np.float64 else T.dtype))
    if isspmatrix_csr(A):
        A = A.tobsr(blocksize=(1, 1), copy=False)
    if isspmatrix_csr(T):
        T = T.tobsr(blocksize=(1, 1), copy=False)
    if T.blocksize[0] != A.blocksize[0]:
        raise ValueError("T row-blocksize should be the same as A blocksize")
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] != T.shape[1]:
        raise ValueError("B is the candidates for the coarse grid.  num_rows(b) = num_cols(T)")
    if B.dtype != np.float64:
        raise _outside("energy smoothing with %s candidates" % B.dtype)
    if A.shape[0] != A.shape[1] or A.blocksize[0] != A.blocksize[1] or A.shape[0] != T.shape[0]:
        raise ValueError("A must be square with square blocks and as many rows as T")

    def finished(M):
        M = bsr_matrix(M, copy=True)
        M.eliminate_zeros()
        return M

    if min(T.nnz, A.nnz) == 0:
        return finished(T)
    R, Cc = T.blocksize
    n_brow, n_bcol = T.shape[0] // R, T.shape[1] // Cc
    if Atilde is None:
        Atilde = csr_matrix((np.ones(len(A.indices)), A.indices.copy(), A.indptr.copy()), shape=(n_brow, n_brow))
    elif not isspmatrix_csr(Atilde):
        raise TypeError("Atilde must be csr_matrix")
    if degree > 0 and Atilde.shape != (n_brow, n_brow):
        raise ValueError("Atilde must have one row per block row of A")

    p = _Plan()
    p.n_brow, p.n_bcol, p.R, p.Cc, p.ND = n_brow, n_bcol, R, Cc, B.shape[1]
    structure = None
    if root:
        p.root_row, IF, PI = _root_structure(Cpt_params[1]["P_I"], Cpt_params[1]["I_F"], n_brow, n_bcol, R, Cc)
        structure = (IF, PI)
    p.Sp, p.Sj = sparsity_pattern(T, Atilde, int(degree), prefilter, structure)
    if len(p.Sj) == 0:
        return finished(T)
    if p.root_row is not None:
        p.root_at = p.Sp[p.root_row].astype(np.int64)
    p.Tx, inside = _scatter(T, p.Sp, p.Sj)
    p.Tp, p.Tj, p.Tdata = _ic(T.indptr), _ic(T.indices), _dc(T.data).ravel()
    if (root and B.shape[1] > A.blocksize[0]) or "secondpass" in postfilter:
        # the initial fit drops the blocks of T outside the pattern and re-fits T B_c = B_f
        if Bf is None:
            raise ValueError("the fine candidates Bf are needed to fit T B_c = B_f")
        Bf = np.asarray(Bf)
        if Bf.ndim != 2 or Bf.shape != (T.shape[0], B.shape[1]):
            raise ValueError("Bf is the candidates for the fine grid.  Bf.shape = (num_rows(T), num_cols(B))")
        if Bf.dtype != np.float64:
            raise _outside("energy smoothing with %s candidates" % Bf.dtype)
        p.Bf = _dc(Bf).ravel()
        inside = np.ones(len(T.indices), dtype=bool)
    if device is True and not inside.all():
        raise _outside("the device route for a tentative prolongator with blocks outside Atilde^degree T "
                       "(Atilde without a stored diagonal)")
    p.Ap, p.Aj, p.Ax = _ic(A.indptr), _ic(A.indices), _dc(A.data).ravel()
    p.Bc = _dc(B).ravel()
    p.BtBinv = _dc(compute_BtBinv(_dc(B), p.Sp, p.Sj, n_brow, Cc)).ravel()
    p.Dinv = _dc(_weights(A, weighting))

    Tx, _ = attempt(route(device, DEVICE_AUTO) if inside.all() else False,
                    lambda: _cg_device(p, int(maxiter), float(tol), _trace, _times),
                    lambda: _cg_host(p, int(maxiter), float(tol), _trace),
                    (NotImplementedError, ValueError, MemoryError, _lib.AmgError))      # whatever _lib.check raises
    P = bsr_matrix((Tx.reshape(-1, R, Cc), p.Sj.copy(), p.Sp.copy()), shape=T.shape)
    if not inside.all():                    # T's blocks outside the pattern are never updated: x + 0.0
        P = P + bsr_matrix((T.data * (~inside)[:, None, None], T.indices, T.indptr), shape=T.shape)
        P.sort_indices()
    P.eliminate_zeros()
    if len(postfilter) == 0 or "secondpass" in postfilter:
        return P
    # smooth.py:1163-1196: filter the smoothed prolongator by scalar rows, then one second pass that re-fits
    # T B_c = B_f on the filtered pattern and takes a single CG step there
    from .util import filter_matrix_rows, truncate_rows
    if "theta" in postfilter and "k" in postfilter:
        keep = filter_matrix_rows(P, postfilter["theta"])
        keep_k = truncate_rows(P, postfilter["k"])
        keep.data[:] = 1.0
        keep_k.data[:] = 1.0
        keep = keep + keep_k
        keep.data[:] = 1.0
        filtered = bsr_matrix(P.multiply(keep), blocksize=P.blocksize)
    elif "k" in postfilter:
        filtered = truncate_rows(P, postfilter["k"])
    else:
        filtered = filter_matrix_rows(P, postfilter["theta"])
    return energy_prolongation_smoother(A, filtered, Atilde, B, Bf, Cpt_params, krylov=krylov, maxiter=1, tol=1e-8, degree=0,
                                        weighting=weighting, prefilter={}, postfilter={"secondpass": True}, device=device,
                                        _trace=_trace, _times=_times)
