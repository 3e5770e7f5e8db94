"""Drop-in for the hot-path part of ``pyamg.amg_core`` (the SWIG module of the
reference, /root/reference/pyamg/amg_core/amg_core.i:184-195), backed by HIP
kernels on MI355X through libamgcore_hip.so.

Same call signatures as the SWIG wrappers: numpy arrays are passed whole (one
argument per C++ ``(T*, int size)`` pair) and mutated in place; the return value
is None.  Like the reference, every entry takes float32, float64, complex64 or
complex128 values with int32 indices: the dtype of the value arrays picks the
native instantiation (symbol suffix ``_f32``, ``_f64``, ``_c64``, ``_c128``).
Like the SWIG overload dispatcher (amg_core_wrap.cxx:9209-9215) a call whose
value arrays do not share one of those dtypes, or whose index arrays are not
int32, raises ``NotImplementedError``; non-contiguous arrays raise ``TypeError``.
"""
import numpy as np

from . import _lib

__all__ = ["gauss_seidel", "bsr_gauss_seidel", "jacobi", "bsr_jacobi", "gauss_seidel_indexed",
           "jacobi_ne", "gauss_seidel_ne", "gauss_seidel_nr", "block_jacobi", "block_gauss_seidel",
           "csr_matvec", "bsr_matvec", "overlapping_schwarz_csr", "extract_subblocks",
           "incomplete_mat_mult_csr", "apply_distance_filter", "apply_absolute_distance_filter", "min_blocks",
           "incomplete_mat_mult_bsr", "satisfy_constraints_helper", "calc_BtB", "truncate_rows_csr",
           "maximal_independent_set_parallel", "maximal_independent_set_k_parallel", "cljp_naive_splitting", "classical_strength_of_connection",
           "maximum_row_value", "rs_direct_interpolation_pass1", "rs_direct_interpolation_pass2"]

_INDEX = np.dtype(np.intc)


def _overload_error(name):
    return NotImplementedError(
        "Wrong number or type of arguments for overloaded function '%s' "
        "(values: one of float32, float64, complex64, complex128; indices: int32)" % name)


def _check_arrays(name, kinds, args):
    """The SWIG typechecks: int32 index arrays, value arrays of ONE supported dtype, 1-d, contiguous.
    Returns the symbol suffix of that dtype."""
    suffix = None
    for kind, a in zip(kinds, args):
        if kind not in "IV":
            continue
        if not isinstance(a, np.ndarray):
            raise TypeError("%s: numpy array expected" % name)
        if kind == "I":
            if a.dtype != _INDEX:
                raise _overload_error(name)
        else:
            s = _lib.VALUE_SUFFIX.get(a.dtype)
            if s is None or (suffix is not None and s != suffix):
                raise _overload_error(name)
            suffix = s
        if a.ndim != 1:
            raise ValueError("%s: array must have 1 dimension" % name)
        if not a.flags.c_contiguous:
            raise TypeError("%s: array must be contiguous" % name)
    return suffix


def _call(name, *args):
    """Forward one call of the flat table to the native entry of the value dtype."""
    kinds, sized = _lib.FLAT_TABLE[name]
    if len(args) != len(kinds):
        raise TypeError("%s: %d arguments expected" % (name, len(kinds)))
    suffix = _check_arrays(name, kinds, args)
    if suffix is None and name in _lib.FLAT_F64_ONLY:
        suffix = "f64"              # an entry of index arrays alone has the one instantiation
    if name in _lib.FLAT_F64_ONLY and suffix != "f64":
        raise _overload_error(name)
    vptr, real = _lib.VALUE_CTYPES[suffix]
    cargs = []
    for kind, a in zip(kinds, args):
        if kind in "IV":
            cargs.append(a.ctypes.data_as(_lib.c_int_p if kind == "I" else vptr))
            if sized:
                cargs.append(len(a))
        elif kind == "i":
            cargs.append(int(a))
        else:
            cargs.append(real(float(a)))
    _lib.check(getattr(_lib.lib(), "amgcore_%s_%s" % (name, suffix))(*cargs))


def gauss_seidel(Ap, Aj, Ax, x, b, row_start, row_stop, row_step):
    _call("gauss_seidel", Ap, Aj, Ax, x, b, row_start, row_stop, row_step)


def bsr_gauss_seidel(Ap, Aj, Ax, x, b, row_start, row_stop, row_step, blocksize):
    _call("bsr_gauss_seidel", Ap, Aj, Ax, x, b, row_start, row_stop, row_step, blocksize)


def jacobi(Ap, Aj, Ax, x, b, temp, row_start, row_stop, row_step, omega):
    _call("jacobi", Ap, Aj, Ax, x, b, temp, row_start, row_stop, row_step, omega)


def bsr_jacobi(Ap, Aj, Ax, x, b, temp, row_start, row_stop, row_step, blocksize, omega):
    _call("bsr_jacobi", Ap, Aj, Ax, x, b, temp, row_start, row_stop, row_step, blocksize, omega)


def gauss_seidel_indexed(Ap, Aj, Ax, x, b, Id, row_start, row_stop, row_step):
    _call("gauss_seidel_indexed", Ap, Aj, Ax, x, b, Id, row_start, row_stop, row_step)


def jacobi_ne(Ap, Aj, Ax, x, b, Tx, temp, row_start, row_stop, row_step, omega):
    _call("jacobi_ne", Ap, Aj, Ax, x, b, Tx, temp, row_start, row_stop, row_step, omega)


def gauss_seidel_ne(Ap, Aj, Ax, x, b, row_start, row_stop, row_step, Tx, omega):
    _call("gauss_seidel_ne", Ap, Aj, Ax, x, b, row_start, row_stop, row_step, Tx, omega)


def gauss_seidel_nr(Ap, Aj, Ax, x, z, col_start, col_stop, col_step, Tx, omega):
    _call("gauss_seidel_nr", Ap, Aj, Ax, x, z, col_start, col_stop, col_step, Tx, omega)


def block_jacobi(Ap, Aj, Ax, x, b, Tx, temp, row_start, row_stop, row_step, omega, blocksize):
    _call("block_jacobi", Ap, Aj, Ax, x, b, Tx, temp, row_start, row_stop, row_step, omega, blocksize)


def block_gauss_seidel(Ap, Aj, Ax, x, b, Tx, row_start, row_stop, row_step, blocksize):
    _call("block_gauss_seidel", Ap, Aj, Ax, x, b, Tx, row_start, row_stop, row_step, blocksize)


def csr_matvec(n_row, n_col, Ap, Aj, Ax, Xx, Yx):
    """scipy.sparse._sparsetools.csr_matvec signature: Yx += A * Xx."""
    _call("csr_matvec", n_row, n_col, Ap, Aj, Ax, Xx, Yx)


def bsr_matvec(n_brow, n_bcol, R, C, Ap, Aj, Ax, Xx, Yx):
    """scipy.sparse._sparsetools.bsr_matvec signature: Yx += A * Xx."""
    _call("bsr_matvec", n_brow, n_bcol, R, C, Ap, Aj, Ax, Xx, Yx)


def overlapping_schwarz_csr(Ap, Aj, Ax, x, b, Tx, Tp, Sj, Sp, nsdomains, nrows, row_start, row_stop, row_step):
    """relaxation.h:935-1007: one sweep of multiplicative overlapping Schwarz (HIP, by dependency levels)"""
    _call("overlapping_schwarz_csr", Ap, Aj, Ax, x, b, Tx, Tp, Sj, Sp, nsdomains, nrows, row_start, row_stop,
          row_step)


def incomplete_mat_mult_csr(Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, Sx, dimen):
    """evolution_strength.h:575-699: Sx[ptr] = <A[row, :], B[:, col]> on the pattern of S (A, S sorted CSR; B sorted
    CSC); float64"""
    _call("incomplete_mat_mult_csr", Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, Sx, dimen)


def apply_distance_filter(n_row, epsilon, Sp, Sj, Sx):
    """evolution_strength.h:136-167: per row, off-diagonal values >= epsilon * (smallest off-diagonal value) become
    0.0 and the diagonal 1.0, in place; float64"""
    _call("apply_distance_filter", n_row, epsilon, Sp, Sj, Sx)


def apply_absolute_distance_filter(n_row, epsilon, Sp, Sj, Sx):
    """evolution_strength.h:61-83: off-diagonal values >= epsilon become 0.0 and the diagonal 1.0, in place; float64"""
    _call("apply_absolute_distance_filter", n_row, epsilon, Sp, Sj, Sx)


def min_blocks(n_blocks, blocksize, Sx, Tx):
    """evolution_strength.h:213-237: Tx[i] = the smallest non-zero value of block i of Sx (DBL_MAX when it has
    none); float64"""
    _call("min_blocks", n_blocks, blocksize, Sx, Tx)


def incomplete_mat_mult_bsr(Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, Sx, n_brow, n_bcol, brow_A, bcol_A, bcol_B):
    """smoothed_aggregation.h:797-869: Sx += A * B on the block pattern of S (BSR, rows in any order; of two slots of
    one row with the same column the later receives everything); float64"""
    _call("incomplete_mat_mult_bsr", Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, Sx, n_brow, n_bcol, brow_A, bcol_A, bcol_B)


def satisfy_constraints_helper(RowsPerBlock, ColsPerBlock, num_block_rows, NullDim, x, y, z, Sp, Sj, Sx):
    """smoothed_aggregation.h:556-605: x = conj(B_c), y = U * B_c, z = BtBinv, all raveled; every block (i, j) of S
    loses y_i * (z_i * x_j^T), in place; float64"""
    _call("satisfy_constraints_helper", RowsPerBlock, ColsPerBlock, num_block_rows, NullDim, x, y, z, Sp, Sj, Sx)


def calc_BtB(NullDim, Nnodes, ColsPerBlock, b, BsqCols, x, Sp, Sj):
    """smoothed_aggregation.h:656-734: x[i] = B_i^T B_i over the columns of block row i of S, from the products b of
    the candidates' columns; float64"""
    _call("calc_BtB", NullDim, Nnodes, ColsPerBlock, b, BsqCols, x, Sp, Sj)


def truncate_rows_csr(n_row, k, Sp, Sj, Sx):
    """smoothed_aggregation.h:898-960: every row longer than k keeps its k entries of largest magnitude, chosen and
    ordered as the reference's quicksort leaves them; the other entries become 0.0; Sj and Sx in place; float64"""
    _call("truncate_rows_csr", n_row, k, Sp, Sj, Sx)


def classical_strength_of_connection(n_row, theta, Ap, Aj, Ax, Sp, Sj, Sx):
    """ruge_stuben.h:46-93: Sp, Sj and Sx (as long as A's arrays) receive the diagonal of A and the off-diagonals with
    |a_ij| >= theta * max_k!=i |a_ik|, in A's stored order; float64"""
    _call("classical_strength_of_connection", n_row, theta, Ap, Aj, Ax, Sp, Sj, Sx)


def maximum_row_value(n_row, x, Ap, Aj, Ax):
    """ruge_stuben.h:110-130: x[i] = the largest magnitude of row i (DBL_MIN for an empty row); float64"""
    _call("maximum_row_value", n_row, x, Ap, Aj, Ax)


def rs_direct_interpolation_pass1(n_nodes, Sp, Sj, splitting, Bp):
    """ruge_stuben.h:497-516: the row offsets Bp of the direct-interpolation prolongator for the strength matrix S and
    the C/F splitting (1 = C, 0 = F); Bp[n_nodes] is its number of entries"""
    _call("rs_direct_interpolation_pass1", n_nodes, Sp, Sj, splitting, Bp)


def rs_direct_interpolation_pass2(n_nodes, Ap, Aj, Ax, Sp, Sj, Sx, splitting, Bp, Bj, Bx):
    """ruge_stuben.h:520-595: the columns Bj (in coarse numbering) and weights Bx of the prolongator whose offsets Bp
    pass 1 returned; float64"""
    _call("rs_direct_interpolation_pass2", n_nodes, Ap, Aj, Ax, Sp, Sj, Sx, splitting, Bp, Bj, Bx)


def extract_subblocks(Ap, Aj, Ax, Tx, Tp, Sj, Sp, nsdomains, nrows):
    """relaxation.h:836-899 (setup helper of the Schwarz smoother; runs on the host)"""
    from ._host import host_lib
    n = "extract_subblocks"
    suffix = _check_arrays(n, "IIVVIII", (Ap, Aj, Ax, Tx, Tp, Sj, Sp))
    if len(Sp) < nsdomains + 1 or len(Tp) < nsdomains + 1 or (nsdomains and len(Tx) < Tp[nsdomains]):
        raise ValueError("extract_subblocks: pointer arrays too short")
    fn = host_lib().amgsetup_extract_subblocks if suffix == "f64" else \
        getattr(host_lib(), "amgsetup_extract_subblocks_" + suffix)
    vptr = _lib.VALUE_CTYPES[suffix][0]
    fn(_lib.ip(Ap), _lib.ip(Aj), Ax.ctypes.data_as(vptr), Tx.ctypes.data_as(vptr), _lib.ip(Tp), _lib.ip(Sj),
       _lib.ip(Sp), int(nsdomains), int(nrows))


def _graph_arrays(name, n, index_arrays, value_arrays=()):
    """the typechecks of the two graph entries: int32 index arrays and float64 value arrays, 1-d, contiguous, long
    enough for n vertices"""
    for a in tuple(index_arrays) + tuple(value_arrays):
        if not isinstance(a, np.ndarray):
            raise TypeError("%s: numpy array expected" % name)
        if a.ndim != 1:
            raise ValueError("%s: array must have 1 dimension" % name)
        if not a.flags.c_contiguous:
            raise TypeError("%s: array must be contiguous" % name)
    if any(a.dtype != _INDEX for a in index_arrays) or any(a.dtype != np.float64 for a in value_arrays):
        raise NotImplementedError("Wrong number or type of arguments for overloaded function '%s' "
                                  "(indices and states: int32; weights: float64)" % name)
    if n < 0:
        raise ValueError("%s: negative size" % name)


def maximal_independent_set_parallel(num_rows, Ap, Aj, active, C, F, x, y, max_iters):
    """graph.h:90-156 run to completion on the device (csrc/split.hip): the active entries of x (int32) become C or F
    by Luby's rounds on the weights y (float64), the larger index winning a tie; the graph is taken as handed in and is
    expected to be structurally symmetric.  Returns the number of vertices that became C.  Only max_iters == -1: a
    limited number of in-place sweeps depends on the sweep order."""
    import ctypes
    n = "maximal_independent_set_parallel"
    num_rows = int(num_rows)
    _graph_arrays(n, num_rows, (Ap, Aj, x), (y,))
    if int(max_iters) != -1:
        raise NotImplementedError("%s: a sweep limit (max_iters=%d) is outside the restated setup" % (n, int(max_iters)))
    if len(Ap) < num_rows + 1 or len(x) < num_rows or len(y) < num_rows or (num_rows and len(Aj) < Ap[num_rows]):
        raise ValueError("%s: arrays shorter than the graph" % n)
    before = int(np.count_nonzero(x[:num_rows] == C))
    rounds = ctypes.c_int(0)
    _lib.check(_lib.lib().amg_mis_device(num_rows, Ap.ctypes.data, Aj.ctypes.data, y.ctypes.data, int(active), int(C), int(F),
                                         x.ctypes.data, ctypes.byref(rounds), None))
    return int(np.count_nonzero(x[:num_rows] == C)) - before


def maximal_independent_set_k_parallel(num_rows, Ap, Aj, k, x, y, max_iters):
    """graph.h:501-589 on the host (csrc/setup_host.cpp; the device route is pyamg_amd.graph.maximal_independent_set_k):
    x (int32) becomes 1 for the members of a distance-k independent set and 0 for the others, by at most max_iters
    rounds (-1: until the set is maximal) on the weights y (float64), the larger index winning a tie.  The graph is
    taken as handed in."""
    from .graph import mis_k
    n = "maximal_independent_set_k_parallel"
    num_rows = int(num_rows)
    _graph_arrays(n, num_rows, (Ap, Aj, x), (y,))
    if int(k) < 1:
        raise ValueError("%s: k must be at least 1" % n)
    if len(Ap) < num_rows + 1 or len(x) < num_rows or len(y) < num_rows or (num_rows and len(Aj) < Ap[num_rows]):
        raise ValueError("%s: arrays shorter than the graph" % n)
    if num_rows and (Ap[0] != 0 or np.any(np.diff(Ap[:num_rows + 1]) < 0)
                     or (Ap[num_rows] and (Aj[:Ap[num_rows]].min() < 0 or Aj[:Ap[num_rows]].max() >= num_rows))):
        raise ValueError("%s: not a CSR graph of num_rows vertices" % n)
    if num_rows:
        mis_k(num_rows, Ap, Aj, int(k), x, y, int(max_iters), device=False)


def cljp_naive_splitting(n, Sp, Sj, Tp, Tj, splitting, colorflag):
    """ruge_stuben.h:316-480: the CLJP splitting (1 = C, 0 = F) of the strength graph S with transpose T into
    splitting (int32), in place.  The start weights (glibc rand() after srand(2448422), or colour / ncolors for
    colorflag == 1, plus the in-degree) are computed on the host, the selection loop runs on the device
    (csrc/split.hip)."""
    import ctypes
    from .graph import _host
    name = "cljp_naive_splitting"
    n = int(n)
    _graph_arrays(name, n, (Sp, Sj, Tp, Tj, splitting))
    if len(Sp) < n + 1 or len(Tp) < n + 1 or len(splitting) < n or (n and (len(Sj) < Sp[n] or len(Tj) < Tp[n])):
        raise ValueError("%s: arrays shorter than the graph" % name)
    if n and (Sp[0] != 0 or np.any(np.diff(Sp[:n + 1]) < 0) or (Sp[n] and (Sj[:Sp[n]].min() < 0 or Sj[:Sp[n]].max() >= n))):
        raise ValueError("%s: S is not a CSR graph of n vertices" % name)
    weight = np.empty(n, dtype=np.float64)
    _host().amgsetup_cljp_weights(n, _lib.ip(Sp), _lib.ip(Sj), int(colorflag), _lib.dp(weight))
    _lib.check(_lib.lib().amg_cljp_device(n, Sp.ctypes.data, Sj.ctypes.data, Tp.ctypes.data, Tj.ctypes.data, weight.ctypes.data,
                                          splitting.ctypes.data, None, None))
