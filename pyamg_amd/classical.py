"""Classical (Ruge-Stuben) AMG setup -- restates pyamg/classical/classical.py:22-188 and pyamg/classical/split.py of
the reference: classical strength (theta) -> C/F splitting -> interpolation -> R = P^T -> Galerkin R*A*P.
Returns a pyamg_amd.multilevel_solver.

Interpolation is the reference's direct interpolation or, beyond the reference, extended+i (``extended_interpolation``,
``ruge_stuben_solver(..., interpolation='extended_i')``): the distance-two formula of De Sterck, Falgout, Nolting and
Yang (2008, eq. 4.10) with BoomerAMG's sign filter, optionally truncated to ``max_per_row`` entries per row.  It is
what PMIS needs: an F row without a strong C neighbour interpolates from the C neighbours of its strong F neighbours.
Its arithmetic is DESIGN.md section 8j, and its host route (csrc/setup_host.cpp) and device route (csrc/classical.hip)
return the same bits for an operator and a strength matrix stored in any row order without duplicate columns.

C/F splittings (1 = C, 0 = F): ``RS`` (first pass of Ruge-Stuben, sequential by construction, host only) and the
reference's parallel coarsenings ``PMIS``, ``PMISc``, ``CLJP`` and ``CLJPc``, each by one of two routes that return the
same integers:

  host    the reference's sweeps restated in csrc/setup_host.cpp;
  device  Luby's rounds / the CLJP selection passes in HBM (csrc/split.hip); weights and colourings come from the host.

Classical strength and direct interpolation have the same two routes with the same bits (csrc/classical.hip, DESIGN.md
section 8i); their device route takes A as canonical CSR (sorted rows, no duplicate columns, no stored zeros, finite
values).  ``ruge_stuben_solver(..., device=True)`` with classical strength and ``CF`` 'PMIS' or 'CLJP' builds the whole
hierarchy in HBM from one upload of A_0: every level's strength, graph, weights, splitting and
either interpolation, then R = P^T by the device transpose (``transpose``: the order and bits of P.T.tocsr()) and R A P
by the device sparse product (csrc/spgemm.hip); the coarse operator stays where the product left it for the next
level, and each level downloads what the host hierarchy keeps.  Where the product refuses a level (a row too long for
its tables, 2^31 entries) that level's transpose and product run on the host and a new chain begins.  With another
``CF`` strength and interpolation take their device routes one by one, and R = P^T and the Galerkin product run on the
host.  ``LAST_BUILD`` records the route of the last build.

``device=True`` takes the device route and raises NotImplementedError for what it cannot take (a sweep limit, a
structurally unsymmetric graph); ``device=False`` is the host route; ``device=None`` is the host route unless
``DEVICE_AUTO`` and a GPU, and then falls back to the host route where the device route refuses.

The global numpy RNG is drawn where the reference draws it: rand(n) once per PMIS / PMISc call, after the colouring's
own draw.  CLJP's weights come from glibc srand(2448422) / rand(), the process's C generator, as in the reference.
Other strength measures raise NotImplementedError.
"""
import ctypes as C
from warnings import warn

import numpy as np
from scipy.sparse import SparseEfficiencyWarning, csr_matrix, isspmatrix_csr

from . import graph
from ._host import attempt, dp as _dp, host_lib, i32 as _i32, ip as _ip, outside, route
from .aggregation import symmetric_strength_of_connection
from .graph import vertex_coloring
from .multilevel import multilevel_solver
from .smoothing import change_smoothers

__all__ = ["ruge_stuben_solver", "classical_strength_of_connection", "RS", "direct_interpolation",
           "extended_interpolation", "transpose", "PMIS", "PMISc", "CLJP", "CLJPc", "MIS", "preprocess"]

# What device=None does when a GPU is present: the host route.  profiles/r16_splitting.txt did not justify the device
# route of a splitting alone; profiles/r17_classical_level.txt would justify the chained level
# (section 8i), a switch left to a change of its own.
DEVICE_AUTO = False

_lib = host_lib                 # the name tests/test_setup_golden.py imports


def _operator_order(A, what, product_order=False):
    """What the device routes of strength and interpolation take: a square float64 CSR operator without duplicate
    columns, stored zeros or non-finite values whose rows are sorted (canonical CSR).  Only then are A's values at S's
    positions, in S's order, what C.multiply(A) returns.  product_order: also rows that are not sorted, as scipy's
    sparse product leaves the Galerkin operator; the host route then meets every row of S from its last entry to its
    first (scipy's element-wise product of operands that are not canonical emits a row in reverse).  Returns whether
    that is the case.  Anything else is a refusal, raised before the device library is touched."""
    if not isspmatrix_csr(A):
        raise outside("%s of an operator that is not CSR" % what)
    if A.shape[0] != A.shape[1] or A.dtype != np.float64 or A.nnz >= 2 ** 31:
        raise outside("%s of an operator that is not square float64 with fewer than 2^31 entries" % what)
    if A.nnz and not (np.all(A.data != 0) and np.all(np.isfinite(A.data))):
        raise outside("%s of an operator with stored zeros or non-finite values" % what)
    if _sorted_unique_rows(A):
        if not A.has_canonical_format:
            raise outside("%s of an operator whose format flags deny its sorted rows" % what)
        return False
    if not product_order:
        raise outside("%s of an operator with unsorted rows or duplicated columns" % what)
    keys = np.sort(_entry_keys(A))
    if np.any(keys[1:] == keys[:-1]) or A.has_canonical_format:
        raise outside("%s of an operator with duplicated columns" % what)
    return True


def _entry_keys(A):
    return np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr)) * A.shape[1] + A.indices


def _sorted_unique_rows(A):
    if A.nnz < 2:
        return True
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return not np.any((rows[1:] == rows[:-1]) & (np.diff(A.indices.astype(np.int64)) <= 0))


def _scaled_strength(Sp, Sj, Sx, shape):
    """|S| with every row divided by its largest entry (util/utils.py scale_rows_by_largest_entry, by division)"""
    S = csr_matrix((Sx, Sj, Sp), shape=shape)
    S.data = np.abs(S.data)
    counts = np.diff(S.indptr)
    nz = counts > 0
    largest = np.ones(S.shape[0])
    if S.nnz:
        largest[nz] = np.maximum.reduceat(S.data, S.indptr[:-1][nz])
    largest[largest == 0] = 1.0
    S.data = S.data / np.repeat(largest, counts)
    return S


def _strength_host(A, theta):
    if not isspmatrix_csr(A):
        warn("Implicit conversion of A to csr", SparseEfficiencyWarning)
        A = csr_matrix(A)
    if theta < 0 or theta > 1:
        raise ValueError("expected theta in [0,1]")
    Ap, Aj, Ax = _i32(A.indptr), _i32(A.indices), np.ascontiguousarray(A.data, dtype=np.float64)
    Sp = np.empty_like(Ap); Sj = np.empty_like(Aj); Sx = np.empty_like(Ax)
    nnz = host_lib().amgsetup_classical_strength(A.shape[0], float(theta), _ip(Ap), _ip(Aj), _dp(Ax), _ip(Sp), _ip(Sj),
                                                 _dp(Sx))
    return _scaled_strength(Sp, Sj[:nnz], Sx[:nnz], A.shape)


def _strength_device(A, theta, product_order=False):
    from . import amg_core
    _operator_order(A, "the device route of classical strength", product_order)
    if theta < 0 or theta > 1:
        raise ValueError("expected theta in [0,1]")
    Ap, Aj, Ax = _i32(A.indptr), _i32(A.indices), np.ascontiguousarray(A.data, dtype=np.float64)
    Sp = np.empty_like(Ap); Sj = np.empty_like(Aj); Sx = np.empty_like(Ax)
    amg_core.classical_strength_of_connection(A.shape[0], float(theta), Ap, Aj, Ax, Sp, Sj, Sx)
    nnz = int(Sp[-1])
    return _scaled_strength(Sp, Sj[:nnz], Sx[:nnz], A.shape)


def _strength(A, theta=0.0, device=None, product_order=False):
    return attempt(route(device, DEVICE_AUTO), lambda: _strength_device(A, theta, product_order),
                   lambda: _strength_host(A, theta))


def classical_strength_of_connection(A, theta=0.0, device=None):
    """pyamg/strength.py:111-210, amg_core/ruge_stuben.h:46-99.  device: where the strength kernel runs (module
    docstring); both routes return the same bits."""
    return _strength(A, theta, device)


def remove_diagonal(S):
    """pyamg/util/utils.py:1775-1830"""
    if not isspmatrix_csr(S):
        raise TypeError("expected csr_matrix")
    if S.shape[0] != S.shape[1]:
        raise ValueError("expected square matrix, shape=%s" % (S.shape,))
    S = S.tocoo()
    mask = S.row != S.col
    from scipy.sparse import coo_matrix
    return coo_matrix((S.data[mask], (S.row[mask], S.col[mask])), shape=S.shape).tocsr()


def RS(S):
    """pyamg/classical/split.py:110-158: first pass of the Ruge-Stuben splitting (C=1, F=0)"""
    if not isspmatrix_csr(S):
        raise TypeError("expected csr_matrix")
    S = remove_diagonal(S)
    T = S.T.tocsr()
    splitting = np.empty(S.shape[0], dtype=np.intc)
    host_lib().amgsetup_rs_cf_splitting(S.shape[0], _ip(_i32(S.indptr)), _ip(_i32(S.indices)), _ip(_i32(T.indptr)),
                                        _ip(_i32(T.indices)), _ip(splitting))
    return splitting


def PMIS(S, device=None):
    """pyamg/classical/split.py:159-193: the Parallel Modified Independent Set splitting: Luby's set on S + S^T with the
    weights in-degree + rand()"""
    S = remove_diagonal(S)
    weights, G, S, T = preprocess(S)
    return MIS(G, weights, device=device)


def PMISc(S, method="JP", device=None):
    """split.py:196-238: PMIS with the random weights perturbed by a vertex colouring ('MIS', 'JP' or 'LDF', computed
    on the host)"""
    S = remove_diagonal(S)
    weights, G, S, T = preprocess(S, coloring_method=method)
    return MIS(G, weights, device=device)


def cljp_device(n, Sp, Sj, Tp, Tj, weight, splitting, times=None):
    """amg_cljp_device on start weights; splitting in place.  Returns the number of passes.  times: a list that
    receives (upload, passes, fetch) in milliseconds."""
    from . import _lib
    passes = C.c_int(0)
    ms = (C.c_double * 3)()
    _lib.check(_lib.lib().amg_cljp_device(n, Sp.ctypes.data, Sj.ctypes.data, Tp.ctypes.data, Tj.ctypes.data, weight.ctypes.data,
                                          splitting.ctypes.data, C.byref(passes), ms))
    if times is not None:
        times.extend([ms[0], ms[1], ms[2]])
    return passes.value


def CLJP(S, color=False, device=None):
    """split.py:241-292: the CLJP splitting (amg_core/ruge_stuben.h:316-480); color: start from colour weights (CLJP-c)
    instead of glibc rand()"""
    if not isspmatrix_csr(S):
        raise TypeError("expected csr_matrix")
    S = remove_diagonal(S)
    colorid = 1 if color else 0
    T = S.T.tocsr()
    n = S.shape[0]
    splitting = np.empty(n, dtype=np.intc)
    Sp, Sj, Tp, Tj = _i32(S.indptr), _i32(S.indices), _i32(T.indptr), _i32(T.indices)
    L = host_lib()
    if route(device, DEVICE_AUTO) is not False:
        # the device loop takes every graph: nothing to fall back from
        weight = np.empty(n, dtype=np.float64)
        L.amgsetup_cljp_weights(n, _ip(Sp), _ip(Sj), colorid, _dp(weight))
        cljp_device(n, Sp, Sj, Tp, Tj, weight, splitting)
    else:
        L.amgsetup_cljp_naive_splitting(n, _ip(Sp), _ip(Sj), _ip(Tp), _ip(Tj), _ip(splitting), colorid)
    return splitting


def CLJPc(S, device=None):
    """split.py:295-331: CLJP in colour"""
    S = remove_diagonal(S)
    return CLJP(S, color=True, device=device)


def MIS(G, weights, maxiter=None, device=None):
    """split.py:334-383: Luby's maximal independent set of G (diagonal ignored) for the given vertex weights; maxiter:
    a limit on the in-place sweeps (host route only).  Returns 1 for the set, 0 beside it, -1 where a sweep limit left
    a vertex undecided."""
    if not isspmatrix_csr(G):
        raise TypeError("expected csr_matrix")
    if maxiter is not None and maxiter < 0:
        raise ValueError("maxiter must be >= 0")
    if maxiter is not None and device is True:
        raise outside("the device route of an independent set with a sweep limit")
    G = remove_diagonal(G)
    mis = np.full(G.shape[0], -1, dtype=np.intc)
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    if maxiter is None:
        maxiter = -1
    graph.luby(G.shape[0], _i32(G.indptr), _i32(G.indices), -1, 1, 0, mis, weights, int(maxiter), device, DEVICE_AUTO)
    return mis


def preprocess(S, coloring_method=None):
    """split.py:387-447: S with ones, T = S^T, G = S + T and the start weights in-degree + rand (+ colour) / colours.
    Returns (weights, G, S, T)."""
    if not isspmatrix_csr(S):
        raise TypeError("expected csr_matrix")
    if S.shape[0] != S.shape[1]:
        raise ValueError("expected square matrix, shape=%s" % (S.shape,))
    N = S.shape[0]
    S = csr_matrix((np.ones(S.nnz, dtype="int8"), S.indices, S.indptr), shape=(N, N))
    T = S.T.tocsr()
    G = S + T
    G.data[:] = 1
    weights = np.bincount(S.indices, minlength=N).astype(np.int64)      # T.sum(axis=1): who depends on i
    if coloring_method is None:
        weights = weights + np.random.rand(len(weights))
    else:
        coloring = vertex_coloring(G, coloring_method)
        num_colors = coloring.max() + 1
        weights = weights + (np.random.rand(len(weights)) + coloring) / num_colors
    return (weights, G, S, T)


def _interpolation_host(A, Cm, splitting):
    if not isspmatrix_csr(A):
        raise TypeError("expected csr_matrix for A")
    if not isspmatrix_csr(Cm):
        raise TypeError("expected csr_matrix for C")
    Cm = Cm.copy()
    Cm.data[:] = 1.0
    Cm = csr_matrix(Cm.multiply(A))
    n = A.shape[0]
    splitting = _i32(splitting)
    Cp, Cj, Cx = _i32(Cm.indptr), _i32(Cm.indices), np.ascontiguousarray(Cm.data, dtype=np.float64)
    Ap, Aj, Ax = _i32(A.indptr), _i32(A.indices), np.ascontiguousarray(A.data, dtype=np.float64)
    Pp = np.empty(n + 1, dtype=np.intc)
    nnz = host_lib().amgsetup_rs_direct_interpolation_pass1(n, _ip(Cp), _ip(Cj), _ip(splitting), _ip(Pp))
    Pj = np.empty(nnz, dtype=np.intc)
    Px = np.empty(nnz, dtype=np.float64)
    host_lib().amgsetup_rs_direct_interpolation_pass2(n, _ip(Ap), _ip(Aj), _dp(Ax), _ip(Cp), _ip(Cj), _dp(Cx),
                                                      _ip(splitting), _ip(Pp), _ip(Pj), _dp(Px))
    return csr_matrix((Px, Pj, Pp))


def pattern_values(A, Cm, reverse=False):
    """C.multiply(A) without the product, for an A without duplicate columns and a C with unique columns per row: the
    entries of C's pattern that A stores, with A's values.  Sorted rows of both: in C's order.  reverse (rows that are
    not sorted): every row from C's last entry to its first.  Returns (indptr, indices, data)."""
    n = A.shape[0]
    keys_a, keys_c = _entry_keys(A), _entry_keys(Cm)
    if reverse:                             # rows that are not sorted: search a sorted copy of A's keys
        order = np.argsort(keys_a, kind="stable")
        at = np.searchsorted(keys_a[order], keys_c)
        found = at < len(keys_a)
        at = order[np.minimum(at, max(len(keys_a) - 1, 0))] if len(keys_a) else at
    else:
        at = np.searchsorted(keys_a, keys_c)
        found = at < len(keys_a)
    found[found] = keys_a[at[found]] == keys_c[found]
    rows_c = np.repeat(np.arange(n), np.diff(Cm.indptr))[found]
    Cp = np.zeros(n + 1, dtype=np.intc)
    np.cumsum(np.bincount(rows_c, minlength=n), out=Cp[1:])
    Cj, Cx = _i32(Cm.indices[found]), np.ascontiguousarray(A.data[at[found]], dtype=np.float64)
    if reverse and len(Cj):
        back = Cp[rows_c] + Cp[rows_c + 1] - 1 - np.arange(len(Cj))
        Cj, Cx = np.ascontiguousarray(Cj[back]), np.ascontiguousarray(Cx[back])
    return Cp, Cj, Cx


def _interpolation_device(A, Cm, splitting, product_order=False):
    from . import amg_core
    what = "the device route of direct interpolation"
    reverse = _operator_order(A, what, product_order)
    if not isspmatrix_csr(Cm) or Cm.shape != A.shape:
        raise outside("%s on a strength matrix that is not CSR of A's shape" % what)
    if reverse:
        keys = np.sort(_entry_keys(Cm))
        if np.any(keys[1:] == keys[:-1]) or Cm.has_canonical_format:
            raise outside("%s on a strength matrix with duplicated columns or sorted rows beside an unsorted A" % what)
    elif not _sorted_unique_rows(Cm) or not Cm.has_canonical_format:
        raise outside("%s on a strength matrix with unsorted rows or duplicated columns" % what)
    n = A.shape[0]
    splitting = _i32(splitting)
    if splitting.shape != (n,):
        raise ValueError("expected one splitting value per row")
    Cp, Cj, Cx = pattern_values(A, Cm, reverse)
    Ap, Aj, Ax = _i32(A.indptr), _i32(A.indices), np.ascontiguousarray(A.data, dtype=np.float64)
    Pp = np.empty(n + 1, dtype=np.intc)
    amg_core.rs_direct_interpolation_pass1(n, Cp, Cj, splitting, Pp)
    Pj = np.empty(int(Pp[-1]), dtype=np.intc)
    Px = np.empty(int(Pp[-1]), dtype=np.float64)
    amg_core.rs_direct_interpolation_pass2(n, Ap, Aj, Ax, Cp, Cj, Cx, splitting, Pp, Pj, Px)
    return csr_matrix((Px, Pj, Pp))


def _interpolation(A, Cm, splitting, device=None, product_order=False):
    return attempt(route(device, DEVICE_AUTO), lambda: _interpolation_device(A, Cm, splitting, product_order),
                   lambda: _interpolation_host(A, Cm, splitting))


def direct_interpolation(A, Cm, splitting, device=None):
    """pyamg/classical/interpolate.py:13-75.  device: where the two passes run (module docstring); both routes return
    the same bits."""
    return _interpolation(A, Cm, splitting, device)


def _extended_arguments(A, Cm, splitting, max_per_row):
    """the checks both routes of extended+i make -> (n, Ap, Aj, Ax, Sp, Sj, splitting, q); q: 0 without truncation"""
    if not isspmatrix_csr(A):
        raise TypeError("expected csr_matrix for A")
    if not isspmatrix_csr(Cm):
        raise TypeError("expected csr_matrix for C")
    if A.shape[0] != A.shape[1] or Cm.shape != A.shape:
        raise ValueError("expected a square operator and a strength matrix of its shape")
    n = A.shape[0]
    splitting = _i32(splitting)
    if splitting.shape != (n,):
        raise ValueError("expected one splitting value per row")
    if np.any((splitting != 0) & (splitting != 1)):
        raise ValueError("expected a splitting of 0 (F) and 1 (C)")
    if max_per_row is not None and max_per_row < 1:
        raise ValueError("expected max_per_row >= 1")
    for M, what in ((A, "A"), (Cm, "C")):
        if M.nnz >= 2 ** 31:
            raise ValueError("expected fewer than 2^31 entries in %s" % what)
        if not _sorted_unique_rows(M):
            keys = np.sort(_entry_keys(M))
            if np.any(keys[1:] == keys[:-1]):
                raise ValueError("duplicated columns in a row of %s" % what)
    return (n, _i32(A.indptr), _i32(A.indices), np.ascontiguousarray(A.data, dtype=np.float64), _i32(Cm.indptr), _i32(Cm.indices),
            splitting, 0 if max_per_row is None else int(max_per_row))


def _extended_host(n, Ap, Aj, Ax, Sp, Sj, splitting, q):
    L = host_lib()
    Pp = np.empty(n + 1, dtype=np.intc)
    nnz = L.amgsetup_extended_interpolation_count(n, _ip(Sp), _ip(Sj), _ip(splitting), _ip(Pp))
    if nnz < 0:
        raise ValueError("the prolongator would hold 2^31 entries or more")
    Pj = np.empty(nnz, dtype=np.intc)
    Px = np.empty(nnz, dtype=np.float64)
    L.amgsetup_extended_interpolation_fill(n, _ip(Ap), _ip(Aj), _dp(Ax), _ip(Sp), _ip(Sj), _ip(splitting), _ip(Pp), _ip(Pj), _dp(Px))
    if q:
        Tp, Tj, Tx = np.empty_like(Pp), np.empty_like(Pj), np.empty_like(Px)
        kept = L.amgsetup_truncate_interpolation(n, q, _ip(Pp), _ip(Pj), _dp(Px), _ip(Tp), _ip(Tj), _dp(Tx))
        Pp, Pj, Px = Tp, Tj[:kept].copy(), Tx[:kept].copy()
    return Pp, Pj, Px


def _extended_device(n, Ap, Aj, Ax, Sp, Sj, splitting, q, times=None):
    """amg_extended_interpolation_device and its fetch.  times: a list that receives (upload, stages, fetch) in
    milliseconds."""
    from . import _lib
    handle = C.c_void_p()
    ms = (C.c_double * 2)()
    Pp = np.empty(n + 1, dtype=np.intc)
    _lib.check(_lib.lib().amg_extended_interpolation_device(n, Ap.ctypes.data, Aj.ctypes.data, Ax.ctypes.data, Sp.ctypes.data,
                                                            Sj.ctypes.data, splitting.ctypes.data, q, Pp.ctypes.data, C.byref(handle), ms))
    nnz = int(Pp[-1])
    (Pj, Px), fetch_ms = _lib.fetch_result(handle, _lib.lib().amg_extended_interpolation_fetch, [(nnz, np.intc), (nnz, np.float64)])
    if times is not None:
        times.extend([ms[0], ms[1], fetch_ms])
    return Pp, Pj, Px


def _extended(A, Cm, splitting, max_per_row=None, device=None):
    args = _extended_arguments(A, Cm, splitting, max_per_row)
    Pp, Pj, Px = attempt(route(device, DEVICE_AUTO), lambda: _extended_device(*args), lambda: _extended_host(*args))
    return csr_matrix((Px, Pj, Pp), shape=(args[0], int(args[6].sum())))


def extended_interpolation(A, Cm, splitting, max_per_row=None, device=None):
    """Extended+i (distance-two) interpolation, DESIGN.md section 8j: an F row interpolates from its strong C neighbours
    and from those of its strong F neighbours.  Only the pattern of Cm is used; rows of A and Cm in any stored order,
    without duplicate columns.  max_per_row: keep that many entries of largest magnitude per row, rescaled to the
    row's sum.  device: where the passes run (module docstring); both routes return the same bits."""
    return _extended(A, Cm, splitting, max_per_row, device)


_INTERPOLATIONS = {"direct": 0, "extended_i": 1}


def _interpolation_choice(interpolation):
    """'direct', 'extended_i' or ('extended_i', {'max_per_row': q}) -> (name, max_per_row or None)"""
    name, kwargs = unpack_arg(interpolation)
    if not isinstance(name, str) or name not in _INTERPOLATIONS:
        raise NotImplementedError("interpolation=%r is outside the restated setup" % (name,))
    if set(kwargs) - ({"max_per_row"} if name == "extended_i" else set()):
        raise TypeError("unexpected arguments for %s interpolation: %s" % (name, sorted(kwargs)))
    q = kwargs.get("max_per_row")
    if q is not None and q < 1:
        raise ValueError("expected max_per_row >= 1")
    return name, q


_CHAINED_SPLITTINGS = {"PMIS": 0, "CLJP": 1}
LEVEL_STAGES = ("upload", "strength", "graph", "splitting", "interpolation", "fetch")


def _level_arguments(A, theta, CF):
    """What both device level builders check and look up before their first call: (n, kind, draw).  draw() returns the n
    start values, drawn where the host route draws them: rand(n) of the global numpy RNG for PMIS, glibc rand() after
    srand(2448422) for CLJP."""
    if theta < 0 or theta > 1:
        raise ValueError("expected theta in [0,1]")
    n = A.shape[0]
    if n == 0:
        raise outside("the device route of a classical level without rows")
    kind = _CHAINED_SPLITTINGS[CF]

    def draw():
        if kind == 0:
            return np.ascontiguousarray(np.random.rand(n))
        r = np.empty(n, dtype=np.float64)
        host_lib().amgsetup_cljp_random(n, _dp(r))
        return r
    return n, kind, draw


def _level_specs(n, p_nnz):
    return [(n, np.intc), (n + 1, np.intc), (p_nnz, np.intc), (p_nnz, np.float64)]


def _csr_specs(n, nnz, wanted=True):
    return [(n + 1, np.intc), (nnz, np.intc), (nnz, np.float64)] if wanted else [None] * 3


def classical_level_device(A, theta, CF, keep=False, times=None, product_order=False, interpolation="direct"):
    """One level in HBM from one upload of A (amg_classical_level_build): classical strength, the strength graph and
    its transpose, the start weights, the PMIS or CLJP splitting and the interpolation chosen (ruge_stuben_solver's
    ``interpolation``).  Returns (splitting, P, S);
    S, the scaled strength matrix, only with keep (None otherwise).  The random start values are drawn on the host
    (_level_arguments).  times: a list that receives the milliseconds of LEVEL_STAGES.  product_order: _operator_order."""
    from . import _lib
    name, q = _interpolation_choice(interpolation)
    reverse = _operator_order(A, "the device route of a classical level", product_order)
    n, kind, draw = _level_arguments(A, theta, CF)
    Ap, Aj, Ax = _i32(A.indptr), _i32(A.indices), np.ascontiguousarray(A.data, dtype=np.float64)
    r = draw()
    handle = C.c_void_p()
    sizes = (C.c_long * 2)()
    ms = (C.c_double * 6)()
    _lib.check(_lib.lib().amg_classical_level_build(n, Ap.ctypes.data, Aj.ctypes.data, Ax.ctypes.data, float(theta), kind,
                                                    int(reverse), r.ctypes.data, _INTERPOLATIONS[name], q or 0, C.byref(handle),
                                                    sizes, None, ms))
    (splitting, Pp, Pj, Px, Sp, Sj, Sx), _ = _lib.fetch_result(handle, _lib.lib().amg_classical_level_fetch,
                                                               _level_specs(n, sizes[1]) + _csr_specs(n, sizes[0], keep), ms)
    if times is not None:
        times.extend(ms[k] for k in range(6))
    S = csr_matrix((Sx, Sj, Sp), shape=A.shape) if keep else None
    shape = None if name == "direct" else (n, int(splitting.sum()))
    return splitting, csr_matrix((Px, Pj, Pp), shape=shape), S


_PARALLEL_SPLITTINGS = {"PMIS": PMIS, "PMISc": PMISc, "CLJP": CLJP, "CLJPc": CLJPc}


def unpack_arg(v):
    if isinstance(v, tuple):
        return v[0], v[1]
    return v, {}


def ruge_stuben_solver(A, strength=("classical", {"theta": 0.25}), CF="RS",
                       presmoother=("gauss_seidel", {"sweep": "symmetric"}),
                       postsmoother=("gauss_seidel", {"sweep": "symmetric"}),
                       max_levels=10, max_coarse=500, keep=False, device=None, interpolation="direct", **kwargs):
    """Create a multilevel solver using Classical AMG (pyamg/classical/classical.py:22-116)

    CF : 'RS', 'PMIS', 'PMISc', 'CLJP' or 'CLJPc', or (name, {'device': True | False | None}) for the four parallel
    coarsenings: where their selection loop runs (module docstring).  PMIS and PMISc draw the global numpy RNG once
    per level.
    device : where classical strength and interpolation run, and with CF 'PMIS' or 'CLJP' the whole level
    (module docstring); every route builds the same hierarchy.
    interpolation : 'direct' (the reference's), 'extended_i' or ('extended_i', {'max_per_row': q})
    (extended_interpolation); another name raises NotImplementedError before a level is built."""
    _interpolation_choice(interpolation)
    levels = [multilevel_solver.level()]
    if not isspmatrix_csr(A):
        try:
            A = csr_matrix(A)
            warn("Implicit conversion of A to CSR", SparseEfficiencyWarning)
        except Exception:
            raise TypeError("Argument A must have type csr_matrix, or be convertible to csr_matrix")
    A = A.astype(np.float64) if A.dtype != np.float64 else A
    if A.shape[0] != A.shape[1]:
        raise ValueError("expected square matrix")
    levels[-1].A = A
    LAST_BUILD["uploads"] = 0
    LAST_BUILD["levels"] = []
    chain = _Chain()
    try:
        while len(levels) < max_levels and levels[-1].A.shape[0] > max_coarse:
            extend_hierarchy(levels, strength, CF, keep, device, interpolation, chain)
    finally:
        chain.close()
    ml = multilevel_solver(levels, **kwargs)
    change_smoothers(ml, presmoother, postsmoother)
    return ml


def _stages(A, strength, CF, device, interpolation="direct"):
    """strength, splitting and interpolation one by one -> (C, splitting, P)"""
    fn, kwargs = unpack_arg(strength)
    if fn == "symmetric":
        Cm = symmetric_strength_of_connection(A, **kwargs)
    elif fn == "classical":
        Cm = _strength(A, device=device, product_order=True, **kwargs)
    elif fn is None:
        Cm = A
    else:
        raise NotImplementedError("strength=%r is outside the restated setup" % (fn,))
    fn, kwargs = unpack_arg(CF)
    if fn == "RS":
        splitting = RS(Cm)
    elif fn in _PARALLEL_SPLITTINGS:
        splitting = _PARALLEL_SPLITTINGS[fn](Cm, **kwargs)
    else:
        raise NotImplementedError("C/F splitting %r is outside the restated setup" % (fn,))
    name, q = _interpolation_choice(interpolation)
    if name == "direct":
        return Cm, splitting, _interpolation(A, Cm, splitting, device, product_order=True)
    return Cm, splitting, _extended(A, Cm, splitting, q, device)


def _chain_options(strength, CF):
    """(theta, splitting name) where the whole level runs in HBM: strength is classical with theta alone and CF is PMIS
    or CLJP not sent to the host; None otherwise"""
    fn, kwargs = unpack_arg(strength)
    name, cf_kwargs = unpack_arg(CF)
    if fn != "classical" or set(kwargs) - {"theta"} or name not in _CHAINED_SPLITTINGS:
        return None
    if set(cf_kwargs) - {"device"} or cf_kwargs.get("device", True) is False:
        return None
    return kwargs.get("theta", 0.0), name


def _chained(A, strength, CF, keep, interpolation="direct"):
    """the level in HBM from an upload of its own (_chain_options); None otherwise"""
    options = _chain_options(strength, CF)
    if options is None:
        return None
    times = []
    LAST_BUILD["uploads"] += 1
    splitting, P, S = classical_level_device(A, options[0], options[1], keep=keep, times=times, product_order=True,
                                             interpolation=interpolation)
    _record_level(resident=True, times=dict(zip(LEVEL_STAGES, times)))
    return S, splitting, P


# The route of the last ruge_stuben_solver build, for the tests and tools/bench_classical_hierarchy.py.  uploads: operators
# sent to HBM by the level routes (one per chain, one per level of the per-level route).  levels: one record per level
# built: chained (its transpose and Galerkin product ran in HBM on the chain's resident operator), resident (the level
# itself was built in HBM), reversed (what the level entry was told about the row order; None on the host), times
# (milliseconds by stage: CHAIN_STAGES or LEVEL_STAGES), products (the tables of R * A and (R * A) * P, _lib.SPGEMM_TABLES)
# and transpose (_lib.TRANSPOSE_ROUTE_FIELDS).
LAST_BUILD = {"uploads": 0, "levels": []}
CHAIN_STAGES = ("upload", "strength", "graph", "splitting", "interpolation", "transpose", "galerkin", "fetch")
# What tools/bench_classical_hierarchy.py turns off to time the per-level route (every level uploads A_l, transposes and
# multiplies on the host); not an option of the setup.
_RESIDENT_CHAIN = True
# a coarse operator of this many entries or more does not fit the host's 32-bit index arrays: the level's product is
# treated as refused, as the device library itself refuses it
_PRODUCT_ENTRIES_LIMIT = 2 ** 31


def _record_level(chained=False, resident=False, reversed=None, times=None, products=None, transpose=None):
    LAST_BUILD["levels"].append({"chained": chained, "resident": resident, "reversed": reversed, "times": times or {},
                                 "products": products, "transpose": transpose})


def _transpose_device(P):
    from . import _lib
    what = "the device route of a transpose"
    if P.dtype != np.float64 or P.nnz >= 2 ** 31 or max(P.shape) >= 2 ** 31 - 1:
        raise outside("%s of a matrix that is not float64 with fewer than 2^31 entries" % what)
    n_row, n_col = P.shape
    Pp, Pj, Px = _i32(P.indptr), _i32(P.indices), np.ascontiguousarray(P.data, dtype=np.float64)
    Rp = np.empty(n_col + 1, dtype=np.intc)
    handle = C.c_void_p()
    _lib.check(_lib.lib().amg_csr_transpose_device(n_row, n_col, Pp.ctypes.data, Pj.ctypes.data, Px.ctypes.data, Rp.ctypes.data,
                                                   C.byref(handle)))
    nnz = int(Rp[-1])
    (Rj, Rx), _ = _lib.fetch_result(handle, _lib.lib().amg_csr_transpose_fetch, [(nnz, np.intc), (nnz, np.float64)])
    return _transposed(Rp, Rj, Rx, (n_col, n_row))


def _transposed(Rp, Rj, Rx, shape):
    """the arrays of a device transpose as the object P.T.tocsr() returns: scipy's conversion declares its rows sorted"""
    R = csr_matrix((Rx, Rj, Rp), shape=shape)
    R.has_sorted_indices = True
    return R


def transpose(P, device=None):
    """R = P^T of a CSR matrix exactly as P.T.tocsr() returns it (scipy's csr_tocsc): row c of R holds the entries of
    column c of P by ascending row of P and, within a row of P, in stored order; duplicates stay, values keep their
    bits.  device: the host route is P.T.tocsr(), the device route the kernels of csrc/transpose.hip (DESIGN.md section
    8k, float64 only); both return the same bits."""
    if not isspmatrix_csr(P):
        raise TypeError("expected csr_matrix")
    return attempt(route(device, DEVICE_AUTO), lambda: _transpose_device(P), lambda: P.T.tocsr())


class _Chain:
    """the resident chain of one ruge_stuben_solver call: the handle of amg_classical_chain_begin and what the last
    level's flags said about the operator it left in HBM"""

    def __init__(self):
        self.handle = None
        self.reversed = 0
        self.finite = True

    def close(self):
        if self.handle is not None:
            from . import _lib
            handle, self.handle = self.handle, None
            _lib.lib().amg_classical_chain_free(handle)


def _chain_level_call(handle, theta, kind, r, interpolation, q, sizes, flags, ms):
    """amg_classical_chain_level -> 0 or _lib.CHAIN_PRODUCT_REFUSED (the tests wrap it to see the calls)"""
    from . import _lib
    rc = _lib.lib().amg_classical_chain_level(handle, float(theta), kind, r.ctypes.data, interpolation, q, sizes, flags, None, ms)
    if rc != _lib.CHAIN_PRODUCT_REFUSED:
        _lib.check(rc)
    return rc


def _chain_level(levels, chain, theta, CF, keep, interpolation):
    """One level on the chain's resident operator (amg_classical_chain_level / _fetch): strength, splitting and
    interpolation as classical_level_device builds them, then R = P^T and R A P in HBM; the host hierarchy receives
    what it keeps.  The first level of a chain vets and uploads A.  Where the product is refused the level is finished
    on the host from the fetched splitting, P and S, and the chain ends."""
    from . import _lib
    A = levels[-1].A
    name, q = _interpolation_choice(interpolation)
    what = "the device route of a classical level"
    if chain.handle is None:
        reverse = _operator_order(A, what, True)
    elif not chain.finite:
        # what _operator_order would say about the operator in HBM, from the flags of the product that left it there
        raise outside("%s of an operator with stored zeros or non-finite values" % what)
    else:
        reverse = bool(chain.reversed)
    n, kind, draw = _level_arguments(A, theta, CF)
    if chain.handle is None:
        Ap, Aj, Ax = _i32(A.indptr), _i32(A.indices), np.ascontiguousarray(A.data, dtype=np.float64)
        handle = C.c_void_p()
        _lib.check(_lib.lib().amg_classical_chain_begin(n, Ap.ctypes.data, Aj.ctypes.data, Ax.ctypes.data, int(reverse),
                                                        C.byref(handle)))
        chain.handle, chain.reversed, chain.finite = handle, int(reverse), True
        LAST_BUILD["uploads"] += 1
    r = draw()
    sizes = (C.c_long * 5)()
    flags = (C.c_int * _lib.CHAIN_FLAG_FIELDS)()
    ms = (C.c_double * len(CHAIN_STAGES))()
    rc = _chain_level_call(chain.handle, theta, kind, r, _INTERPOLATIONS[name], q or 0, sizes, flags, ms)
    s_nnz, p_nnz, r_nnz, c_nnz, n_coarse = (int(v) for v in sizes)
    refused = rc == _lib.CHAIN_PRODUCT_REFUSED or c_nnz >= _PRODUCT_ENTRIES_LIMIT
    # the handle is the chain, which _Chain.close frees: nothing to release where an allocation fails
    arrays = _lib.allocate(_level_specs(n, p_nnz) + _csr_specs(n_coarse, r_nnz, not refused) + _csr_specs(n_coarse, c_nnz, not refused)
                           + _csr_specs(n, s_nnz, keep))
    splitting, Pp, Pj, Px, Rp, Rj, Rx, Cp, Cj, Cx, Sp, Sj, Sx = arrays
    _lib.check(_lib.lib().amg_classical_chain_fetch(chain.handle, *(None if a is None else a.ctypes.data for a in arrays), ms))
    _record_level(chained=not refused, resident=True, reversed=int(reverse), times=dict(zip(CHAIN_STAGES, ms)),
                  products=(_lib.SPGEMM_TABLES[flags[2]], _lib.SPGEMM_TABLES[flags[3]]),
                  transpose=dict(zip(_lib.TRANSPOSE_ROUTE_FIELDS, (int(v) for v in flags[4:8]))))
    P = csr_matrix((Px, Pj, Pp), shape=None if name == "direct" else (n, int(splitting.sum())))
    if refused:
        chain.close()
        R = P.T.tocsr()
        Ac = R * A * P
    else:
        chain.reversed, chain.finite = int(not flags[0]), bool(flags[1])
        R = _transposed(Rp, Rj, Rx, (n_coarse, n))
        Ac = csr_matrix((Cx, Cj, Cp), shape=(n_coarse, n_coarse))
    if keep:
        levels[-1].C = csr_matrix((Sx, Sj, Sp), shape=A.shape)
        levels[-1].splitting = splitting
    levels[-1].P = P
    levels[-1].R = R
    levels.append(multilevel_solver.level())
    levels[-1].A = Ac


def extend_hierarchy(levels, strength, CF, keep, device=None, interpolation="direct", chain=None):
    """classical.py:120-188.  chain: the resident chain of the calling ruge_stuben_solver (_Chain); with it, a level that
    _chain_options takes is built, transposed and multiplied in HBM."""
    A = levels[-1].A
    way = route(device, DEVICE_AUTO)
    options = _chain_options(strength, CF) if chain is not None and _RESIDENT_CHAIN and way is not False else None
    if options is not None:
        try:
            return _chain_level(levels, chain, options[0], options[1], keep, interpolation)
        except NotImplementedError:
            chain.close()
            if way is True:
                raise
        except BaseException:
            chain.close()
            raise
        way = False                         # the refusal is answered by the host route, as attempt() would

    def on_device():
        built = _chained(A, strength, CF, keep, interpolation)
        return built if built is not None else _stages(A, strength, CF, way, interpolation)

    recorded = len(LAST_BUILD["levels"])
    Cm, splitting, P = attempt(way, on_device, lambda: _stages(A, strength, CF, False, interpolation))
    if len(LAST_BUILD["levels"]) == recorded:
        _record_level()
    R = P.T.tocsr()
    if keep:
        levels[-1].C = Cm
        levels[-1].splitting = splitting
    levels[-1].P = P
    levels[-1].R = R
    levels.append(multilevel_solver.level())
    A = R * A * P
    levels[-1].A = A
