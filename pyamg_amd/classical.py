"""Classical (Ruge-Stuben) AMG setup -- restates pyamg/classical/classical.py:22-188 and pyamg/classical/split.py of
the reference: classical strength (theta) -> C/F splitting -> direct interpolation -> R = P^T -> Galerkin R*A*P.
Returns a pyamg_amd.multilevel_solver.

C/F splittings (1 = C, 0 = F): ``RS`` (first pass of Ruge-Stuben, sequential by construction, host only) and the
reference's parallel coarsenings ``PMIS``, ``PMISc``, ``CLJP`` and ``CLJPc``, each by one of two routes that return the
same integers:

  host    the reference's sweeps restated in csrc/setup_host.cpp;
  device  Luby's rounds / the CLJP selection passes in HBM (csrc/split.hip); weights and colourings come from the host.

``device=True`` takes the device route and raises NotImplementedError for what it cannot take (a sweep limit, a
structurally unsymmetric graph); ``device=False`` is the host route; ``device=None`` is the host route unless
``DEVICE_AUTO`` and a GPU, and then falls back to the host route where the device route refuses.

The global numpy RNG is drawn where the reference draws it: rand(n) once per PMIS / PMISc call, after the colouring's
own draw.  CLJP's weights come from glibc srand(2448422) / rand(), the process's C generator, as in the reference.
Strength, interpolation and the Galerkin product run on the host.  Other strength measures raise NotImplementedError.
"""
import ctypes as C
from warnings import warn

import numpy as np
from scipy.sparse import SparseEfficiencyWarning, csr_matrix, isspmatrix_csr

from . import graph
from ._host import dp as _dp, host_lib, i32 as _i32, ip as _ip, outside, route
from .aggregation import symmetric_strength_of_connection
from .graph import vertex_coloring
from .multilevel import multilevel_solver
from .smoothing import change_smoothers

__all__ = ["ruge_stuben_solver", "classical_strength_of_connection", "RS", "direct_interpolation",
           "PMIS", "PMISc", "CLJP", "CLJPc", "MIS", "preprocess"]

# What device=None does when a GPU is present: the host route until the measurement in profiles/r16_splitting.txt says
# otherwise.
DEVICE_AUTO = False

_lib = host_lib                 # the name tests/test_setup_golden.py imports

def classical_strength_of_connection(A, theta=0.0):
    """pyamg/strength.py:111-210, amg_core/ruge_stuben.h:46-99"""
    if not isspmatrix_csr(A):
        warn("Implicit conversion of A to csr", SparseEfficiencyWarning)
        A = csr_matrix(A)
    if theta < 0 or theta > 1:
        raise ValueError("expected theta in [0,1]")
    Ap, Aj, Ax = _i32(A.indptr), _i32(A.indices), np.ascontiguousarray(A.data, dtype=np.float64)
    Sp = np.empty_like(Ap); Sj = np.empty_like(Aj); Sx = np.empty_like(Ax)
    nnz = host_lib().amgsetup_classical_strength(A.shape[0], float(theta), _ip(Ap), _ip(Aj), _dp(Ax), _ip(Sp), _ip(Sj),
                                                 _dp(Sx))
    S = csr_matrix((Sx[:nnz], Sj[:nnz], Sp), shape=A.shape)
    S.data = np.abs(S.data)
    # scale_rows_by_largest_entry
    counts = np.diff(S.indptr)
    nz = counts > 0
    largest = np.ones(S.shape[0])
    if S.nnz:
        largest[nz] = np.maximum.reduceat(S.data, S.indptr[:-1][nz])
    largest[largest == 0] = 1.0
    S.data = S.data / np.repeat(largest, counts)
    return S


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


def direct_interpolation(A, Cm, splitting):
    """pyamg/classical/interpolate.py:13-75"""
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


_PARALLEL_SPLITTINGS = {"PMIS": PMIS, "PMISc": PMISc, "CLJP": CLJP, "CLJPc": CLJPc}


def unpack_arg(v):
    if isinstance(v, tuple):
        return v[0], v[1]
    return v, {}


def ruge_stuben_solver(A, strength=("classical", {"theta": 0.25}), CF="RS",
                       presmoother=("gauss_seidel", {"sweep": "symmetric"}),
                       postsmoother=("gauss_seidel", {"sweep": "symmetric"}),
                       max_levels=10, max_coarse=500, keep=False, **kwargs):
    """Create a multilevel solver using Classical AMG (pyamg/classical/classical.py:22-116)

    CF : 'RS', 'PMIS', 'PMISc', 'CLJP' or 'CLJPc', or (name, {'device': True | False | None}) for the four parallel
    coarsenings: where their selection loop runs (module docstring).  PMIS and PMISc draw the global numpy RNG once
    per level."""
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
    while len(levels) < max_levels and levels[-1].A.shape[0] > max_coarse:
        extend_hierarchy(levels, strength, CF, keep)
    ml = multilevel_solver(levels, **kwargs)
    change_smoothers(ml, presmoother, postsmoother)
    return ml


def extend_hierarchy(levels, strength, CF, keep):
    """classical.py:120-188"""
    A = levels[-1].A
    fn, kwargs = unpack_arg(strength)
    if fn == "symmetric":
        Cm = symmetric_strength_of_connection(A, **kwargs)
    elif fn == "classical":
        Cm = classical_strength_of_connection(A, **kwargs)
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
    P = direct_interpolation(A, Cm, splitting)
    R = P.T.tocsr()
    if keep:
        levels[-1].C = Cm
        levels[-1].splitting = splitting
    levels[-1].P = P
    levels[-1].R = R
    levels.append(multilevel_solver.level())
    A = R * A * P
    levels[-1].A = A
