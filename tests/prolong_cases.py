"""Designed inputs and plain-Python models (loops, one rounding per operation) for the three smoothed-aggregation stages of
DESIGN.md section 8m: symmetric strength, the tentative prolongator and Jacobi prolongation smoothing.  Shared by
tests/test_prolong_cases_host.py and tests/test_gpu_prolong_stages.py.

Every case is built once (functools.lru_cache), when a test first asks for it and not when the tests are collected
(the *_names functions list the cases without building them), and never written to: the routes under test get copies.
"""
import functools
import math

import numpy as np
import scipy.sparse as sps

from pyamg_amd.aggregation import fit_candidates, mis_aggregation, standard_aggregation, symmetric_strength_of_connection
from pyamg_amd.gallery import poisson
from pyamg_amd.util import approximate_spectral_radius, get_diagonal, scale_rows

THETAS = (0, 0.25, 0.5)
STAR = 700


def same_matrix(a, b):
    """format, shape, the dtypes and the three arrays"""
    if a.format != b.format or a.shape != b.shape:
        return False
    if a.format == "bsr" and a.blocksize != b.blocksize:
        return False
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
               for x, y in ((a.indptr, b.indptr), (a.indices, b.indices), (a.data, b.data)))


def _csr_from_rows(rows, n_col):
    Ap = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.intc)
    Aj = np.array([j for r in rows for j, _ in r], dtype=np.intc)
    Ax = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return sps.csr_matrix((Ax, Aj, Ap), shape=(len(rows), n_col))


# --------------------------------------------------------------------------------------------------------- strength
@functools.lru_cache(maxsize=None)
def designed_operator():
    """760 unsorted rows of mixed sign with the rows the device kernels can get wrong: 0 a star of 700 entries, 5 without a
    diagonal, 6 with its diagonal stored twice, 7 empty, 8 with off-diagonals that every theta > 0 drops, 9 of stored
    zeros only, 11 with an off-diagonal column stored twice."""
    rng = np.random.RandomState(11)
    n = 760
    rows = []
    for i in range(n):
        cols = [int(c) for c in rng.choice(n, rng.randint(1, 6), replace=False) if c != i]
        row = [(c, float(np.round(rng.randn(), 3))) for c in cols]
        row.append((i, float((1.0 + rng.rand()) * (1 if rng.rand() < 0.7 else -1))))
        order = rng.permutation(len(row))
        rows.append([row[k] for k in order])
    star = [(c, float(np.round(rng.randn(), 2)) or 0.5) for c in rng.permutation(STAR)]
    rows[0] = [(c, 3.0 if c == 0 else v) for c, v in star]
    rows[5] = [(c, v) for c, v in rows[5] if c != 5] + [(2, -0.75)]
    rows[6] = [(6, 1.25), (3, -0.5), (6, -0.5), (700, 2.0)]
    rows[7] = []
    rows[8] = [(10, 1e-3), (8, 100.0), (12, -1e-3), (11, 1e-3)]
    rows[9] = [(3, 0.0), (9, 0.0), (4, -0.0)]
    rows[11] = rows[11] + [(40, 0.5), (40, -2.0)]
    return _csr_from_rows(rows, n)


def strength_names():
    return ["%s_theta_%g" % (kind, theta) for theta in THETAS for kind in ("poisson_9x9", "designed")]


@functools.lru_cache(maxsize=None)
def strength_cases():
    """name -> (A, theta).  Poisson 9 x 9 with theta = 0.25 puts every off-diagonal exactly on the threshold
    (1 >= 0.0625 * 4 * 4): all of them are kept."""
    out = {}
    for theta in THETAS:
        out["poisson_9x9_theta_%g" % theta] = (poisson((9, 9), format="csr"), theta)
        out["designed_theta_%g" % theta] = (designed_operator(), theta)
    return out


def model_strength(A, theta):
    """(Sp, Sj, Sx) of symmetric_strength_of_connection by loops"""
    n = A.shape[0]
    Ap, Aj, Ax = A.indptr, A.indices, A.data
    diags = []
    for i in range(n):
        d = 0.0
        for jj in range(Ap[i], Ap[i + 1]):
            if Aj[jj] == i:
                d = d + float(Ax[jj])
        diags.append(abs(d))
    t2 = theta * theta
    Sp, Sj, Sx = [0], [], []
    for i in range(n):
        eps = t2 * diags[i]
        kept = []
        for jj in range(Ap[i], Ap[i + 1]):
            j, a = int(Aj[jj]), float(Ax[jj])
            if j == i or a * a >= eps * diags[j]:
                kept.append((j, abs(a)))
        largest = 0.0
        for _, v in kept:
            if largest < v:
                largest = v
        if largest == 0.0:
            largest = 1.0
        Sj += [j for j, _ in kept]
        Sx += [v / largest for _, v in kept]
        Sp.append(len(Sj))
    return np.array(Sp, dtype=Ap.dtype), np.array(Sj, dtype=Aj.dtype), np.array(Sx, dtype=np.float64)


# --------------------------------------------------------------------------------------------- tentative prolongator
BLOCKS = ((1, 1), (1, 3), (2, 3), (3, 6))
SIZES = (1, 2, 63, 64, 65, STAR)


@functools.lru_cache(maxsize=None)
def designed_aggregates():
    """AggOp with aggregates of 1, 2, 63, 64, 65 and 700 members scattered over 905 nodes, 10 of them unaggregated"""
    rng = np.random.RandomState(12)
    n = sum(SIZES) + 10
    agg = np.full(n, -1)
    agg[rng.permutation(n)[:sum(SIZES)]] = np.repeat(np.arange(len(SIZES)), SIZES)
    mask = agg >= 0
    Tp = np.concatenate(([0], np.cumsum(mask))).astype(np.intc)
    return sps.csr_matrix((np.ones(Tp[-1], dtype=np.int8), agg[mask].astype(np.intc), Tp), shape=(n, len(SIZES)))


def fit_names():
    return [name for K1, K2 in BLOCKS
            for name in ["random_%dx%d" % (K1, K2)] + (["equal_columns_%dx%d" % (K1, K2)] if K2 >= 3 else [])]


@functools.lru_cache(maxsize=None)
def fit_cases():
    """name -> (AggOp, B).  The aggregates of 1 and 2 members have fewer rows than the 3 or 6 candidates."""
    AggOp = designed_aggregates()
    n = AggOp.shape[0]
    members = AggOp.tocsc()
    out = {}
    for K1, K2 in BLOCKS:
        rng = np.random.RandomState(100 * K1 + K2)
        B = rng.randn(n * K1, K2)
        B[3, 0] = -0.0
        out["random_%dx%d" % (K1, K2)] = (AggOp, B)
        if K2 >= 3:
            E = B.copy()
            E[:, 1] = E[:, 0]               # the second column falls under the threshold: a zero column, a zero in R
            nodes = members.indices[members.indptr[3]:members.indptr[4]]
            for r in range(K1):
                E[nodes * K1 + r, 2] = 0.0  # a candidate that is zero on the aggregate of 64
            out["equal_columns_%dx%d" % (K1, K2)] = (AggOp, E)
    return out


def model_fit(AggOp, B, tol=1e-10):
    """(Tp, Tj, Tx (entries, K1, K2), R (N_coarse * K2, K2)) of fit_candidates by loops: smoothed_aggregation.h:341-452
    on the members of every aggregate in ascending order"""
    n, nc = AggOp.shape
    K1, K2 = B.shape[0] // n, B.shape[1]
    Tp, Tj = AggOp.indptr, AggOp.indices
    members = [[] for _ in range(nc)]
    for i in range(n):
        for jj in range(Tp[i], Tp[i + 1]):
            members[Tj[jj]].append((i, jj))
    Tx = np.zeros((Tp[-1], K1, K2))
    R = np.zeros((nc, K2, K2))
    for a in range(nc):
        q = [[float(B[i * K1 + r, c]) for c in range(K2)] for i, _ in members[a] for r in range(K1)]
        for bj in range(K2):
            norm = 0.0
            for row in q:
                norm = norm + row[bj] * row[bj]
            threshold = tol * math.sqrt(norm)
            for bi in range(bj):
                dot = 0.0
                for row in q:
                    dot = dot + row[bi] * row[bj]
                for row in q:
                    row[bj] = row[bj] - dot * row[bi]
                R[a, bi, bj] = dot
            norm = 0.0
            for row in q:
                norm = norm + row[bj] * row[bj]
            norm = math.sqrt(norm)
            scale = 0.0
            if norm > threshold:
                scale = 1.0 / norm
                R[a, bj, bj] = norm
            for row in q:
                row[bj] = row[bj] * scale
        for m, (_, jj) in enumerate(members[a]):
            Tx[jj] = q[m * K1:(m + 1) * K1]
    return Tp, Tj, Tx, R.reshape(-1, K2)


# ------------------------------------------------------------------------------------------------- Jacobi smoothing
def _as(M, fmt):
    M = sps.csr_matrix(M)
    if fmt == "csr":
        return M
    return sps.bsr_matrix((M.data.reshape(-1, 1, 1), M.indices, M.indptr), shape=M.shape)


def _reorder_rows(S, order):
    """S with every row's entries stored in the order `order(length)` gives (an index array)"""
    S = sps.csr_matrix(S).copy()
    for i in range(S.shape[0]):
        lo, hi = S.indptr[i], S.indptr[i + 1]
        k = lo + order(hi - lo)
        S.indices[lo:hi], S.data[lo:hi] = S.indices[k], S.data[k]
    S.has_sorted_indices = False
    return S


@functools.lru_cache(maxsize=None)
def designed_smoothing_operands():
    """(S, T, T_reversed).  S: designed_operator() with its duplicates summed, row 20 left with only its diagonal (under
    'local' with omega = 1 its row of P is T - T, an exact zero that is dropped), row 30 with a stored zero as its
    diagonal, and every row stored in a shuffled order.  Both weightings leave S with sorted rows (get_diagonal sorts it
    in place, and so does np.abs through scipy's sum_duplicates), so a product W * P touches the rows of P in ascending
    node order and comes out in the reverse of that.
    T: 95 aggregates of eight consecutive nodes numbered with the nodes, one entry per row, rows 7, 15 and 16 empty; the
    star row of S meets 88 of them.  The product comes out in descending columns and the subtraction takes scipy's
    general order.
    T_reversed: the same aggregates numbered against the nodes.  The first product then comes out canonical, with rows
    of up to 88 entries against T's rows of one entry or none, and the subtraction takes the merge."""
    S = designed_operator().copy().tolil()      # (tolil sums duplicates in place)
    S[20, :] = 0.0
    S[20, 20] = 2.0
    S = S.tocsr()
    S.eliminate_zeros()
    S[30, 30] = 0.0
    rng = np.random.RandomState(13)
    n = S.shape[0]
    agg = np.arange(n) // 8
    mask = np.ones(n, dtype=bool)
    mask[[7, 15, 16]] = False
    Tp = np.concatenate(([0], np.cumsum(mask))).astype(np.intc)
    B = 1.0 + rng.rand(n, 1)

    def tentative(numbers):
        AggOp = sps.csr_matrix((np.ones(Tp[-1], dtype=np.int8), numbers[mask].astype(np.intc), Tp), shape=(n, agg.max() + 1))
        return fit_candidates(AggOp, B)[0]
    return _reorder_rows(S, rng.permutation), tentative(agg), tentative(agg.max() - agg)


def _jacobi_specs():
    """name -> (operands, format of S, format of T, omega, degree, weighting), without building anything"""
    out = {}
    weightings = ("diagonal", "local", "block")
    k = 0

    def formats():
        return ("csr", "bsr")[k % 2], ("csr", "bsr")[(k // 2) % 2]
    for weighting in weightings:
        for degree in (1, 2):
            for omega in ((1.0, 4.0 / 3.0) if weighting == "local" else (4.0 / 3.0,)):
                sf, tf = formats()
                out["designed_%s_degree%d_omega%.2f_S%s_T%s" % (weighting, degree, omega, sf, tf)] = ("designed", sf, tf, omega, degree, weighting)
                k += 1
    for weighting, omega in (("local", 1.0), ("local", 4.0 / 3.0), ("diagonal", 4.0 / 3.0)):
        for degree in (1, 2):
            sf, tf = formats()
            out["reversed_%s_degree%d_omega%.2f_S%s_T%s" % (weighting, degree, omega, sf, tf)] = ("reversed", sf, tf, omega, degree, weighting)
            k += 1
    for grid in ((12, 12), (6, 6, 6)):
        for agg_name in ("standard", "mis"):
            for degree in (0, 1, 2, 3):
                weighting = weightings[k % 3]
                sf, tf = formats()
                out["poisson_%s_%s_degree%d_%s_S%s_T%s" % ("x".join(map(str, grid)), agg_name, degree, weighting, sf, tf)] = (
                    (grid, agg_name), sf, tf, 4.0 / 3.0, degree, weighting)
                k += 1
    return out


def jacobi_names():
    return list(_jacobi_specs())


@functools.lru_cache(maxsize=None)
def jacobi_cases():
    """name -> dict(S, T, omega, degree, weighting): the degrees 0 .. 3, the three weightings and both formats of S and of
    T over the designed operands with T (general order) and with T_reversed (canonical merge in the first step) and
    over the aggregates of standard_aggregation and mis_aggregation on Poisson 12 x 12 and 6^3"""
    S, T, T_rev = designed_smoothing_operands()
    operands = {"designed": (S, T), "reversed": (S, T_rev)}
    for grid in ((12, 12), (6, 6, 6)):
        A = poisson(grid, format="csr")
        Cm = symmetric_strength_of_connection(A)
        y = np.random.RandomState(14).rand(A.shape[0])
        for agg_name, AggOp in (("standard", standard_aggregation(Cm)[0]), ("mis", mis_aggregation(Cm, y, device=False)[0])):
            operands[(grid, agg_name)] = (A, fit_candidates(AggOp, np.ones((A.shape[0], 1)))[0])
    return {name: dict(S=_as(operands[key][0], sf), T=_as(operands[key][1], tf), omega=omega, degree=degree, weighting=weighting)
            for name, (key, sf, tf, omega, degree, weighting) in _jacobi_specs().items()}


def find_jacobi_case(prefix, S=None, T=None, **want):
    """the first case whose name starts with prefix, with S and T in the given formats and the given settings"""
    for name, c in jacobi_cases().items():
        if name.startswith(prefix) and S in (None, c["S"].format) and T in (None, c["T"].format) \
                and all(c[k] == v for k, v in want.items()):
            return name
    raise KeyError((prefix, S, T, want))


def jacobi_weights(S, omega, weighting):
    """(dinv, w) of the smoothing step by the public host pieces, which both routes keep on the host: S is sorted in
    place (by get_diagonal, or by np.abs under 'local') and np.random is drawn from once where the weighting is 'diagonal'"""
    if weighting in ("diagonal", "block"):
        dinv = get_diagonal(S, inv=True)
        return dinv, float(omega / approximate_spectral_radius(scale_rows(S, dinv, copy=True)))
    sums = np.ravel(abs(S) * np.ones((S.shape[0], 1)))
    dinv = np.zeros_like(sums)
    dinv[sums != 0] = 1.0 / np.abs(sums[sums != 0])
    return dinv, float(omega)


def _canonical(n, Ap, Aj):
    return all(Aj[jj - 1] < Aj[jj] for i in range(n) for jj in range(Ap[i] + 1, Ap[i + 1]))


def _model_matmat(n, Ap, Aj, Ax, Bp, Bj, Bx):
    """scipy's csr_matmat: sums from zero in traversal order, output in reverse order of first touch, zeros dropped"""
    Cp, Cj, Cx = [0], [], []
    for i in range(n):
        order, sums = [], {}
        for jj in range(Ap[i], Ap[i + 1]):
            j, v = Aj[jj], Ax[jj]
            for kk in range(Bp[j], Bp[j + 1]):
                k = Bj[kk]
                if k not in sums:
                    sums[k] = 0.0
                    order.append(k)
                sums[k] = sums[k] + v * Bx[kk]
        for k in reversed(order):
            if sums[k] != 0:
                Cj.append(k)
                Cx.append(sums[k])
        Cp.append(len(Cj))
    return Cp, Cj, Cx


def _model_minus(n, Ap, Aj, Ax, Bp, Bj, Bx, steps=None):
    """scipy's csr_minus_csr: the merge of csr_binop_csr_canonical where both operands are canonical, else the linked list
    of csr_binop_csr_general"""
    Cp, Cj, Cx = [0], [], []
    canonical = _canonical(n, Ap, Aj) and _canonical(n, Bp, Bj)
    if steps is not None:       # (routine taken, longest row of the left operand, longest row of the right operand)
        steps.append(("merge" if canonical else "general", max(Ap[i + 1] - Ap[i] for i in range(n)),
                      max(Bp[i + 1] - Bp[i] for i in range(n))))
    for i in range(n):
        a = [(Aj[jj], Ax[jj]) for jj in range(Ap[i], Ap[i + 1])]
        b = [(Bj[jj], Bx[jj]) for jj in range(Bp[i], Bp[i + 1])]
        if canonical:
            row, ia, ib = [], 0, 0
            while ia < len(a) and ib < len(b):
                if a[ia][0] == b[ib][0]:
                    row.append((a[ia][0], a[ia][1] - b[ib][1]))
                    ia, ib = ia + 1, ib + 1
                elif a[ia][0] < b[ib][0]:
                    row.append((a[ia][0], a[ia][1] - 0.0))
                    ia += 1
                else:
                    row.append((b[ib][0], 0.0 - b[ib][1]))
                    ib += 1
            row += [(j, v - 0.0) for j, v in a[ia:]] + [(j, 0.0 - v) for j, v in b[ib:]]
        else:
            order, left, right = [], {}, {}
            for side, entries in ((left, a), (right, b)):
                for j, v in entries:
                    if j not in left and j not in right:
                        order.append(j)
                    side[j] = side.get(j, 0.0) + v
            row = [(j, left.get(j, 0.0) - right.get(j, 0.0)) for j in reversed(order)]
        for j, v in row:
            if v != 0:
                Cj.append(j)
                Cx.append(v)
        Cp.append(len(Cj))
    return Cp, Cj, Cx


def model_jacobi(S, T, dinv, w, degree, steps=None):
    """The smoothed prolongator by loops, in T's format: W = (S * dinv) * w, then `degree` times P - W * P.  steps: a list
    that receives what every subtraction did (see _model_minus)."""
    n = S.shape[0]
    Sp, Sj, Sx = S.indptr.tolist(), S.indices.tolist(), np.ravel(S.data).tolist()
    Wx = list(Sx)
    for i in range(n):
        for jj in range(Sp[i], Sp[i + 1]):
            Wx[jj] = (Sx[jj] * float(dinv[i])) * w
    Pp, Pj, Px = T.indptr.tolist(), T.indices.tolist(), np.ravel(T.data).tolist()
    for _ in range(degree):
        Xp, Xj, Xx = _model_matmat(n, Sp, Sj, Wx, Pp, Pj, Px)
        Pp, Pj, Px = _model_minus(n, Pp, Pj, Px, Xp, Xj, Xx, steps)
    Pp, Pj, Px = np.array(Pp, dtype=np.intc), np.array(Pj, dtype=np.intc), np.array(Px, dtype=np.float64)
    if T.format == "bsr":
        return sps.bsr_matrix((Px.reshape(-1, 1, 1), Pj, Pp), shape=T.shape)
    return sps.csr_matrix((Px, Pj, Pp), shape=T.shape)


# -------------------------------------------------------------------------------------------------- degenerate sizes
# Matrices without rows, without stored entries and of one row: the shapes at which an upload has no bytes, an
# allocation no size and a branch nothing to launch.
def _no_entries(shape, dtype=np.float64):
    return sps.csr_matrix(shape, dtype=dtype)


def degenerate_strength_names():
    return ["%s_theta_%g" % (kind, theta) for theta in (0, 0.25) for kind in ("no_rows", "no_entries_3x3", "one_by_one")]


@functools.lru_cache(maxsize=None)
def degenerate_strength_cases():
    """name -> (A, theta)"""
    out = {}
    for theta in (0, 0.25):
        out["no_rows_theta_%g" % theta] = (_no_entries((0, 0)), theta)
        out["no_entries_3x3_theta_%g" % theta] = (_no_entries((3, 3)), theta)
        out["one_by_one_theta_%g" % theta] = (sps.csr_matrix(np.array([[2.0]])), theta)
    return out


def degenerate_fit_names():
    return ["no_members_3x1", "second_aggregate_empty_3x2"]


@functools.lru_cache(maxsize=None)
def degenerate_fit_cases():
    """name -> (AggOp, B), K1 = K2 = 1.  An aggregate without members leaves a zero in R and no block in T."""
    B = np.array([[1.0], [2.0], [3.0]])
    one = sps.csr_matrix((np.ones(1, dtype=np.int8), np.array([0], dtype=np.intc), np.array([0, 0, 1, 1], dtype=np.intc)), shape=(3, 2))
    return {"no_members_3x1": (_no_entries((3, 1), np.int8), B), "second_aggregate_empty_3x2": (one, B)}


def degenerate_jacobi_names():
    return ["%s_degree%d" % (kind, degree) for kind in ("no_entries_in_T", "no_entries_in_S", "one_by_one") for degree in (1, 2)]


@functools.lru_cache(maxsize=None)
def degenerate_jacobi_cases():
    """name -> dict(S, T, omega, degree, weighting), weighting 'local' (with 'diagonal' an S without entries has a zero
    spectral radius, which the host route divides by)"""
    tridiagonal = sps.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(3, 3), format="csr")
    columns = sps.csr_matrix((np.ones(3), np.array([0, 0, 1], dtype=np.intc), np.arange(4, dtype=np.intc)), shape=(3, 2))
    operands = {"no_entries_in_T": (tridiagonal, _no_entries((3, 2))), "no_entries_in_S": (_no_entries((3, 3)), columns),
                "one_by_one": (sps.csr_matrix(np.array([[2.0]])), sps.csr_matrix(np.array([[1.0]])))}
    return {"%s_degree%d" % (kind, degree): dict(S=S, T=T, omega=4.0 / 3.0, degree=degree, weighting="local")
            for kind, (S, T) in operands.items() for degree in (1, 2)}


def degenerate_graph_names():
    return ["no_vertices", "three_isolated_vertices", "identity_3x3"]


@functools.lru_cache(maxsize=None)
def degenerate_graphs():
    """name -> (Cm, y) for mis_aggregation.  A vertex without an off-diagonal entry is no root: the last two give zero
    aggregates."""
    return {"no_vertices": (_no_entries((0, 0), np.int8), np.zeros(0)),
            "three_isolated_vertices": (_no_entries((3, 3), np.int8), np.array([0.5, 0.25, 0.75])),
            "identity_3x3": (sps.identity(3, dtype=np.int8, format="csr"), np.array([0.5, 0.25, 0.75]))}
