"""TEST INFRASTRUCTURE: the evolution strength fixtures of tests/golden/evolution/ (tools/gen_golden_evolution.py)
and few-line sequential models of the four native kernels of amg_core/evolution_strength.h."""
import hashlib
import os

import numpy as np
import scipy.sparse as sps

import golden_io

EVO = os.path.join(golden_io.GOLDEN, "evolution")
PROBLEMS = ("aniso_40x40", "aniso_17x23", "aniso_9x31", "iso_12x12", "unsym_400")
KS = (1, 2, 4)
ARGS = {"incomplete_mat_mult_csr": ("Ap", "Aj", "Ax", "Bp", "Bj", "Bx", "Sp", "Sj", "Sx", "dimen"),
        "apply_distance_filter": ("n_row", "epsilon", "Sp", "Sj", "Sx")}
DBL_MAX = np.finfo(np.float64).max

_cache = {}


def problem(name):
    """-> dict(A, B (or None), epsilon, k -> dict(rho, C, calls=[(kernel, args dict, expected output)]))"""
    if name in _cache:
        return _cache[name]
    z = np.load(os.path.join(EVO, name + ".npz"), allow_pickle=False)
    A = sps.csr_matrix((z["A_data"], z["A_indices"], z["A_indptr"]), shape=tuple(int(v) for v in z["A_shape"]))
    out = {"A": A, "B": z["B"] if "B" in z.files else None, "epsilon": float(z["epsilon"])}
    for k in KS:
        key = "k%d" % k
        C = sps.csr_matrix((z[key + "_C_data"], z[key + "_C_indices"], z[key + "_C_indptr"]), shape=A.shape)
        calls = []
        for ci, kernel in enumerate(str(s) for s in z[key + "_calls"]):
            pre = "%s_call%d__" % (key, ci)
            args = {a: z[pre + a] for a in ARGS[kernel]}
            calls.append((kernel, args, z[pre + "Sx_out"]))
        out[k] = {"rho": float(z[key + "_rho"]), "C": C, "calls": calls}
    _cache[name] = out
    return out


def flat_kernels():
    return np.load(os.path.join(EVO, "flat_kernels.npz"), allow_pickle=False)


def load_hier(name):
    """golden_io.load_hier for a hier_<name>.npz of tests/golden/evolution/"""
    keep = golden_io.GOLDEN
    golden_io.GOLDEN = EVO
    try:
        return golden_io.load_hier(name)
    finally:
        golden_io.GOLDEN = keep


def _first_difference(a, b):
    if a.shape != b.shape:
        return "%d and %d items" % (a.size, b.size)
    at = int(np.flatnonzero(a != b)[0])
    return "first at %d: %r and %r" % (at, a[at], b[at])


def same_bits(C, G):
    """two CSR matrices with the same arrays, stored order included"""
    assert C.shape == G.shape
    assert np.array_equal(C.indptr, G.indptr), "row offsets differ (%s)" % _first_difference(C.indptr, G.indptr)
    assert np.array_equal(C.indices, G.indices), \
        "columns (or their stored order) differ (%s)" % _first_difference(C.indices, G.indices)
    assert np.array_equal(C.data, G.data), \
        "values differ (%s): worst %g" % (_first_difference(C.data, G.data), np.abs(C.data - G.data).max())


def deviation(M, G):
    """the same() measure of tests/test_setup_golden.py as a number: identical sparsity asserted, the largest value
    difference over the largest magnitude of G returned"""
    M = sps.csr_matrix(M); G = sps.csr_matrix(G)
    M.sort_indices(); G.sort_indices()
    assert M.shape == G.shape
    assert np.array_equal(M.indptr, G.indptr) and np.array_equal(M.indices, G.indices), "sparsity differs"
    return np.abs(M.data - G.data).max() / np.abs(G.data).max()


# --------------------------------------------------------------------------- sequential models
def model_incomplete_mat_mult(Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, n):
    Sx = np.zeros(len(Sj))
    for row in range(n):
        for ptr in range(Sp[row], Sp[row + 1]):
            a, b, s = Ap[row], Bp[Sj[ptr]], 0.0
            while a < Ap[row + 1] and b < Bp[Sj[ptr] + 1]:
                if Aj[a] == Bj[b]:
                    s += Ax[a] * Bx[b]
                    a += 1; b += 1
                elif Aj[a] < Bj[b]:
                    a += 1
                else:
                    b += 1
            Sx[ptr] = s
    return Sx


def model_incomplete_entries(Ap, Aj, Ax, Bp, Bj, Bx, rows, cols):
    """model_incomplete_mat_mult for the listed entries (row, col) only: the products of the columns that row `row` of
    A and column `col` of B (CSC) share, added in index order from 0.0 -- what the merge adds.  Rows of A and columns
    of B hold sorted, unique indices."""
    out = np.zeros(len(rows))
    for q, (row, col) in enumerate(zip(rows, cols)):
        a0, b0 = Ap[row], Bp[col]
        _, ia, ib = np.intersect1d(Aj[a0:Ap[row + 1]], Bj[b0:Bp[col + 1]], assume_unique=True, return_indices=True)
        s = 0.0
        for a, b in zip(ia, ib):
            s += Ax[a0 + a] * Bx[b0 + b]
        out[q] = s
    return out


def model_distance_filter(n, epsilon, Sp, Sj, Sx, absolute=False):
    Sx = Sx.copy()
    for i in range(n):
        thr = epsilon
        if not absolute:
            m = DBL_MAX
            for jj in range(Sp[i], Sp[i + 1]):
                if Sj[jj] != i and Sx[jj] < m:
                    m = Sx[jj]
            thr = epsilon * m
        for jj in range(Sp[i], Sp[i + 1]):
            if Sj[jj] == i:
                Sx[jj] = 1.0
            elif Sx[jj] >= thr:
                Sx[jj] = 0.0
    return Sx


def model_min_blocks(n_blocks, blocksize, Sx):
    Tx = np.empty(n_blocks)
    for i in range(n_blocks):
        m = DBL_MAX
        for v in Sx[i * blocksize:(i + 1) * blocksize]:
            if v != 0.0 and v < m:
                m = v
        Tx[i] = m
    return Tx


# --------------------------------------------------------------------------- large problems (from seeds)
# The device pipeline (csrc/strength.hip) is meant for operators of util.DEVICE_RHO_MIN_ROWS = 200 000 rows and more,
# and at that size its library calls run other code than on the fixtures above.  Limits read from the rocPRIM headers
# of the ROCm release the project builds with:
#   rocprim/device/device_radix_sort.hpp (radix_sort_impl), device_radix_sort_config.hpp (radix_sort_config):
#     size <= 256 * 4 = 1024 items         one block sorts everything (radix_sort_block_sort)
#     size <= merge_sort_limit = 1024 * 1024   merge sort (keys wider than 2 bytes)
#     above                                 onesweep, here over all 64 key bits = 8 passes of 8 bits
#   rocprim/device/device_scan.hpp: one block's items (block_size * items_per_thread, a few thousand) are scanned by a
#     single block; above that the multi-block look-back scan runs.
# Keys are (row << 32) | column, so rows above 65 536 set key bits 48 and up.  Both builders therefore assert
# nnz > 2**20 and n > 65 536 and may not be shrunk below that.
SORT_ONE_BLOCK = 1024
SORT_MERGE_LIMIT = 2 ** 20
LARGE = ("large_grid", "large_unsym")
LARGE_EPSILON = 4.0


def stencil_matrix(stencil, nx, ny):
    """{(dy, dx): value} on an nx x ny grid, x fastest, couplings that leave the grid cut off; sorted CSR, int32"""
    idx = np.arange(nx * ny, dtype=np.int64).reshape(ny, nx)
    rows, cols, vals = [], [], []
    for (dy, dx), v in sorted(stencil.items()):
        src = idx[max(0, -dy):ny - max(0, dy), max(0, -dx):nx - max(0, dx)]
        rows.append(src.ravel()); cols.append(src.ravel() + dy * nx + dx); vals.append(np.full(src.size, v))
    A = sps.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nx * ny, nx * ny)).tocsr()
    A.sort_indices()
    A.indices = A.indices.astype(np.intc); A.indptr = A.indptr.astype(np.intc)
    return A


def fixture_stencil(name="aniso_40x40", nx=40, ny=40):
    """the 9-point stencil of a committed grid fixture, read from an interior row; rebuilding the fixture's grid from it
    gives the fixture's own arrays (asserted)"""
    A = problem(name)["A"]
    i = (ny // 2) * nx + nx // 2
    st = {}
    for jj in range(A.indptr[i], A.indptr[i + 1]):
        d = int(A.indices[jj]) - i
        dy = (d + nx // 2) // nx
        st[(dy, d - dy * nx)] = float(A.data[jj])
    assert sorted(st) == [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    R = stencil_matrix(st, nx, ny)
    assert np.array_equal(R.indptr, A.indptr) and np.array_equal(R.indices, A.indices) and np.array_equal(R.data, A.data)
    return st


def large_grid():
    """-> A, B: the stencil of aniso_40x40 on a 480 x 481 grid (230 880 rows, 2 072 158 entries) and a candidate that is
    not constant, so that the measure is unsymmetric before its symmetrisation"""
    if "large_grid" not in _cache:
        A = stencil_matrix(fixture_stencil(), 480, 481)
        n = A.shape[0]
        B = 1.0 + 0.25 * np.random.RandomState(1).rand(n)
        assert n == 230880 and A.nnz == 2072158
        assert A.nnz > SORT_MERGE_LIMIT and n > 65536
        _cache["large_grid"] = (A, B)
    A, B = _cache["large_grid"]
    return A.copy(), B.copy()


UNSYM_SEED = 12


def large_unsym(seed=UNSYM_SEED):
    """-> A, B: 150 000 rows, about 7 random off-diagonal entries per row (4 drawn per row, 3 of them mirrored with a
    magnitude of their own and the same sign, so that most couplings have a partner and powers of the operator keep
    entries on its pattern without cancelling on the diagonal, while the pattern is not symmetric; duplicates
    summed), magnitudes in [0.25, 1] with a random sign, diagonal
    4 + rand; row 23 carries 3000 more entries of magnitude 0.01 .. 0.05 and the diagonal 6; every 9973rd row from 19
    on is empty; rows with i % 7919 == 7 store no diagonal; no stored zeros, rows sorted.  B in [0.5, 1.5], every 9th
    entry negated, B[[3, 23, 50]] = 0.  Magnitudes stay away from zero so that no sign decision of the measure sits
    within rounding of zero (the generator's knife-edge check)."""
    if ("large_unsym", seed) not in _cache:
        n, drawn, mirrored = 150000, 4, 3
        rng = np.random.RandomState(seed)
        signed = lambda lo, hi, size: rng.uniform(lo, hi, size) * rng.choice([-1.0, 1.0], size)
        rows = np.repeat(np.arange(n), drawn)
        cols = rng.randint(0, n, n * drawn)
        back = np.tile(np.arange(drawn) < mirrored, n)
        r = np.concatenate([rows, cols[back]]); c = np.concatenate([cols, rows[back]])
        sign = rng.choice([-1.0, 1.0], rows.size)
        vals = rng.uniform(0.25, 1.0, r.size) * np.concatenate([sign, sign[back]])
        off = r != c
        R = sps.coo_matrix((vals[off], (r[off], c[off])), shape=(n, n)).tocsr()            # sums duplicates
        diag = 4.0 + rng.rand(n)
        diag[23] = 6.0
        diag[np.arange(n) % 7919 == 7] = 0.0
        long_cols = rng.choice(n, 3000, replace=False)
        long_cols = long_cols[long_cols != 23]
        E = sps.coo_matrix((signed(0.01, 0.05, long_cols.size), (np.full(long_cols.size, 23), long_cols)), shape=(n, n)).tocsr()
        keep = np.ones(n)
        keep[19::9973] = 0.0
        A = sps.csr_matrix(sps.diags(keep) * (R + E + sps.diags(diag)))
        A.eliminate_zeros()
        A.sort_indices()
        A.indices = A.indices.astype(np.intc); A.indptr = A.indptr.astype(np.intc)
        B = rng.uniform(0.5, 1.5, n)
        B[::9] *= -1.0
        B[[3, 23, 50]] = 0.0
        length = np.diff(A.indptr)
        assert A.nnz > SORT_MERGE_LIMIT and n > 65536
        assert A.has_canonical_format and not np.any(A.data == 0.0)
        assert length.max() == length[23] >= 3000 and np.count_nonzero(length == 0) == 16 and length[19] == 0
        assert A[7, 7] == 0.0 and A[7926, 7926] == 0.0 and A[23, 23] == 6.0
        P = sps.csr_matrix((np.ones(A.nnz, dtype=np.int8), A.indices, A.indptr), shape=A.shape)
        assert (P != P.T).nnz > 100000                      # the pattern itself is not symmetric
        _cache[("large_unsym", seed)] = (A, B)
    A, B = _cache[("large_unsym", seed)]
    return A.copy(), B.copy()


def large_problem(name):
    return {"large_grid": large_grid, "large_unsym": large_unsym}[name]()


def sha(a, dtype):
    """SHA-256 of an array's values as little-endian dtype ('<i4', '<f8') bytes"""
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dtype).tobytes()).hexdigest()


def digests(M):
    """(indptr, indices, data) digests of a CSR matrix"""
    return sha(M.indptr, "<i4"), sha(M.indices, "<i4"), sha(M.data, "<f8")


def rows_of(M, lo, hi):
    """rows lo..hi-1 of a CSR matrix verbatim: (offsets from 0, columns, values)"""
    a, b = int(M.indptr[lo]), int(M.indptr[hi])
    return (M.indptr[lo:hi + 1] - a).astype(np.intc), M.indices[a:b].astype(np.intc), M.data[a:b].astype(np.float64)


def large_digests():
    """tests/golden/evolution/large_digests.npz: name -> dict(A=(3 digests), B=digest, k -> dict(rho, nnz, C=(3 digests),
    head=(rows 0-31), tail=(last 32 rows)))"""
    if "large_digests" in _cache:
        return _cache["large_digests"]
    z = np.load(os.path.join(EVO, "large_digests.npz"), allow_pickle=False)
    assert float(z["epsilon"]) == LARGE_EPSILON
    out = {}
    for name in LARGE:
        s = lambda key: str(z["%s__%s" % (name, key)])
        d = {"A": (s("A_indptr_sha"), s("A_indices_sha"), s("A_data_sha")), "B": s("B_sha")}
        for k in KS:
            pre = "%s__k%d_" % (name, k)
            d[k] = {"rho": float(z[pre + "rho"]), "nnz": int(z[pre + "nnz"]),
                    "C": tuple(str(z[pre + w + "_sha"]) for w in ("indptr", "indices", "data")),
                    "head": tuple(z[pre + "head_" + w] for w in ("indptr", "indices", "data")),
                    "tail": tuple(z[pre + "tail_" + w] for w in ("indptr", "indices", "data"))}
        out[name] = d
    _cache["large_digests"] = out
    return out


def assert_large_digests(C, rec, what):
    """C against one k-record of large_digests(): the verbatim rows first (they say where), then size and digests"""
    n = C.shape[0]
    for part, lo, hi in (("head", 0, 32), ("tail", n - 32, n)):
        for got, want, arr in zip(rows_of(C, lo, hi), rec[part], ("offsets", "columns", "values")):
            assert np.array_equal(got, want), "%s: %s of rows %d..%d differ from the reference" % (what, arr, lo, hi - 1)
    assert C.nnz == rec["nnz"], "%s: %d entries, the reference has %d" % (what, C.nnz, rec["nnz"])
    for got, want, arr in zip(digests(C), rec["C"], ("indptr", "indices", "data")):
        assert got == want, "%s: digest of %s differs from the reference" % (what, arr)
