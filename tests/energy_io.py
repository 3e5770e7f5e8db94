"""TEST INFRASTRUCTURE: the energy smoothing fixtures of tests/golden/energy/ (tools/gen_golden_energy.py) and
sequential models of the three native helpers of amg_core/smoothed_aggregation.h, of the block-row product and of the
inner product both routes of pyamg_amd/smooth.py share."""
import json
import os

import numpy as np
import scipy.sparse as sps

import golden_io

ENERGY = os.path.join(golden_io.GOLDEN, "energy")
PROBLEMS = ("aniso_40x40_symmetric", "aniso_40x40_evolution", "aniso_17x23", "elasticity_12x12", "c5_elasticity",
            "random_spd_150")
ARGS = {"incomplete_mat_mult_bsr": ("Ap", "Aj", "Ax", "Bp", "Bj", "Bx", "Sp", "Sj", "Sx", "n_brow", "n_bcol", "brow_A", "bcol_A",
                                    "bcol_B"),
        "satisfy_constraints_helper": ("RowsPerBlock", "ColsPerBlock", "num_block_rows", "NullDim", "x", "y", "z", "Sp", "Sj", "Sx"),
        "calc_BtB": ("NullDim", "Nnodes", "ColsPerBlock", "b", "BsqCols", "x", "Sp", "Sj")}
OUTPUT = {"incomplete_mat_mult_bsr": "Sx", "satisfy_constraints_helper": "Sx", "calc_BtB": "x"}

_cache = {}


def _get(z, key):
    """an array of the file; a stored "=other" stands for the array under that key"""
    v = z[key]
    while v.dtype.kind == "U" and v.ndim == 0 and str(v).startswith("="):
        v = z[str(v)[1:]]
    return v


def _matrix(z, key):
    R, Cc = (int(v) for v in z[key + "_blocksize"])
    shape = tuple(int(v) for v in z[key + "_shape"])
    data, indices, indptr = _get(z, key + "_data"), _get(z, key + "_indices"), _get(z, key + "_indptr")
    if key in ("A", "Atilde") and (R, Cc) == (1, 1):
        return sps.csr_matrix((data, indices, indptr), shape=shape)
    return sps.bsr_matrix((data.reshape(-1, R, Cc), indices, indptr), shape=shape)


def problem(name):
    """-> dict(A, Atilde, T, Bc, B, sets=[dict(options, Sp, Sj, BtBinv, P, trace (rows of <R, Z>, alpha, beta),
    calls=[(kernel, args dict, expected output)])])"""
    if name in _cache:
        return _cache[name]
    z = np.load(os.path.join(ENERGY, name + ".npz"), allow_pickle=False)
    out = {k: _matrix(z, k) for k in ("A", "Atilde", "T")}
    out["Bc"] = _get(z, "Bc")
    out["B"] = _get(z, "B")
    out["sets"] = []
    for q, opt in enumerate(json.loads(str(z["options_json"]))):
        pre = "s%d_" % q
        calls = []
        for ci, kernel in enumerate(str(s) for s in z[pre + "calls"]):
            args = {a: _get(z, "%scall%d__%s" % (pre, ci, a)) for a in ARGS[kernel]}
            args = {a: (v if v.ndim else v.item()) for a, v in args.items()}
            calls.append((kernel, args, _get(z, "%scall%d__out" % (pre, ci))))
        out["sets"].append({"options": opt, "Sp": _get(z, pre + "pattern_indptr"), "Sj": _get(z, pre + "pattern_indices"),
                            "BtBinv": _get(z, pre + "BtBinv"), "P": _matrix(z, pre + "P"), "trace": z[pre + "trace"],
                            "calls": calls})
    _cache[name] = out
    return out


def all_sets():
    """(problem, set index) of every recorded option set"""
    return [(name, q) for name in PROBLEMS for q in range(len(problem(name)["sets"]))]


def recorded_calls(kernel=None):
    """(problem, set index, call index) of the recorded native calls"""
    return [(name, q, ci) for name in PROBLEMS for q, s in enumerate(problem(name)["sets"])
            for ci, c in enumerate(s["calls"]) if kernel is None or c[0] == kernel]


def load_hier(name):
    """golden_io.load_hier for a hier_<name>.npz of tests/golden/energy/"""
    keep = golden_io.GOLDEN
    golden_io.GOLDEN = ENERGY
    try:
        return golden_io.load_hier(name)
    finally:
        golden_io.GOLDEN = keep


def same_bits(P, G):
    """two BSR matrices with the same three arrays, stored order included"""
    assert P.shape == G.shape and P.blocksize == G.blocksize
    assert np.array_equal(P.indptr, G.indptr), "block row offsets differ"
    assert np.array_equal(P.indices, G.indices), "block columns (or their stored order) differ"
    assert np.array_equal(P.data, G.data), "values differ: worst %g" % np.abs(P.data - G.data).max()


def deviation(M, G):
    """the same() measure of tests/test_setup_golden.py as a number: identical sparsity asserted, the largest value
    difference over the largest magnitude of G returned"""
    M = sps.csr_matrix(M); G = sps.csr_matrix(G)
    M.sort_indices(); G.sort_indices()
    assert M.shape == G.shape
    assert np.array_equal(M.indptr, G.indptr) and np.array_equal(M.indices, G.indices), "sparsity differs"
    return np.abs(M.data - G.data).max() / np.abs(G.data).max()


# --------------------------------------------------------------------------- sequential models
def model_incomplete_mat_mult_bsr(Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, Sx, n_brow, n_bcol, brow_A, bcol_A, bcol_B):
    """smoothed_aggregation.h:797-869 with the gemm of linalg.h:420-447 scalar by scalar"""
    R, N, Cc = brow_A, bcol_A, bcol_B
    Sx = Sx.copy()
    A3, B3, S3 = Ax.reshape(-1, R, N), Bx.reshape(-1, N, Cc), Sx.reshape(-1, R, Cc)
    slot = {}
    for i in range(n_brow):
        slot.clear()
        for jj in range(Sp[i], Sp[i + 1]):
            slot[int(Sj[jj])] = jj                          # a column stored twice: the later slot
        for jj in range(Ap[i], Ap[i + 1]):
            j = Aj[jj]
            for kk in range(Bp[j], Bp[j + 1]):
                at = slot.get(int(Bj[kk]))
                if at is None:
                    continue
                for m in range(N):                          # S(r, c) += A(r, m) * B(m, c), m ascending for every (r, c)
                    S3[at] += A3[jj][:, m:m + 1] * B3[kk][m:m + 1, :]
    return Sx


def model_satisfy_constraints(RowsPerBlock, ColsPerBlock, num_block_rows, NullDim, x, y, z, Sp, Sj, Sx):
    """smoothed_aggregation.h:556-605"""
    R, Cc, ND = RowsPerBlock, ColsPerBlock, NullDim
    Sx = Sx.copy()
    S3 = Sx.reshape(-1, R, Cc)
    Bt, UB, Binv = x.reshape(-1, Cc, ND), y.reshape(-1, R, ND), z.reshape(-1, ND, ND)
    for i in range(num_block_rows):
        for j in range(Sp[i], Sp[i + 1]):
            Cm = np.zeros((ND, Cc))
            for k in range(ND):                             # Cm(d, c) += BtBinv_i(d, k) * B(c, k)
                Cm += Binv[i][:, k:k + 1] * Bt[Sj[j]][:, k][None, :]
            update = np.zeros((R, Cc))
            for d in range(ND):                             # update(r, c) += UB_i(r, d) * Cm(d, c)
                update += UB[i][:, d:d + 1] * Cm[d:d + 1, :]
            S3[j] -= update
    return Sx


def model_calc_BtB(NullDim, Nnodes, ColsPerBlock, b, BsqCols, Sp, Sj):
    """smoothed_aggregation.h:656-734"""
    ND = NullDim
    Bsq = b.reshape(-1, BsqCols)
    src = np.zeros((ND, ND), dtype=int)
    at = 0
    for m in range(ND):
        for n in range(m, ND):
            src[m, n] = src[n, m] = at + (n - m)
        at += ND - m
    x = np.zeros((Nnodes, ND, ND))
    for i in range(Nnodes):
        for j in range(Sp[i], Sp[i + 1]):
            for k in range(Sj[j] * ColsPerBlock, (Sj[j] + 1) * ColsPerBlock):
                x[i] += Bsq[k][src]
    return x.ravel()


def model_block_row_product(n_brow, R, Cc, ND, Sp, Sj, Ux, B):
    """UB = U * B, from 0.0, blocks left to right, the columns of a block left to right"""
    U3, B2 = Ux.reshape(-1, R, Cc), B.reshape(-1, ND)
    UB = np.zeros((n_brow, R, ND))
    for i in range(n_brow):
        for jj in range(Sp[i], Sp[i + 1]):
            for c in range(Cc):
                UB[i] += U3[jj][:, c:c + 1] * B2[Sj[jj] * Cc + c][None, :]
    return UB.ravel()


def model_inner_product(n_brow, bs, Sp, X, Y):
    """<X, Y>: a block row's products in stored order from 0.0, then 256 consecutive values (0.0 past the end) added by
    halving, level after level; and the number of non-zero scalars of X"""
    v = np.zeros(n_brow)
    for i in range(n_brow):
        s = 0.0
        for q in range(Sp[i] * bs, Sp[i + 1] * bs):
            s += X[q] * Y[q]
        v[i] = s
    while True:
        pad = (-len(v)) % 256
        v = np.concatenate([v, np.zeros(pad)]).reshape(-1, 256)
        stride = 128
        while stride >= 1:
            v[:, :stride] = v[:, :stride] + v[:, stride:2 * stride]
            stride //= 2
        v = v[:, 0].copy()
        if len(v) == 1:
            return v[0], float(np.count_nonzero(X))


def pattern_case(rng, n_brow, n_bcol, R, N, Cc, n_blocks_S, sorted_rows=False, empty_row=None, fill=True):
    """random BSR operands for incomplete_mat_mult_bsr with exactly n_blocks_S blocks in S: -> the 14 arguments.
    Rows are shuffled unless sorted_rows; empty_row: a block row that is empty in A, B (as row of B) and S."""
    def rows(n_r, n_c, total, per_row_max):
        counts = np.zeros(n_r, dtype=int)
        free = [r for r in range(n_r) if r != empty_row]
        while counts.sum() < total:
            r = free[rng.randint(len(free))]
            if counts[r] < min(per_row_max, n_c):
                counts[r] += 1
        p = np.concatenate([[0], np.cumsum(counts)]).astype(np.intc)
        j = np.concatenate([rng.choice(n_c, c, replace=False) if not sorted_rows else np.sort(rng.choice(n_c, c, replace=False))
                            for c in counts] + [np.zeros(0, dtype=int)]).astype(np.intc)
        return p, j
    Ap, Aj = rows(n_brow, n_brow, min(4 * n_brow, n_brow * n_brow // 2), 6)
    Bp, Bj = rows(n_brow, n_bcol, min(4 * n_brow, n_brow * n_bcol // 2), 6)
    Sp, Sj = rows(n_brow, n_bcol, n_blocks_S, n_bcol)
    Ax = rng.uniform(-1.0, 1.0, len(Aj) * R * N)
    Bx = rng.uniform(-1.0, 1.0, len(Bj) * N * Cc)
    Sx = rng.uniform(-1.0, 1.0, len(Sj) * R * Cc) if fill else np.zeros(len(Sj) * R * Cc)
    return [Ap, Aj, Ax, Bp, Bj, Bx, Sp, Sj, Sx, n_brow, n_bcol, R, N, Cc]
