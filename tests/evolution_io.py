"""TEST INFRASTRUCTURE: the evolution strength fixtures of tests/golden/evolution/ (tools/gen_golden_evolution.py)
and few-line sequential models of the four native kernels of amg_core/evolution_strength.h."""
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


def same_bits(C, G):
    """two CSR matrices with the same arrays, stored order included"""
    assert C.shape == G.shape
    assert np.array_equal(C.indptr, G.indptr), "row offsets differ"
    assert np.array_equal(C.indices, G.indices), "columns (or their stored order) differ"
    assert np.array_equal(C.data, G.data), "values differ: worst %g" % np.abs(C.data - G.data).max()


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
