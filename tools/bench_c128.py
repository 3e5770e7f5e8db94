#!/usr/bin/env python3
"""Complex128 resident hierarchy: time Chebyshev(2) V-cycles on a 3-D magnetic Laplacian (n^3 unknowns, unit-modulus
edge phases plus a small shift) and the same cycles on its real float64 counterpart (|A|, CSR-stream kernels:
AMG_STENCIL=0 AMG_PATTERN=0 AMG_SELL=0) for a like-for-like ratio.  Prints one JSON line.

Hierarchy: piecewise-constant 2x2x2 aggregation down to <= 1000 unknowns, Galerkin products by scipy, dense coarse
solve; Chebyshev coefficients from a Gershgorin bound (no estimate).  Device events time `--cycles` V-cycles after
`--warmup` ones.  Usage:  python tools/bench_c128.py [--n 160] [--cycles 20] [--warmup 3]

--sa builds the hierarchy with pyamg_amd.smoothed_aggregation_solver instead (symmetry='hermitian', max_coarse=1000,
Chebyshev(2) smoothers from the estimated spectral radius), prints the setup seconds on stderr and in the JSON line
("setup_s"), and turns AMG_SETUP_VERBOSE on so that the library prints its stage split; AMG_SETUP_DEVICE_GALERKIN=0
selects scipy's Galerkin products (the library's default for complex levels; the tool lowers
util.DEVICE_GALERKIN_C128_MIN_ROWS to the float64 row gate so that the device products run).  The float64 counterpart is then the float64 setup of |A|.
"""
import argparse
import json
import os
import sys

os.environ.setdefault("AMG_STENCIL", "0")
os.environ.setdefault("AMG_PATTERN", "0")
os.environ.setdefault("AMG_SELL", "0")

import numpy as np  # noqa: E402
import scipy.linalg  # noqa: E402
import scipy.sparse as sps  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def magnetic3d(n, shift, seed):
    rng = np.random.RandomState(seed)
    T = sps.diags([np.ones(n - 1), np.ones(n - 1)], [-1, 1], format="csr")
    I = sps.identity(n, format="csr")
    G = (sps.kron(sps.kron(T, I), I) + sps.kron(sps.kron(I, T), I) + sps.kron(sps.kron(I, I), T)).tocoo()
    up = G.row < G.col
    r, c = G.row[up], G.col[up]
    ph = np.exp(1j * rng.uniform(-np.pi, np.pi, size=r.size))
    N = n ** 3
    W = sps.coo_matrix((np.concatenate([ph, ph.conj()]), (np.concatenate([r, c]), np.concatenate([c, r]))),
                       shape=(N, N)).tocsr()
    deg = np.asarray(abs(W).sum(axis=1)).ravel()
    A = (sps.diags(deg + shift) - W).tocsr().astype(np.complex128)
    A.sort_indices()
    return A


def agg1d(n):
    m = (n + 1) // 2
    return sps.csr_matrix((np.ones(n), (np.arange(n), np.arange(n) // 2)), shape=(n, m))


def hierarchy(A, n):
    import pyamg_amd
    from pyamg_amd.chebyshev import chebyshev_polynomial_coefficients
    levels, Ak, nk = [], A, n
    while True:
        lvl = pyamg_amd.multilevel_solver.level()
        lvl.A = Ak
        levels.append(lvl)
        if Ak.shape[0] <= 1000:
            break
        a = agg1d(nk)
        P = sps.kron(sps.kron(a, a), a, format="csr")
        lvl.P, lvl.R = P, P.T.tocsr()
        Ak = sps.csr_matrix(lvl.R @ Ak @ P)
        Ak.sort_indices()
        nk = (nk + 1) // 2
    M = np.asarray(scipy.linalg.pinv(levels[-1].A.toarray()), dtype=Ak.dtype)
    ml = pyamg_amd.multilevel_solver(levels, coarse_solver=("dense", {"M": M}))
    specs = []
    for lvl in levels[:-1]:
        rho = float(abs(lvl.A).sum(axis=1).max())               # Gershgorin bound
        co = -chebyshev_polynomial_coefficients(rho / 30.0, 1.1 * rho, 2)[:-1]
        specs.append(("polynomial", {"coefficients": co}))
    pyamg_amd.change_smoothers(ml, specs, specs)
    return ml


def sa_hierarchy(A):
    import time
    import pyamg_amd
    cheb = ("chebyshev", {"degree": 2})
    # the Galerkin products of the complex levels on the device, from the row gate of the float64 setup on
    pyamg_amd.util.DEVICE_GALERKIN_C128_MIN_ROWS = pyamg_amd.util.DEVICE_RHO_MIN_ROWS
    np.random.seed(0)
    t0 = time.perf_counter()
    ml = pyamg_amd.smoothed_aggregation_solver(A, symmetry="hermitian", max_coarse=1000, presmoother=cheb, postsmoother=cheb)
    dt = time.perf_counter() - t0
    print("[bench_c128] smoothed_aggregation_solver (%s, %d unknowns): %.2f s, levels %s"
          % (A.dtype, A.shape[0], dt, [lvl.A.shape[0] for lvl in ml.levels]), file=sys.stderr, flush=True)
    return ml, dt


def time_cycles(ml, b, cycles, warmup):
    dev = ml.device_hierarchy()
    x = np.zeros_like(b)
    dev.solve(b, x, 0.0, warmup, "V", x0_zero=True, fixed=True)
    x[:] = 0
    dev.solve(b, x, 0.0, cycles, "V", x0_zero=True, fixed=True)
    return dev.last_solve_ms() / cycles, int(dev.device_bytes()), x


def level0_bytes(ml, vb):
    """bytes one V-cycle moves on level 0 by its kernels' own operands: two Chebyshev(2) applications (2 row
    passes each: A + 4 vectors), the residual (A + 3 vectors), R r (R + 1 vector), x += P e (P + 2 vectors)"""
    L = ml.levels[0]

    def mat(M):
        return M.nnz * (vb + 4) + (M.shape[0] + 1) * 4
    n = L.A.shape[0]
    return 5 * mat(L.A) + mat(L.R) + mat(L.P) + (16 + 3 + 1 + 2) * n * vb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=160)
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-f64", action="store_true")
    ap.add_argument("--sa", action="store_true", help="build the hierarchy with smoothed_aggregation_solver")
    a = ap.parse_args()
    if a.sa:
        os.environ.setdefault("AMG_SETUP_VERBOSE", "1")
    A = magnetic3d(a.n, 0.05, seed=1)
    rng = np.random.RandomState(2)
    b = rng.rand(A.shape[0]) + 1j * rng.rand(A.shape[0])
    setup_s = None
    if a.sa:
        ml, setup_s = sa_hierarchy(A)
    else:
        ml = hierarchy(A, a.n)
    ms, dbytes, x = time_cycles(ml, b, a.cycles, a.warmup)
    out = {"metric": "c128_vcycle_ms", "n": a.n, "unknowns": int(A.shape[0]), "levels": len(ml.levels),
           "ms_per_cycle": ms, "device_bytes": dbytes, "level0_bytes_per_cycle": level0_bytes(ml, 16),
           "finite": bool(np.all(np.isfinite(x)))}
    out["level0_TBps"] = out["level0_bytes_per_cycle"] / (ms * 1e-3) / 1e12
    if a.sa:
        out["hierarchy"] = "smoothed_aggregation"
        out["setup_s"] = setup_s
        out["device_galerkin"] = os.environ.get("AMG_SETUP_DEVICE_GALERKIN", "1") != "0"
    del ml
    if not a.skip_f64:
        Ar = sps.csr_matrix((np.abs(A.data), A.indices, A.indptr), shape=A.shape)
        if a.sa:
            mlr, out["f64_setup_s"] = sa_hierarchy(Ar)
        else:
            mlr = hierarchy(Ar, a.n)
        ms64, _, _ = time_cycles(mlr, np.ascontiguousarray(b.real), a.cycles, a.warmup)
        out["f64_csr_ms_per_cycle"] = ms64
        out["f64_level0_bytes_per_cycle"] = level0_bytes(mlr, 8)
        out["ratio_c128_over_f64"] = ms / ms64
    print(json.dumps(out))


if __name__ == "__main__":
    main()
