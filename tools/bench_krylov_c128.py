#!/usr/bin/env python3
"""GMRES(20) around the complex128 cycle, host vectors against device vectors: wall clock per iteration.

The 100^3 magnetic Laplacian (10^6 unknowns) of tests/test_gpu_hier_c128.py, one hierarchy (SA aggregates of |A|,
symmetric Gauss-Seidel + Chebyshev smoothers, dense coarse solve), the same tol and restart length for

  scipy   ml.solve(b, accel=scipy.sparse.linalg.gmres): every cycle copies its vector to the device and back, the
          orthogonalisation runs in numpy;
  device  pyamg_amd.krylov_c128.gmres(A, b, restrt=20, M=ml.aspreconditioner()): vectors stay in HBM.

Both end on the host with x, so the host clock around each call includes all device work.  One warm-up of each, then
the two alternate; one JSON line with the median wall time, the iterations (history entries after the first) and the
time per iteration of each, and the true relative residuals.
Usage:  python tools/bench_krylov_c128.py [--n 100] [--tol 1e-8] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.linalg
import scipy.sparse as sps
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RESTART = 20


def magnetic3d(n, shift, seed):
    rng = np.random.RandomState(seed)
    T = sps.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")
    eye = sps.identity(n, format="csr")
    L = (sps.kron(sps.kron(T, eye), eye) + sps.kron(sps.kron(eye, T), eye) + sps.kron(sps.kron(eye, eye), T)).tocoo()
    off = L.row < L.col
    r, c = L.row[off], L.col[off]
    ph = np.exp(1j * rng.uniform(-np.pi, np.pi, size=r.size))
    N = L.shape[0]
    W = sps.coo_matrix((np.concatenate([ph, ph.conj()]), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(N, N))
    deg = np.asarray(abs(W).sum(axis=1)).ravel()
    A = (sps.diags(deg + shift) - W).tocsr().astype(np.complex128)
    A.sort_indices()
    return A


def hierarchy(A):
    import pyamg_amd
    Ar = sps.csr_matrix((np.abs(A.data), A.indices, A.indptr), shape=A.shape)
    mlr = pyamg_amd.smoothed_aggregation_solver(Ar, max_coarse=500, max_levels=4)
    levels, Ak = [], A
    for i, lr in enumerate(mlr.levels):
        lvl = pyamg_amd.multilevel_solver.level()
        lvl.A = Ak
        if i < len(mlr.levels) - 1:
            lvl.P = sps.csr_matrix(lr.P)
            lvl.R = lvl.P.T.tocsr()
            Ak = sps.csr_matrix(lvl.R @ Ak @ lvl.P)
        levels.append(lvl)
    M = np.ascontiguousarray(scipy.linalg.pinv(levels[-1].A.toarray()), dtype=np.complex128)
    ml = pyamg_amd.multilevel_solver(levels, coarse_solver=("dense", {"M": M}))
    nl = len(levels) - 1
    cheb = ("polynomial", {"coefficients": [-0.1, 0.9, 1.4]})
    pyamg_amd.change_smoothers(ml, [("gauss_seidel", {"sweep": "symmetric"})] + [cheb] * (nl - 1), [cheb] * nl)
    return ml


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--outer", type=int, default=10, help="restart cycles allowed")
    a = ap.parse_args()
    import pyamg_amd
    from pyamg_amd import krylov_c128
    if pyamg_amd.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    A = magnetic3d(a.n, 0.05, seed=3)
    ml = hierarchy(A)
    rng = np.random.RandomState(5)
    b = rng.rand(A.shape[0]) + 1j * rng.rand(A.shape[0])
    M = ml.aspreconditioner()

    def scipy_path():
        res = []
        # scipy's gmres restarts after 20 inner iterations by default; with a callback it counts maxiter in inner ones
        x = ml.solve(b, tol=a.tol, maxiter=a.outer * RESTART, accel=spla.gmres, residuals=res)
        return x, res

    def device_path():
        res = []
        x, _ = krylov_c128.gmres(ml.levels[0].A, b, tol=a.tol, restrt=RESTART, maxiter=a.outer, M=M, residuals=res)
        return x, res

    out = {"n": a.n, "unknowns": int(A.shape[0]), "levels": len(ml.levels), "tol": a.tol, "restart": RESTART}
    paths = {"scipy": scipy_path, "device": device_path}
    times = {k: [] for k in paths}
    last = {}
    for k, fn in paths.items():
        fn()                                  # warm-up: code objects, the device mirror, first allocations
    for _ in range(a.reps):
        for k, fn in paths.items():
            t0 = time.perf_counter()
            last[k] = fn()
            times[k].append(time.perf_counter() - t0)
    normb = np.linalg.norm(b)
    for k in paths:
        x, res = last[k]
        its = len(res) - 1
        t = float(np.median(times[k]))
        out[k] = {"wall_s": round(t, 4), "wall_s_all": [round(v, 4) for v in times[k]], "iterations": its,
                  "ms_per_iteration": round(1e3 * t / max(its, 1), 3),
                  "true_relative_residual": float(np.linalg.norm(b - A @ x) / normb)}
    out["speedup_per_iteration"] = round(out["scipy"]["ms_per_iteration"] / out["device"]["ms_per_iteration"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
