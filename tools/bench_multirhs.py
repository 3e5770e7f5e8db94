#!/usr/bin/env python3
"""solve_many: time the batched cycle for k = 1, 2, 4, 8 right-hand sides on the metric's configuration (3-D Poisson
size^3, smoothed aggregation, Chebyshev(2) V-cycles; --smoother gauss_seidel: symmetric Gauss-Seidel).  For every k:
`--cycles` steps (cycle + per-column residual norms, no early stop) after `--warmup` ones, timed with device events.
Prints one JSON line: ms per step, ms per step and column, resident bytes, and the byte model's figure per step.

With --one-vector the one-vector engine (solve(), compressed operator forms) runs the same number of steps in the same
process for a like-for-like ms per step.  The yardstick of DESIGN.md section 9c is
    ratio = 8 x (bench.py ms per step) / (k = 8 ms per step).
Usage:  python tools/bench_multirhs.py [size] [--smoother chebyshev|gauss_seidel] [--ks 1,2,4,8] [--cycles 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def build(size, smoother):
    from pyamg_amd.aggregation import poisson, smoothed_aggregation_solver
    t0 = time.time()
    A = poisson((size, size, size))
    np.random.seed(0)
    sm = ("chebyshev", {"degree": 2}) if smoother == "chebyshev" else ("gauss_seidel", {"sweep": "symmetric"})
    ml = smoothed_aggregation_solver(A, presmoother=sm, postsmoother=sm)
    log("[bench_multirhs] setup %.1fs" % (time.time() - t0))
    log(repr(ml))
    return ml


def model_bytes(ml, k):
    """bytes one step (V-cycle + outer residual) moves if every operator streams once per application as plain CSR
    (12 B per entry + 4 B per row) and every vector operand of a kernel moves once (8 k B per row): per application of
    A the gathered operand and the epilogue's vectors.  Polynomial smoothers: one application per coefficient (first:
    b, r, h; later: r, h or r, x twice); Gauss-Seidel sweeps: x twice and b; jacobi: temp copy, b, x."""
    def mat(M):
        return M.nnz * 12 + (M.shape[0] + 1) * 4

    def smoother(fn, A):
        d = getattr(fn, "desc", None) or {}
        name, it, n = d.get("name"), int(d.get("iterations", 1)), A.shape[0]
        if name == "polynomial":
            nc = len(d["coefficients"])
            return it * (nc * mat(A) + (4 + 4 * (nc - 1)) * n * 8 * k)
        if name in ("gauss_seidel", "sor"):
            sweeps = 2 if d.get("sweep") == "symmetric" else 1
            return it * sweeps * (mat(A) + 3 * n * 8 * k) + (it * 4 * n * 8 * k if name == "sor" else 0)
        if name == "jacobi":
            return it * (mat(A) + 6 * n * 8 * k)
        return 0

    mats = vecs = 0
    for i, lvl in enumerate(ml.levels[:-1]):
        n, nc = lvl.A.shape[0], lvl.P.shape[1]
        mats += smoother(lvl.presmoother, lvl.A) + smoother(lvl.postsmoother, lvl.A)
        mats += mat(lvl.A) + mat(lvl.R) + mat(lvl.P)
        vecs += (3 * n + (n + nc) + (nc + 2 * n) + nc) * 8 * k         # residual, R r, x += P e, coarse x = 0
    A0 = ml.levels[0].A
    mats += mat(A0)
    vecs += 4 * A0.shape[0] * 8 * k                                       # outer residual and its norm
    return mats + vecs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("size", type=int, nargs="?", default=500)
    ap.add_argument("--smoother", default="chebyshev", choices=["chebyshev", "gauss_seidel"])
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one-vector", action="store_true", help="also time solve() of the one-vector engine")
    a = ap.parse_args()
    ks = [int(v) for v in a.ks.split(",")]

    ml = build(a.size, a.smoother)
    n = ml.levels[0].A.shape[0]
    out = {"metric": "solve_many_ms_per_step", "size": a.size, "unknowns": int(n), "smoother": a.smoother,
           "levels": len(ml.levels), "cycles": a.cycles, "k": {}}
    rs = np.random.RandomState(0)
    if a.one_vector:
        dev1 = ml.device_hierarchy()
        b, x = rs.rand(n), np.zeros(n)
        dev1.solve(b, x, 0.0, a.warmup, "V", x0_zero=True, fixed=True)
        dev1.solve(b, x, 0.0, a.cycles, "V", fixed=True)
        out["one_vector_ms_per_step"] = dev1.last_solve_ms() / a.cycles
        out["one_vector_device_bytes"] = int(dev1.device_bytes())
        log("[bench_multirhs] one vector: %.3f ms per step" % out["one_vector_ms_per_step"])
        ml._invalidate_device()
    t0 = time.time()
    dev = ml.device_hierarchy_multi()
    log("[bench_multirhs] upload %.1fs, %.1f GB in HBM" % (time.time() - t0, dev.device_bytes() / 1e9))
    out["device_bytes"] = int(dev.device_bytes())
    for k in ks:
        B = rs.rand(n, k)
        X = np.zeros((n, k))
        dev.solve(B, X, 0.0, a.warmup, "V", x0_zero=True, fixed=True)
        res = dev.solve(B, X, 0.0, a.cycles, "V", fixed=True)
        ms = dev.last_solve_ms() / a.cycles
        mb = model_bytes(ml, k)
        out["k"][str(k)] = {"ms_per_step": ms, "ms_per_step_and_column": ms / k, "model_bytes_per_step": mb,
                            "model_TBps": mb / (ms * 1e-3) / 1e12,
                            "finite": bool(np.all(np.isfinite(X))),
                            "last_residuals": [float(r[-1]) for r in res]}
        log("[bench_multirhs] k = %d: %.3f ms per step, %.3f per column, model %.2f GB = %.2f TB/s"
            % (k, ms, ms / k, mb / 1e9, mb / (ms * 1e-3) / 1e12))
        del B, X
    print(json.dumps(out))


if __name__ == "__main__":
    main()
