"""Wall time per call of the flat amg_core entries in float32 / complex64 / complex128 (float64 for comparison)
on the 3-D Poisson operator at 128^3.  One JSON line per (entry, dtype).

A flat call stages its operands over PCIe and copies the mutated vectors back, so these wall times are
dominated by the copies; kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool.
Usage:  python tools/bench_dtypes.py [--n 128] [--steps 3] [--entries csr_matvec,jacobi,...] [--dtypes f32,c64,...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyamg_amd import amg_core  # noqa: E402
from pyamg_amd.aggregation import poisson  # noqa: E402

DTYPES = {"f64": np.float64, "f32": np.float32, "c64": np.complex64, "c128": np.complex128}


def operands(A, dt, rng):
    def v(k):
        r = rng.randn(k)
        if np.dtype(dt).kind == "c":
            r = r + 1j * rng.randn(k)
        return np.ascontiguousarray(r.astype(dt))
    Ax = A.data.astype(dt)
    if np.dtype(dt).kind == "c":
        Ax = (Ax + 0.01j).astype(dt)
    return Ax, v


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=128)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--entries", default="csr_matvec,jacobi,gauss_seidel,gauss_seidel_ne,jacobi_ne")
    p.add_argument("--dtypes", default="f64,f32,c64,c128")
    a = p.parse_args()
    A = poisson((a.n, a.n, a.n)).tocsr()
    A.sort_indices()
    Ap, Aj = A.indptr.astype(np.intc), A.indices.astype(np.intc)
    n = A.shape[0]
    for tag in a.dtypes.split(","):
        dt = DTYPES[tag]
        rng = np.random.RandomState(0)
        Ax, vec = operands(A, dt, rng)
        x0, b = vec(n), vec(n)
        w = np.array([0.7], dtype=dt)
        D = np.ascontiguousarray((1.0 / np.asarray(abs(A).power(2).sum(axis=1)).ravel()).astype(dt))
        calls = {
            "csr_matvec": lambda x: amg_core.csr_matvec(n, n, Ap, Aj, Ax, b, x),
            "jacobi": lambda x: amg_core.jacobi(Ap, Aj, Ax, x, b, np.zeros(n, dt), 0, n, 1, w),
            "gauss_seidel": lambda x: amg_core.gauss_seidel(Ap, Aj, Ax, x, b, 0, n, 1),
            "gauss_seidel_ne": lambda x: amg_core.gauss_seidel_ne(Ap, Aj, Ax, x, b, 0, n, 1, D, 0.9),
            "jacobi_ne": lambda x: amg_core.jacobi_ne(Ap, Aj, Ax, x, b, D, np.zeros(n, dt), 0, n, 1, w),
        }
        for entry in a.entries.split(","):
            x = x0.copy()
            calls[entry](x)                           # warm-up: first launch, allocator
            t = time.perf_counter()
            for _ in range(a.steps):
                calls[entry](x)
            ms = (time.perf_counter() - t) / a.steps * 1e3
            print(json.dumps(dict(entry=entry, dtype=tag, rows=n, nnz=int(A.nnz), steps=a.steps,
                                  wall_ms_per_call=round(ms, 3), finite=bool(np.all(np.isfinite(x))))), flush=True)


if __name__ == "__main__":
    main()
