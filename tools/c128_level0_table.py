#!/usr/bin/env python3
"""Level-0 kernels of a complex128 V-cycle, by their own bytes, from a rocprofv3 kernel trace of tools/bench_c128.py.

Level-0 launches are told apart by grid size (one thread per row of A_0, 256 rows per workgroup) and by the
epilogue in the kernel name; bytes per launch come from the operator's shape (A_0 rebuilt from the same seed):
  residual      A + x + b + r                   = A + 3 vectors
  Chebyshev 1   A + x + b, writes r and h       = A + 4 vectors
  Chebyshev 2   A + h + r, reads and writes x   = A + 4 vectors
  P e add       P + e (coarse) + x read/write
with A = 20 B per entry + 4 B per row pointer and 16 B per vector entry.  Usage:
  python tools/c128_level0_table.py KERNEL_TRACE.csv --n 160 [--peak 8.0]
"""
import argparse
import csv
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--n", type=int, default=160)
    ap.add_argument("--peak", type=float, default=8.0, help="TB/s the fractions are taken of")
    a = ap.parse_args()
    import bench_c128
    A = bench_c128.magnetic3d(a.n, 0.05, seed=1)
    n0, nnz = A.shape[0], A.nnz
    n1 = ((a.n + 1) // 2) ** 3
    vec = 16 * n0
    Ab = 20 * nnz + 4 * (n0 + 1)
    Pb = 20 * n0 + 4 * (n0 + 1)              # piecewise-constant aggregation: one entry per row
    bytes_of = {"EpiResid": Ab + 3 * vec, "EpiPoly0": Ab + 4 * vec, "EpiPolyStep": Ab + 4 * vec,
                "EpiAdd": Pb + 16 * n1 + 2 * vec}
    label = {"EpiResid": "residual r = b - A x", "EpiPoly0": "Chebyshev step 1 (r, h = c0 r)",
             "EpiPolyStep": "Chebyshev step 2 (x += c1 r + A h)", "EpiAdd": "prolongation x += P e"}
    grid = ((n0 + 255) // 256) * 256
    dur = defaultdict(list)
    with open(a.trace) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "csr_rows" not in name or int(r["Grid_Size_X"]) != grid:
                continue
            for k in bytes_of:
                if "%s<" % k in name:
                    dur[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9)
    print("level 0: %d unknowns, %d entries; %s" % (n0, nnz, os.path.basename(a.trace)))
    print("%-36s %6s %10s %10s %9s %6s" % ("kernel", "calls", "mean_us", "MB", "TB/s", "frac"))
    for k in ("EpiResid", "EpiPoly0", "EpiPolyStep", "EpiAdd"):
        if not dur[k]:
            continue
        t = sum(dur[k]) / len(dur[k])
        tbs = bytes_of[k] / t / 1e12
        print("%-36s %6d %10.1f %10.1f %9.2f %6.2f" % (label[k], len(dur[k]), t * 1e6, bytes_of[k] / 1e6, tbs,
                                                     tbs / a.peak))


if __name__ == "__main__":
    main()
