#!/usr/bin/env python3
"""MIS(2) aggregation: the host route against the device route (pyamg_amd/aggregation.py,
csrc/setup_host.cpp, csrc/misagg.hip) on the symmetric strength patterns (theta = 0) of Poisson 500 x 500 and 100^3,
with the host's standard_aggregation beside them for scale.

Every column is the public call -- argument checks, the symmetry check, transfers and the assembly of AggOp included --
except upload / rounds / fetch, which are the device entry's own clock.  The weights are RandomState(0).rand(n), the same
for both routes; the results are compared entry for entry.  Every timing is the median of --repeat runs after one
warm-up run, in milliseconds.  The table is what profiles/r21_mis_aggregation.txt holds.

--table prints README.md's table instead: smoothed_aggregation_solver and rootnode_solver with aggregate='standard' and
'mis' on Poisson 40 x 40, the rotated anisotropic 40 x 40 operator of the evolution fixtures and Poisson 12^3
(max_coarse=20, seed 0, default symmetric Gauss-Seidel, V-cycles to tol=1e-8 from zero on RandomState(7).rand(n)).

Usage:  python tools/bench_mis_aggregation.py [--repeat 5] [--out FILE] [--table]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_classical import median, same, timed, verdict  # noqa: E402
from pyamg_amd import _host  # noqa: E402
from pyamg_amd.aggregation import mis_aggregation, standard_aggregation, symmetric_strength_of_connection  # noqa: E402
from pyamg_amd.gallery import poisson  # noqa: E402


def case(name, grid, repeat):
    Cm = symmetric_strength_of_connection(poisson(grid, format="csr"))
    n = Cm.shape[0]
    y = np.random.RandomState(0).rand(n)
    std, host, dev, parts, ok = [], [], [], [], True
    for it in range(repeat + 1):
        (S, _), ts = timed(lambda: standard_aggregation(Cm))
        (H, Hc), th = timed(lambda: mis_aggregation(Cm, y, device=False))
        times, rounds = [], []
        (D, Dc), td = timed(lambda: mis_aggregation(Cm, y, device=True, times=times, rounds=rounds))
        ok = ok and same(H, D) and np.array_equal(Hc, Dc)
        if it:
            std.append(ts); host.append(th); dev.append(td); parts.append(times)
    split = " ".join("%8.1f" % median([p[k] for p in parts]) for k in range(3))
    return "%-16s %9d %10d %9d %9d %6d %9.1f %9.1f %9.1f  %s  %s" % (name, n, Cm.nnz, S.shape[1], H.shape[1], rounds[0], median(std),
                                                                    median(host), median(dev), split, verdict(ok))


def table():
    import pyamg_amd
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import classical_io
    problems = (("Poisson 40x40", poisson((40, 40), format="csr")), ("rotated aniso 40x40", classical_io.operator("aniso_40x40")),
                ("Poisson 12^3", poisson((12, 12, 12), format="csr")))
    out = ["| problem | solver | aggregate | level sizes | operator complexity | cycles |", "|---|---|---|---|---|---|"]
    for name, A in problems:
        b = np.random.RandomState(7).rand(A.shape[0])
        for solver in ("smoothed_aggregation_solver", "rootnode_solver"):
            for aggregate in ("standard", "mis"):
                np.random.seed(0)
                ml = getattr(pyamg_amd, solver)(A, aggregate=aggregate, max_coarse=20)
                res = []
                ml.solve(b, tol=1e-8, maxiter=300, residuals=res)
                out.append("| %s | %s | %s | %s | %.2f | %d |" % (name, solver, aggregate, "/".join(str(l.A.shape[0]) for l in ml.levels),
                                                                ml.operator_complexity(), len(res) - 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(new):
        for line in new:
            lines.append(line)
            print(line, flush=True)
    if a.table:
        say(table())
        return
    say(["MIS(2) aggregation on symmetric strength patterns (theta = 0); milliseconds, median of %d runs after one warm-up" % a.repeat,
         "host: csrc/setup_host.cpp on %d threads; device: csrc/misagg.hip" % _host.host_lib().amgsetup_num_threads(),
         "standard / mis host / mis device: the public calls; upload rounds fetch: the device entry's own clock",
         "%-16s %9s %10s %9s %9s %6s %9s %9s %9s  %8s %8s %8s" % ("problem", "rows", "nnz(C)", "agg std", "agg mis", "rounds", "standard",
                                                                 "mis host", "mis dev", "upload", "rounds", "fetch")])
    for name, grid in (("poisson 500x500", (500, 500)), ("poisson 100^3", (100, 100, 100))):
        say([case(name, grid, a.repeat)])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
