#!/usr/bin/env python3
"""The smoothed-aggregation stages of DESIGN.md section 8m -- symmetric strength (theta = 0.1), fit_candidates (one
candidate, the aggregates of standard_aggregation) and Jacobi prolongation smoothing (degree 1, weighting 'diagonal') --
by the host route and by the device route (pyamg_amd/aggregation.py, csrc/prolong.hip) on Poisson 500 x 500 and 100^3.

host / device: the public calls, argument checks, transfers and the assembly of the result included; for the smoothing
also the part both routes keep on the host (the diagonal, the scaled copy of S and the spectral-radius estimate, which
runs on the device above util.DEVICE_RHO_MIN_ROWS on either route), which the row "jacobi weights" times alone.
upload / in HBM / fetch: the device entry's own clock.  The results are compared array for array.  Every timing is the
median of --repeat runs after one warm-up run, in milliseconds.  The table is what profiles/r22_sa_stages.txt holds.

Usage:  python tools/bench_sa_stages.py [--repeat 5] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_classical import median, same, timed, verdict  # noqa: E402
from pyamg_amd import _host, aggregation  # noqa: E402
from pyamg_amd.aggregation import (fit_candidates, jacobi_prolongation_smoother, standard_aggregation,  # noqa: E402
                                   symmetric_strength_of_connection)
from pyamg_amd.gallery import poisson  # noqa: E402

THETA = 0.1                 # keeps every entry of both operators (0.01 * 16 and 0.01 * 36 lie below 1)


def stages(name, grid, repeat):
    A = poisson(grid, format="csr")
    n = A.shape[0]
    Cm = symmetric_strength_of_connection(A, THETA)
    AggOp = standard_aggregation(Cm)[0]
    B = np.ones((n, 1))
    T = fit_candidates(AggOp, B)[0]

    def smooth(device, times=None):
        np.random.seed(0)
        if hasattr(A, "rho"):
            del A.rho
        return jacobi_prolongation_smoother(A, T, Cm, B, device=device, times=times)
    calls = (("strength", lambda d, t: symmetric_strength_of_connection(A, THETA, device=d, times=t), same),
             ("fit_candidates", lambda d, t: fit_candidates(AggOp, B, device=d, times=t),
              lambda h, g: same(h[0], g[0]) and h[1].tobytes() == g[1].tobytes()),
             ("jacobi", smooth, same))
    out = []
    for stage, fn, equal in calls:
        host, dev, parts, ok = [], [], [], True
        for it in range(repeat + 1):
            H, th = timed(lambda: fn(False, None))
            times = []
            D, td = timed(lambda: fn(True, times))
            ok = ok and equal(H, D)
            if it:
                host.append(th); dev.append(td); parts.append(times)
        entries = (D[0] if isinstance(D, tuple) else D).nnz
        split = " ".join("%8.1f" % median([p[k] for p in parts]) for k in range(3))
        out.append("%-16s %-15s %9d %10d %9.1f %9.1f  %s  %s" % (name, stage, n, entries, median(host), median(dev), split, verdict(ok)))
    shared = []
    for it in range(repeat + 1):
        np.random.seed(0)
        _, t = timed(lambda: aggregation._jacobi_weights(A, 4.0 / 3.0, "diagonal"))
        if it:
            shared.append(t)
    out.append("%-16s %-15s %9d %10s %9.1f %9s" % (name, "jacobi weights", n, "-", median(shared), "-"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(new):
        for line in new:
            lines.append(line)
            print(line, flush=True)
    say(["smoothed-aggregation stages, host route against device route; milliseconds, median of %d runs after one warm-up" % a.repeat,
         "host: numpy, scipy and csrc/setup_host.cpp on %d threads; device: csrc/prolong.hip" % _host.host_lib().amgsetup_num_threads(),
         "host / device: the public calls; upload, in HBM, fetch: the device entry's own clock",
         "%-16s %-15s %9s %10s %9s %9s  %8s %8s %8s" % ("problem", "stage", "rows", "entries", "host", "device", "upload", "in HBM", "fetch")])
    for name, grid in (("poisson 500x500", (500, 500)), ("poisson 100^3", (100, 100, 100))):
        say(stages(name, grid, a.repeat))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
