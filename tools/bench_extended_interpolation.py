#!/usr/bin/env python3
"""Extended+i interpolation: the host route against the device route (pyamg_amd/classical.py, csrc/setup_host.cpp,
csrc/classical.hip) on Poisson 100^3 with theta = 0.25 and the PMIS splitting.

  stage   extended_interpolation (on the host route's PMIS splitting) with device=False and device=True, without
          truncation and with max_per_row = 4: the public call, argument checks, transfers and the Python around it
          included; beside it direct_interpolation, for scale.  The device entry's own clock: upload, stages, fetch.
  level   one level -- strength, PMIS, extended+i -- by the host route's three calls and by the chained entry
          (classical_level_device), whose own clock splits it into classical.LEVEL_STAGES.

Every timing is the median of --repeat runs after one warm-up run, in milliseconds; results of the two routes are
compared bit for bit.  The table is what profiles/r19_extended_interpolation.txt holds.

Usage:  python tools/bench_extended_interpolation.py [--repeat 5] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_classical import THETA, median, same, timed, verdict  # noqa: E402
from pyamg_amd import _host, classical  # noqa: E402
from pyamg_amd.gallery import poisson  # noqa: E402

CHOICES = (("extended+i", None), ("extended+i, 4 per row", 4))


def stage(name, A, S, splitting, q, repeat):
    args = classical._extended_arguments(A, S, splitting, q)
    host, dev, parts, ok = [], [], [], True
    for it in range(repeat + 1):
        H, th = timed(lambda: classical.extended_interpolation(A, S, splitting, max_per_row=q, device=False))
        D, td = timed(lambda: classical.extended_interpolation(A, S, splitting, max_per_row=q, device=True))
        times = []
        classical._extended_device(*args, times=times)
        ok = ok and same(H, D)
        if it:
            host.append(th); dev.append(td); parts.append(times)
    split = " ".join("%8.1f" % median([p[k] for p in parts]) for k in range(3))
    return "%-24s %9d %10d %10d %9.1f %9.1f %6.2f  %s  %s" % (name, A.shape[0], A.nnz, H.nnz, median(host), median(dev),
                                                             median(host) / median(dev), split, verdict(ok))


def direct(A, S, splitting, repeat):
    host, dev, ok = [], [], True
    for it in range(repeat + 1):
        H, th = timed(lambda: classical.direct_interpolation(A, S, splitting, device=False))
        D, td = timed(lambda: classical.direct_interpolation(A, S, splitting, device=True))
        ok = ok and same(H, D)
        if it:
            host.append(th); dev.append(td)
    return "%-24s %9d %10d %10d %9.1f %9.1f %6.2f  %26s  %s" % ("direct", A.shape[0], A.nnz, H.nnz, median(host), median(dev),
                                                               median(host) / median(dev), "", verdict(ok))


def host_level(A, q):
    S = classical.classical_strength_of_connection(A, THETA, device=False)
    splitting = classical.PMIS(S, device=False)
    return splitting, classical.extended_interpolation(A, S, splitting, max_per_row=q, device=False)


def level(name, A, q, repeat):
    choice = "extended_i" if q is None else ("extended_i", {"max_per_row": q})
    host, dev, parts, ok = [], [], [], True
    for it in range(repeat + 1):
        np.random.seed(0)
        (sh, Ph), th = timed(lambda: host_level(A, q))
        times = []
        np.random.seed(0)
        (sd, Pd, _), td = timed(lambda: classical.classical_level_device(A, THETA, "PMIS", times=times, interpolation=choice))
        ok = ok and np.array_equal(sh, sd) and same(Ph, Pd)
        if it:
            host.append(th); dev.append(td); parts.append(times)
    split = " ".join("%8.1f" % median([p[k] for p in parts]) for k in range(len(classical.LEVEL_STAGES)))
    return "%-24s %9d %9.1f %9.1f %6.2f  %s  %s" % (name, A.shape[0], median(host), median(dev), median(host) / median(dev), split,
                                                   verdict(ok))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    A = poisson((100, 100, 100), format="csr")
    S = classical.classical_strength_of_connection(A, THETA, device=False)
    np.random.seed(0)
    splitting = classical.PMIS(S, device=False)
    lines = []
    head = ["extended+i interpolation on Poisson 100^3, theta = %.2f, PMIS (%d of %d points are C); milliseconds, median of %d runs "
             "after one warm-up" % (THETA, int(splitting.sum()), A.shape[0], a.repeat),
             "host: csrc/setup_host.cpp on %d threads; device: csrc/classical.hip" % _host.host_lib().amgsetup_num_threads(),
             "", "stage: the public call with device=False / device=True; the device entry's own clock: upload stages fetch",
             "%-24s %9s %10s %10s %9s %9s %6s  %8s %8s %8s" % ("interpolation", "rows", "nnz(A)", "nnz(P)", "host", "device", "ratio",
                                                               "upload", "stages", "fetch")]

    def say(new):
        for line in new:
            lines.append(line)
            print(line, flush=True)
    say(head)
    say([direct(A, S, splitting, a.repeat)])
    for name, q in CHOICES:
        say([stage(name, A, S, splitting, q, a.repeat)])
    say(["", "level: strength + PMIS + interpolation; the chained entry's own clock: " + " ".join(classical.LEVEL_STAGES),
         "%-24s %9s %9s %9s %6s  %s" % ("interpolation", "rows", "host", "device", "ratio",
                                        " ".join("%8s" % s[:8] for s in classical.LEVEL_STAGES))])
    for name, q in CHOICES:
        say([level(name, A, q, a.repeat)])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
