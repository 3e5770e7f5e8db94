#!/usr/bin/env python3
"""Evolution strength of connection, k = 2: the host path against the device pipeline (pyamg_amd/strength.py) on
3-D Poisson and gallery.tet_diffusion, each at one size below and one above util.DEVICE_RHO_MIN_ROWS.

rho is estimated once per operator and handed to both paths, so the table shows the measure alone; the pipeline's
time is split into upload, stages and fetch (the first two from amg_evolution_strength_device's own clock, which
synchronises the device at both ends).  Every timing is the median of --repeat runs after one warm-up run; the two
results are compared bit for bit.  The table is what profiles/r13_evolution_strength.txt holds and what decides
strength.DEVICE_AUTO.

Usage:  python tools/bench_evolution.py [--repeat 5] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyamg_amd import strength, util  # noqa: E402
from pyamg_amd.gallery import poisson, tet_diffusion  # noqa: E402


def median(v):
    return float(np.median(np.asarray(v)))


def measure(name, A, repeat):
    n = A.shape[0]
    b = np.ones(n)
    D = A.diagonal()
    Dinv = np.where(D != 0, 1.0 / np.where(D != 0, D, 1.0), 1.0)
    np.random.seed(0)
    rho = float(util.approximate_spectral_radius(util.scale_rows(A, Dinv, copy=True)))
    Ac = strength._canonical_csr(A)
    host, up, st, fe, tot = [], [], [], [], []
    H = Dm = None
    for it in range(repeat + 1):
        t0 = time.perf_counter()
        H = strength.evolution_strength_of_connection(A, None, epsilon=4.0, k=2, device=False, rho=rho)
        t1 = time.perf_counter()
        times = []
        Dm = strength._device_measure(Ac, b, rho, 4.0, 2, True, times=times)
        t2 = time.perf_counter()
        if it:                          # the first run warms both paths up
            host.append((t1 - t0) * 1e3); tot.append((t2 - t1) * 1e3)
            up.append(times[0]); st.append(times[1]); fe.append(times[2])
    same = (np.array_equal(H.indptr, Dm.indptr) and np.array_equal(H.indices, Dm.indices) and np.array_equal(H.data, Dm.data))
    return "%-22s %9d %10d %10.1f %9.1f %9.1f %9.1f %10.1f %7.2f  %s" % (
        name, n, A.nnz, median(host), median(up), median(st), median(fe), median(tot), median(host) / median(tot),
        "same bits" if same else "DIFFERENT")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["evolution strength of connection, k = 2, epsilon = 4, one candidate; milliseconds, median of %d runs" % a.repeat,
             "DEVICE_RHO_MIN_ROWS = %d; host path: numpy / scipy + csrc/setup_host.cpp; pipeline: csrc/strength.hip" % util.DEVICE_RHO_MIN_ROWS,
             "%-22s %9s %10s %10s %9s %9s %9s %10s %7s" % ("operator", "rows", "nnz", "host", "upload", "stages", "fetch",
                                                          "pipeline", "ratio")]
    cases = [("poisson 40^3", lambda: poisson((40, 40, 40))), ("poisson 64^3", lambda: poisson((64, 64, 64))),
             ("tet_diffusion 40^3", lambda: tet_diffusion(40)), ("tet_diffusion 60^3", lambda: tet_diffusion(60))]
    for name, make in cases:
        lines.append(measure(name, make(), a.repeat))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
