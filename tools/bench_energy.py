#!/usr/bin/env python3
"""Energy-minimisation prolongation smoothing, CG with maxiter 4, degree 1, 'local' weighting on symmetric strength:
the host route against the device route (pyamg_amd/smooth.py) on 3-D Poisson and gallery.tet_diffusion, the operators
of tools/bench_evolution.py.

Strength, aggregation and the tentative prolongator are built once per operator and handed to both routes.  What both
routes share and compute on the host (the sparsity pattern, BtBinv, the row weights: "prepare") is timed apart; the
host column is the CG iteration of csrc/setup_host.cpp with the thread count printed in the header; the device route
is split into upload, iterations and fetch (the first two from amg_energy_smooth_device's own clock, which
synchronises the device at both ends).  Every timing is the median of --repeat runs after one warm-up run; the two
results are compared bit for bit.  The table is what profiles/r14_energy_smoothing.txt holds; smooth.DEVICE_AUTO is
decided on it.

--rootnode measures root-node smoothing instead (Cpt_params true: the operators of util.get_Cpt_params, T scaled by
util.scale_T, the root blocks held at the identity), once with one candidate and once with two (ones and a linear
ramp), so that the initial fit T B_c = B_f is inside the timed iteration.  profiles/r15_rootnode.txt holds that table.

Usage:  python tools/bench_energy.py [--rootnode] [--repeat 5] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyamg_amd import smooth  # noqa: E402
from pyamg_amd.aggregation import fit_candidates, host_lib, standard_aggregation, symmetric_strength_of_connection  # noqa: E402
from pyamg_amd.gallery import poisson, tet_diffusion  # noqa: E402


def median(v):
    return float(np.median(np.asarray(v)))


def measure(name, A, repeat, rootnode=False, candidates=1):
    n = A.shape[0]
    C = symmetric_strength_of_connection(A)
    AggOp, Cnodes = standard_aggregation(C)
    B = np.ones((n, 1)) if candidates == 1 else np.column_stack([np.ones(n), np.linspace(0.0, 1.0, n)])
    if rootnode:
        from pyamg_amd.util import get_Cpt_params, scale_T
        T, _ = fit_candidates(AggOp, B[:, :1])
        par = get_Cpt_params(A, Cnodes, AggOp, T)
        T = scale_T(T, par["P_I"], par["I_F"])
        Bc, Bf, cpt = par["P_I"].T * B, B, (True, par)
    else:
        T, Bc = fit_candidates(AggOp, B)
        Bf, cpt = None, (False, {})
    opt = dict(maxiter=4, degree=1, weighting="local")
    prep, host, up, it_ms, fe, tot = [], [], [], [], [], []
    H = Dm = None
    for run in range(repeat + 1):
        t0 = time.perf_counter()
        H = smooth.energy_prolongation_smoother(A, T, C, Bc, Bf, cpt, device=False, **opt)
        t1 = time.perf_counter()
        times = []
        Dm = smooth.energy_prolongation_smoother(A, T, C, Bc, Bf, cpt, device=True, _times=times, **opt)
        t2 = time.perf_counter()
        if run:                         # the first run warms both routes up
            device_cg = sum(times)
            shared = (t2 - t1) * 1e3 - device_cg            # pattern, BtBinv, weights, the final eliminate_zeros
            prep.append(shared); host.append((t1 - t0) * 1e3 - shared)
            up.append(times[0]); it_ms.append(times[1]); fe.append(times[2]); tot.append(device_cg)
    same = (np.array_equal(H.indptr, Dm.indptr) and np.array_equal(H.indices, Dm.indices) and np.array_equal(H.data, Dm.data))
    return "%-24s %9d %10d %10d %9.1f %9.1f %9.1f %10.1f %9.1f %9.1f %7.2f  %s" % (
        name, n, A.nnz, len(H.indices), median(prep), median(host), median(up), median(it_ms), median(fe), median(tot),
        median(host) / median(tot), "same bits" if same else "DIFFERENT")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rootnode", action="store_true", help="root-node smoothing, with one and with two candidates")
    a = ap.parse_args()
    what = "root-node energy prolongation smoothing" if a.rootnode else "energy prolongation smoothing"
    lines = ["%s: cg, maxiter 4, degree 1, weighting 'local', symmetric strength, %s; milliseconds, median of %d runs"
             % (what, "one candidate, then two (with the initial fit)" if a.rootnode else "one candidate", a.repeat),
             "host CG: numpy + csrc/setup_host.cpp on %d OpenMP threads; device: csrc/energy.hip; prepare: host work both routes share"
             % host_lib().amgsetup_num_threads(),
             "host CG = (host route) - prepare, prepare = (device route) - device; ratio = host CG / device",
             "%-24s %9s %10s %10s %9s %9s %9s %10s %9s %9s %7s" % ("operator", "rows", "nnz(A)", "blocks(P)", "prepare", "host CG", "upload",
                                                                "iterations", "fetch", "device", "ratio")]
    cases = [("poisson 40^3", lambda: poisson((40, 40, 40))), ("poisson 64^3", lambda: poisson((64, 64, 64))),
             ("tet_diffusion 40^3", lambda: tet_diffusion(40)), ("tet_diffusion 60^3", lambda: tet_diffusion(60))]
    for candidates in ((1, 2) if a.rootnode else (1,)):
        for name, make in cases:
            label = name if not a.rootnode else "%s, B %d" % (name, candidates)
            lines.append(measure(label, make(), a.repeat, a.rootnode, candidates))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
