#!/usr/bin/env python3
"""Classical AMG levels: the host route against the device route (pyamg_amd/classical.py, csrc/classical.hip) on
Poisson 500 x 500 and 100^3 with theta = 0.25, the operators of tools/bench_splitting.py.

  stages   classical_strength_of_connection and direct_interpolation (on the host route's PMIS splitting), each with
           device=False and device=True: the public call, transfers and the Python around it included.
  levels   one level -- strength, splitting, interpolation -- by the host route's three calls and by the chained entry
           (classical_level_device), whose own clock splits it into upload, strength, graph (with the start weights),
           splitting, interpolation and fetch; the device is synchronised at every boundary.
  setup    ruge_stuben_solver's loop (max_levels 10, max_coarse 500) with a clock around every step, levels by the host
           route and by the chained entry: strength, splitting, interpolation, transpose (P.T.tocsr()) and Galerkin
           (R * A * P), the last two on the host either way.

Every timing is the median of --repeat runs after one warm-up run, in milliseconds; results of the two routes are
compared bit for bit.  The table is what profiles/r17_classical_level.txt holds.

Usage:  python tools/bench_classical.py [--repeat 5] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyamg_amd import classical  # noqa: E402
from pyamg_amd.gallery import poisson  # noqa: E402

THETA = 0.25
SPLIT = {"PMIS": classical.PMIS, "CLJP": classical.CLJP}


def median(v):
    return float(np.median(np.asarray(v)))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def same(M, G):
    return M.shape == G.shape and all(np.asarray(a).tobytes() == np.asarray(b).tobytes()
                                      for a, b in ((M.indptr, G.indptr), (M.indices, G.indices), (M.data, G.data)))


def verdict(ok):
    return "same bits" if ok else "DIFFERENT"


def stages(name, A, repeat):
    S = classical.classical_strength_of_connection(A, THETA, device=False)
    np.random.seed(0)
    splitting = classical.PMIS(S, device=False)
    out = []
    for stage, fn in (("strength", lambda d: classical.classical_strength_of_connection(A, THETA, device=d)),
                      ("interpolation", lambda d: classical.direct_interpolation(A, S, splitting, device=d))):
        host, dev, ok = [], [], True
        for it in range(repeat + 1):
            H, th = timed(lambda: fn(False))
            D, td = timed(lambda: fn(True))
            ok = ok and same(H, D)
            if it:
                host.append(th); dev.append(td)
        out.append("%-16s %-14s %9d %10d %9.1f %9.1f %6.2f  %s" % (name, stage, A.shape[0], A.nnz, median(host), median(dev),
                                                                   median(host) / median(dev), verdict(ok)))
    return out


def host_level(A, cf):
    S = classical.classical_strength_of_connection(A, THETA, device=False)
    splitting = SPLIT[cf](S, device=False)
    return splitting, classical.direct_interpolation(A, S, splitting, device=False)


def levels(name, A, cf, repeat):
    host, dev, parts, ok = [], [], [], True
    for it in range(repeat + 1):
        np.random.seed(0)
        (sh, Ph), th = timed(lambda: host_level(A, cf))
        times = []
        np.random.seed(0)
        (sd, Pd, _), td = timed(lambda: classical.classical_level_device(A, THETA, cf, times=times))
        ok = ok and np.array_equal(sh, sd) and same(Ph, Pd)
        if it:
            host.append(th); dev.append(td); parts.append(times)
    split = " ".join("%8.1f" % median([p[k] for p in parts]) for k in range(len(classical.LEVEL_STAGES)))
    return "%-16s %-5s %9d %9.1f %9.1f %6.2f  %s  %s" % (name, cf, A.shape[0], median(host), median(dev), median(host) / median(dev),
                                                          split, verdict(ok))


STEPS = ("strength", "splitting", "interpolation", "transpose", "galerkin")


def setup(A, cf, chained, max_levels=10, max_coarse=500):
    """ruge_stuben_solver's loop with a clock around every step -> (operators, milliseconds per step)"""
    ms = dict.fromkeys(STEPS, 0.0)
    ops = [A]
    while len(ops) < max_levels and ops[-1].shape[0] > max_coarse:
        A = ops[-1]
        if chained:
            times = []
            _, P, _ = classical.classical_level_device(A, THETA, cf, times=times, product_order=True)
            t = dict(zip(classical.LEVEL_STAGES, times))
            ms["strength"] += t["upload"] + t["strength"]
            ms["splitting"] += t["graph"] + t["splitting"]
            ms["interpolation"] += t["interpolation"] + t["fetch"]
        else:
            S, t = timed(lambda: classical.classical_strength_of_connection(A, THETA, device=False))
            ms["strength"] += t
            splitting, t = timed(lambda: SPLIT[cf](S, device=False))
            ms["splitting"] += t
            P, t = timed(lambda: classical.direct_interpolation(A, S, splitting, device=False))
            ms["interpolation"] += t
        R, t = timed(lambda: P.T.tocsr())
        ms["transpose"] += t
        Ac, t = timed(lambda: R * A * P)
        ms["galerkin"] += t
        ops.append(Ac)
    return ops, ms


def setups(name, A, cf, repeat):
    out = []
    kept = {}
    for route, chained in (("host", False), ("device", True)):
        runs, total = [], []
        for it in range(repeat + 1):
            np.random.seed(0)
            (ops, ms), t = timed(lambda: setup(A, cf, chained))
            if it:
                runs.append(ms); total.append(t)
        kept[route] = ops
        med = {k: median([r[k] for r in runs]) for k in STEPS}
        whole = median(total)
        out.append("%-16s %-5s %-6s %2d %9.1f  " % (name, cf, route, len(ops), whole) +
                   " ".join("%8.1f (%4.1f%%)" % (med[k], 100.0 * med[k] / whole) for k in STEPS))
    ok = len(kept["host"]) == len(kept["device"]) and all(same(a, b) for a, b in zip(kept["host"], kept["device"]))
    out[-1] += "  " + verdict(ok)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    operators = (("poisson 500x500", poisson((500, 500), format="csr")), ("poisson 100^3", poisson((100, 100, 100), format="csr")))
    lines = ["classical AMG levels, theta = %.2f; milliseconds, median of %d runs after one warm-up" % (THETA, a.repeat),
             "host: csrc/setup_host.cpp (one thread) and scipy; device: csrc/classical.hip",
             "", "stages: the public call with device=False / device=True",
             "%-16s %-14s %9s %10s %9s %9s %6s" % ("operator", "stage", "rows", "nnz(A)", "host", "device", "ratio")]

    def say(new):
        for line in new:
            lines.append(line)
            print(line, flush=True)
    for name, A in operators:
        say(stages(name, A, a.repeat))
    say(["", "levels: strength + splitting + interpolation; the device route's own clock: " + " ".join(classical.LEVEL_STAGES),
         "%-16s %-5s %9s %9s %9s %6s  %s" % ("operator", "split", "rows", "host", "device", "ratio",
                                             " ".join("%8s" % s[:8] for s in classical.LEVEL_STAGES))])
    for name, A in operators:
        for cf in ("PMIS", "CLJP"):
            say([levels(name, A, cf, a.repeat)])
    say(["", "setup: ruge_stuben_solver's loop (max_coarse 500), levels by the host route / by the chained entry; share of the whole",
         "%-16s %-5s %-6s %2s %9s  " % ("operator", "split", "route", "lv", "total") + " ".join("%16s" % s for s in STEPS)])
    for name, A in operators:
        for cf in ("PMIS", "CLJP"):
            say(setups(name, A, cf, a.repeat))
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
