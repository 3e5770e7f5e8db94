#!/usr/bin/env python3
"""Whole classical setups: ruge_stuben_solver (theta 0.25, max_levels 10, max_coarse 500) on Poisson 500 x 500 and
100^3 with PMIS and CLJP, direct and extended+i interpolation, built three ways in one process:

  host       device=False: csrc/setup_host.cpp and scipy;
  per-level  device=True with the resident chain switched off (classical._RESIDENT_CHAIN): every level uploads A_l and
             builds strength, splitting and interpolation in HBM; R = P^T and R A P run on the host (the route before
             the chain);
  chain      device=True: one upload of A_0, every level with its transpose and Galerkin product in HBM
             (amg_classical_chain_*).

Every timing is the wall clock around the whole call (every device entry ends in a synchronising copy), the median and
the range of --repeat runs after one warm-up run (fewer where --case-seconds cuts a long case short; every line says
how many), in milliseconds; the three routes alternate inside every repeat.  The
stage table sums what classical.LAST_BUILD recorded over the levels of the last run; `other` is the rest of the call
(the host transpose and product of the per-level route, the Python around the entries, the solver object).  The three
hierarchies are compared bit for bit.  The table is what profiles/r20_classical_hierarchy.txt holds.

Usage:  python tools/bench_classical_hierarchy.py [--repeat 5] [--case-seconds S] [--operator 2d|3d] [--out FILE] [--small]
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

ROUTES = ("host", "per-level", "chain")
STAGES = classical.CHAIN_STAGES


def build(A, cf, interpolation, route):
    classical._RESIDENT_CHAIN = route == "chain"
    try:
        np.random.seed(0)
        t0 = time.perf_counter()
        ml = classical.ruge_stuben_solver(A, CF=cf, max_coarse=500, device=route != "host", interpolation=interpolation)
        ms = (time.perf_counter() - t0) * 1e3
    finally:
        classical._RESIDENT_CHAIN = True
    stages = dict.fromkeys(STAGES, 0.0)
    for record in classical.LAST_BUILD["levels"]:
        for stage, t in record["times"].items():
            stages[stage] += t
    return ml, ms, stages, classical.LAST_BUILD["uploads"], list(classical.LAST_BUILD["levels"])


def same(a, b):
    if [l.A.shape for l in a.levels] != [l.A.shape for l in b.levels]:
        return False
    for x, y in zip(a.levels, b.levels):
        for key in ("A", "P", "R"):
            if hasattr(x, key) != hasattr(y, key):
                return False
            if hasattr(x, key):
                M, G = getattr(x, key), getattr(y, key)
                if M.shape != G.shape or any(np.asarray(p).tobytes() != np.asarray(q).tobytes()
                                             for p, q in ((M.indptr, G.indptr), (M.indices, G.indices), (M.data, G.data))):
                    return False
    return True


def case(name, A, cf, interpolation, repeat, say, case_seconds=0.0):
    times = {r: [] for r in ROUTES}
    last = {}
    started = time.perf_counter()
    for it in range(repeat + 1):
        if it > 1 and case_seconds and time.perf_counter() - started > case_seconds:
            break                                               # a long case: fewer repeats, said in its line
        for route in ROUTES:
            last[route] = build(A, cf, interpolation, route)
            print("[%s %s %s] run %d %-9s %9.1f ms" % (name, cf, interpolation, it, route, last[route][1]), file=sys.stderr, flush=True)
            if it:
                times[route].append(last[route][1])
    ok = same(last["host"][0], last["per-level"][0]) and same(last["host"][0], last["chain"][0])
    ml = last["chain"][0]
    say("%s, %s, %s: %d runs, levels %s, operator complexity %.2f, %s" % (
        name, cf, interpolation, len(times["chain"]), "/".join(str(l.A.shape[0]) for l in ml.levels),
        sum(l.A.nnz for l in ml.levels) / float(ml.levels[0].A.nnz), "same bits on all three routes" if ok else "DIFFERENT"))
    for route in ROUTES:
        t = np.asarray(times[route])
        _, _, stages, uploads, _ = last[route]
        whole = last[route][1]
        line = "  %-9s %9.1f [%9.1f .. %9.1f] up %2d |" % (route, np.median(t), t.min(), t.max(), uploads)
        if route != "host":
            line += " ".join("%8.1f" % stages[s] for s in STAGES) + " %8.1f" % (whole - sum(stages.values()))
        say(line)
    forms = [r["transpose"] for r in last["chain"][4]]
    say("  chain: products %s; transpose rows lane/lds/hbm %s" % (
        " ".join("%s+%s" % r["products"] for r in last["chain"][4]),
        " ".join("%d/%d/%d" % (f["lane_rows"], f["lds_rows"], f["hbm_rows"]) for f in forms)))
    return np.median(times["per-level"]) / np.median(times["chain"]), np.median(times["host"]) / np.median(times["chain"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case-seconds", type=float, default=0.0,
                    help="stop repeating a case that has taken this long (at least one timed run); 0: always --repeat runs")
    ap.add_argument("--operator", choices=("2d", "3d"), default=None, help="only Poisson 500 x 500 / only Poisson 100^3")
    ap.add_argument("--small", action="store_true", help="60 x 60 and 12^3: a rehearsal of the tool, not a measurement")
    a = ap.parse_args()
    if a.small:
        operators = (("poisson 60x60", poisson((60, 60), format="csr")), ("poisson 12^3", poisson((12, 12, 12), format="csr")))
    else:
        operators = (("poisson 500x500", poisson((500, 500), format="csr")), ("poisson 100^3", poisson((100, 100, 100), format="csr")))
    operators = tuple(o for k, o in zip(("2d", "3d"), operators) if a.operator in (None, k))
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
        if a.out:                               # rewritten line by line: a run that is cut short leaves what it had
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    say("classical setups: ruge_stuben_solver, theta = 0.25, max_coarse 500; milliseconds, median [min .. max] of up to %d runs after "
        "one warm-up, routes alternating" % a.repeat)
    say("stage columns (last run, summed over levels): " + " ".join(STAGES) + " other; up: operators uploaded by the level routes")
    ratios = []
    for name, A in operators:
        for cf in ("PMIS", "CLJP"):
            for interpolation in ("direct", "extended_i"):
                ratios.append((name, cf, interpolation) + case(name, A, cf, interpolation, a.repeat, say, a.case_seconds))
    say("")
    say("%-16s %-5s %-11s %18s %14s" % ("operator", "split", "interp", "per-level / chain", "host / chain"))
    for name, cf, interpolation, per_level, host in ratios:
        say("%-16s %-5s %-11s %18.2f %14.2f" % (name, cf, interpolation, per_level, host))


if __name__ == "__main__":
    main()
