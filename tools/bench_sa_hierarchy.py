#!/usr/bin/env python3
"""Whole smoothed-aggregation setups with MIS(2) aggregation: smoothed_aggregation_solver(A, aggregate='mis') with its
defaults (symmetric strength, one Jacobi step, max_coarse 500, candidate improvement on level 0) on Poisson 500 x 500
and 100^3, built four ways in one process:

  host-generic  device=False, fast=False: numpy, scipy and csrc/setup_host.cpp, every level with keep's extras;
  host          device=False: the default of the host route;
  per-stage     device=True with the resident chain switched off (aggregation._RESIDENT_CHAIN): every stage uploads its
                operands and fetches its result; R = P^T and R A P run on the host (the route before the chain);
  chain         device=True: one upload of A_0 and B_0, every level with its transpose and Galerkin product in HBM
                (amg_sa_chain_*).

Every timing is the wall clock around the whole call (every device entry ends in a synchronising copy), the median and
the range of --repeat runs after one warm-up run (fewer where --case-seconds cuts a long case short; every line says
how many), in milliseconds; the four routes alternate inside every repeat.  The stage table sums what
aggregation.LAST_BUILD recorded over the chained levels of the last run; `other` is the rest of the call: candidate
improvement, the draws, the diagonal and the spectral radius on the host, the Python around the entries, the solver
object.  The hierarchies are compared bit for bit in every run.  The table is what profiles/r24_sa_chain.txt holds.

Usage:  python tools/bench_sa_hierarchy.py [--repeat 5] [--case-seconds S] [--operator 2d|3d] [--out FILE] [--small]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyamg_amd import aggregation  # noqa: E402
from pyamg_amd.gallery import poisson  # noqa: E402

ROUTES = {"host-generic": {"device": False, "fast": False}, "host": {"device": False}, "per-stage": {"device": True},
          "chain": {"device": True}}
STAGES = aggregation.CHAIN_STAGES


def build(A, route):
    aggregation._RESIDENT_CHAIN = route == "chain"
    try:
        np.random.seed(0)
        t0 = time.perf_counter()
        ml = aggregation.smoothed_aggregation_solver(A, aggregate="mis", **ROUTES[route])
        ms = (time.perf_counter() - t0) * 1e3
    finally:
        aggregation._RESIDENT_CHAIN = True
    stages = dict.fromkeys(STAGES, 0.0)
    for record in aggregation.LAST_BUILD["levels"]:
        for stage, t in record["times"].items():
            stages[stage] += t
    return ml, ms, stages, aggregation.LAST_BUILD["uploads"], list(aggregation.LAST_BUILD["levels"]), np.random.get_state()[1].tobytes()


def same(a, b):
    if [l.A.shape for l in a.levels] != [l.A.shape for l in b.levels]:
        return False
    for x, y in zip(a.levels, b.levels):
        if np.asarray(x.B).tobytes() != np.asarray(y.B).tobytes():
            return False
        for key in ("A", "P", "R"):
            if hasattr(x, key) != hasattr(y, key):
                return False
            if hasattr(x, key):
                M, G = getattr(x, key), getattr(y, key)
                if M.format != G.format or M.shape != G.shape or any(
                        np.asarray(p).dtype != np.asarray(q).dtype or np.asarray(p).tobytes() != np.asarray(q).tobytes()
                        for p, q in ((M.indptr, G.indptr), (M.indices, G.indices), (M.data, G.data))):
                    return False
    return True


def case(name, A, repeat, say, case_seconds=0.0):
    times = {r: [] for r in ROUTES}
    last = {}
    ok = True
    started = time.perf_counter()
    for it in range(repeat + 1):
        if it > 1 and case_seconds and time.perf_counter() - started > case_seconds:
            break                                               # a long case: fewer repeats, said in its line
        for route in ROUTES:
            last[route] = build(A.copy(), route)
            print("[%s] run %d %-12s %9.1f ms" % (name, it, route, last[route][1]), file=sys.stderr, flush=True)
            if it:
                times[route].append(last[route][1])
        ok = ok and all(same(last["host-generic"][0], last[r][0]) and last["host-generic"][5] == last[r][5] for r in ROUTES)
    ml = last["chain"][0]
    say("%s: %d runs, levels %s, operator complexity %.2f, %s" % (
        name, len(times["chain"]), "/".join(str(l.A.shape[0]) for l in ml.levels),
        sum(l.A.nnz for l in ml.levels) / float(ml.levels[0].A.nnz),
        "same bits and the same RNG position on all four routes in every run" if ok else "DIFFERENT"))
    for route in ROUTES:
        t = np.asarray(times[route])
        _, whole, stages, uploads, _, _ = last[route]
        line = "  %-12s %9.1f [%9.1f .. %9.1f] up %2d |" % (route, np.median(t), t.min(), t.max(), uploads)
        if route == "chain":
            line += " ".join("%8.1f" % stages[s] for s in STAGES) + " %8.1f" % (whole - sum(stages.values()))
        say(line)
    records = last["chain"][4]
    say("  chain: chained levels %d of %d; strength modes %s; products %s; transpose rows lane/lds/hbm %s" % (
        sum(1 for r in records if r["chained"]), len(records), " ".join(str(r["strength_mode"]) for r in records),
        " ".join("%s+%s" % r["products"] for r in records if r["products"]),
        " ".join("%d/%d/%d" % (r["transpose"]["lane_rows"], r["transpose"]["lds_rows"], r["transpose"]["hbm_rows"])
                 for r in records if r["transpose"])))
    med = {r: np.median(times[r]) for r in ROUTES}
    return med["per-stage"] / med["chain"], med["host"] / med["chain"], med["host-generic"] / med["chain"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case-seconds", type=float, default=0.0,
                    help="stop repeating a case that has taken this long (at least one timed run); 0: always --repeat runs")
    ap.add_argument("--operator", choices=("2d", "3d"), default=None, help="only Poisson 500 x 500 / only Poisson 100^3")
    ap.add_argument("--small", action="store_true", help="60 x 60 and 12^3 with max_coarse 20: a rehearsal of the tool, not a measurement")
    a = ap.parse_args()
    if a.small:
        operators = (("poisson 60x60", poisson((60, 60), format="csr")), ("poisson 12^3", poisson((12, 12, 12), format="csr")))
        for opts in ROUTES.values():
            opts["max_coarse"] = 20
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
    say("smoothed-aggregation setups: smoothed_aggregation_solver(aggregate='mis'), defaults; milliseconds, median [min .. max] of up "
        "to %d runs after one warm-up, routes alternating" % a.repeat)
    say("stage columns of the chain (last run, summed over levels): " + " ".join(STAGES) + " other; up: operators uploaded by the chain")
    ratios = []
    for name, A in operators:
        ratios.append((name,) + case(name, A, a.repeat, say, a.case_seconds))
    say("")
    say("%-16s %18s %14s %22s" % ("operator", "per-stage / chain", "host / chain", "host-generic / chain"))
    for name, per_stage, host, generic in ratios:
        say("%-16s %18.2f %14.2f %22.2f" % (name, per_stage, host, generic))


if __name__ == "__main__":
    main()
