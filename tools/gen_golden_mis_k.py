#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (development container only): the fixture of the distance-k independent set.

Stages the REFERENCE through oracle/ref_env.py, as tools/gen_golden_splitting.py does, and calls its own native
maximal_independent_set_k_parallel (amg_core/graph.h:501-589) on the designed graphs of tests/mis_cases.py, for every
(k, max_iters) pair those graphs run with.  Writes tests/golden/mis_k/cases.npz, arrays only:

  names                          the graphs, in order
  <graph>__Ap, __Aj, __y         the graph as handed to the reference (int32, int32, float64)
  <graph>__k<k>__m<max_iters>__x the reference's x (int32)
  runs                           one row (graph index, k, max_iters) per recorded x

The graph without vertices is recorded with an empty x and without a call.
Usage:  make -C oracle ref && python tools/gen_golden_mis_k.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_env  # noqa: E402
import mis_cases  # noqa: E402


def main():
    pyamg = ref_env.stage()
    core = pyamg.amg_core
    out, table = {}, []
    names = list(mis_cases.graphs())
    for gi, name in enumerate(names):
        g = mis_cases.graphs()[name]
        for a in ("Ap", "Aj", "y"):
            out["%s__%s" % (name, a)] = np.array(g[a])
        for k, m in mis_cases.runs(name):
            x = np.full(g["n"], -7, dtype=np.intc)
            if g["n"]:
                core.maximal_independent_set_k_parallel(g["n"], np.array(g["Ap"]), np.array(g["Aj"]), k, x, np.array(g["y"]), m)
            assert np.all((x == 0) | (x == 1))
            out[mis_cases.key(name, k, m)] = x
            table.append((gi, k, m))
            print("%-24s k=%d max_iters=%2d  n=%4d members=%d" % (name, k, m, g["n"], int(x.sum())))
    out["names"] = np.array(names, dtype="U40")
    out["runs"] = np.array(table, dtype=np.intc)
    os.makedirs(os.path.dirname(mis_cases.FIXTURE), exist_ok=True)
    np.savez_compressed(mis_cases.FIXTURE, **out)
    size = os.path.getsize(mis_cases.FIXTURE)
    assert size < 1000000, "%s: %d bytes" % (mis_cases.FIXTURE, size)
    print("%s: %d runs, %.0f KB" % (mis_cases.FIXTURE, len(table), size / 1024))


if __name__ == "__main__":
    main()
