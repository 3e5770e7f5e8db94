#!/usr/bin/env python3
"""The parallel C/F splittings: the host route against the device route (pyamg_amd/classical.py, csrc/split.hip) on the
classical strength matrices (theta = 0.25) of Poisson 500 x 500 and 100^3.

Per operator and method (PMIS, CLJP) the selection loop is timed on the same inputs by both routes -- Luby's loop on the
graph and weights split.preprocess built from seed 0, the CLJP loop on its start weights -- with the device route split
into upload, rounds (or passes) and fetch by the entry's own clock, which synchronises the device at both ends; "device"
is the wall time of the whole route, its host-side symmetry check included.  "call" is the public function as a user
calls it (remove_diagonal, transposes and weights included).  Every timing is the median of --repeat runs after one
warm-up run; the two results are compared integer for integer.  Last, the share of ruge_stuben_solver's setup time that
the splitting takes on Poisson 500 x 500 (host route).  The table is what profiles/r16_splitting.txt holds; what
device=None does (DEVICE_AUTO) is decided on it.

Usage:  python tools/bench_splitting.py [--repeat 5] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyamg_amd import classical, graph  # noqa: E402
from pyamg_amd.gallery import poisson  # noqa: E402


def median(v):
    return float(np.median(np.asarray(v)))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def row(name, method, n, nnz, host, parts, dev, count, call_h, call_d, same):
    up, loop, fetch = (median([p[k] for p in parts]) for k in range(3))
    return "%-16s %-5s %9d %10d %9.1f %8.1f %8.1f %7.1f %9.1f %6.2f %7d %10.1f %10.1f  %s" % (
        name, method, n, nnz, median(host), up, loop, fetch, median(dev), median(host) / median(dev), count, median(call_h),
        median(call_d), "same integers" if same else "DIFFERENT")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def measure_pmis(name, S, repeat):
    S0 = classical.remove_diagonal(S)
    np.random.seed(0)
    weights, G, _, _ = classical.preprocess(S0)
    G = classical.remove_diagonal(G)
    n = G.shape[0]
    Ap, Aj = np.ascontiguousarray(G.indptr, dtype=np.intc), np.ascontiguousarray(G.indices, dtype=np.intc)
    y = np.ascontiguousarray(weights, dtype=np.float64)
    L = graph._host()
    host, dev, parts, call_h, call_d = [], [], [], [], []
    same, rounds = True, 0
    for it in range(repeat + 1):
        xh, xd = np.full(n, -1, dtype=np.intc), np.full(n, -1, dtype=np.intc)
        _, th = timed(lambda: L.amgsetup_mis_parallel(n, _ip(Ap), _ip(Aj), -1, 1, 0, _ip(xh), _dp(y), -1))
        times = []
        (_, rounds), td = timed(lambda: graph._luby_device(n, Ap, Aj, -1, 1, 0, xd, y, times=times))
        np.random.seed(0)
        H, tch = timed(lambda: classical.PMIS(S, device=False))
        np.random.seed(0)
        D, tcd = timed(lambda: classical.PMIS(S, device=True))
        same = same and np.array_equal(xh, xd) and np.array_equal(H, D) and np.array_equal(H, xh)
        if it:                              # the first run warms both routes up
            host.append(th); dev.append(td); parts.append(times); call_h.append(tch); call_d.append(tcd)
    return row(name, "PMIS", n, S0.nnz, host, parts, dev, rounds, call_h, call_d, same)


def measure_cljp(name, S, repeat):
    S0 = classical.remove_diagonal(S)
    T = S0.T.tocsr()
    n = S0.shape[0]
    ic = lambda a: np.ascontiguousarray(a, dtype=np.intc)
    Sp, Sj, Tp, Tj = ic(S0.indptr), ic(S0.indices), ic(T.indptr), ic(T.indices)
    L = graph._host()
    w0 = np.empty(n)
    L.amgsetup_cljp_weights(n, _ip(Sp), _ip(Sj), 0, _dp(w0))
    host, dev, parts, call_h, call_d = [], [], [], [], []
    same, passes = True, 0
    for it in range(repeat + 1):
        sh, sd = np.empty(n, dtype=np.intc), np.empty(n, dtype=np.intc)
        wh = w0.copy()
        _, th = timed(lambda: L.amgsetup_cljp_select(n, _ip(Sp), _ip(Sj), _ip(Tp), _ip(Tj), _dp(wh), _ip(sh)))
        times = []
        passes, td = timed(lambda: classical.cljp_device(n, Sp, Sj, Tp, Tj, w0, sd, times=times))
        H, tch = timed(lambda: classical.CLJP(S, device=False))
        D, tcd = timed(lambda: classical.CLJP(S, device=True))
        same = same and np.array_equal(sh, sd) and np.array_equal(H, D) and np.array_equal(H, sh)
        if it:
            host.append(th); dev.append(td); parts.append(times); call_h.append(tch); call_d.append(tcd)
    return row(name, "CLJP", n, S0.nnz, host, parts, dev, passes, call_h, call_d, same)


def setup_share(A, cf, repeat):
    """median setup time of ruge_stuben_solver(A, CF=cf) on the host route and the part of it spent in the splitting"""
    inner = classical._PARALLEL_SPLITTINGS[cf]
    spent = [0.0]

    def clocked(S, **kw):
        out, ms = timed(lambda: inner(S, **kw))
        spent[0] += ms
        return out
    total, split = [], []
    classical._PARALLEL_SPLITTINGS[cf] = clocked
    try:
        for it in range(repeat + 1):
            spent[0] = 0.0
            np.random.seed(0)
            ml, ms = timed(lambda: classical.ruge_stuben_solver(A, CF=(cf, {"device": False})))
            if it:
                total.append(ms); split.append(spent[0])
    finally:
        classical._PARALLEL_SPLITTINGS[cf] = inner
    return "ruge_stuben_solver(poisson 500 x 500, CF=%r), host route: setup %.1f ms, of which splitting %.1f ms (%.1f %%), %d levels" % (
        cf, median(total), median(split), 100.0 * median(split) / median(total), len(ml.levels))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["C/F splittings of the classical strength matrix (theta = 0.25); milliseconds, median of %d runs after one warm-up" % a.repeat,
             "host: csrc/setup_host.cpp (one thread); device: csrc/split.hip; count: Luby rounds / CLJP passes on the device",
             "%-16s %-5s %9s %10s %9s %8s %8s %7s %9s %6s %7s %10s %10s" % (
                 "operator", "split", "rows", "nnz(S)", "host", "upload", "rounds", "fetch", "device", "ratio", "count", "call host",
                 "call dev")]
    A500 = poisson((500, 500), format="csr")
    for name, A in (("poisson 500x500", A500), ("poisson 100^3", poisson((100, 100, 100), format="csr"))):
        S = classical.classical_strength_of_connection(A, 0.25)
        for measure in (measure_pmis, measure_cljp):
            lines.append(measure(name, S, a.repeat))
            print(lines[-1], flush=True)
    for cf in ("PMIS", "CLJP"):
        lines.append(setup_share(A500, cf, a.repeat))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
