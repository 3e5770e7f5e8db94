#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (development container only): the fixtures of the parallel C/F splittings.

Runs the REFERENCE -- its Python staged by oracle/ref_env.py on its own native module oracle/_ref/_amg_core.so, as
tools/gen_golden_evolution.py does -- and records, under tests/golden/splitting/ (a directory of its own:
golden_io._all_cases() lists the hier_*.npz files of tests/golden/ itself):

  <problem>.npz     the strength matrix S, the graph G = pattern of S + S^T (diagonal removed), and with
                    np.random.seed(0) before each call: PMIS, PMISc ('JP', 'MIS', 'LDF'), CLJP, CLJPc, MIS(G, ones),
                    vertex_coloring(G) by the three methods and maximal_independent_set(G) by both algorithms -- each
                    result, plus the arguments, results and return value of every call it made into the native module
                    (pyamg.classical.split.amg_core and pyamg.graph.amg_core wrapped by a Recorder)
  hier_rs_pmis_2d.npz, hier_rs_cljp_2d.npz
                    ruge_stuben_solver(poisson 40 x 40, CF=..., max_coarse=20) and its solve in the hier_*.npz layout of
                    oracle/gen_golden.py
  reference_summary.json
                    level sizes, operator complexity and iterations of the reference for CF = 'RS', 'PMIS', 'CLJP' on
                    Poisson 40 x 40 (the table of README.md)

Problems (built here from seeds): classical strength (theta = 0.25) of Poisson 17 x 23 and 40 x 40 and of the rotated
anisotropic 9-point operator 40 x 40 of the evolution fixtures (a denser S, which turns out symmetric at this theta),
and one random structurally unsymmetric S of 400 rows with an empty row, a row of about 300 entries and vertices nobody
depends on.

Every fixture must exercise the tie rule: the generator asserts that some recorded MIS call of each problem has two
adjacent vertices of equal weight (MIS(G, ones), the reference's own docstring example, makes every edge a tie).
Usage:  make -C oracle ref && python tools/gen_golden_splitting.py
"""
import json
import os
import sys

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_env  # noqa: E402
import gen_golden  # noqa: E402
import gen_golden_evolution as gge  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "splitting")

# arguments of the native entries in call order, and which of them hold results afterwards
ARGS = {"maximal_independent_set_serial": ("num_rows", "Ap", "Aj", "active", "C", "F", "x"),
        "maximal_independent_set_parallel": ("num_rows", "Ap", "Aj", "active", "C", "F", "x", "y", "max_iters"),
        "vertex_coloring_mis": ("num_rows", "Ap", "Aj", "x"),
        "vertex_coloring_jones_plassmann": ("num_rows", "Ap", "Aj", "x", "z"),
        "vertex_coloring_LDF": ("num_rows", "Ap", "Aj", "x", "y"),
        "cljp_naive_splitting": ("n", "Sp", "Sj", "Tp", "Tj", "splitting", "colorflag")}
OUTPUTS = {"maximal_independent_set_serial": ("x",), "maximal_independent_set_parallel": ("x",),
           "vertex_coloring_mis": ("x",), "vertex_coloring_jones_plassmann": ("x", "z"), "vertex_coloring_LDF": ("x",),
           "cljp_naive_splitting": ("splitting",)}
# arguments that arrive uninitialised (np.empty): only their result is kept
PURE_OUTPUT = {"vertex_coloring_mis": ("x",), "vertex_coloring_jones_plassmann": ("x",), "vertex_coloring_LDF": ("x",),
               "cljp_naive_splitting": ("splitting",)}


class Recorder(gge.Recorder):
    """the evolution tool's Recorder for the graph entries, which also keeps what a call returns"""
    NAMES = tuple(ARGS)

    def __init__(self, core):
        gge.Recorder.__init__(self, core, keep=self.NAMES)

    def __getattr__(self, name):
        fn = getattr(self._core, name)
        if name not in self.NAMES:
            return fn

        def wrapped(*args):
            before = [np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in args]
            ret = fn(*args)
            after = [np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in args]
            self.calls.append((name, before, after, ret))
            return ret
        return wrapped


def put_calls(out, tag, calls):
    names = []
    for ci, (name, before, after, ret) in enumerate(calls):
        pre = "%s__c%d__" % (tag, ci)
        for arg, v in zip(ARGS[name], before):
            if arg not in PURE_OUTPUT.get(name, ()):
                out[pre + arg] = np.asarray(v)
        for arg in OUTPUTS[name]:
            out[pre + arg + "_out"] = np.asarray(after[ARGS[name].index(arg)])
        out[pre + "ret"] = np.array(-1 if ret is None else ret)
        names.append(name)
    out[tag + "__calls"] = np.array(names, dtype="U40")


def recorded(modules, fn):
    """fn() with np.random.seed(0) and the native module of every listed reference module wrapped"""
    core = modules[0].amg_core
    rec = Recorder(core)
    for m in modules:
        m.amg_core = rec
    try:
        np.random.seed(0)
        result = fn()
    finally:
        for m in modules:
            m.amg_core = core
    return np.asarray(result), rec.calls


def random_unsymmetric(seed=11, n=400):
    """a strength pattern that is not symmetric: row 19 empty, row 23 with about 300 entries, columns 5, 77, 123 and 300
    empty (nobody depends on those vertices), a few diagonal entries for remove_diagonal to take out"""
    rng = np.random.RandomState(seed)
    M = sps.random(n, n, density=0.012, random_state=rng, format="lil", data_rvs=lambda s: rng.uniform(0.1, 1.0, s))
    M[23, rng.choice(n, 300, replace=False)] = 0.5
    for i in range(0, n, 7):
        M[i, i] = 1.0
    M[19, :] = 0.0
    for c in (5, 77, 123, 300):
        M[:, c] = 0.0
    S = sps.csr_matrix(M)
    S.eliminate_zeros()
    S.sort_indices()
    S.indices = S.indices.astype(np.intc)
    S.indptr = S.indptr.astype(np.intc)
    counts = np.diff(S.indptr)
    indeg = np.bincount(S.indices, minlength=n)
    assert counts[19] == 0 and counts[23] >= 290 and all(indeg[c] == 0 for c in (5, 77, 123, 300))
    assert (abs(S - S.T) > 0).nnz > 0
    return S


def graph_of(pyamg, S):
    """G as split.preprocess builds it from S without its diagonal"""
    S0 = pyamg.util.utils.remove_diagonal(S)
    S1 = sps.csr_matrix((np.ones(S0.nnz, dtype="int8"), S0.indices, S0.indptr), shape=S0.shape)
    G = S1 + S1.T.tocsr()
    G.data[:] = 1
    G = sps.csr_matrix(G)
    G.sort_indices()
    return G


def has_tie(calls):
    for name, before, after, ret in calls:
        if name != "maximal_independent_set_parallel":
            continue
        n, Ap, Aj, y = before[0], before[1], before[2], before[7]
        rows = np.repeat(np.arange(n), np.diff(Ap))
        if np.any((rows != Aj) & (y[rows] == y[Aj])):
            return True
    return False


def gen_problem(pyamg, name, S):
    import pyamg.classical.split as split
    import pyamg.graph as graph
    S = sps.csr_matrix(S)
    G = graph_of(pyamg, S)
    n = S.shape[0]
    out = {"S_indptr": S.indptr.astype(np.intc), "S_indices": S.indices.astype(np.intc), "S_data": S.data.astype(np.float64),
           "G_indptr": G.indptr.astype(np.intc), "G_indices": G.indices.astype(np.intc), "n": np.array(n)}
    both = (split, graph)
    runs = [("PMIS", lambda: split.PMIS(S.copy())),
            ("PMISc_JP", lambda: split.PMISc(S.copy(), method="JP")),
            ("PMISc_MIS", lambda: split.PMISc(S.copy(), method="MIS")),
            ("PMISc_LDF", lambda: split.PMISc(S.copy(), method="LDF")),
            ("CLJP", lambda: split.CLJP(S.copy())),
            ("CLJPc", lambda: split.CLJPc(S.copy())),
            ("MIS_ones", lambda: split.MIS(G.astype(np.float64), np.ones((n, 1)).ravel())),
            ("color_MIS", lambda: graph.vertex_coloring(G, "MIS")),
            ("color_JP", lambda: graph.vertex_coloring(G, "JP")),
            ("color_LDF", lambda: graph.vertex_coloring(G, "LDF")),
            ("mis_serial", lambda: graph.maximal_independent_set(G, "serial")),
            ("mis_parallel", lambda: graph.maximal_independent_set(G, "parallel"))]
    tie = False
    report = []
    for tag, fn in runs:
        result, calls = recorded(both, fn)
        out[tag] = result.astype(np.intc)
        put_calls(out, tag, calls)
        tie = tie or has_tie(calls)
        report.append("%s=%d(%d calls)" % (tag, int(result.max()) if tag.startswith("color") else int(result.sum()), len(calls)))
    assert tie, "%s: no recorded MIS call has two adjacent vertices of equal weight" % name
    out["tags"] = np.array([t for t, _ in runs], dtype="U20")
    path = os.path.join(OUT, "%s.npz" % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1000000, "%s: %d bytes" % (path, size)
    print("%-16s n=%d nnz(S)=%d symmetric=%s %5.0f KB  %s" % (name, n, S.nnz, (abs(S - S.T) > 0).nnz == 0, size / 1024,
                                                              " ".join(report)))


def gen_summary(pyamg, A):
    out = {}
    for cf in ("RS", "PMIS", "CLJP"):
        np.random.seed(0)
        ml = pyamg.ruge_stuben_solver(A, CF=cf, max_coarse=20)
        b = np.random.rand(A.shape[0])
        res = []
        ml.solve(b, tol=1e-8, residuals=res)
        out[cf] = {"levels": [int(l.A.shape[0]) for l in ml.levels], "operator_complexity": float(ml.operator_complexity()),
                   "iterations": len(res) - 1}
        print("summary %-5s %r" % (cf, out[cf]))
    with open(os.path.join(OUT, "reference_summary.json"), "w") as f:
        json.dump({"problem": "poisson 40x40, ruge_stuben_solver(max_coarse=20), V-cycles to 1e-8, seed 0", "CF": out}, f, indent=1,
                  sort_keys=True)
        f.write("\n")


def main():
    os.makedirs(OUT, exist_ok=True)
    pyamg = ref_env.stage()
    from pyamg.strength import classical_strength_of_connection as css
    gen_problem(pyamg, "poisson_17x23", css(ref_env.poisson((17, 23)), 0.25))
    gen_problem(pyamg, "poisson_40x40", css(ref_env.poisson((40, 40)), 0.25))
    gen_problem(pyamg, "aniso_40x40", css(gge.anisotropic(pyamg, 40, 40, 0.01, np.pi / 6), 0.25))
    gen_problem(pyamg, "unsym_400", random_unsymmetric())
    gen_golden.OUT = OUT
    gs = ("gauss_seidel", {"sweep": "symmetric"})
    A = ref_env.poisson((40, 40))
    for cf in ("PMIS", "CLJP"):
        gen_golden.gen_hier(pyamg, "rs_%s_2d" % cf.lower(), A,
                            lambda A, cf=cf, **kw: pyamg.ruge_stuben_solver(A, CF=cf, max_coarse=20, **kw), gs, gs, dict(tol=1e-8))
    gen_summary(pyamg, A)


if __name__ == "__main__":
    main()
