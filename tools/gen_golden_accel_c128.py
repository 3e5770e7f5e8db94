#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (development container only): Krylov-accelerated solves on the complex128 hierarchy fixtures.

Rebuilds, with the seeds of tools/gen_golden_hier_c128.py, the reference hierarchies whose levels are stored in
tests/golden/hier_c128/<case>.npz -- every level's A must equal the stored one bit for bit, and one
aspreconditioner() matvec the stored Mb, so a test can build the device hierarchy from that fixture -- and runs the
REFERENCE's ml.solve(b, x0, tol, maxiter, cycle, accel=<method>, residuals=...) on each.  Recorded per solve:

  tests/golden/accel_c128/<case>__<method>.npz    case, b, x0, x, residuals (real parts, float64), meta_json
                                                  (method, cycle, tol, maxiter, restrt, iterations)

Arrays and JSON only.  The coarse solver is the stored coarse_pinv applied with sequential row sums, as in the
hierarchy fixtures.  tol is stepped (x 1.37) until no history entry lies within 1e-6 relative of tol * residuals[0],
the quantity every method's stopping test compares with; a case other than one_level that takes fewer than 3
iterations fails the run.
Usage:  make -C oracle ref && python tools/gen_golden_accel_c128.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_env  # noqa: E402
import c128_cycle  # noqa: E402
from gen_golden_hier_c128 import (PinvCoarse, block_system, magnetic_laplacian,  # noqa: E402
                                  shifted_laplacian)

OUT = os.path.join(ROOT, "tests", "golden", "accel_c128")

GS = ("gauss_seidel", {"sweep": "symmetric"})
SYM, HERM = dict(symmetry="symmetric"), dict(symmetry="hermitian")


def hierarchies():
    """case -> (A, pre, post, build_kw, seed), as main() of gen_golden_hier_c128.py builds them"""
    As = shifted_laplacian(32, 0.5)
    Am = magnetic_laplacian((32, 32), 0.05, seed=7)
    sor = ("sor", {"omega": 1.2, "sweep": "symmetric"})
    jac = ("jacobi", {"omega": 4.0 / 3.0, "iterations": 2})
    bgs = ("block_gauss_seidel", {"sweep": "symmetric"})
    cheb = ("chebyshev", {"degree": 2})
    return {
        "gs_sym_V_shifted2d": (As, GS, GS, SYM, 0),
        "sor_W_shifted2d": (As, sor, sor, SYM, 1),
        "jacobi_F_x0_magnetic2d": (Am, jac, jac, HERM, 2),
        "sa_default_magnetic2d": (Am, bgs, bgs, HERM, 3),
        "cheb2_magnetic3d": (magnetic_laplacian((12, 12, 12), 0.05, seed=11), cheb, cheb, HERM, 4),
        "bsr_bjac_gs": (block_system(16, 2.0), ("block_jacobi", {"omega": 0.7}), GS, SYM, 5),
        "one_level": (shifted_laplacian(8, 0.5), GS, GS, dict(SYM, max_levels=1), 8),
    }


# (case, cycle, random x0, [(method, restrt, maxiter)])
SOLVES = [
    ("cheb2_magnetic3d", "V", False, [("cg", None, 40), ("bicgstab", None, 40), ("gmres", None, 40), ("fgmres", None, 40)]),
    ("sa_default_magnetic2d", "V", True, [("cg", None, 40), ("gmres", None, 40)]),
    ("gs_sym_V_shifted2d", "V", False, [("bicgstab", None, 40), ("fgmres", None, 40), ("gmres", 3, 4)]),
    ("sor_W_shifted2d", "W", False, [("fgmres", None, 40)]),
    ("jacobi_F_x0_magnetic2d", "F", True, [("gmres", None, 40), ("bicgstab", None, 40)]),
    ("bsr_bjac_gs", "V", False, [("bicgstab", None, 40), ("gmres", None, 40)]),
    ("one_level", "V", False, [("gmres", None, 40)]),
]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rebuild(pyamg, case, spec, cycle):
    """the reference hierarchy of a stored fixture, checked against it"""
    A, pre, post, build_kw, seed = spec
    g = c128_cycle.load(case)
    np.random.seed(seed)
    pc = PinvCoarse()
    pc.M = np.ascontiguousarray(g["coarse"][1]["M"], dtype=np.complex128)      # the stored operator, not a new pinv
    kw = dict(max_coarse=30, presmoother=pre, postsmoother=post, coarse_solver=pc)
    kw.update(build_kw)
    ml = pyamg.smoothed_aggregation_solver(A, **kw)
    assert len(ml.levels) == len(g["levels"]), case
    for lvl, L in zip(ml.levels, g["levels"]):
        for M, S in ((lvl.A, L["A"]),) + (((lvl.P, L["P"]), (lvl.R, L["R"])) if "P" in L else ()):
            M = M.asformat(S.format)
            assert M.shape == S.shape and same_bits(M.indptr, S.indptr.astype(M.indptr.dtype)), case
            assert same_bits(M.indices, S.indices.astype(M.indices.dtype)), case
            assert same_bits(np.ravel(M.data).astype(np.complex128), np.ravel(S.data)), "%s: operator differs from the fixture" % case
    if cycle == g["meta"]["cycle"]:
        assert same_bits(np.asarray(ml.aspreconditioner(cycle=cycle) * g["b"]), g["Mb"]), "%s: cycle differs from the fixture" % case
    return ml, g


def solve(pyamg, ml, b, x0, cycle, method, restrt, maxiter, tol):
    res = []
    if restrt is None:
        x = ml.solve(b, x0=x0, tol=tol, maxiter=maxiter, cycle=cycle, accel=method, residuals=res)
    else:       # ml.solve has no restrt: the call it would make (multilevel.py:398-403), with restrt
        x = getattr(pyamg.krylov, method)(ml.levels[0].A, b, x0=x0, tol=tol, restrt=restrt, maxiter=maxiter,
                                          M=ml.aspreconditioner(cycle=cycle), residuals=res)[0]
    res = np.array([complex(r).real for r in res], dtype=np.float64)
    return np.asarray(x, dtype=np.complex128).ravel(), res


def main():
    os.makedirs(OUT, exist_ok=True)
    pyamg = ref_env.stage()
    specs = hierarchies()
    for case, cycle, x0_random, runs in SOLVES:
        ml, g = rebuild(pyamg, case, specs[case], cycle)
        n = ml.levels[0].A.shape[0]
        b = np.array(g["b"])
        rng = np.random.RandomState(1000 + specs[case][4])
        x0 = (rng.rand(n) + 1j * rng.rand(n)) if x0_random else None
        for method, restrt, maxiter in runs:
            tol = 1e-8
            for _ in range(20):
                x, res = solve(pyamg, ml, b, x0, cycle, method, restrt, maxiter, tol)
                thr = tol * res[0]
                if np.all(np.abs(res - thr) > 1e-6 * thr):
                    break
                tol *= 1.37
            else:
                raise RuntimeError("%s %s: no tolerance clear of the residual history" % (case, method))
            its = len(res) - 1
            if its < 3 and case != "one_level":
                raise RuntimeError("%s %s: only %d iterations" % (case, method, its))
            meta = {"case": case, "method": method, "cycle": cycle, "tol": tol, "maxiter": maxiter, "restrt": restrt,
                    "iterations": its}
            out = {"case": np.array(case), "b": b, "x0": np.zeros(n, dtype=np.complex128) if x0 is None else x0,
                   "x": x, "residuals": res, "meta_json": np.array(json.dumps(meta))}
            path = os.path.join(OUT, "%s__%s.npz" % (case, method))
            np.savez_compressed(path, **out)
            print("%-24s %-9s iters=%2d  tol=%.3e  r0=%.3e  rN=%.3e  %5.0f KB" %
                  (case, method, its, tol, res[0], res[-1], os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
