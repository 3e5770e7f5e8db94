#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (development container only): the complex128 hierarchy fixtures.

Runs the REFERENCE -- its Python staged by oracle/ref_env.py on its own native module oracle/_ref/_amg_core.so,
as oracle/gen_golden.py does -- on complex128 problems built from seeds, and records each hierarchy and solve in
the hier_*.npz layout (levels A/P/R, smoother constants, coarse operator, b, x0, x, residuals, x_iter1, x_iter2)
plus Mb, one aspreconditioner() matvec of b:

  tests/golden/hier_c128/<case>.npz

(a directory of its own: golden_io.hier_cases() lists the float64 hier_*.npz files of tests/golden/).
Except in the relaxation-coarse case the coarse solver is a callable that applies pinv(A_coarse) with sequential
row sums from zero, each complex product spelled out in separate real ufunc calls (numpy's complex array product
is FMA-contracted on AVX-512 hosts); the fixture stores that matrix as coarse_pinv.
Usage:  make -C oracle ref && python tools/gen_golden_hier_c128.py
"""
import json
import os
import sys

import numpy as np
import scipy.linalg
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_env  # noqa: E402
from gen_golden import closure_vars, put_mat, smoother_desc  # noqa: E402
from c128_cycle import dense_apply  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "hier_c128")


# --------------------------------------------------------------------------- problems (from seeds)
def shifted_laplacian(n, sigma):
    """2-D Laplacian + i sigma I: complex symmetric"""
    L = ref_env.poisson((n, n))
    return sps.csr_matrix(L + 1j * sigma * sps.identity(L.shape[0]), dtype=np.complex128)


def magnetic_laplacian(grid, shift, seed):
    """graph Laplacian of the grid with unit-modulus edge phases e^{i theta_e} plus shift I: Hermitian positive
    definite; rows sorted"""
    rng = np.random.RandomState(seed)
    L = ref_env.poisson(grid).tocoo()
    off = L.row < L.col
    r, c = L.row[off], L.col[off]
    ph = np.exp(1j * rng.uniform(-np.pi, np.pi, size=r.size))
    n = L.shape[0]
    W = sps.coo_matrix((np.concatenate([ph, ph.conj()]), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n))
    deg = np.asarray(abs(W).sum(axis=1)).ravel()
    A = sps.diags(deg + shift) - W
    A = sps.csr_matrix(A, dtype=np.complex128)
    A.sort_indices()
    return A


def with_decoupled_rows(A, rows, d=2.0):
    """A with the given unknowns cut off from the rest (their rows and columns cleared, diagonal d): the aggregation
    leaves them out, so P has empty rows there and x_i is set by the smoothers alone"""
    A = sps.lil_matrix(A)
    for i in rows:
        A[i, :] = 0
        A[:, i] = 0
        A[i, i] = d
    A = sps.csr_matrix(A, dtype=np.complex128)
    A.eliminate_zeros()
    A.sort_indices()
    return A


def block_system(n, sigma):
    """2x2-block BSR: kron(2-D Laplacian, [[2, 1], [1, 2]]) + i sigma I"""
    L = ref_env.poisson((n, n))
    A = sps.kron(L, np.array([[2.0, 1.0], [1.0, 2.0]])) + 1j * sigma * sps.identity(2 * L.shape[0])
    return sps.bsr_matrix(A, blocksize=(2, 2), dtype=np.complex128)


class PinvCoarse(object):
    """coarse solver callable: pinv(A_coarse) applied in sequential order (c128_cycle.dense_apply)"""
    def __init__(self):
        self.M = None

    def __call__(self, A, b):
        if self.M is None:
            self.M = np.ascontiguousarray(scipy.linalg.pinv(A.toarray()), dtype=np.complex128)
        return dense_apply(self.M, np.ravel(b))


def record_desc(out, key, spec, fn, lvl):
    d = smoother_desc(out, key, spec, fn, lvl)
    cv = closure_vars(fn)
    if d.get("has_Dinv"):
        out[key + "_Dinv"] = np.ravel(np.asarray(cv["Dinv"])).astype(np.complex128)      # complex block inverses
    return d


def gen(pyamg, name, A, pre, post, cycle="V", tol=1e-8, maxiter=40, x0_random=False, seed=0, coarse="pinv",
        build_kw=None, negzero=False, negzero_rows=None):
    np.random.seed(seed)
    pc = PinvCoarse()
    kw = dict(max_coarse=30, presmoother=pre, postsmoother=post,
              coarse_solver=pc if coarse == "pinv" else coarse)
    kw.update(build_kw or {})
    ml = pyamg.smoothed_aggregation_solver(A, **kw)
    n = A.shape[0]
    rng = np.random.RandomState(seed + 1)
    b = rng.rand(n) + 1j * rng.rand(n) - (0.5 + 0.5j)
    if negzero:
        b.real[::3] = -0.0
        b.imag[::5] = -0.0
    if negzero_rows is not None:
        # b_i = (-0, -v) on decoupled rows: Gauss-Seidel sets x_i = (-0, -v/2), and SOR's blend x w + x_old (1 - w)
        # (w > 1) gives +0 in the real part under numpy's promoted product, -0 under component-wise scaling
        b[negzero_rows] = -0.0 - 1j * (0.5 + rng.rand(len(negzero_rows)))
        b.real[negzero_rows] = -0.0
    x0 = (rng.rand(n) + 1j * rng.rand(n)) if x0_random else None
    for _ in range(20):
        its, res = [], []
        x = ml.solve(b, x0=x0, tol=tol, maxiter=maxiter, cycle=cycle, residuals=res,
                     callback=lambda xk: its.append(np.array(xk, copy=True)))
        # no stop decision within 1e-6 relative of tol * ||b||
        thr = tol * np.linalg.norm(b)
        if np.all(np.abs(np.array(res) - thr) > 1e-6 * thr):
            break
        tol *= 1.37
    else:
        raise RuntimeError("%s: no tolerance clear of the residual history" % name)
    Mb = ml.aspreconditioner(cycle=cycle) * b
    out = {}
    meta = {"name": name, "nlevels": len(ml.levels), "cycle": cycle, "tol": tol, "maxiter": maxiter,
            "coarse": "dense" if coarse == "pinv" else list(coarse), "levels": []}
    pre_l = pre if isinstance(pre, list) else [pre]
    post_l = post if isinstance(post, list) else [post]
    for i, lvl in enumerate(ml.levels):
        put_mat(out, "A%d" % i, lvl.A)
        if i < len(ml.levels) - 1:
            put_mat(out, "P%d" % i, lvl.P)
            put_mat(out, "R%d" % i, lvl.R)
            meta["levels"].append({
                "pre": record_desc(out, "pre%d" % i, pre_l[min(i, len(pre_l) - 1)], lvl.presmoother, lvl),
                "post": record_desc(out, "post%d" % i, post_l[min(i, len(post_l) - 1)], lvl.postsmoother, lvl)})
    if coarse == "pinv":
        if pc.M is None:
            pc(ml.levels[-1].A, np.zeros(ml.levels[-1].A.shape[0], dtype=np.complex128))
        out["coarse_pinv"] = pc.M
    else:
        out["coarse_pinv"] = np.zeros((0, 0), dtype=np.complex128)
    out["b"] = b
    out["x0"] = np.zeros(n, dtype=np.complex128) if x0 is None else x0
    out["x"] = np.asarray(x)
    out["residuals"] = np.array(res)
    its = its or [np.asarray(x)]
    out["x_iter1"] = its[0]
    out["x_iter2"] = its[1] if len(its) > 1 else its[0]
    out["Mb"] = np.asarray(Mb)
    for k in ("b", "x0", "x", "x_iter1", "x_iter2", "Mb"):
        assert out[k].dtype == np.complex128, (name, k, out[k].dtype)
    out["meta_json"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, "%s.npz" % name)
    np.savez_compressed(path, **out)
    print("%-24s levels=%d iters=%d  r0=%.3e  rN=%.3e  %6.0f KB" %
          (name, len(ml.levels), len(res) - 1, res[0], res[-1], os.path.getsize(path) / 1024))


def main():
    os.makedirs(OUT, exist_ok=True)
    pyamg = ref_env.stage()
    sym = dict(symmetry="symmetric")
    herm = dict(symmetry="hermitian")
    gs = ("gauss_seidel", {"sweep": "symmetric"})
    As = shifted_laplacian(32, 0.5)
    Am = magnetic_laplacian((32, 32), 0.05, seed=7)
    gen(pyamg, "gs_sym_V_shifted2d", As, gs, gs, "V", build_kw=sym)
    gen(pyamg, "sor_W_shifted2d", As, ("sor", {"omega": 1.2, "sweep": "symmetric"}),
        ("sor", {"omega": 1.2, "sweep": "symmetric"}), "W", build_kw=sym, seed=1)
    gen(pyamg, "jacobi_F_x0_magnetic2d", Am, ("jacobi", {"omega": 4.0 / 3.0, "iterations": 2}),
        ("jacobi", {"omega": 4.0 / 3.0, "iterations": 2}), "F", x0_random=True, build_kw=herm, seed=2)
    gen(pyamg, "sa_default_magnetic2d", Am, ("block_gauss_seidel", {"sweep": "symmetric"}),
        ("block_gauss_seidel", {"sweep": "symmetric"}), "V", build_kw=herm, seed=3)
    gen(pyamg, "cheb2_magnetic3d", magnetic_laplacian((12, 12, 12), 0.05, seed=11), ("chebyshev", {"degree": 2}),
        ("chebyshev", {"degree": 2}), "V", build_kw=herm, seed=4)
    gen(pyamg, "bsr_bjac_gs", block_system(16, 2.0), ("block_jacobi", {"omega": 0.7}), gs, "V",
        build_kw=sym, seed=5)
    gen(pyamg, "coarse_gs10", As, gs, gs, "V", coarse=("gauss_seidel", {"iterations": 10}), build_kw=sym, seed=6)
    gen(pyamg, "one_level", shifted_laplacian(8, 0.5), gs, gs, "V", build_kw=dict(sym, max_levels=1), seed=8)
    dec = np.arange(37, 1024, 97)
    gen(pyamg, "sor_negzero", with_decoupled_rows(As, dec), ("sor", {"omega": 1.2}), ("sor", {"omega": 1.2}), "V",
        build_kw=sym, seed=10, negzero_rows=dec)
    gen(pyamg, "poly_negzero", Am, ("richardson", {"omega": 0.9}), ("chebyshev", {"degree": 3}), "V",
        build_kw=herm, seed=9, negzero=True)


if __name__ == "__main__":
    main()
