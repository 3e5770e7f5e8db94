#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (development container only): the evolution strength-of-connection fixtures.

Runs the REFERENCE -- its Python staged by oracle/ref_env.py on its own native module oracle/_ref/_amg_core.so, as
oracle/gen_golden.py does -- and records, under tests/golden/evolution/ (a directory of its own:
golden_io._all_cases() lists the hier_*.npz files of tests/golden/ itself):

  <problem>.npz        A (CSR arrays), the candidate B, and for k = 1, 2, 4: rho (the reference's estimate of the
                       spectral radius of Dinv A, seed 0), the returned C, and the arguments and results of every call
                       evolution_strength_of_connection made into its native module (pyamg.strength.amg_core wrapped)
  flat_kernels.npz     direct calls of min_blocks and apply_absolute_distance_filter, which the measure itself never
                       reaches with blocks larger than one entry
  hier_sa_evolution_2d.npz   one SA hierarchy and its solve in the hier_*.npz layout of oracle/gen_golden.py
  large_digests.npz    the two problems of working size built by tests/evolution_io.py (large_grid, large_unsym; the same
                       builders the tests call), k = 1, 2, 4: rho, nnz of C, SHA-256 of C's three arrays, of A's three
                       arrays and of B, rows 0-31 and the last 32 rows of C verbatim.  Results of this size do not fit a
                       committed file; only the distance filter's input is kept while recording, for the check below.

Problems (built here from seeds): rotated anisotropic diffusion, Q1 finite elements on an nx x ny grid (9-point
stencil from the reference's gallery.diffusion_stencil_2d), and one structurally unsymmetric random operator with
a missing diagonal entry, a stored zero diagonal, an empty row and one long row, with zeros and negative values in B.

No drop decision may sit on a knife edge: for every problem and k the generator measures the relative distance of
every value from the threshold it is compared with (distance filter, |ratio| < 1e-4, angle, sqrt(eps)), asserts it is
at least 1e-6 and prints the smallest.  The ratios are recomputed here with scipy products (rounding-level
differences from the reference's values do not matter at 1e-6).
Usage:  make -C oracle ref && python tools/gen_golden_evolution.py [large]
"""
import os
import sys

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_env  # noqa: E402
import gen_golden  # noqa: E402
import evolution_io as eio  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "evolution")
KS = (1, 2, 4)
MIN_GAP = 1e-6
np.mat = np.asmatrix            # the reference's strength.py builds its candidates with np.mat


# --------------------------------------------------------------------------- problems (from seeds)
def stencil_matrix(stencil, nx, ny):
    """the 3 x 3 stencil on an nx x ny grid (x fastest), couplings that leave the grid cut off; sorted CSR"""
    rows, cols, vals = [], [], []
    idx = np.arange(nx * ny).reshape(ny, nx)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            v = float(stencil[dy + 1][dx + 1])
            if v == 0.0:
                continue
            ys = slice(max(0, -dy), ny - max(0, dy))
            xs = slice(max(0, -dx), nx - max(0, dx))
            src = idx[ys, xs]
            dst = idx[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
            rows.append(src.ravel()); cols.append(dst.ravel()); vals.append(np.full(src.size, v))
    A = sps.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nx * ny, nx * ny)).tocsr()
    A.sort_indices()
    A.indices = A.indices.astype(np.intc)
    A.indptr = A.indptr.astype(np.intc)
    return A


def anisotropic(pyamg, nx, ny, eps, theta):
    from pyamg.gallery.diffusion import diffusion_stencil_2d
    return stencil_matrix(np.asarray(diffusion_stencil_2d(epsilon=eps, theta=theta, type="FE")), nx, ny)


def unsymmetric(seed=5, n=400):
    """random pattern, not symmetric: row 7 stores no diagonal, row 11 stores a zero diagonal, row 19 is empty, row 23
    holds about 300 entries; B has zeros and negative entries"""
    rng = np.random.RandomState(seed)
    M = sps.random(n, n, density=0.012, random_state=rng, format="lil", data_rvs=lambda s: rng.uniform(-1.0, 1.0, s))
    for i in range(n):
        M[i, i] = 4.0 + rng.rand()
    long_cols = rng.choice(n, 300, replace=False)
    M[23, long_cols] = rng.uniform(-0.05, 0.05, 300)
    M[23, 23] = 6.0
    M[19, :] = 0.0
    M[7, 7] = 0.0
    A = sps.csr_matrix(M)
    A.eliminate_zeros()
    A = sps.lil_matrix(A)
    A = sps.csr_matrix(A)
    A.sort_indices()
    # a STORED zero on the diagonal of row 11
    A[11, 11] = 0.0
    A.sort_indices()
    assert A[7, 7] == 0 and A.indptr[20] == A.indptr[19] and np.diff(A.indptr)[23] >= 290
    assert 11 in A.indices[A.indptr[11]:A.indptr[12]] and (abs(A - A.T) > 0).nnz > 0
    A.indices = A.indices.astype(np.intc)
    A.indptr = A.indptr.astype(np.intc)
    B = rng.uniform(0.5, 1.5, n)
    B[::9] *= -1.0
    B[[3, 23, 50]] = 0.0
    return A, B


# --------------------------------------------------------------------------- recording
class Recorder(object):
    """stands in for pyamg.strength.amg_core: forwards everything, keeps the arguments and results of the calls"""
    NAMES = ("incomplete_mat_mult_csr", "apply_distance_filter", "min_blocks", "apply_absolute_distance_filter",
             "evolution_strength_helper")

    def __init__(self, core, keep=NAMES):
        self._core = core
        self.keep = keep
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._core, name)
        if name not in self.NAMES or name not in self.keep:
            return fn

        def wrapped(*args):
            before = [np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in args]
            fn(*args)
            after = [np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in args]
            self.calls.append((name, before, after))
        return wrapped


ARGS = {"incomplete_mat_mult_csr": ("Ap", "Aj", "Ax", "Bp", "Bj", "Bx", "Sp", "Sj", "Sx", "dimen"),
        "apply_distance_filter": ("n_row", "epsilon", "Sp", "Sj", "Sx"),
        "apply_absolute_distance_filter": ("n_row", "epsilon", "Sp", "Sj", "Sx"),
        "min_blocks": ("n_blocks", "blocksize", "Sx", "Tx")}
OUTPUT = {"incomplete_mat_mult_csr": "Sx", "apply_distance_filter": "Sx", "apply_absolute_distance_filter": "Sx",
          "min_blocks": "Tx"}


def put_call(out, prefix, name, before, after):
    for arg, v in zip(ARGS[name], before):
        out["%s__%s" % (prefix, arg)] = np.asarray(v)
    o = OUTPUT[name]
    out["%s__%s_out" % (prefix, o)] = np.asarray(after[ARGS[name].index(o)])


def gaps(A, B, rho, k, epsilon, filter_call, core=None):
    """smallest relative distance of a compared value from its threshold: (distance filter, 1e-4 rule, angle rule,
    sqrt(eps) rule); the ratios from scipy products.  core: the reference's native module, for operators whose full
    k-th power does not fit memory: the last squaring is then its product on the pattern of A."""
    n = A.shape[0]
    Ac = A.copy(); Ac.eliminate_zeros(); Ac.sort_indices()
    D = A.diagonal(); Dinv = np.where(D != 0, 1.0 / np.where(D != 0, D, 1.0), 1.0)
    M = (sps.eye(n, format="csr") - (1.0 / rho) * sps.diags(Dinv) * A).T.tocsr()
    At = M
    for _ in range(int(np.log2(k)) - (1 if core is not None else 0)):
        At = At * At
    if k > 1 and core is not None:
        At.sort_indices()
        Bc = At.tocsc(); Bc.sort_indices()
        pat = Ac.copy()
        core.incomplete_mat_mult_csr(At.indptr, At.indices, At.data, Bc.indptr, Bc.indices, Bc.data, pat.indptr, pat.indices,
                                     pat.data, n)
        At = pat
    elif k > 1:
        pat = Ac.copy(); pat.data[:] = 1.0
        At = At.multiply(pat).tocsr()
    At.eliminate_zeros(); At.sort_indices()
    b = np.array(B, dtype=float).ravel(); b[b == 0] = 1.0
    rows = np.repeat(np.arange(n), np.diff(At.indptr))
    zt = (At.diagonal() / b)[rows] * b[At.indices]
    data = At.data
    off = rows != At.indices
    ratio = zt / data
    g_ratio = np.min(np.abs(np.abs(ratio) - 1e-4) / 1e-4)
    # the sign of zt * data is safe while neither factor is within rounding of zero, measured against the row's largest
    rowmax = np.zeros(n); np.maximum.at(rowmax, rows, np.abs(data))
    nz = zt != 0
    g_angle = min(np.min(np.abs(data) / rowmax[rows]), np.min(np.abs(zt[nz]) / np.abs(zt[nz]).max()))
    val = np.abs(1.0 - ratio)
    live = off & (np.abs(ratio) >= 1e-4) & (zt * data >= 0) & (val != 0)
    se = np.sqrt(np.finfo(float).eps)
    g_sqrt = np.min(np.abs(val[live] - se) / se) if live.any() else np.inf
    g_filter = np.inf
    if filter_call is not None:
        _, before, _ = filter_call
        n_row, eps_, Sp, Sj, Sx = before
        r = np.repeat(np.arange(n_row), np.diff(Sp))
        offd = Sj != r
        rowmin = np.full(n_row, np.inf); np.minimum.at(rowmin, r[offd], Sx[offd])
        if offd.any():
            thr = eps_ * rowmin[r[offd]]
            g_filter = np.min(np.abs(Sx[offd] - thr) / thr)
    return g_filter, g_ratio, g_angle, g_sqrt


def gen_problem(pyamg, name, A, B=None, epsilon=4.0):
    import pyamg.strength as rs
    out = {"A_indptr": A.indptr.astype(np.intc), "A_indices": A.indices.astype(np.intc), "A_data": A.data.copy(),
           "A_shape": np.array(A.shape, dtype=np.int64), "epsilon": np.array(epsilon)}
    if B is not None:
        out["B"] = np.asarray(B, dtype=np.float64).copy()
    worst = [np.inf] * 4
    for k in KS:
        core = rs.amg_core
        rec = Recorder(core)
        rs.amg_core = rec
        try:
            np.random.seed(0)
            Ain = A.copy()                                  # the reference sorts / prunes its argument in place
            Bin = None if B is None else np.array(B, dtype=np.float64).reshape(-1, 1)
            Cm = rs.evolution_strength_of_connection(Ain, Bin, epsilon=epsilon, k=k)
        finally:
            rs.amg_core = core
        # the estimate the reference drew: the same call on the same seed
        np.random.seed(0)
        D = A.diagonal(); Dinv = np.zeros_like(D); Dinv[D != 0] = 1.0 / D[D != 0]; Dinv[D == 0] = 1.0
        rho = pyamg.util.linalg.approximate_spectral_radius(pyamg.util.utils.scale_rows(A, Dinv, copy=True))
        key = "k%d" % k
        out[key + "_rho"] = np.array(float(rho))
        Cm = sps.csr_matrix(Cm)
        out[key + "_C_indptr"] = Cm.indptr.astype(np.intc)
        out[key + "_C_indices"] = Cm.indices.astype(np.intc)
        out[key + "_C_data"] = Cm.data.astype(np.float64)
        names = []
        filt = None
        for ci, (cname, before, after) in enumerate(rec.calls):
            put_call(out, "%s_call%d" % (key, ci), cname, before, after)
            names.append(cname)
            if cname == "apply_distance_filter":
                filt = (cname, before, after)
        out[key + "_calls"] = np.array(names, dtype="U40")
        g = gaps(A, np.ones(A.shape[0]) if B is None else B, float(rho), k, epsilon, filt)
        assert min(g) >= MIN_GAP, "%s k=%d: a drop decision within %g of its threshold: %r" % (name, k, MIN_GAP, g)
        worst = [min(a, b_) for a, b_ in zip(worst, g)]
        print("%-18s k=%d rho=%.15g nnz(C)=%d calls=%s gaps: filter %.2e ratio %.2e angle %.2e sqrt(eps) %.2e"
              % (name, k, rho, Cm.nnz, ",".join(names) or "-", g[0], g[1], g[2], g[3]))
    path = os.path.join(OUT, "%s.npz" % name)
    np.savez_compressed(path, **out)
    print("%-18s %6.0f KB, smallest gaps %s" % (name, os.path.getsize(path) / 1024, ", ".join("%.2e" % w for w in worst)))


def gen_large(pyamg, core, epsilon=eio.LARGE_EPSILON):
    """digests of the reference's results on the two problems of working size"""
    import pyamg.strength as rs
    out = {"epsilon": np.array(epsilon)}
    U = lambda text: np.array(text, dtype="U64")
    for name in eio.LARGE:
        A, B = eio.large_problem(name)
        for arr, d in zip(("indptr", "indices", "data"), eio.digests(A)):
            out["%s__A_%s_sha" % (name, arr)] = U(d)
        out["%s__B_sha" % name] = U(eio.sha(B, "<f8"))
        worst = [np.inf] * 4
        for k in KS:
            rec = Recorder(rs.amg_core, keep=("apply_distance_filter",))
            keep = rs.amg_core
            rs.amg_core = rec
            try:
                np.random.seed(0)
                Cm = rs.evolution_strength_of_connection(A.copy(), B.copy().reshape(-1, 1), epsilon=epsilon, k=k)
            finally:
                rs.amg_core = keep
            np.random.seed(0)
            D = A.diagonal(); Dinv = np.zeros_like(D); Dinv[D != 0] = 1.0 / D[D != 0]; Dinv[D == 0] = 1.0
            rho = float(pyamg.util.linalg.approximate_spectral_radius(pyamg.util.utils.scale_rows(A, Dinv, copy=True)))
            Cm = sps.csr_matrix(Cm)
            pre = "%s__k%d_" % (name, k)
            out[pre + "rho"] = np.array(rho)
            out[pre + "nnz"] = np.array(Cm.nnz, dtype=np.int64)
            for arr, d in zip(("indptr", "indices", "data"), eio.digests(Cm)):
                out[pre + arr + "_sha"] = U(d)
            n = Cm.shape[0]
            for part, lo, hi in (("head", 0, 32), ("tail", n - 32, n)):
                for arr, v in zip(("indptr", "indices", "data"), eio.rows_of(Cm, lo, hi)):
                    out[pre + part + "_" + arr] = v
            (filt,) = rec.calls
            g = gaps(A, B, rho, k, epsilon, filt, core=core)
            assert min(g) >= MIN_GAP, "%s k=%d: a drop decision within %g of its threshold: %r" % (name, k, MIN_GAP, g)
            worst = [min(a, b_) for a, b_ in zip(worst, g)]
            print("%-18s k=%d rho=%.15g nnz(C)=%d gaps: filter %.2e ratio %.2e angle %.2e sqrt(eps) %.2e"
                  % (name, k, rho, Cm.nnz, g[0], g[1], g[2], g[3]))
        print("%-18s smallest gaps %s" % (name, ", ".join("%.2e" % w for w in worst)))
    path = os.path.join(OUT, "large_digests.npz")
    np.savez_compressed(path, **out)
    print("large_digests.npz  %6.0f KB" % (os.path.getsize(path) / 1024))


def gen_flat(core):
    """direct calls of the two entries the measure never reaches with real blocks"""
    rng = np.random.RandomState(3)
    out = {}
    Sx = rng.uniform(-1.0, 1.0, 257 * 4)
    Sx[rng.rand(Sx.size) < 0.4] = 0.0
    Sx[8:12] = 0.0                                          # a block without a non-zero value
    Tx = np.zeros(257)
    core.min_blocks(257, 4, Sx, Tx)
    out.update(min_blocks__n_blocks=np.array(257), min_blocks__blocksize=np.array(4), min_blocks__Sx=Sx, min_blocks__Tx_out=Tx)
    S = sps.random(130, 130, density=0.08, random_state=rng, format="csr")
    S.setdiag(rng.rand(130)); S = sps.csr_matrix(S); S.sort_indices()
    Sp, Sj = S.indptr.astype(np.intc), S.indices.astype(np.intc)
    before = S.data.copy(); x = S.data.copy()
    core.apply_absolute_distance_filter(130, 0.5, Sp, Sj, x)
    assert np.min(np.abs(before - 0.5)) > 1e-6
    out.update(absfilter__n_row=np.array(130), absfilter__epsilon=np.array(0.5), absfilter__Sp=Sp, absfilter__Sj=Sj,
               absfilter__Sx=before, absfilter__Sx_out=x)
    np.savez_compressed(os.path.join(OUT, "flat_kernels.npz"), **out)
    print("flat_kernels.npz")


def main():
    os.makedirs(OUT, exist_ok=True)
    pyamg = ref_env.stage()
    sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))
    import _amg_core as core
    if sys.argv[1:] == ["large"]:                           # only large_digests.npz
        gen_large(pyamg, core)
        return
    gen_problem(pyamg, "aniso_40x40", anisotropic(pyamg, 40, 40, 0.01, np.pi / 6))
    gen_problem(pyamg, "aniso_17x23", anisotropic(pyamg, 17, 23, 0.001, np.pi / 4))
    gen_problem(pyamg, "aniso_9x31", anisotropic(pyamg, 9, 31, 0.1, 1.0))
    gen_problem(pyamg, "iso_12x12", anisotropic(pyamg, 12, 12, 1.0, 0.0))
    Au, Bu = unsymmetric()
    gen_problem(pyamg, "unsym_400", Au, Bu)
    gen_flat(core)
    # one SA hierarchy with its solve, in the layout of oracle/gen_golden.py
    gen_golden.OUT = OUT
    gs = ("block_gauss_seidel", {"sweep": "symmetric"})
    gen_golden.gen_hier(pyamg, "sa_evolution_2d", anisotropic(pyamg, 40, 40, 0.01, np.pi / 6),
                        lambda A, **kw: pyamg.smoothed_aggregation_solver(
                            A, strength=("evolution", {"k": 2, "epsilon": 4.0}), max_coarse=20, **kw),
                        gs, gs, dict(tol=1e-8))
    gen_large(pyamg, core)


if __name__ == "__main__":
    main()
