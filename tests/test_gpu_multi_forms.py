"""The multi-RHS engine (csrc/hier_multi.hip) on the designed irregular operators of tests/multi_cases.py, driven through
the C ABI (amg_hierm_*): every comparison is bit for bit with the oracle (oracle_lib.Hierarchy), which
tests/test_multi_cases_host.py holds equal to a plain NumPy model of the kernels.

Transfer cycle: two levels without smoothers, X = x0 + P (M (R (b - A x0))) -- EpiResid, EpiStore on a rectangular R
with long rows, dense_apply_multi and EpiAdd, through csr_rows_multi or csr_rows_direct by the nnz <= 12 n rule.
Smoother cycles: a coarse level of one unknown whose correction is zero, so the cycle is the pre-smoother, x + 0 and
the post-smoother -- EpiJacobi / EpiJacobiBsr1, gs_level_multi in both roundings, sor_blend_multi, EpiPoly0,
EpiPolyStep, add_to_multi.  Every family runs at k = 1, 2, 3, 4, 5, 8 columns on a handle created for k, and at k = 3 on
a handle created for 8.  The guard row behind every host array must come back unchanged."""
import ctypes

import numpy as np
import pytest

import multi_cases as mc
import vector_models as vm

pytestmark = pytest.mark.gpu

CASES = mc.cases()
NAMES = [c.name for c in CASES]
C = mc.by_name()
LABELS = [label for label, _ in mc.SMOOTHERS]
KIND = {"jacobi": 1, "gauss_seidel": 2, "sor": 3, "polynomial": 4}
SWEEP = {"forward": 0, "backward": 1, "symmetric": 2}
AMG_SOLVE_NO_EARLY_STOP = 2


def padded(a, dtype):
    """the array itself, or one element where it is empty (a valid address for an array nobody reads)"""
    a = np.ascontiguousarray(a, dtype=dtype)
    return a if a.size else np.zeros(1, dtype=dtype)


class Handle(object):
    """an amg_hierm handle built from (nrows, ncols, Ap, Aj, Ax) operators"""

    def __init__(self, kmax, levels, M=None, coarse_smoother=None):
        from pyamg_amd import _lib
        self._lib = _lib
        self.L = _lib.lib()
        self.h = ctypes.c_void_p()
        _lib.check(self.L.amg_hierm_create(len(levels), 0, kmax, ctypes.byref(self.h)))
        try:
            for l, lvl in enumerate(levels):
                self.matrix(l, 0, lvl["A"], lvl.get("bsr", False))
                if l < len(levels) - 1:
                    self.matrix(l, 1, lvl["P"])
                    self.matrix(l, 2, lvl["R"])
                    for which, key in ((0, "pre"), (1, "post")):
                        d, keep = self.desc(lvl.get(key, mc.NONE))
                        _lib.check(self.L.amg_hierm_set_smoother(self.h, l, which, d))
            if M is not None:
                M = np.ascontiguousarray(M, dtype=np.float64)
                _lib.check(self.L.amg_hierm_set_coarse_dense(self.h, _lib.dp(M), M.shape[0]))
            if coarse_smoother is not None:
                d, keep = self.desc(coarse_smoother)
                _lib.check(self.L.amg_hierm_set_coarse_smoother(self.h, d))
            _lib.check(self.L.amg_hierm_finalize(self.h))
        except Exception:
            self.close()
            raise

    def matrix(self, lvl, which, csr, bsr=False):
        n, nc, Ap, Aj, Ax = csr
        Ap, Aj, Ax = padded(Ap, np.intc), padded(Aj, np.intc), padded(Ax, np.float64)
        assert len(Ap) == n + 1
        self._lib.check(self.L.amg_hierm_set_matrix(self.h, lvl, which, 1 if bsr else 0, n, nc, 1, 1, Ap.ctypes.data,
                                                    Aj.ctypes.data, Ax.ctypes.data))

    def desc(self, d):
        s = self._lib.SmootherDesc()
        keep = None
        if d.get("name") is None:
            s.kind = 0
            return s, keep
        s.kind = KIND[d["name"]]
        s.iterations = int(d.get("iterations", 1))
        s.sweep = SWEEP[d.get("sweep", "forward")]
        s.omega = float(d.get("omega", 1.0))
        if "coefficients" in d:
            keep = np.ascontiguousarray(d["coefficients"], dtype=np.float64)
            s.ncoef, s.coef = len(keep), self._lib.dp(keep)
        return s, keep

    def cycle(self, B, X):
        """one V cycle of the k columns of B, X ((n + 1, k) with the guard row): X's first n rows are overwritten"""
        k = B.shape[1]
        assert B.flags.c_contiguous and X.flags.c_contiguous and X.shape == B.shape
        self._lib.check(self.L.amg_hierm_cycle(self.h, k, B.ctypes.data, X.ctypes.data, 0, 0))

    def close(self):
        if self.h:
            self.L.amg_hierm_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def transfer_handle(case, kmax):
    return Handle(kmax, [{"A": case.A, "P": case.P, "R": case.R}, {"A": case.A1}], M=case.M)


def smoother_handle(case, label, bsr, kmax):
    desc = dict(mc.SMOOTHERS)[label]
    R, P = mc.smoother_transfers(case.n)
    return Handle(kmax, [{"A": case.Ad, "bsr": bsr, "P": P, "R": R, "pre": desc, "post": desc}, {"A": mc.SMOOTHER_A1}],
                  M=mc.SMOOTHER_M)


def run(handle, case, cols, nan_cols=()):
    """the cycle of the given columns of the case's B8 / X8 (nan_cols: positions filled with NaN instead); returns X
    after checking both guard rows and that B came back as it went"""
    B, X = mc.take(case.B8, cols), mc.take(case.X8, cols)
    for p in nan_cols:
        B[:-1, p] = np.nan
        X[:-1, p] = np.nan
    B0 = B.copy()
    handle.cycle(B, X)
    assert mc.bit_mismatches(B, B0) == 0, "B was written"
    assert np.all(X[-1] == mc.GUARD), "the guard row of X was written"
    return X[:-1]


def check_columns(X, want, cols, skip=(), what=""):
    for p, j in enumerate(cols):
        if p in skip:
            continue
        bad = mc.bit_mismatches(X[:, p], want[:, j])
        assert bad == 0, "%s: column %d (position %d of %d): %d rows differ, max |d| = %g" % (
            what, j, p, len(cols), bad, np.nanmax(np.abs(X[:, p] - want[:, j])))


# ------------------------------------------------------------------------------------------------ transfer cycle
@pytest.mark.parametrize("kmax, k", mc.KMAX_PAIRS)
@pytest.mark.parametrize("name", NAMES)
def test_transfer_cycle(name, kmax, k):
    case = C[name]
    want = mc.oracle_transfer(case)
    with transfer_handle(case, kmax) as h:
        cols = list(range(k))
        check_columns(run(h, case, cols), want, cols, what="%s transfer kmax %d" % (name, kmax))


# ------------------------------------------------------------------------------------------------ smoother cycles
@pytest.mark.parametrize("bsr", [False, True], ids=["csr", "bsr1"])
@pytest.mark.parametrize("label", LABELS)
@pytest.mark.parametrize("name", NAMES)
def test_smoother_cycle(name, label, bsr):
    case = C[name]
    want = mc.oracle_smoother(case, label, bsr)
    for kmax, k in mc.KMAX_PAIRS:
        with smoother_handle(case, label, bsr, kmax) as h:
            cols = list(range(k))
            check_columns(run(h, case, cols), want, cols, what="%s %s kmax %d" % (name, label, kmax))


# ------------------------------------------------------------------------------------------------ batch invariance
PERMUTATION = [7, 2, 5, 0, 3, 6, 1, 4]


def invariance(h, case, want, what):
    check_columns(run(h, case, list(range(8))), want, list(range(8)), what=what + " k = 8")
    for j in (0, 3, 7):                                             # alone
        check_columns(run(h, case, [j]), want, [j], what=what + " alone")
    check_columns(run(h, case, PERMUTATION), want, PERMUTATION, what=what + " permuted")
    # beside NaN-filled neighbours: in the same lane (two columns per lane) and in the other lanes of the row
    check_columns(run(h, case, [5, 0], nan_cols=[1]), want, [5, 0], skip=[1], what=what + " [5, NaN]")
    check_columns(run(h, case, [0, 3, 0, 1], nan_cols=[0, 2]), want, [0, 3, 0, 1], skip=[0, 2], what=what + " [NaN, 3, NaN, 1]")
    check_columns(run(h, case, [6, 0, 0, 0, 4, 0, 0], nan_cols=[1, 2, 3, 5, 6]), want, [6, 0, 0, 0, 4, 0, 0],
                  skip=[1, 2, 3, 5, 6], what=what + " [6, NaN x 3, 4, NaN x 2]")


@pytest.mark.parametrize("name", NAMES)
def test_batch_invariance_of_the_transfer_cycle(name):
    case = C[name]
    with transfer_handle(case, 8) as h:
        invariance(h, case, mc.oracle_transfer(case), name + " transfer")


@pytest.mark.parametrize("label, bsr", [("jacobi", False), ("jacobi", True), ("gs_symmetric", False), ("sor", True),
                                        ("poly3", False)])
@pytest.mark.parametrize("name", NAMES)
def test_batch_invariance_of_the_smoother_cycles(name, label, bsr):
    case = C[name]
    with smoother_handle(case, label, bsr, 8) as h:
        invariance(h, case, mc.oracle_smoother(case, label, bsr), "%s %s" % (name, label))


# ------------------------------------------------------------------------------------------------ the norm tree
G = vm.MULTI_NORM_GRID
NORM_CASES = [(n, k) for n in (1, 257, G, G + 1) for k in (1, 3, 8)] + [(2 * G + 3, 2)]


@pytest.mark.parametrize("n, k", NORM_CASES)
def test_residual_norm_is_the_fixed_tree(n, k):
    """one level, a diagonal A, a Jacobi coarse smoother: residuals[j][0] = ||b_j - A x_j|| through EpiResid and
    norm_partial_multi / norm_final_multi.  The residual is exact to model (b - (0 + d x)), the tree is
    vector_models.multi_norm_model.  n = 524288 fills the grid (every lane one row), one more gives lane 0 of workgroup 0
    a second row, 1048579 = 2 * 524288 + 3 gives three lanes a third."""
    from pyamg_amd import _lib
    assert 2 * G + 3 == 1048579
    rng = np.random.RandomState(1000 + n % 1000 + k)
    d = (0.5 + rng.rand(n)) * rng.choice([-1.0, 1.0], n)
    A = (n, n, np.arange(n + 1, dtype=np.intc), np.arange(n, dtype=np.intc), d)
    B = rng.uniform(-1.0, 1.0, size=(n + 1, k)) * (10.0 ** (3.0 * np.arange(k) - 9.0))
    X = rng.uniform(-1.0, 1.0, size=(n + 1, k)) * (10.0 ** (3.0 * np.arange(k) - 9.0))
    if k >= 3:
        B[:, 2] = X[:, 2] = 0.0
    B[n] = X[n] = mc.GUARD
    r = np.subtract(B[:-1], np.add(0.0, np.multiply(d[:, None], X[:-1])))
    want = [vm.multi_norm_model(r[:, j]) for j in range(k)]
    res = np.full((k, 2), -1.0)
    nres = np.zeros(k, dtype=np.intc)
    with Handle(k, [{"A": A}], coarse_smoother={"name": "jacobi", "omega": 0.7, "iterations": 1}) as h:
        _lib.check(h.L.amg_hierm_solve(h.h, k, B.ctypes.data, X.ctypes.data, 0.0, 1, 0, _lib.dp(res), _lib.ip(nres),
                                       AMG_SOLVE_NO_EARLY_STOP))
    assert np.all(nres == 2) and np.all(np.isfinite(res))
    assert np.all(X[n] == mc.GUARD) and np.all(B[n] == mc.GUARD)
    for j in range(k):
        assert np.float64(res[j, 0]).view(np.int64) == np.float64(want[j]).view(np.int64), \
            "n %d k %d column %d: %r, model %r" % (n, k, j, res[j, 0], want[j])
    if k >= 3:
        assert res[2, 0] == 0.0
    assert len(set(res[:, 0])) == k                     # the columns' norms are orders of magnitude apart
