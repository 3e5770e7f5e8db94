"""The sliced form's layout (csrc/sell.hip): one header record per slice (entry and code-word offsets, width, coded flag,
window origins) and one (row, length) pair per slot.  Smallest operators that reach every path of it: the form needs
>= 2^16 rows, 8..48 entries per row on average and <= 15 % padding."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sps

PLANTED = (0, 32, 33, 47, 48, 49, 64, 65)        # widths around one pass (32), pass + tail, and two passes
OFFS = np.array([-30000, -4100, 0, 4100, 30000])


def _clustered(n, m, lens, stride):
    """CSR arrays whose row i holds lens[i] DISTINCT columns in five clusters around stride * i: at most ~10 windows of
    4096 columns per slice of 64 rows, so its slices are coded"""
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    rows = np.repeat(np.arange(n), lens)
    k = np.arange(indptr[-1]) - indptr[rows]
    cols = (stride * rows + OFFS[k % 5] + 3 * (k // 5)) % m
    return indptr, cols


@functools.lru_cache(maxsize=None)
def _square():
    """70001 rows (not a multiple of the window of 256) of 20..30 entries; planted: three sets of rows of exactly
    0 / 32 / 33 / 47 / 48 / 49 / 64 / 65 entries (one set inside a single window) and three rows of 100..300; columns
    clustered (coded slices), a band of rows scattered over all columns (slices that keep 32-bit columns), and single
    scattered rows inside otherwise clustered slices"""
    rng = np.random.RandomState(23)
    n = 70001
    lens = rng.randint(20, 31, size=n)
    lens[[2000 + 300 * i for i in range(len(PLANTED))]] = PLANTED        # one per window
    lens[[30720 + 3 * i for i in range(len(PLANTED))]] = PLANTED         # all inside the window of rows 30720 .. 30975
    lens[rng.choice(np.arange(50000, 69000), size=len(PLANTED), replace=False)] = PLANTED
    lens[[1234, 44444, n - 1]] = (100, 217, 300)
    indptr, cols = _clustered(n, n, lens, 1)
    scattered = list(range(20000, 21000)) + list(range(40000, 40400, 50)) + [30721]
    for i in scattered:
        cols[indptr[i]:indptr[i + 1]] = rng.choice(n, size=lens[i], replace=False)
    A = sps.csr_matrix((rng.randn(indptr[-1]), cols.astype(np.intc), indptr.astype(np.intc)), shape=(n, n))
    assert np.array_equal(np.diff(A.indptr), lens)
    return A


@functools.lru_cache(maxsize=None)
def _rect():
    """66000 x 140000: at least twice as many columns as rows, so the windows are 64 rows (one slice) and only rows of
    nearly equal length keep the padding under 15 %"""
    rng = np.random.RandomState(29)
    n, m = 66000, 140000
    lens = rng.randint(25, 29, size=n)
    lens[[100, 20000, 20001, 65999]] = (0, 33, 48, 49)
    indptr, cols = _clustered(n, m, lens, 2)
    for i in range(33000, 33300):
        cols[indptr[i]:indptr[i + 1]] = rng.choice(m, size=lens[i], replace=False)
    return sps.csr_matrix((rng.randn(indptr[-1]), cols.astype(np.intc), indptr.astype(np.intc)), shape=(n, m))


def _layout(A):
    """what build_sell stores for A, recomputed: slices, padded entries, code words, coded slices"""
    n, m = A.shape
    sigma = 64 if m >= 2 * n else 256
    lens = np.diff(A.indptr)
    nwin = -(-n // sigma)
    nslices = nwin * (sigma // 64)
    entries = words = coded = 0
    hi = A.indices >> 12
    for w0 in range(0, n, sigma):
        wl = lens[w0:w0 + sigma]
        order = np.argsort(-wl, kind="stable")                          # longest first, ties in row order
        for s0 in range(0, sigma, 64):
            rows = w0 + order[s0:s0 + 64]
            w = int(lens[rows[0]]) if rows.size else 0
            entries += 64 * w
            words += 64 * ((w + 1) // 2)
            wins = np.unique(np.concatenate([hi[A.indptr[r]:A.indptr[r + 1]] for r in rows])) if rows.size else ()
            coded += len(wins) <= 16
    return nslices, entries, words, coded


class _Hier(object):
    """a bare amg_hier with one stored operator (level 0: A, or the restriction of a two-level hierarchy)"""

    def __init__(self, M, which=0, coef=None):
        from pyamg_amd import _lib
        self._lib, self.L = _lib, _lib.lib()
        self.which, self.shape = which, M.shape
        self.h = self.L.amg_hier_create(2 if which else 1, 0)
        assert self.h
        self.keep = [np.ascontiguousarray(M.indptr, dtype=np.intc), np.ascontiguousarray(M.indices, dtype=np.intc),
                     np.ascontiguousarray(M.data, dtype=np.float64)]
        _lib.check(self.L.amg_hier_set_matrix(self.h, 0, which, 0, M.shape[0], M.shape[1], 1, 1, self.keep[0].ctypes.data,
                                              self.keep[1].ctypes.data, self.keep[2].ctypes.data, 0))
        if coef is not None:
            d = _lib.SmootherDesc()
            co = np.ascontiguousarray(coef, dtype=np.float64)
            self.keep.append(co)
            d.kind, d.iterations, d.ncoef, d.coef, d.blocksize = 4, 1, len(co), _lib.dp(co), 1
            _lib.check(self.L.amg_hier_set_smoother(self.h, 0, 0, d))
            _lib.check(self.L.amg_hier_finalize(self.h))

    def matvec(self, x):
        y = np.zeros(self.shape[0])
        self._lib.check(self.L.amg_hier_matvec(self.h, 0, self.which, self._lib.dp(x), self._lib.dp(y)))
        return y

    def relax(self, b, x):
        x = x.copy()
        self._lib.check(self.L.amg_hier_relax(self.h, 0, 0, self._lib.dp(b), self._lib.dp(x)))
        return x

    def close(self):
        if self.h:
            self.L.amg_hier_destroy(self.h)
            self.h = None


def _poly_reference(A, coef, b, x):
    """relaxation.py:593-668 with scipy's csr_matvec: r = b - A x; h = c0 r; h = c r + A h ...; x + h"""
    r = b - A @ x
    h = coef[0] * r
    for c in coef[1:]:
        h = c * r + A @ h
    return r, x + h


@pytest.fixture
def sell_switches():
    from pyamg_amd import _lib
    L = _lib.lib()
    L.amg_hier_device_bytes.restype = C.c_long
    L.amg_hier_operator_bytes.restype = C.c_double
    yield L
    L.amg_set_sell_form(1)
    L.amg_set_sell_index16(1)


@pytest.mark.gpu
@pytest.mark.parametrize("idx16", [1, 0])
def test_square_operator_with_planted_widths_same_bits(sell_switches, idx16):
    """y = A x and r = b - A x (the one-coefficient polynomial step x + 1.0 * (b - A x)), and the two- and
    three-coefficient polynomial steps (residual, step and last modes) from the sliced form = from the CSR kernel =
    scipy, bit for bit, with the 16-bit codes and with 32-bit columns"""
    L = sell_switches
    A = _square()
    n = A.shape[0]
    rng = np.random.RandomState(3)
    x, b = rng.randn(n), rng.randn(n)
    L.amg_set_sell_form(1)
    L.amg_set_sell_index16(idx16)
    ref_y = A @ x
    for coef in ([1.0], [0.3, -0.7], [0.3, -0.7, 1.9]):
        op = _Hier(A, coef=coef)
        try:
            out = {}
            for on in (1, 0):
                L.amg_set_sell_form(on)
                assert L.amg_hier_operator_form(op.h, 0) == (3 if on else 0)       # no silent fall-back
                out[on] = (op.matvec(x), op.relax(b, x))
            L.amg_set_sell_form(1)
            if idx16:                                     # codes built, then switched off: the same slices from 32-bit columns
                L.amg_set_sell_index16(0)
                assert np.array_equal(op.matvec(x), ref_y) and np.array_equal(op.relax(b, x), out[1][1])
                L.amg_set_sell_index16(1)
            r, xn = _poly_reference(A, coef, b, x)
            assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][0], ref_y)
            assert np.array_equal(out[1][1], out[0][1]), coef
            assert np.array_equal(out[1][1], xn), coef
            if len(coef) == 1:
                assert np.array_equal(out[1][1], x + r)                           # r = b - A x itself
        finally:
            op.close()


@pytest.mark.gpu
@pytest.mark.parametrize("idx16", [1, 0])
def test_rectangular_operator_as_restriction_same_bits(sell_switches, monkeypatch, idx16):
    """66000 x 140000 (windows of 64 rows) applied as R of a two-level hierarchy: sliced = CSR kernel = scipy; that R
    did take the form shows in the device bytes"""
    L = sell_switches
    R = _rect()
    x = np.random.RandomState(5).randn(R.shape[1])
    L.amg_set_sell_form(1)
    L.amg_set_sell_index16(idx16)
    monkeypatch.setenv("AMG_SELL", "0")
    op = _Hier(R, which=2)
    plain = L.amg_hier_device_bytes(op.h)
    op.close()
    monkeypatch.delenv("AMG_SELL")
    op = _Hier(R, which=2)
    try:
        assert L.amg_hier_device_bytes(op.h) > plain + 12 * R.nnz
        out = {}
        for on in (1, 0):
            L.amg_set_sell_form(on)
            out[on] = op.matvec(x)
        assert np.array_equal(out[1], out[0]) and np.array_equal(out[1], R @ x)
    finally:
        op.close()


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [2, 3])
def test_chebyshev_hierarchy_same_iterates(sell_switches, degree):
    """poisson((96, 90, 84)), SA, Chebyshev of degree 2 and 3 (degree 3: the first / step / last modes), 5 iterations:
    iterates and residual histories with A_1, R, P from the sliced form = without"""
    from pyamg_amd.aggregation import poisson, smoothed_aggregation_solver
    L = sell_switches
    sm = ("chebyshev", {"degree": degree})
    np.random.seed(2)
    ml = smoothed_aggregation_solver(poisson((96, 90, 84)), presmoother=sm, postsmoother=sm)
    b = np.random.rand(ml.levels[0].A.shape[0])
    out = {}
    for on in (1, 0):
        L.amg_set_sell_form(on)
        ml._invalidate_device()
        res = []
        x = ml.solve(b, tol=1e-30, maxiter=5, residuals=res)
        if on:
            assert L.amg_hier_operator_form(ml.device_hierarchy().h, 1) == 3
        out[on] = (x, np.array(res))
    assert np.array_equal(out[1][0], out[0][0])
    assert np.array_equal(out[1][1], out[0][1])


@pytest.mark.gpu
@pytest.mark.parametrize("idx16", [1, 0])
def test_accounting_follows_the_layout(sell_switches, monkeypatch, idx16):
    """amg_hier_operator_bytes(h, 0, 1) = the bytes one application streams from the layout, and the device bytes of the
    form = the layout's arrays, both recomputed here from the slices, the padded entries and the coded slices"""
    L = sell_switches
    A = _square()
    n = A.shape[0]
    nslices, entries, words, coded = _layout(A)
    assert nslices == 4 * 274 and entries <= 1.15 * A.nnz and coded >= 0.5 * nslices and coded < nslices
    L.amg_set_sell_form(1)
    L.amg_set_sell_index16(idx16)
    monkeypatch.setenv("AMG_SELL", "0")
    op = _Hier(A)
    plain = L.amg_hier_device_bytes(op.h)
    op.close()
    monkeypatch.delenv("AMG_SELL")
    op = _Hier(A)
    try:
        assert L.amg_hier_operator_form(op.h, 0) == 3
        # slots: (row, length) pairs; headers: 96 B; entries: 4 + 8 B; code words (built only with the codes on)
        new = 8 * 64 * nslices + 96 * nslices + 12 * entries + (4 * words if idx16 else 0)
        assert L.amg_hier_device_bytes(op.h) - plain == new
        # the layout before: 4 + 2 B per slot, entry offsets, and with the codes their offsets, a flag and 64 B of origins
        old = 6 * 64 * nslices + 8 * (nslices + 1) + 12 * entries + ((4 * words + 65 * nslices + 8 * (nslices + 1)) if idx16 else 0)
        grew = (143 * nslices - 16) if idx16 else (216 * nslices - 8)
        assert grew > 0 and new - old == grew
        f16 = coded / nslices if idx16 else 0.0
        # entries (2 B less per entry of a coded slice), slots and headers (with the codes on: origins included), then x, b and r
        moved = (12.0 - 2.0 * f16) * entries + (8.0 * 64.0 + (96.0 if idx16 else 32.0)) * nslices + 8.0 * n + 8.0 * n + 8.0 * n
        assert L.amg_hier_operator_bytes(op.h, 0, 1) == pytest.approx(moved, rel=1e-14)
    finally:
        op.close()
