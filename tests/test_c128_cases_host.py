"""The complex128 row-kernel cases of tests/c128_cases.py cross the boundaries they are built for, and the model the
device test compares against is the float64 model of tests/multi_cases.py (itself held to the oracle) on real data, and
scipy's product to rounding on complex data.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sps

import c128_cases as cc
import multi_cases as mc

APPLY = cc.apply_cases()
TRANSFER = cc.transfer_cases()
A_BY = dict((c.name, c) for c in APPLY)
T_BY = dict((c.name, c) for c in TRANSFER)


def as_scipy(A, magnitude=False):
    """copies: scipy sums duplicates in place when asked for |A|, and the cases' arrays are shared"""
    Ax = np.abs(A.Ax) if magnitude else A.Ax.copy()
    if A.bsr:
        return sps.bsr_matrix((Ax, A.Aj.copy(), A.Ap.copy()), shape=(A.nrows, A.ncols))
    return sps.csr_matrix((Ax.ravel(), A.Aj.copy(), A.Ap.copy()), shape=(A.nrows, A.ncols))


def test_restated_constants_and_boundaries():
    assert cc.CHUNK == 1024 and cc.ROWS_PER_WG == 256
    for f in ("medium", "long_staged", "short_staged_1100"):
        A = A_BY["csr_" + f].A
        assert cc.straddling_rows(A), f
        spans = [(e1 - e0 + cc.CHUNK - 1) // cc.CHUNK for _, _, e0, e1 in
                 mc.workgroup_entries((A.nrows, A.ncols, A.Ap, A.Aj, None), cc.ROWS_PER_WG)]
        assert max(spans) >= 3, (f, spans)
    assert np.diff(A_BY["csr_long_staged"].A.Ap).max() > 6 * cc.CHUNK          # a row of more than six chunks
    assert cc.empty_workgroups(A_BY["csr_short_staged_1100"].A) and cc.empty_workgroups(A_BY["csr_empty_300"].A)
    # remainders: one below, at and one above 256 rows, and one row behind three full workgroups
    assert [A_BY["csr_short_%d" % n].A.nrows for n in (1, 255, 256, 257, 769)] == [1, 255, 256, 257, 769]
    # the restriction's rows cross chunks in one workgroup of 37 rows
    assert cc.straddling_rows(T_BY["csr_medium"].R) and cc.straddling_rows(T_BY["csr_long_staged"].R)


def test_block_operators():
    for bs in (2, 3):
        for f in cc.BSR_PATTERNS:
            A = A_BY["bsr%d_%s" % (bs, f)].A
            assert A.bsr and A.R == A.C == bs and A.nrows == A.ncols == A.nb * bs
            assert A.nrows % 256 != 0 and A.nb % 256 != 0
            assert A.Ax.shape == (A.Ap[-1], bs, bs)
            assert np.any(np.all(A.Ax.reshape(len(A.Ax), -1) == 0, axis=1))      # a stored zero block
    assert A_BY["bsr3_short_staged_1100"].A.nrows == 3300 and A_BY["bsr2_short_257"].A.nrows == 514
    L = np.diff(A_BY["bsr2_short_staged_1100"].A.Ap)
    assert np.all(L[300:812] == 0)                 # point rows 600..1623: four whole workgroups of bsr_rows read nothing
    for f in cc.BSR_TRANSFER_FAMILIES:
        t = T_BY["bsr_" + f]
        n0 = t.A.nrows
        assert n0 % 2 == 0 and not t.A.bsr
        assert (t.R.R, t.R.C, t.R.nrows, t.R.ncols) == (1, 2, cc.N1, n0)
        assert (t.P.R, t.P.C, t.P.nrows, t.P.ncols) == (2, 1, n0, cc.N1)
        assert np.diff(t.R.Ap).max() > 50 and np.any(np.diff(t.P.Ap) == 0)


def test_values_are_complex_with_real_and_imaginary_entries():
    for case in APPLY:
        v = case.A.Ax.ravel()
        if len(v) < 300:
            continue
        nz = v != 0
        assert np.count_nonzero(nz & (v.imag == 0)) > 0 and np.count_nonzero(nz & (v.real == 0)) > 0, case.name
        assert np.count_nonzero((v.real != 0) & (v.imag != 0)) > 0.7 * len(v)
        assert np.count_nonzero(~nz) > 0
        x = case.x
        assert x[-1] == cc.GUARD and np.any(np.signbit(x.real) & (x.real == 0)) and np.any(np.signbit(x.imag) & (x.imag == 0))


@pytest.mark.parametrize("case", APPLY, ids=repr)
def test_apply_model_is_the_product(case):
    want = as_scipy(case.A) @ case.x[:-1]
    got = case.want()
    assert got.shape == want.shape and np.all(np.isfinite(got.view(np.float64)))
    scale = as_scipy(case.A, magnitude=True) @ np.abs(case.x[:-1])
    L = max(int(np.diff(case.A.Ap).max()) * case.A.C, 1) if case.A.nb else 1
    assert np.all(np.abs(got - want) <= (L + 4) * 2.0 ** -52 * scale)
    if case.A.Ap[-1] > 100:
        assert np.count_nonzero(got) > 0.3 * len(got)


@pytest.mark.parametrize("family", ["short_257", "medium", "short_staged_1100"])
def test_model_on_real_data_is_the_float64_model(family):
    """with every imaginary part zero the complex model's real parts are the float64 row sums of multi_cases.row_sum,
    which test_multi_cases_host holds equal to the oracle"""
    c = mc.by_name()[family]
    n, nc, Ap, Aj, Ax = c.A
    A = cc.Bsr(n, nc, 1, 1, Ap, Aj, Ax.astype(np.complex128), False)
    x = c.X8[:-1, 4]
    got = cc.rows_through(A, x.astype(np.complex128))
    want = mc.rows_through(c.A, x[:, None])[0][:, 0]
    assert mc.bit_mismatches(got.real, want) == 0 and not np.any(got.imag)


@pytest.mark.parametrize("case", TRANSFER, ids=repr)
def test_transfer_model_is_the_cycle(case):
    A, R, P = as_scipy(case.A), as_scipy(case.R), as_scipy(case.P)
    b, x0 = case.b[:-1], case.x0[:-1]
    want = x0 + P @ (case.M @ (R @ (b - A @ x0)))
    got = case.want()
    assert np.all(np.isfinite(got.view(np.float64)))
    assert np.allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
    if len(x0) > 1:
        assert cc.bit_mismatches(got, x0) > len(x0) // 4        # the correction reaches the rows
