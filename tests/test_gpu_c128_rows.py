"""The row kernels of the complex128 engine (csrc/hier_c128.hip: csr_rows, bsr_rows, dense_apply and the EpiStore,
EpiResid, EpiAdd epilogues) on the designed operators of tests/c128_cases.py, through the C ABI (amg_hierx_*), bit for
bit against the NumPy model there: rows across several LDS chunks of 1024 products, workgroups with nothing to read,
row counts off a multiple of 256, 2 x 2 and 3 x 3 blocks, and transfer operators in 1 x 2 and 2 x 1 blocks.  The
smoothers are out of scope: their kernels are typed_kernels.hpp's, which the flat table pins in four dtypes."""
import ctypes

import numpy as np
import pytest

import c128_cases as cc

pytestmark = pytest.mark.gpu

APPLY = cc.apply_cases()
TRANSFER = cc.transfer_cases()


def padded(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a if a.size else np.zeros(1, dtype=dtype)


class Handle(object):
    """an amg_hierx handle of complex128 operators (c128_cases.Bsr) without smoothers"""

    def __init__(self, levels, M=None):
        from pyamg_amd import _lib
        self._lib = _lib
        self.L = _lib.lib()
        self.h = ctypes.c_void_p()
        _lib.check(self.L.amg_hierx_create(_lib.AMG_VALUE_C128, len(levels), 0, ctypes.byref(self.h)))
        try:
            for l, lvl in enumerate(levels):
                self.matrix(l, 0, lvl["A"])
                if l < len(levels) - 1:
                    self.matrix(l, 1, lvl["P"])
                    self.matrix(l, 2, lvl["R"])
            if M is not None:
                M = np.ascontiguousarray(M, dtype=np.complex128)
                _lib.check(self.L.amg_hierx_set_coarse_dense(self.h, M.ctypes.data, M.shape[0]))
            _lib.check(self.L.amg_hierx_finalize(self.h))
        except Exception:
            self.close()
            raise

    def matrix(self, lvl, which, A):
        Ap, Aj, Ax = padded(A.Ap, np.intc), padded(A.Aj, np.intc), padded(A.Ax, np.complex128)
        self._lib.check(self.L.amg_hierx_set_matrix(self.h, lvl, which, 1 if A.bsr else 0, A.nrows, A.ncols, A.R, A.C,
                                                    Ap.ctypes.data, Aj.ctypes.data, Ax.ctypes.data))

    def close(self):
        if self.h:
            self.L.amg_hierx_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@pytest.mark.parametrize("case", APPLY, ids=repr)
def test_apply(case):
    """amg_hierx_apply on level 0: y = A x on device vectors, each with a guard entry behind the last"""
    import torch
    from pyamg_amd import _lib
    A = case.A
    n = A.nrows
    x = torch.from_numpy(case.x.view(np.float64).copy()).cuda()
    y0 = np.full(n + 1, cc.GUARD, dtype=np.complex128)
    y = torch.from_numpy(y0.view(np.float64).copy()).cuda()
    with Handle([{"A": A}]) as h:
        torch.cuda.synchronize()
        _lib.check(h.L.amg_hierx_apply(h.h, 0, x.data_ptr(), y.data_ptr()))
        torch.cuda.synchronize()
        got = y.cpu().numpy().view(np.complex128)
        xb = x.cpu().numpy().view(np.complex128)
    assert got[n] == cc.GUARD, "the guard entry of y was written"
    assert cc.bit_mismatches(xb, case.x) == 0, "x was written"
    bad = cc.bit_mismatches(got[:n], case.want())
    assert bad == 0, "%s: %d parts differ, max |d| = %g" % (case.name, bad, np.abs(got[:n] - case.want()).max())


@pytest.mark.parametrize("case", TRANSFER, ids=repr)
def test_transfer_cycle(case):
    """amg_hierx_cycle of a smoother-free two-level hierarchy with a dense coarse operator: x0 + P (M (R (b - A x0)))"""
    from pyamg_amd import _lib
    n = case.A.nrows
    b, x = case.b.copy(), case.x0.copy()
    with Handle([{"A": case.A, "P": case.P, "R": case.R}, {"A": case.A1}], M=case.M) as h:
        _lib.check(h.L.amg_hierx_cycle(h.h, b.ctypes.data, x.ctypes.data, 0, 0))
    assert x[n] == cc.GUARD and cc.bit_mismatches(b, case.b) == 0
    bad = cc.bit_mismatches(x[:n], case.want())
    assert bad == 0, "%s: %d parts differ, max |d| = %g" % (case.name, bad, np.abs(x[:n] - case.want()).max())
