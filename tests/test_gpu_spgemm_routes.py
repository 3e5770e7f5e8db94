"""Every route of the device sparse product (csrc/spgemm.hip matmat()) on the MI355X, pinned to scipy's csr_matmat bit
for bit: for every case of tests/spgemm_cases.py and both value types the route record (amg_spgemm_last_route) equals
what the model of the policy predicts, the product has the reference's row pointer, columns and value bytes, and the
library holds as many device buffers afterwards as before -- refusals included.  tests/test_spgemm_cases_host.py proves
on the CPU that each case has the property it is named for and that reference, scipy and the host product agree."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import spgemm_cases as sc

pytestmark = pytest.mark.gpu

DEVICE_IDS = [(d, n) for d, n in sc.case_ids() if sc.cases(d)[n].device]


def _device_product(A, B, dtype):
    """(return code, (Cp, Cj, Cx) or None) of amg_csr_matmat_device / _c128 on the operands exactly as stored"""
    from pyamg_amd import _lib
    L = _lib.lib()
    z = sc.NP_DTYPE[dtype]
    Ap, Aj, Ax = (np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.intc),
                  np.ascontiguousarray(A.data, dtype=z))
    Bp, Bj, Bx = (np.ascontiguousarray(B.indptr, dtype=np.int64), np.ascontiguousarray(B.indices, dtype=np.intc),
                  np.ascontiguousarray(B.data, dtype=z))
    Cp = np.empty(A.shape[0] + 1, dtype=np.int64)
    g = C.c_void_p()
    entry = L.amg_csr_matmat_device if dtype == sc.F64 else L.amg_csr_matmat_device_c128
    rc = entry(A.shape[0], A.shape[1], B.shape[1], Ap.ctypes.data, Aj.ctypes.data, Ax.ctypes.data,
               Bp.ctypes.data, Bj.ctypes.data, Bx.ctypes.data, Cp.ctypes.data, C.byref(g))
    if rc != 0:
        assert not g.value
        return rc, None
    Cj = np.empty(int(Cp[-1]), dtype=np.intc)
    Cx = np.empty(int(Cp[-1]), dtype=z)
    fetch = L.amg_galerkin_fetch if dtype == sc.F64 else L.amg_galerkin_fetch_c128
    _lib.check(fetch(g, Cj.ctypes.data, Cx.ctypes.data))
    return 0, (Cp, Cj, Cx)


@pytest.mark.parametrize("dtype,name", DEVICE_IDS)
def test_route_and_bits(dtype, name):
    from pyamg_amd import _lib
    c = sc.cases(dtype)[name]
    want_rc, want = sc.predicted(dtype, name)
    live = _lib.live_buffers()
    rc, out = _device_product(c.A, c.B, dtype)
    rec = _lib.spgemm_last_route()
    assert _lib.live_buffers() == live
    assert rc == want_rc and rec == want, (rc, rec)
    if rc != 0:
        # refused by the bound computed on the host: the guard's own message, no error of the runtime behind it
        assert rc == _lib.AMG_EINVAL and b"too large for per-thread tables" in _lib.lib().amg_last_error()
        return
    Cp, Cj, Cx = out
    Rp, Rj, Rx = sc.reference(dtype, name)
    assert np.array_equal(Cp, Rp)
    assert np.array_equal(Cj, Rj)
    assert Cx.tobytes() == Rx.tobytes()         # every bit: signs of zeros, and the NaNs that inf * 0 and inf - inf create


# --------------------------------------------------------------------------------------------- duplicate columns
def _with_duplicates(A, seed):
    """A (CSR, sorted) with one stored entry of every third row split in two entries of the same column, next to each
    other; the rows stay sorted, the matrix they sum to is A (the halves are exact)"""
    A = sps.csr_matrix(A).copy()
    A.sort_indices()
    rng = np.random.RandomState(seed)
    rows = []
    for i in range(A.shape[0]):
        lo, hi = A.indptr[i], A.indptr[i + 1]
        cols, vals = A.indices[lo:hi].tolist(), A.data[lo:hi].tolist()
        if i % 3 == 0 and hi > lo:
            k = int(rng.randint(0, hi - lo))
            cols.insert(k, cols[k])
            vals[k] = vals[k] * 0.5
            vals.insert(k, vals[k])
        rows.append((cols, vals))
    indptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.intc)
    M = sps.csr_matrix((np.array([v for r in rows for v in r[1]], dtype=A.dtype),
                        np.array([c for r in rows for c in r[0]], dtype=np.intc), indptr), shape=A.shape)
    assert M.has_sorted_indices and not M.has_canonical_format and abs(M - A).max() == 0
    return M


def _bits(M):
    M = sps.csr_matrix(M)
    return M.indptr.tobytes(), M.indices.tobytes(), np.ascontiguousarray(M.data).tobytes()


def test_float64_operator_with_duplicate_columns_keeps_the_host_products(monkeypatch):
    """smoothed_aggregation_solver on an operator that stores a column twice in a row: level 0's Galerkin product is
    not handed to the device (util.galerkin_device is not called for it), the coarse operator has scipy's bits for
    (R A) P on the operator as stored, the hierarchy equals the one built with the device products switched off, and the
    coarser levels -- products, each column once -- do go through the device"""
    import pyamg_amd
    from pyamg_amd import util
    from pyamg_amd.aggregation import poisson
    A = _with_duplicates(poisson((20, 20, 20)), seed=1)
    monkeypatch.setattr(util, "DEVICE_RHO_MIN_ROWS", 100)
    calls = []
    orig = util.galerkin_device

    def counted(A_, R, P, n_coarse):
        out = orig(A_, R, P, n_coarse)
        calls.append((A_.shape[0], out is not None))
        return out
    monkeypatch.setattr(util, "galerkin_device", counted)
    built = {}
    for env in ("1", "0"):
        monkeypatch.setenv("AMG_SETUP_DEVICE_GALERKIN", env)
        np.random.seed(0)
        built[env] = pyamg_amd.smoothed_aggregation_solver(A.copy(), max_coarse=50)
        if env == "1":
            assert calls and all(ok for _, ok in calls), calls           # coarser levels: device products
            assert all(n < A.shape[0] for n, _ in calls), calls         # level 0: never handed over
            n_calls = len(calls)
    assert len(calls) == n_calls                                        # switched off: no call at all
    dev, host = built["1"], built["0"]
    assert len(dev.levels) == len(host.levels) >= 3
    for ld, lh in zip(dev.levels, host.levels):
        assert _bits(ld.A) == _bits(lh.A)
    l0 = dev.levels[0]
    stored = sps.csr_matrix((l0.A.data.reshape(-1), l0.A.indices, l0.A.indptr), shape=l0.A.shape)
    assert not stored.has_canonical_format                              # still the operator as handed in
    ref = (sps.csr_matrix(l0.R) @ stored) @ sps.csr_matrix(l0.P)
    ref.sort_indices()                      # (level 1's own extension sorted its rows in place, as the reference does)
    assert _bits(dev.levels[1].A) == _bits(ref)


def test_complex128_operator_with_duplicate_columns_keeps_scipys_products(monkeypatch):
    """aggregation._galerkin_c128_device: an operator with a column twice in a row is declined before anything is handed
    to the device (the caller then forms R * A * P with scipy); the same operator without the duplicates goes through
    the device and has scipy's bits"""
    import c128_cycle
    from pyamg_amd import aggregation, util
    g = c128_cycle.load("cheb2_magnetic3d")
    A, P, R = (sps.csr_matrix(g["levels"][0][k]) for k in ("A", "P", "R"))
    monkeypatch.setattr(util, "DEVICE_RHO_MIN_ROWS", 1)
    monkeypatch.setattr(util, "DEVICE_GALERKIN_C128_MIN_ROWS", 1)
    monkeypatch.setenv("AMG_SETUP_DEVICE_GALERKIN", "1")
    calls = []
    orig = util.galerkin_device

    def counted(*a):
        calls.append(1)
        return orig(*a)
    monkeypatch.setattr(util, "galerkin_device", counted)
    Ac = aggregation._galerkin_c128_device(R, A, P)
    assert calls == [1] and Ac is not None
    assert _bits(Ac) == _bits((R @ A) @ P)
    D = _with_duplicates(A, seed=2)
    assert aggregation._galerkin_c128_device(R, D, P) is None and calls == [1]
    U = (R @ A) @ P                                                     # unsorted, each column once: goes through
    assert not U.has_sorted_indices and aggregation._columns_once(U)
    assert not aggregation._columns_once(D) and aggregation._columns_once(A)
