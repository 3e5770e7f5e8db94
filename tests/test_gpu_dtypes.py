"""float32 / complex64 / complex128 flat table on the GPU: bit-exact against fixtures recorded from the
reference's own compiled kernels (tools/gen_golden_dtypes.py) and, at sizes that span many workgroups and
wide dependency levels, live against the reference's native module when it has been built."""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import scipy.sparse as sps

from pyamg_amd import amg_core, relaxation

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DTYPES = {"f32": np.float32, "c64": np.complex64, "c128": np.complex128}


def bit_mismatches(a, b):
    """entries whose bits differ (so -0.0 against +0.0 counts); a NaN matches any NaN: the sign and payload of a
    NaN that an invalid operation creates are the processor's (x86 and CDNA make different ones)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    real = np.float32 if a.dtype in (np.float32, np.complex64) else np.float64
    u = np.uint32 if real == np.float32 else np.uint64
    ra, rb = a.view(real).reshape(len(a), -1), b.view(real).reshape(len(b), -1)
    differ = (ra.view(u) != rb.view(u)) & ~(np.isnan(ra) & np.isnan(rb))
    return int(np.count_nonzero(differ.any(axis=1)))


def same_bits(a, b):
    return bit_mismatches(a, b) == 0


def _load(name):
    return np.load(os.path.join(GOLDEN, name))


KERNELS = _load("kernels_dtypes.npz")
DIVISION = _load("division_dtypes.npz")
RELAX = _load("relaxation_dtypes.npz")


def run_recorded(z, case):
    call = json.loads(str(z[case + "__call"]))
    live = {a[1]: z[a[2]].copy() for a in call["args"] if a[0] == "a"}
    getattr(amg_core, call["fn"])(*[live[a[1]] if a[0] == "a" else a[1] for a in call["args"]])
    assert call["out"], case
    for name, key in call["out"].items():
        want = z[key]
        bad = bit_mismatches(live[name], want)
        assert bad == 0, "%s: %s differs in %d of %d entries" % (case, name, bad, len(want))


@pytest.mark.parametrize("case", [str(c) for c in KERNELS["cases"]])
def test_kernel_bit_exact_vs_reference(case):
    run_recorded(KERNELS, case)


@pytest.mark.parametrize("case", [str(c) for c in DIVISION["cases"]])
def test_division_sweep_bit_exact(case):
    run_recorded(DIVISION, case)


def _relax_system(tag, sname, fmt):
    k = "system_%s@%s" % (sname, tag)
    A = sps.csr_matrix((RELAX[k + "__data"], RELAX[k + "__indices"], RELAX[k + "__indptr"]))
    if fmt == "bsr2":
        A = A.tobsr(blocksize=(2, 2))
    return A


@pytest.mark.parametrize("case", [str(c) for c in RELAX["cases"]])
def test_relaxation_bit_exact_vs_reference(case):
    meta = json.loads(str(RELAX[case + "__call"]))
    A = _relax_system(meta["dtype"], meta["system"], meta["fmt"])
    if meta["fn"] == "gauss_seidel_nr":
        A = A.tocsc()
    x = RELAX[case + "__x0"].copy()
    b = RELAX[case + "__b"].copy()
    kw = dict(meta["kwargs"])
    prefix = case + "__kw_"
    for k in RELAX.files:
        if k.startswith(prefix):
            kw[k[len(prefix):]] = RELAX[k]
    args = meta["args"]        # lists stay lists: coefficients are Python floats there, as in the reference's call
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        getattr(relaxation, meta["fn"])(A, x, b, *args, **kw)
    assert same_bits(x, RELAX[case + "__x"]), case


def test_single_precision_loop():
    """relaxation/tests/test_relaxation.py:36-42 on our functions (plus the normal-equation sweeps)"""
    A = sps.diags([-np.ones(3), 2 * np.ones(4), -np.ones(3)], [-1, 0, 1], format="csr").astype("float32")
    cases = [(relaxation.gauss_seidel, (), {}), (relaxation.jacobi, (), {}), (relaxation.block_jacobi, (), {}),
             (relaxation.block_gauss_seidel, (), {}), (relaxation.jacobi_ne, (), {}), (relaxation.schwarz, (), {}),
             (relaxation.sor, (0.5,), {}), (relaxation.gauss_seidel_indexed, ([1, 0],), {}),
             (relaxation.polynomial, ([0.6, 0.1],), {}), (relaxation.gauss_seidel_ne, (), {}),
             (relaxation.gauss_seidel_nr, (), {})]
    for method, args, kwargs in cases:
        b = np.arange(A.shape[0], dtype="float32")
        x = 0 * b
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            method(A.copy(), x, b, *args, **kwargs)
        assert x.dtype == np.float32 and np.all(np.isfinite(x)) and np.any(x != 0), method.__name__


# ------------------------------------------------------------------ live, larger, against the reference module
def _reference_core():
    path = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(path, "_amg_core.so")):
        pytest.skip("the reference's native module (oracle/_ref) has not been built here")
    if path not in sys.path:
        sys.path.insert(0, path)
    import _amg_core
    return _amg_core


def _cplx(v, dt, rng):
    v = np.asarray(v, dtype=np.float64)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.randn(*v.shape)
    return np.ascontiguousarray(v.astype(dt))


def _shifted_poisson(m, dt, rng):
    T = sps.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    A = sps.kronsum(T, T).tocsr()
    A = (A + (0.3 + 0.5j if np.dtype(dt).kind == "c" else 0.3) * sps.identity(m * m)).tocsr()
    A.sort_indices()
    A = A.astype(dt)
    A.data = (A.data + _cplx(0.01 * rng.randn(A.nnz), dt, rng)).astype(dt)
    A.indices = A.indices.astype(np.intc); A.indptr = A.indptr.astype(np.intc)
    return A


@pytest.mark.parametrize("tag", list(DTYPES))
def test_poisson_300_live_vs_reference(tag):
    ref = _reference_core()
    dt = DTYPES[tag]
    rng = np.random.RandomState(300)
    A = _shifted_poisson(300, dt, rng)
    n = A.shape[0]
    x0, b = _cplx(rng.randn(n), dt, rng), _cplx(rng.randn(n), dt, rng)
    for rs, re, rt in ((0, n, 1), (n - 1, -1, -1)):
        xr, xg = x0.copy(), x0.copy()
        ref.gauss_seidel(A.indptr, A.indices, A.data, xr, b, rs, re, rt)
        amg_core.gauss_seidel(A.indptr, A.indices, A.data, xg, b, rs, re, rt)
        assert same_bits(xg, xr), (tag, rt)
    w = np.array([0.7], dtype=dt)
    xr, xg, tr, tg = x0.copy(), x0.copy(), np.zeros(n, dt), np.zeros(n, dt)
    ref.jacobi(A.indptr, A.indices, A.data, xr, b, tr, 0, n, 1, w)
    amg_core.jacobi(A.indptr, A.indices, A.data, xg, b, tg, 0, n, 1, w)
    assert same_bits(xg, xr) and same_bits(tg, tr)
    y0 = _cplx(rng.randn(n), dt, rng)
    yr, yg = y0.copy(), y0.copy()
    sps._sparsetools.csr_matvec(n, n, A.indptr, A.indices, A.data, x0, yr)
    amg_core.csr_matvec(n, n, A.indptr, A.indices, A.data, x0, yg)
    assert same_bits(yg, yr)


@pytest.mark.parametrize("tag", list(DTYPES))
def test_bsr3_100k_live_vs_reference(tag):
    ref = _reference_core()
    dt = DTYPES[tag]
    rng = np.random.RandomState(3)
    nb, bs = 33334, 3
    S = sps.random(nb, nb, density=4.0 / nb, random_state=rng, format="csr")
    S = (S + S.T + sps.identity(nb)).tocsr()
    S.sort_indices()
    data = _cplx(rng.randn(S.nnz * bs * bs), dt, rng).reshape(S.nnz, bs, bs)
    Ap, Aj = S.indptr.astype(np.intc), S.indices.astype(np.intc)
    for i in range(nb):                                    # dominant diagonal blocks
        for jj in range(Ap[i], Ap[i + 1]):
            if Aj[jj] == i:
                data[jj] += (8.0 * bs * (Ap[i + 1] - Ap[i]) * np.eye(bs)).astype(dt)
    Ax = np.ascontiguousarray(data.ravel())
    n = nb * bs
    x0, b = _cplx(rng.randn(n), dt, rng), _cplx(rng.randn(n), dt, rng)
    diag_at = np.array([jj for i in range(nb) for jj in range(Ap[i], Ap[i + 1]) if Aj[jj] == i])
    Dinv = np.ascontiguousarray(np.linalg.inv(data[diag_at]).astype(dt).ravel())
    for rs, re, rt in ((0, nb, 1), (nb - 1, -1, -1)):
        xr, xg = x0.copy(), x0.copy()
        ref.bsr_gauss_seidel(Ap, Aj, Ax, xr, b, rs, re, rt, bs)
        amg_core.bsr_gauss_seidel(Ap, Aj, Ax, xg, b, rs, re, rt, bs)
        assert same_bits(xg, xr), (tag, "bsr_gauss_seidel", rt)
        xr, xg = x0.copy(), x0.copy()
        ref.block_gauss_seidel(Ap, Aj, Ax, xr, b, Dinv, rs, re, rt, bs)
        amg_core.block_gauss_seidel(Ap, Aj, Ax, xg, b, Dinv, rs, re, rt, bs)
        assert same_bits(xg, xr), (tag, "block_gauss_seidel", rt)
    yr, yg = np.zeros(n, dt), np.zeros(n, dt)
    sps._sparsetools.bsr_matvec(nb, nb, bs, bs, Ap, Aj, Ax, x0, yr)
    amg_core.bsr_matvec(nb, nb, bs, bs, Ap, Aj, Ax, x0, yg)
    assert same_bits(yg, yr)
