"""complex128 setup on the MI355X: the Galerkin products of csrc/spgemm.hip instantiated for complex128 against
scipy's csr_matmat bit for bit (row pointer, unsorted column order, both parts of every value, -0.0 != +0.0), and
smoothed_aggregation_solver on a complex operator end to end -- device products and scipy products give the same
bytes, and the hierarchy solves on the resident complex128 engine."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import c128_cycle
import golden_io

pytestmark = pytest.mark.gpu


def _arrays(M):
    M = sps.csr_matrix(M)
    return (np.ascontiguousarray(M.indptr, dtype=np.int64), np.ascontiguousarray(M.indices, dtype=np.intc),
            np.ascontiguousarray(M.data, dtype=np.complex128))


def _device_matmat(A, B):
    from pyamg_amd import _lib
    L = _lib.lib()
    A = sps.csr_matrix(A); B = sps.csr_matrix(B)
    (Ap, Aj, Ax), (Bp, Bj, Bx) = _arrays(A), _arrays(B)
    Cp = np.empty(A.shape[0] + 1, dtype=np.int64)
    g = C.c_void_p()
    _lib.check(L.amg_csr_matmat_device_c128(A.shape[0], A.shape[1], B.shape[1], Ap.ctypes.data, Aj.ctypes.data,
                                            Ax.ctypes.data, Bp.ctypes.data, Bj.ctypes.data, Bx.ctypes.data,
                                            Cp.ctypes.data, C.byref(g)))
    Cj = np.empty(int(Cp[-1]), dtype=np.intc); Cx = np.empty(int(Cp[-1]), dtype=np.complex128)
    # the float64 fetch refuses a complex product and leaves it in place
    assert L.amg_galerkin_fetch(g, Cj.ctypes.data, Cx.ctypes.data) == _lib.AMG_EINVAL
    _lib.check(L.amg_galerkin_fetch_c128(g, Cj.ctypes.data, Cx.ctypes.data))
    return Cp, Cj, Cx


def _assert_scipys_bits(A, B, what):
    A = sps.csr_matrix(A, dtype=np.complex128); B = sps.csr_matrix(B, dtype=np.complex128)
    Cp, Cj, Cx = _device_matmat(A, B)
    ref = A @ B
    assert ref.dtype == np.complex128
    assert np.array_equal(Cp, ref.indptr), what
    assert np.array_equal(Cj, ref.indices), what
    assert Cx.tobytes() == np.ascontiguousarray(ref.data).tobytes(), what        # both parts, the sign of zero included
    return ref


def _rnd(rng, n, m, k):
    rows = np.repeat(np.arange(n), k); cols = rng.randint(0, m, size=n * k)
    M = sps.csr_matrix((rng.randn(n * k) + 1j * rng.randn(n * k), (rows, cols)), shape=(n, m))
    M.sum_duplicates()
    return M


def test_device_csr_matmat_c128_is_scipys_bit_for_bit():
    """The operand shapes of test_gpu_parity.py::test_device_csr_matmat_is_scipys_bit_for_bit with randn + 1j randn
    values.  Complex tables hold 2048 entries per wave and the lane groups are one step wider than in float64:
      rnd(300,200,5) x rnd(200,150,4), Poisson^2, the unsorted operand   16 lanes per row, tables in LDS
      rnd(1000,50,3) x rnd(50,4000,40)                                    64 lanes per row (right-hand rows of 40)
      mixed x rnd(200,5000,20)                                            32 lanes per row overflow (~550 distinct
                                                                          columns > 480), redone one wave per row
      long x rnd(100,100000,100)   rows of 1000 products with ~995 distinct columns: more than the wave's table
                                   takes (960) but not over 1024 products, so one thread per row with tables in
                                   HBM -- the short rows in the 256-entry tables, the long ones in the large ones
    (the routes as amg_spgemm_last_route records them; tests/test_gpu_spgemm_routes.py asserts the record on small cases)
    plus cancellation in the real part only (entry kept, with the zero as computed), in both parts (entry dropped),
    stored (-0.0, 0.0) entries, an empty matrix (5 x 7 without entries), a left operand without rows and empty rows."""
    from pyamg_amd.aggregation import poisson as native
    rng = np.random.RandomState(5)
    cases = [("random", _rnd(rng, 300, 200, 5), _rnd(rng, 200, 150, 4)),
             ("wide right rows", _rnd(rng, 1000, 50, 3), _rnd(rng, 50, 4000, 40)),
             ("empty matrix", sps.csr_matrix((5, 7), dtype=np.complex128), _rnd(rng, 7, 3, 2)),
             ("no rows", sps.csr_matrix((0, 7), dtype=np.complex128), _rnd(rng, 7, 3, 2))]
    Pn = native((17, 19, 13)).astype(np.complex128)
    Pn.data = Pn.data * np.exp(1j * rng.uniform(-np.pi, np.pi, size=Pn.nnz))
    cases.append(("7-point", Pn, Pn))
    # unsorted left operand (the product of two others, as scipy leaves it)
    U = _rnd(rng, 400, 300, 6) @ _rnd(rng, 300, 350, 5)
    assert not U.has_sorted_indices
    cases.append(("unsorted", U, _rnd(rng, 350, 200, 4)))
    # empty rows in both operands
    E = sps.vstack([_rnd(rng, 40, 60, 3), sps.csr_matrix((25, 60)), _rnd(rng, 40, 60, 2)]).tocsr()
    F = sps.vstack([_rnd(rng, 30, 80, 4), sps.csr_matrix((30, 80))]).tocsr()
    cases.append(("empty rows", E, F))
    mixed = sps.vstack([_rnd(rng, 500, 200, 2), _rnd(rng, 300, 200, 30), _rnd(rng, 200, 200, 1)]).tocsr()
    cases.append(("mixed", mixed, _rnd(rng, 200, 5000, 20)))
    long_rows = sps.vstack([_rnd(rng, 300, 100, 2), _rnd(rng, 40, 100, 10), _rnd(rng, 100, 100, 1)]).tocsr()
    assert np.diff(long_rows.indptr).max() == 10
    cases.append(("one thread per row", long_rows, _rnd(rng, 100, 100000, 100)))
    for what, A, B in cases:
        _assert_scipys_bits(A, B, what)
    # products that cancel in the real part only: the entry stays, its real part the +0.0 the sum gave
    Z = sps.csr_matrix(np.array([[1.0, -1.0, 0.0], [2.0, 0.0, 1.0]], dtype=np.complex128))
    W = sps.csr_matrix(np.array([[3.0 + 4.0j, 4.0], [3.0 + 5.0j, 4.0], [0.0, 5.0j]]))
    ref = _assert_scipys_bits(Z, W, "real part cancels")
    assert ref[0].nnz == 1 and ref[0].data[0].real == 0.0 and ref[0].data[0].imag == -1.0
    # the same with the imaginary part, and with both: (0, 0) is dropped as scipy drops it
    W2 = sps.csr_matrix(np.array([[3.0 + 4.0j, 4.0j], [5.0 + 4.0j, 4.0j], [0.0, 5.0]]))
    ref = _assert_scipys_bits(Z, W2, "imaginary part cancels")
    assert ref[0].nnz == 1 and ref[0].data[0] == -2.0
    W3 = sps.csr_matrix(np.array([[3.0 + 4.0j, 4.0 - 1.0j], [3.0 + 4.0j, 4.0 - 1.0j], [0.0, 5.0]]))
    ref = _assert_scipys_bits(Z, W3, "both parts cancel")
    assert ref[0].nnz == 0 and ref.nnz == 2
    # stored (-0.0, 0.0) entries in either operand: their products are signed zeros that enter the sums
    N = _rnd(rng, 200, 120, 4)
    N.data[::3] = complex(-0.0, 0.0)
    M2 = _rnd(rng, 120, 90, 3)
    M2.data[1::4] = complex(-0.0, 0.0)
    assert np.signbit(N.data.real[0]) and N.nnz == len(N.data)
    _assert_scipys_bits(N, M2, "stored negative zeros")
    _assert_scipys_bits(N, _rnd(rng, 120, 90, 3), "stored negative zeros on the left")


def test_device_csr_matmat_c128_long_rows_and_every_lane_group_width():
    """The shapes of test_gpu_parity.py::test_device_csr_matmat_long_rows_one_wave_per_row: rows of ~2000 products with
    ~730 distinct columns go one wave per row with the table in LDS (it takes 960); ~2700 distinct columns move the
    row's table to HBM; right-hand rows of ~5, ~14, ~30 and ~60 entries select 16 / 32 / 64 / 64 lanes per row."""
    rng = np.random.RandomState(11)
    A = _rnd(rng, 40000, 500, 40)
    _assert_scipys_bits(A, _rnd(rng, 500, 800, 50), "one wave per row")
    _assert_scipys_bits(A[:6000], _rnd(rng, 500, 60000, 70), "tables in HBM")
    for kb in (5, 14, 30, 60):
        lens = rng.randint(0, 9, size=30000)
        rows = np.repeat(np.arange(30000), lens); cols = rng.randint(0, 400, size=rows.size)
        A2 = sps.csr_matrix((rng.randn(rows.size) + 1j * rng.randn(rows.size), (rows, cols)), shape=(30000, 400))
        A2.sum_duplicates()
        _assert_scipys_bits(A2, _rnd(rng, 400, 300, kb), kb)


@pytest.mark.parametrize("case", ["cheb2_magnetic3d", "gs_sym_V_shifted2d"])
def test_device_galerkin_c128_equals_scipy(case):
    """util.galerkin_device (amg_galerkin_device_c128: R*A stays in HBM) = (R @ A) @ P by scipy, bit for bit, on levels 0
    and 1 of a Hermitian and of a complex symmetric fixture"""
    from pyamg_amd import util
    g = c128_cycle.load(case)
    for l in (0, 1):
        A, P, R = (sps.csr_matrix(g["levels"][l][k]) for k in ("A", "P", "R"))
        out = util.galerkin_device(_arrays(A), _arrays(R), _arrays(P), P.shape[1])
        assert out is not None
        Cp, Cj, Cx = out
        ref = (R @ A) @ P
        assert np.array_equal(Cp, ref.indptr) and np.array_equal(Cj, ref.indices)
        assert Cx.dtype == np.complex128 and Cx.tobytes() == np.ascontiguousarray(ref.data).tobytes()
        nxt = sps.csr_matrix(g["levels"][l + 1]["A"])
        assert np.array_equal(ref.indptr, nxt.indptr)         # and it is the next level's operator


def test_device_candidate_improvement_c128_equals_the_host_sweeps(monkeypatch):
    """aggregation._improve on a complex operator at or above the size gate runs the flat complex128 entries on the
    device -- once per candidate, counted at pyamg_amd.relaxation, so that a quiet return to the host loop fails --
    and below the gate it does not touch them; both give the same bits, point and block"""
    from pyamg_amd import aggregation, relaxation, util
    calls = []

    def spy(name):
        orig = getattr(relaxation, name)

        def counted(*a, **kw):
            calls.append(name)
            return orig(*a, **kw)
        monkeypatch.setattr(relaxation, name, counted)
    spy("gauss_seidel")
    spy("block_gauss_seidel")
    # (a block sweep with blocks of one entry is the point sweep, as in smoothing.setup_block_gauss_seidel)
    for case, method, entry in (
            ("cheb2_magnetic3d", ("block_gauss_seidel", {"sweep": "symmetric", "iterations": 4}), "gauss_seidel"),
            ("bsr_bjac_gs", ("block_gauss_seidel", {"sweep": "symmetric", "iterations": 2}), "block_gauss_seidel"),
            ("gs_sym_V_shifted2d", ("gauss_seidel", {"sweep": "backward", "iterations": 1}), "gauss_seidel")):
        A = c128_cycle.load(case)["levels"][0]["A"]
        rng = np.random.RandomState(2)
        B = rng.rand(A.shape[0], 2) + 1j * rng.rand(A.shape[0], 2)
        del calls[:]
        monkeypatch.setattr(util, "DEVICE_RHO_MIN_ROWS", 10 ** 9)
        host = aggregation._improve(method, A, B)
        assert calls == [], case                                 # below the gate: the host sweeps alone
        monkeypatch.setattr(util, "DEVICE_RHO_MIN_ROWS", 1)
        dev = aggregation._improve(method, A, B)
        assert calls == [entry] * B.shape[1], (case, calls)      # one device call per candidate
        assert host.dtype == dev.dtype == np.complex128
        assert dev.tobytes() == host.tobytes(), case
        assert not np.array_equal(dev, B)                        # and the sweeps did something


def _magnetic3d(n, shift, seed):
    rng = np.random.RandomState(seed)
    T = sps.diags([np.ones(n - 1), np.ones(n - 1)], [-1, 1], format="csr")
    I = sps.identity(n, format="csr")
    G = (sps.kron(sps.kron(T, I), I) + sps.kron(sps.kron(I, T), I) + sps.kron(sps.kron(I, I), T)).tocoo()
    up = G.row < G.col
    r, c = G.row[up], G.col[up]
    ph = np.exp(1j * rng.uniform(-np.pi, np.pi, size=r.size))
    N = n ** 3
    W = sps.coo_matrix((np.concatenate([ph, ph.conj()]), (np.concatenate([r, c]), np.concatenate([c, r]))),
                       shape=(N, N)).tocsr()
    deg = np.asarray(abs(W).sum(axis=1)).ravel()
    A = (sps.diags(deg + shift) - W).tocsr().astype(np.complex128)
    A.sort_indices()
    return A


def test_setup_and_solve_end_to_end(monkeypatch):
    """40^3 magnetic Laplacian (64 000 unknowns): the hierarchy built with the Galerkin products on the device has the
    bytes of the one built with scipy's products, and ml.solve converges on the resident complex128 engine; where the
    reference's compiled kernels are present the first two iterates are the host restatement's, bit for bit"""
    import pyamg_amd
    from pyamg_amd import aggregation, util
    A = _magnetic3d(40, 0.05, seed=3)
    cheb = ("chebyshev", {"degree": 2})
    monkeypatch.setattr(util, "DEVICE_RHO_MIN_ROWS", 1000)
    monkeypatch.setattr(util, "DEVICE_GALERKIN_C128_MIN_ROWS", 1000)
    ran = []
    orig = util.galerkin_device

    def counted(*a):
        out = orig(*a)
        ran.append(out is not None)
        return out
    monkeypatch.setattr(util, "galerkin_device", counted)
    built = {}
    for env in ("0", "1"):
        monkeypatch.setenv("AMG_SETUP_DEVICE_GALERKIN", env)
        np.random.seed(0)
        built[env] = pyamg_amd.smoothed_aggregation_solver(A.copy(), symmetry="hermitian", max_coarse=500,
                                                          presmoother=cheb, postsmoother=cheb)
        if env == "0":
            assert ran == []
    host, ml = built["0"], built["1"]
    assert len(ran) >= 2 and all(ran), ran                       # levels 0 and 1 went through the device
    assert len(ml.levels) == len(host.levels) >= 3
    for ld, lh in zip(ml.levels, host.levels):
        for name in ("A", "P", "R"):
            assert hasattr(ld, name) == hasattr(lh, name)
            if hasattr(lh, name):
                D, H = getattr(ld, name), getattr(lh, name)
                assert type(D) is type(H) and D.shape == H.shape and D.dtype == np.complex128
                assert D.indptr.dtype == H.indptr.dtype and D.indices.dtype == H.indices.dtype
                assert D.indptr.tobytes() == H.indptr.tobytes(), name
                assert D.indices.tobytes() == H.indices.tobytes(), name
                assert D.data.tobytes() == H.data.tobytes(), name
    rng = np.random.RandomState(5)
    b = rng.rand(A.shape[0]) + 1j * rng.rand(A.shape[0])
    res, its = [], []
    x = ml.solve(b, tol=1e-8, maxiter=40, residuals=res, callback=lambda xk: its.append(np.array(xk, copy=True)))
    assert x.dtype == np.complex128
    assert np.all(np.isfinite(res)) and len(res) >= 3
    assert res[-1] <= 1e-8 * res[0] or res[-1] <= 1e-8 * np.linalg.norm(b)
    assert len(res) - 1 < 40                                     # it reached the tolerance, not the iteration limit
    assert all(r1 < r0 for r0, r1 in zip(res[:-1], res[1:])), res
    assert np.linalg.norm(b - A @ x) <= 2e-8 * np.linalg.norm(b)
    core = c128_cycle.reference_core()
    if core is not None:
        kind, M = ml.coarse_solver.device_form(ml.levels[-1].A)
        assert kind == "dense"
        g = {"levels": [], "coarse": ("dense", {"M": np.ascontiguousarray(M, dtype=np.complex128)})}
        for lvl in ml.levels:
            L = {"A": lvl.A}
            if hasattr(lvl, "P"):
                L.update(P=lvl.P, R=lvl.R, pre=golden_io.canonical(dict(lvl.presmoother.desc)),
                         post=golden_io.canonical(dict(lvl.postsmoother.desc)))
            g["levels"].append(L)
        ref = c128_cycle.HostCycle(g, core).iterates(b, np.zeros_like(b), 2, "V")
        assert c128_cycle.bit_mismatches(its[0], ref[0]) == 0 and c128_cycle.bit_mismatches(its[1], ref[1]) == 0
