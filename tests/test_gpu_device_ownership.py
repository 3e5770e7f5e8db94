"""Device memory owns itself (csrc/driver.hpp, DevArr): whatever the library allocates while an object is built and used is
freed when the object goes.  amg_dev_live_buffers() counts the library's live device allocations over the whole process,
so every case is exact at tiny sizes: above `base` while the object lives, `base` again once it is closed.

Sizes are the smallest at which each storage form is still built; the form is asserted through the introspection entries.
The sliced BLOCK form needs 2^15 block rows, which no tetrahedral mesh of a few seconds reaches: it is built here from a
random block operator of that many block rows instead."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import evolution_io as eio
import test_gpu_sell_header as sell_header

pytestmark = pytest.mark.gpu

CHEB2 = ("chebyshev", {"degree": 2})
SGS = ("gauss_seidel", {"sweep": "symmetric"})


@pytest.fixture(scope="module")
def live():
    """the counter, after a warm-up that has built, used and closed one hierarchy"""
    from pyamg_amd import _lib
    from pyamg_amd.aggregation import poisson, smoothed_aggregation_solver
    L = _lib.lib()
    L.amg_hier_device_bytes.restype = C.c_long
    L.amg_hier_release_sources.restype = C.c_long
    np.random.seed(0)
    ml = smoothed_aggregation_solver(poisson((12, 12)), presmoother=SGS, postsmoother=SGS, max_coarse=10)
    ml.solve(np.ones(144), maxiter=2)
    ml._invalidate_device()
    return _lib.live_buffers


def _sa(grid, sm, **kw):
    from pyamg_amd.aggregation import poisson, smoothed_aggregation_solver
    np.random.seed(0)
    ml = smoothed_aggregation_solver(poisson(grid), presmoother=sm, postsmoother=sm, **kw)
    return ml, np.random.RandomState(1).rand(ml.levels[0].A.shape[0])


@pytest.fixture(scope="module")
def small2d():
    """one small 2-D SA hierarchy (576 -> ~100 -> ~12 unknowns) whose smoothers the cases change"""
    return _sa((24, 24), ("jacobi", {"omega": 4.0 / 3.0}), max_coarse=10)


def _lives_and_dies(live, ml, use):
    """build the device mirror of ml, use(dev), close: the count rises above base and returns to it"""
    base = live()
    dev = ml.device_hierarchy()
    try:
        built = live()
        assert built > base
        use(dev)
        assert live() >= built
    finally:
        ml._invalidate_device()
    assert live() == base
    return built - base


def test_level0_chain_forms(live):
    """poisson((20, 21, 22)), SA, Chebyshev degree 2: stencil form, value index, plane flags, fused level-0 chain; one
    solve and one W cycle"""
    from pyamg_amd import _lib
    L = _lib.lib()
    ml, b = _sa((20, 21, 22), CHEB2)

    def use(dev):
        assert L.amg_hier_operator_form(dev.h, 0) == 2
        assert L.amg_hier_value_index(dev.h, 0, -1) > 0
        assert L.amg_hier_level0_fused(dev.h) == 1
        assert L.amg_hier_level0_plane_reuse(dev.h) > 0
        res = []
        ml.solve(b, tol=1e-8, maxiter=20, residuals=res)
        assert res[-1] < res[0]
        ml.solve(b, tol=0.0, maxiter=1, cycle="W")
    _lives_and_dies(live, ml, use)


@pytest.mark.parametrize("flow", [0, None])
def test_level_ordered_gauss_seidel_copies(live, flow):
    """the same operator under symmetric Gauss-Seidel: the level-ordered copies with their chains and permuted numbering
    (amg_set_gs_flow(0)), and whatever the default keeps (the dataflow form beside or instead of them)"""
    from pyamg_amd import _lib
    L = _lib.lib()
    ml, b = _sa((20, 21, 22), SGS)
    plain, _ = _sa((20, 21, 22), None)
    try:
        if flow is not None:
            L.amg_set_gs_flow(flow)
        held = {}

        def use(dev):
            held["bytes"] = dev.device_bytes()
            res = []
            ml.solve(b, tol=1e-8, maxiter=30, residuals=res)
            assert res[-1] < res[0]
        nbuf = _lives_and_dies(live, ml, use)
        bare = {}
        nplain = _lives_and_dies(live, plain, lambda dev: bare.update(bytes=dev.device_bytes()))
        assert held["bytes"] > bare["bytes"] and nbuf > nplain          # the schedules' arrays are there and are counted
    finally:
        L.amg_set_gs_flow(1)


def test_sliced_form_with_16_bit_codes(live, monkeypatch):
    """the planted-width square operator of test_gpu_sell_header.py: sliced form, 16-bit codes (their bytes are in the
    accounting)"""
    from pyamg_amd import _lib
    L = _lib.lib()
    A = sell_header._square()
    nslices, entries, words, coded = sell_header._layout(A)
    base = live()
    L.amg_set_sell_form(1)
    L.amg_set_sell_index16(1)
    monkeypatch.setenv("AMG_SELL", "0")
    op = sell_header._Hier(A)
    plain, nplain = L.amg_hier_device_bytes(op.h), live() - base
    op.close()
    assert live() == base
    monkeypatch.delenv("AMG_SELL")
    op = sell_header._Hier(A)
    try:
        assert L.amg_hier_operator_form(op.h, 0) == 3
        assert L.amg_hier_device_bytes(op.h) - plain == 8 * 64 * nslices + 96 * nslices + 12 * entries + 4 * words
        assert live() - base == nplain + 5                  # slots, headers, columns, values, codes
        x = np.random.RandomState(3).randn(A.shape[0])
        assert np.array_equal(op.matvec(x), A @ x)
    finally:
        op.close()
    assert live() == base


def test_release_sources(live, monkeypatch):
    """amg_hier_release_sources on a small Chebyshev hierarchy: the count drops by the arrays released and is back at base
    after close"""
    from pyamg_amd import _lib
    L = _lib.lib()
    monkeypatch.setenv("AMG_RELEASE_SOURCES", "0")
    ml, b = _sa((20, 21, 22), CHEB2)
    base = live()
    dev = ml.device_hierarchy()
    try:
        before = live()
        freed = L.amg_hier_release_sources(dev.h)
        assert freed > 0 and before > live() > base
        res = []
        ml.solve(b, tol=1e-8, maxiter=20, residuals=res)
        assert res[-1] < res[0]
    finally:
        ml._invalidate_device()
    assert live() == base


@pytest.mark.parametrize("smoother", [("block_jacobi", {"omega": 1.0, "blocksize": 3}),
                                      ("block_gauss_seidel", {"sweep": "symmetric", "blocksize": 3})])
def test_bsr_level_own_blocks(live, smoother):
    """tet_diffusion(24) as BSR(3, 3), the smallest mesh of test_config5_*: the level operators live by their own
    blocks; block Gauss-Seidel through the block dataflow form"""
    from pyamg_amd.gallery import tet_diffusion
    from pyamg_amd.aggregation import smoothed_aggregation_solver
    A = tet_diffusion(24, blocksize=3, native=False)
    np.random.seed(0)
    ml = smoothed_aggregation_solver(A, presmoother=smoother, postsmoother=smoother, max_coarse=40)
    b = np.random.RandomState(5).rand(A.shape[0])

    def use(dev):
        assert np.array_equal(dev.matvec(0, 0, b), A * b)         # applied from the blocks: no scalar expansion is held
        res = []
        ml.solve(b, tol=0.0, maxiter=3, residuals=res)
        assert res[-1] < res[0]
    _lives_and_dies(live, ml, use)


def test_reblocked_smoother_copy(live, small2d):
    """a CSR level under a block smoother of block size 2: the smoother holds its own re-blocked copy of A"""
    import pyamg_amd
    ml, b = small2d
    if any(lvl.A.shape[0] % 2 for lvl in ml.levels[:-1]):
        ml, b = _sa((24, 24), None, max_coarse=300)               # two levels: 576 unknowns under the smoother
    sm = ("block_gauss_seidel", {"sweep": "symmetric", "blocksize": 2})
    pyamg_amd.change_smoothers(ml, sm, sm)
    plain, _ = _sa((24, 24), None, max_coarse=10)

    def use(dev):
        res = []
        ml.solve(b, tol=0.0, maxiter=3, residuals=res)
        assert res[-1] < res[0]
    assert _lives_and_dies(live, ml, use) > _lives_and_dies(live, plain, lambda dev: None)


def test_sliced_block_form(live, monkeypatch):
    """2^15 block rows of 3 x 3 blocks, 6..10 blocks each (the smallest operator that gets the sliced block form), block
    Jacobi from it"""
    from pyamg_amd import _lib
    L = _lib.lib()
    rng = np.random.RandomState(7)
    nb, bs = 1 << 15, 3
    lens = rng.randint(5, 10, size=nb)
    indptr = np.zeros(nb + 1, dtype=np.intc)
    np.cumsum(lens + 1, out=indptr[1:])
    cols = np.empty(indptr[-1], dtype=np.intc)
    for i in range(nb):
        off = rng.choice(np.arange(1, 200), size=lens[i], replace=False)
        cols[indptr[i]:indptr[i + 1]] = np.sort(np.concatenate([[i], (i + off) % nb]))
    data = 0.1 * rng.randn(indptr[-1], bs, bs)
    diag = np.flatnonzero(cols == np.repeat(np.arange(nb), lens + 1))
    data[diag] += 4.0 * np.eye(bs)
    A = sps.bsr_matrix((data, cols, indptr), shape=(nb * bs, nb * bs))
    Dinv = np.ascontiguousarray(np.linalg.inv(data[diag]))
    keep = [np.ascontiguousarray(A.indptr, dtype=np.intc), np.ascontiguousarray(A.indices, dtype=np.intc),
            np.ascontiguousarray(np.ravel(A.data))]

    def build():
        h = L.amg_hier_create(1, 0)
        assert h
        _lib.check(L.amg_hier_set_matrix(h, 0, 0, 1, A.shape[0], A.shape[1], bs, bs, keep[0].ctypes.data, keep[1].ctypes.data,
                                         keep[2].ctypes.data, 0))
        return h
    base = live()
    monkeypatch.setenv("AMG_SELL", "0")
    h = build()
    plain, nplain = L.amg_hier_device_bytes(h), live() - base
    L.amg_hier_destroy(h)
    assert live() == base
    monkeypatch.delenv("AMG_SELL")
    h = build()
    try:
        assert L.amg_hier_device_bytes(h) > plain + 8 * A.data.size          # the sliced block form holds the values again
        assert live() - base == nplain + 5                                   # block rows, lengths, offsets, columns, values
        d = _lib.SmootherDesc()
        d.kind, d.iterations, d.omega, d.blocksize, d.Dinv = 5, 1, 1.0, bs, _lib.dp(Dinv)
        _lib.check(L.amg_hier_set_smoother(h, 0, 0, d))
        _lib.check(L.amg_hier_finalize(h))
        b = rng.rand(A.shape[0])
        x = np.zeros(A.shape[0])
        _lib.check(L.amg_hier_relax(h, 0, 0, _lib.dp(b), _lib.dp(x)))
        assert np.allclose(x, np.einsum("kij,kj->ki", Dinv, b.reshape(nb, bs)).ravel(), rtol=1e-13, atol=0.0)
    finally:
        L.amg_hier_destroy(h)
    assert live() == base


@pytest.mark.parametrize("smoother", [("schwarz", {}),
                                      ("jacobi_ne", {}),
                                      ("gauss_seidel_ne", {"sweep": "symmetric"}),
                                      ("gauss_seidel_nr", {"sweep": "symmetric"}),
                                      ("multicolor_gauss_seidel", {"sweep": "symmetric"})])
def test_remaining_smoother_kinds(live, small2d, smoother):
    """Schwarz (subdomain arrays), the normal-equation family (aux[0..1], Dinv, task orders) and indexed Gauss-Seidel on
    the small 2-D hierarchy"""
    import pyamg_amd
    ml, b = small2d
    pyamg_amd.change_smoothers(ml, smoother, smoother)
    plain, _ = _sa((24, 24), None, max_coarse=10)

    def use(dev):
        res = []
        ml.solve(b, tol=0.0, maxiter=4, residuals=res)
        assert res[-1] < res[0]
    assert _lives_and_dies(live, ml, use) > _lives_and_dies(live, plain, lambda dev: None)


def _reset(small2d):
    import pyamg_amd
    ml, b = small2d
    jac = ("jacobi", {"omega": 4.0 / 3.0})
    pyamg_amd.change_smoothers(ml, jac, jac)
    return ml, b


def test_amli_cycle_lazy_vectors(live, small2d):
    """the first AMLI cycle allocates four vectors on every coarse level it visits"""
    ml, b = _reset(small2d)
    assert len(ml.levels) >= 3

    def use(dev):
        ml.solve(b, tol=0.0, maxiter=1)
        before = live()
        ml.solve(b, tol=0.0, maxiter=2, cycle="AMLI")
        assert live() == before + 4 * (len(ml.levels) - 2)          # levels 1 .. n - 2 run the AMLI branch for their coarse level
    _lives_and_dies(live, ml, use)


def test_device_pcg_vectors(live, small2d):
    ml, b = _reset(small2d)

    def use(dev):
        ml.solve(b, tol=0.0, maxiter=1)
        before = live()
        res = []
        ml.solve(b, tol=1e-8, maxiter=30, accel="cg", residuals=res)
        assert res[-1] < res[0]
        assert live() == before + 4
    _lives_and_dies(live, ml, use)


def test_history_regrowth(live, small2d):
    """a longer residual history replaces the shorter one: one buffer either way"""
    ml, b = _reset(small2d)

    def use(dev):
        ml.solve(b, tol=0.0, maxiter=2)
        before = live()
        res = []
        ml.solve(b, tol=0.0, maxiter=40, residuals=res)
        assert len(res) == 41 and live() == before
    _lives_and_dies(live, ml, use)


def test_arnoldi_workspace(live):
    from pyamg_amd import util
    from pyamg_amd.aggregation import poisson
    A = poisson((30, 20))
    base = live()
    op = util._DeviceOperator(A)
    try:
        held = live()
        assert held > base
        v0 = np.random.RandomState(2).rand(A.shape[0])
        H, steps, brk = op.arnoldi(None, v0, 10, 1e-10)
        assert steps == 10 and not brk
        assert live() > held                                          # basis, scaling, coefficients (and the norm scratch)
        grown = live()
        op.arnoldi(None, v0, 15, 1e-10)                               # a larger workspace replaces the smaller one
        assert live() == grown
        op.free_workspace()
        assert live() == grown - 3
    finally:
        op.close()
    assert live() == base


def test_amg_mat_and_its_schedules(live):
    from pyamg_amd import _lib
    from pyamg_amd.aggregation import poisson
    L = _lib.lib()
    A = poisson((12, 11, 10))
    Ap, Aj, Ax = A.indptr.astype(np.intc), A.indices.astype(np.intc), A.data.astype(np.float64)
    base = live()
    mat = L.amg_mat_create(0, A.shape[0], A.shape[1], _lib.ip(Ap), _lib.ip(Aj), _lib.dp(Ax))
    assert mat
    try:
        bare = live()
        assert bare > base
        _lib.check(L.amg_mat_build_gs(mat, None, 0))
        once = live()
        assert once > bare and L.amg_mat_gs_levels(mat) > 1
        _lib.check(L.amg_mat_build_gs(mat, None, 0))              # the second schedule replaces the first
        assert live() == once
    finally:
        L.amg_mat_destroy(mat)
    assert live() == base


def _matmat_operands():
    """test_device_csr_matmat_is_scipys_bit_for_bit: its cancelling 2 x 3 by 3 x 2 pair and its first random pair"""
    rng = np.random.RandomState(5)

    def rnd(n, m, k):
        rows = np.repeat(np.arange(n), k)
        M = sps.csr_matrix((rng.randn(n * k), (rows, rng.randint(0, m, size=n * k))), shape=(n, m))
        M.sum_duplicates()
        return M
    Z = sps.csr_matrix(np.array([[1.0, -1.0, 0.0], [2.0, 0.0, 1.0]]))
    W = sps.csr_matrix(np.array([[3.0, 4.0], [3.0, 4.0], [0.0, 5.0]]))
    return [(Z, W), (rnd(300, 200, 5), rnd(200, 150, 4))]


def test_galerkin_products(live):
    from pyamg_amd import _lib, util
    L = _lib.lib()
    base = live()
    for A, B in _matmat_operands():
        Ap, Aj, Ax = A.indptr.astype(np.int64), A.indices.astype(np.intc), A.data.astype(np.float64)
        Bp, Bj, Bx = B.indptr.astype(np.int64), B.indices.astype(np.intc), B.data.astype(np.float64)
        Cp = np.empty(A.shape[0] + 1, dtype=np.int64)
        g = C.c_void_p()
        _lib.check(L.amg_csr_matmat_device(A.shape[0], A.shape[1], B.shape[1], Ap.ctypes.data, Aj.ctypes.data, Ax.ctypes.data,
                                           Bp.ctypes.data, Bj.ctypes.data, Bx.ctypes.data, Cp.ctypes.data, C.byref(g)))
        assert live() == base + 3                                     # the product waits for its fetch; operands and tables are gone
        Cj = np.empty(int(Cp[-1]), dtype=np.intc)
        Cx = np.empty(int(Cp[-1]))
        _lib.check(L.amg_galerkin_fetch(g, Cj.ctypes.data, Cx.ctypes.data))
        ref = A @ B
        assert np.array_equal(Cp, ref.indptr) and np.array_equal(Cj, ref.indices) and np.array_equal(Cx, ref.data)
        assert live() == base
    # R A P with A taken from a device operator
    A, P = _matmat_operands()[1][0][:200, :200].tocsr(), _matmat_operands()[1][1]
    A = sps.csr_matrix(A + A.T + sps.identity(200))
    R = sps.csr_matrix(P.T)
    op = util.device_operator(A)
    try:
        held = live()
        trip = lambda M: (M.indptr.astype(np.int64), M.indices.astype(np.intc), M.data.astype(np.float64))
        out = util.galerkin_device(A, trip(R), trip(P), R.shape[0])
        assert out is not None
        ref = (R @ A) @ P
        assert np.array_equal(out[0], ref.indptr) and np.array_equal(out[1], ref.indices) and np.array_equal(out[2], ref.data)
        assert live() == held
    finally:
        util.release_device_operator(A)
    assert live() == base


def test_evolution_strength(live):
    from pyamg_amd.strength import evolution_strength_of_connection
    p = eio.problem("aniso_40x40")
    base = live()
    S = evolution_strength_of_connection(p["A"], p["B"], epsilon=p["epsilon"], k=2, rho=p[2]["rho"], device=True)
    eio.same_bits(S, p[2]["C"])
    assert live() == base


def test_failed_finalize(live):
    """a two-level hierarchy is finalised (its vectors exist), then P_0 is replaced by one with a row too many: finalize
    returns AMG_EINVAL and destroy frees everything"""
    from pyamg_amd import _lib
    L = _lib.lib()
    ml, b = _sa((12, 12), None, max_coarse=30)
    assert len(ml.levels) == 2
    base = live()
    dev = ml.device_hierarchy()
    try:
        good = live()
        P = ml.levels[0].P
        bad = sps.vstack([P, sps.csr_matrix((1, P.shape[1]))]).tocsr()
        dev._set_matrix(0, 1, bad)
        assert L.amg_hier_finalize(dev.h) == -1                       # AMG_EINVAL
        assert b"inconsistent" in L.amg_last_error()
        assert live() >= good - 3                                     # level-0 vectors and the other operators are still held
    finally:
        ml._invalidate_device()
    assert live() == base


def test_flat_table_sweeps(live):
    """amgcore_gauss_seidel_f64 and amgcore_bsr_gauss_seidel_f64 build a schedule, sweep and free it"""
    from pyamg_amd import amg_core
    from pyamg_amd.aggregation import poisson
    A = poisson((9, 8))
    n = A.shape[0]
    rng = np.random.RandomState(4)
    b = rng.rand(n)
    base = live()
    x = rng.rand(n)
    x0 = x.copy()
    amg_core.gauss_seidel(A.indptr, A.indices, A.data, x, b, 0, n, 1)
    assert live() == base and not np.array_equal(x, x0)
    Ab = A.tobsr(blocksize=(2, 2))
    x = x0.copy()
    amg_core.bsr_gauss_seidel(Ab.indptr, Ab.indices, np.ravel(Ab.data), x, b, 0, n // 2, 1, 2)
    assert live() == base and not np.array_equal(x, x0)


def _small_operator():
    """Poisson 6 x 6 (36 rows), a checkerboard splitting and a random 48-row R, A, P triple"""
    from pyamg_amd.aggregation import poisson
    A = sps.csr_matrix(poisson((6, 6)))
    A.sort_indices()
    i = np.arange(36)
    splitting = ((i // 6 + i % 6) % 2).astype(np.intc)
    rng = np.random.RandomState(7)
    G = sps.random(48, 48, density=0.1, random_state=rng, format="csr")
    G = sps.csr_matrix(G + G.T + 4.0 * sps.identity(48))
    P = sps.csr_matrix((rng.rand(48), (np.arange(48), np.arange(48) % 12)), shape=(48, 12))
    return A, splitting, sps.csr_matrix(P.T), G, P


def _trip(M, dtype):
    return (M.indptr.astype(np.int64), M.indices.astype(np.intc), M.data.astype(dtype))


def _fetch_site(site):
    """-> (call, cleanup): the Python fetch site `site` on the smallest case its own GPU tests build"""
    import energy_io
    from pyamg_amd import classical, util
    from pyamg_amd.smooth import energy_prolongation_smoother
    from pyamg_amd.strength import evolution_strength_of_connection
    A, splitting, R, G, P = _small_operator()
    if site == "extended":
        S = classical.classical_strength_of_connection(A, 0.25, device=False)
        return (lambda: classical.extended_interpolation(A, S, splitting, device=True)), None
    if site == "level":
        return (lambda: classical.classical_level_device(A, 0.25, "PMIS", keep=True)), None
    if site == "transpose":
        return (lambda: classical.transpose(P, device=True)), None
    if site == "strength":
        return (lambda: evolution_strength_of_connection(A, np.ones(36), epsilon=4.0, k=2, rho=2.0, device=True)), None
    if site == "energy":
        p = energy_io.problem("aniso_17x23")
        return (lambda: energy_prolongation_smoother(p["A"], p["T"], p["Atilde"], p["Bc"], None, (False, {}), device=True)), None
    if site == "galerkin":
        util.device_operator(G)
        return ((lambda: util.galerkin_device(G, _trip(R, np.float64), _trip(P, np.float64), 12)),
                lambda: util.release_device_operator(G))
    assert site == "galerkin_c128"
    return (lambda: util.galerkin_device(_trip(G, np.complex128), _trip(R, np.complex128), _trip(P, np.complex128), 12)), None


@pytest.mark.parametrize("site", ["extended", "level", "transpose", "strength", "energy", "galerkin", "galerkin_c128"])
def test_a_failed_host_allocation_releases_the_device_result(live, monkeypatch, site):
    """Between a device stage's call and its fetch the host arrays are allocated (_lib.fetch_result).  Where that raises,
    the result the handle holds is released before the error reaches the caller: the count is back where it was."""
    from pyamg_amd import _lib
    call, cleanup = _fetch_site(site)
    held = []

    def no_memory(specs):
        held.append(live())
        raise MemoryError("no host memory for %d arrays" % len(specs))
    try:
        base = live()
        monkeypatch.setattr(_lib, "allocate", no_memory)
        with pytest.raises(MemoryError, match="no host memory"):
            call()
        monkeypatch.undo()
        assert held and held[0] > base          # the device call had returned and its result was alive
        assert live() == base
    finally:
        if cleanup:
            cleanup()
