"""CPU: the smoothed-aggregation setup for complex128 operators (pyamg_amd.aggregation, generic path) against the
hierarchies the reference built (tests/golden/hier_c128/*.npz, tools/gen_golden_hier_c128.py): same levels, formats
and sparsity, operators and smoother constants equal to rounding; real input keeps its bytes."""
import hashlib
import json
import os

import numpy as np
import pytest
import scipy.sparse as sps

import c128_cycle
from pyamg_amd import aggregation
from pyamg_amd.aggregation import smoothed_aggregation_solver

GS = ("gauss_seidel", {"sweep": "symmetric"})
SYM = dict(symmetry="symmetric")
HERM = dict(symmetry="hermitian")

# tools/gen_golden_hier_c128.py::main -- (presmoother, postsmoother, build arguments, np.random.seed); max_coarse=30
CASES = {
    "gs_sym_V_shifted2d": (GS, GS, SYM, 0),
    "sor_W_shifted2d": (("sor", {"omega": 1.2, "sweep": "symmetric"}), ("sor", {"omega": 1.2, "sweep": "symmetric"}), SYM, 1),
    "jacobi_F_x0_magnetic2d": (("jacobi", {"omega": 4.0 / 3.0, "iterations": 2}),
                               ("jacobi", {"omega": 4.0 / 3.0, "iterations": 2}), HERM, 2),
    "sa_default_magnetic2d": (("block_gauss_seidel", {"sweep": "symmetric"}),
                              ("block_gauss_seidel", {"sweep": "symmetric"}), HERM, 3),
    "cheb2_magnetic3d": (("chebyshev", {"degree": 2}), ("chebyshev", {"degree": 2}), HERM, 4),
    "bsr_bjac_gs": (("block_jacobi", {"omega": 0.7}), GS, SYM, 5),
    "coarse_gs10": (GS, GS, dict(SYM, coarse_solver=("gauss_seidel", {"iterations": 10})), 6),
    "one_level": (GS, GS, dict(SYM, max_levels=1), 8),
    "sor_negzero": (("sor", {"omega": 1.2}), ("sor", {"omega": 1.2}), SYM, 10),
    "poly_negzero": (("richardson", {"omega": 0.9}), ("chebyshev", {"degree": 3}), HERM, 9),
}


def build(case, A=None):
    pre, post, kw, seed = CASES[case]
    g = c128_cycle.load(case)
    A = g["levels"][0]["A"].copy() if A is None else A
    np.random.seed(seed)
    return g, smoothed_aggregation_solver(A, presmoother=pre, postsmoother=post, max_coarse=30, **kw)


def same(M, G, rtol):
    """tests/test_setup_golden.py::same"""
    M = sps.csr_matrix(M); G = sps.csr_matrix(G)
    M.sort_indices(); G.sort_indices()
    assert M.shape == G.shape
    assert np.array_equal(M.indptr, G.indptr) and np.array_equal(M.indices, G.indices), "sparsity differs"
    scale = np.abs(G.data).max()
    assert np.abs(M.data - G.data).max() <= rtol * scale, np.abs(M.data - G.data).max() / scale


def same_format(M, G):
    assert type(M) is type(G)
    assert M.dtype == np.complex128
    if sps.isspmatrix_bsr(G):
        assert M.blocksize == G.blocksize


def same_constants(d, gd):
    """the smoother constants, with the tolerances of tests/test_setup_golden.py"""
    assert d["name"] == gd["name"]
    for key in ("iterations", "sweep", "blocksize"):
        if key in gd:
            assert d[key] == gd[key], key
    if "omega" in gd:
        assert abs(d["omega"] - gd["omega"]) <= 1e-12 * abs(gd["omega"])
    if "coefficients" in gd:
        assert np.allclose(d["coefficients"], gd["coefficients"], rtol=1e-11, atol=0)
    if gd.get("Dinv") is not None:
        D, GD = np.ravel(d["Dinv"]), np.ravel(gd["Dinv"])
        assert D.dtype == np.complex128
        assert np.abs(D - GD).max() <= 1e-10 * np.abs(GD).max()


def test_the_table_lists_every_fixture():
    assert sorted(CASES) == c128_cycle.cases() and len(CASES) == 10


@pytest.mark.parametrize("case", sorted(CASES))
def test_c128_setup_reproduces_reference_hierarchy(case):
    g, ml = build(case)
    assert len(ml.levels) == g["meta"]["nlevels"]
    for lvl, G in zip(ml.levels, g["levels"]):
        same_format(lvl.A, G["A"])
        same(lvl.A, G["A"], 1e-13)
        if "P" in G:
            same_format(lvl.P, G["P"]); same_format(lvl.R, G["R"])
            same(lvl.P, G["P"], 1e-13)
            same(lvl.R, G["R"], 1e-13)
            same_constants(lvl.presmoother.desc, G["pre"])
            same_constants(lvl.postsmoother.desc, G["post"])
        else:
            assert not hasattr(lvl, "P")


# --------------------------------------------------------------------------- real input keeps its bytes
def _poisson(grid):
    A = None
    for n in grid:
        T = sps.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")
        A = T if A is None else sps.kron(A, sps.identity(n), format="csr") + sps.kron(sps.identity(A.shape[0]), T, format="csr")
    A = sps.csr_matrix(A); A.sort_indices()
    A.indices = A.indices.astype(np.intc); A.indptr = A.indptr.astype(np.intc)
    return A


def _row_sum_bound(M, *args, **kwargs):
    """max_i sum_j |m_ij| in place of the Arnoldi estimate: scipy's sequential row sums, the same bits on every host
    (the estimate's dot products and norms are BLAS reductions, whose last bits depend on the host's vector width)"""
    return float(abs(sps.csr_matrix(M)).sum(axis=1).max())


def real_generic_digests(monkeypatch):
    """sha256 of indptr / indices / data of every operator of hier_sa_gs_3d's problem (Poisson 12^3, max_coarse=30,
    the default candidate improvement) built on the generic path (fast=False) with _row_sum_bound for rho"""
    monkeypatch.setattr(aggregation, "approximate_spectral_radius", _row_sum_bound)
    np.random.seed(0)
    ml = smoothed_aggregation_solver(_poisson((12, 12, 12)), presmoother=GS, postsmoother=GS, max_coarse=30, fast=False)
    out = {}
    for i, lvl in enumerate(ml.levels):
        for name in ("A", "P", "R"):
            if hasattr(lvl, name):
                M = getattr(lvl, name)
                h = hashlib.sha256()
                for arr in (M.indptr, M.indices, M.data):
                    h.update(str(arr.dtype).encode()); h.update(np.ascontiguousarray(arr).tobytes())
                out["%s%d" % (name, i)] = [type(M).__name__, list(M.shape), h.hexdigest()]
    return out


def test_real_input_builds_the_bytes_it_built_before(monkeypatch):
    """tests/golden/setup_real_generic_sha256.json was recorded by real_generic_digests on the commit before complex
    operators were accepted"""
    with open(os.path.join(os.path.dirname(c128_cycle.GOLDEN), "setup_real_generic_sha256.json")) as f:
        before = json.load(f)
    now = real_generic_digests(monkeypatch)
    assert len(now) >= 7 and sorted(now) == sorted(before)
    for key in sorted(before):
        assert now[key] == before[key], key


# --------------------------------------------------------------------------- symmetry, complex64
def _bytes_equal(M, N):
    return (type(M) is type(N) and M.shape == N.shape and np.array_equal(M.indptr, N.indptr)
            and np.array_equal(M.indices, N.indices) and M.data.tobytes() == N.data.tobytes())


def test_restriction_is_the_conjugate_transpose_or_the_transpose():
    _, ml = build("cheb2_magnetic3d")                       # symmetry='hermitian'
    assert len(ml.levels) == 3
    for lvl in ml.levels[:-1]:
        assert np.abs(lvl.P.data.imag).max() > 0
        assert _bytes_equal(lvl.R, lvl.P.conj().T.asformat(lvl.P.format))
        assert not _bytes_equal(lvl.R, lvl.P.T.asformat(lvl.P.format))
    _, ml = build("gs_sym_V_shifted2d")                     # symmetry='symmetric'
    for lvl in ml.levels[:-1]:
        assert np.abs(lvl.P.data.imag).max() > 0
        assert _bytes_equal(lvl.R, lvl.P.T.asformat(lvl.P.format))


def test_complex64_operator_is_raised_to_complex128():
    g = c128_cycle.load("gs_sym_V_shifted2d")
    A = g["levels"][0]["A"].astype(np.complex64)
    assert A.dtype == np.complex64
    np.random.seed(0)
    ml = smoothed_aggregation_solver(A, presmoother=GS, postsmoother=GS, max_coarse=30, symmetry="symmetric")
    assert len(ml.levels) == 3
    for lvl in ml.levels:
        assert lvl.A.dtype == np.complex128 and np.asarray(lvl.B).dtype == np.complex128
        if hasattr(lvl, "P"):
            assert lvl.P.dtype == np.complex128 and lvl.R.dtype == np.complex128
    # the shifted Laplacian's entries (4 + 0.5i, -1) are exact in complex64: the raised operator is the fixture's
    same(ml.levels[1].A, g["levels"][1]["A"], 1e-13)


def test_complex_operators_take_the_generic_path():
    g = c128_cycle.load("gs_sym_V_shifted2d")
    A = g["levels"][0]["A"]
    B = np.ones((A.shape[0], 1), dtype=np.complex128)
    default = ("symmetric", ("standard", {}), ("jacobi", {"omega": 4.0 / 3.0}))
    assert not aggregation._scalar_fast_path_ok(A, B, *default)
    assert aggregation._scalar_fast_path_ok(abs(A).tocsr(), B.real, *default)
    Ab = c128_cycle.load("bsr_bjac_gs")["levels"][0]["A"]
    assert not aggregation._block_fast_path_ok(Ab, B, *default)
    assert aggregation._block_fast_path_ok(abs(Ab).tobsr(blocksize=(2, 2)), B.real, *default)


# --------------------------------------------------------------------------- host sweeps of the candidate improvement
def test_host_complex_sweeps_are_the_reference_kernels_bit_for_bit():
    core = c128_cycle.reference_core()
    if core is None:
        pytest.skip("oracle/_ref is absent")
    L = aggregation.host_lib()
    rng = np.random.RandomState(3)
    # point Gauss-Seidel on a CSR level 0
    A = c128_cycle.load("cheb2_magnetic3d")["levels"][0]["A"]
    n = A.shape[0]
    Ap, Aj = np.ascontiguousarray(A.indptr, dtype=np.intc), np.ascontiguousarray(A.indices, dtype=np.intc)
    Ax = np.ascontiguousarray(A.data)
    b = rng.randn(n) + 1j * rng.randn(n)
    x = rng.randn(n) + 1j * rng.randn(n)
    xr = x.copy()
    for rng_ in ((0, n, 1), (n - 1, -1, -1), (0, n, 2)):
        L.amgsetup_gauss_seidel_c128(aggregation._ip(Ap), aggregation._ip(Aj), Ax.ctypes.data, x.ctypes.data,
                                     b.ctypes.data, *rng_)
        core.gauss_seidel(Ap, Aj, Ax, xr, b, *rng_)
        assert x.tobytes() == xr.tobytes(), rng_
    # block Gauss-Seidel on a BSR(2, 2) level 0, with the fixture's inverted diagonal blocks
    gb = c128_cycle.load("bsr_bjac_gs")
    A = gb["levels"][0]["A"]
    bs = 2
    n = A.shape[0]
    nb = n // bs
    Ap, Aj = np.ascontiguousarray(A.indptr, dtype=np.intc), np.ascontiguousarray(A.indices, dtype=np.intc)
    Ax = np.ascontiguousarray(np.ravel(A.data))
    Dinv = np.ascontiguousarray(np.ravel(gb["levels"][0]["pre"]["Dinv"]), dtype=np.complex128)
    assert Dinv.size == nb * bs * bs
    b = rng.randn(n) + 1j * rng.randn(n)
    x = rng.randn(n) + 1j * rng.randn(n)
    xr = x.copy()
    for rng_ in ((0, nb, 1), (nb - 1, -1, -1)):
        L.amgsetup_block_gauss_seidel_c128(aggregation._ip(Ap), aggregation._ip(Aj), Ax.ctypes.data, x.ctypes.data,
                                           b.ctypes.data, Dinv.ctypes.data, rng_[0], rng_[1], rng_[2], bs)
        core.block_gauss_seidel(Ap, Aj, Ax, xr, b, Dinv, rng_[0], rng_[1], rng_[2], bs)
        assert x.tobytes() == xr.tobytes(), rng_
    # the inverted diagonal blocks the block sweeps take (util.get_block_diag): the reference's pinv_array, bit for bit,
    # on regular, rank-deficient and zero blocks of several sizes
    for bs in (1, 2, 3, 5):
        blocks = rng.randn(12, bs, bs) + 1j * rng.randn(12, bs, bs)
        blocks[0] = 0.0
        blocks[1][:, -1] = blocks[1][:, 0]
        blocks[2] = np.eye(bs)
        mine, ref = blocks.copy(), blocks.copy()
        L.amgsetup_pinv_blocks_c128(mine.ctypes.data, 12, bs)
        core.pinv_array(ref.ravel(), 12, bs, "T")
        assert mine.tobytes() == ref.tobytes(), bs
        assert np.abs(mine[3] @ blocks[3] - np.eye(bs)).max() < 1e-12

