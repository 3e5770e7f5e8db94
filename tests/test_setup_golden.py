"""CPU: our smoothed-aggregation setup (pyamg_amd.aggregation) against the
hierarchies the reference built (tests/golden/hier_sa_*.npz, generated with
np.random.seed(0) before the setup): same level sizes and sparsity, operators and
smoother constants equal to rounding."""
import numpy as np
import pytest
import scipy.sparse as sps

import golden_io
from pyamg_amd.aggregation import (fit_candidates, smoothed_aggregation_solver, standard_aggregation,
                                   symmetric_strength_of_connection)


def poisson(grid):
    A = None
    for n in grid:
        T = sps.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")
        A = T if A is None else sps.kron(A, sps.identity(n), format="csr") + sps.kron(sps.identity(A.shape[0]), T, format="csr")
    A = sps.csr_matrix(A); A.sort_indices()
    A.indices = A.indices.astype(np.intc); A.indptr = A.indptr.astype(np.intc)
    return A


CASES = {
    "sa_jacobi_2d": ((48, 48), ("jacobi", {"omega": 4.0 / 3.0}), dict(max_coarse=30)),
    "sa_cheb2_3d": ((16, 16, 16), ("chebyshev", {"degree": 2}), dict(max_coarse=30)),
    "sa_gs_3d": ((12, 12, 12), ("block_gauss_seidel", {"sweep": "symmetric"}), dict(max_coarse=30)),
}


def same(M, G, rtol):
    M = sps.csr_matrix(M); G = sps.csr_matrix(G)
    M.sort_indices(); G.sort_indices()
    assert M.shape == G.shape
    assert np.array_equal(M.indptr, G.indptr) and np.array_equal(M.indices, G.indices), "sparsity differs"
    scale = np.abs(G.data).max()
    assert np.abs(M.data - G.data).max() <= rtol * scale, np.abs(M.data - G.data).max() / scale


@pytest.mark.parametrize("case", sorted(CASES))
def test_sa_setup_reproduces_reference_hierarchy(case):
    grid, sm, kw = CASES[case]
    g = golden_io.load_hier(case)
    A = poisson(grid)
    np.random.seed(0)
    ml = smoothed_aggregation_solver(A, presmoother=sm, postsmoother=sm, **kw)
    assert len(ml.levels) == g["meta"]["nlevels"]
    for i, (lvl, G) in enumerate(zip(ml.levels, g["levels"])):
        assert type(lvl.A).__name__ == type(G["A"]).__name__        # csr on level 0, bsr(1,1) below
        same(lvl.A, G["A"], 1e-13)
        if "P" in G:
            same(lvl.P, G["P"], 1e-13)
            same(lvl.R, G["R"], 1e-13)
            d, gd = lvl.presmoother.desc, G["pre"]
            assert d["name"] == gd["name"]
            if "omega" in gd:
                assert abs(d["omega"] - gd["omega"]) <= 1e-12 * abs(gd["omega"])
            if "coefficients" in gd:
                assert np.allclose(d["coefficients"], gd["coefficients"], rtol=1e-11, atol=0)


def test_standard_aggregation_kat():
    # hand-run of smoothed_aggregation.h:122-222 on a 6-node chain: pass 1 roots 0 ({0,1}) and
    # 3 ({2,3,4}); pass 2 attaches node 5 to the aggregate of node 4
    A = poisson((6,))
    AggOp, Cpts = standard_aggregation(symmetric_strength_of_connection(A))
    assert AggOp.shape == (6, 2)
    assert np.array_equal(AggOp.indices, [0, 0, 1, 1, 1, 1])
    assert np.array_equal(Cpts, [0, 3])
    # isolated node is left out
    M = sps.csr_matrix(np.array([[1.0, 0, 0], [0, 2.0, -1.0], [0, -1.0, 2.0]]))
    AggOp, Cpts = standard_aggregation(M)
    assert AggOp.shape == (3, 1) and AggOp.nnz == 2


def test_fit_candidates_kat():
    # pyamg/aggregation/tentative.py docstring examples
    AggOp = sps.csr_matrix(np.array([[1, 0], [1, 0], [0, 1], [0, 1]]))
    Q, R = fit_candidates(AggOp, [[1], [1], [1], [1]])
    assert np.allclose(Q.toarray(), [[0.70710678, 0], [0.70710678, 0], [0, 0.70710678], [0, 0.70710678]])
    assert np.allclose(R, [[1.41421356], [1.41421356]])
    Q, R = fit_candidates(AggOp, [[1, 0], [1, 1], [1, 2], [1, 3]])
    assert np.allclose(Q.toarray(), [[0.70710678, -0.70710678, 0, 0], [0.70710678, 0.70710678, 0, 0],
                                     [0, 0, 0.70710678, -0.70710678], [0, 0, 0.70710678, 0.70710678]])
    assert np.allclose(R, [[1.41421356, 0.70710678], [0, 0.70710678], [1.41421356, 3.53553391], [0, 0.70710678]])
    AggOp = sps.csr_matrix(np.array([[1, 0], [1, 0], [0, 0], [0, 1]]))
    Q, R = fit_candidates(AggOp, [[1], [1], [1], [1]])
    assert np.allclose(Q.toarray(), [[0.70710678, 0], [0.70710678, 0], [0, 0], [0, 1]])
    assert np.allclose(R, [[1.41421356], [1.0]])


def test_native_poisson_generator_matches_kronecker_sum():
    from pyamg_amd.aggregation import poisson as native
    for grid in ((7,), (5, 4), (3, 4, 5), (1, 6, 1)):
        A = native(grid); K = poisson(grid) if len(grid) > 1 or True else None
        assert A.shape == K.shape and A.nnz == K.nnz
        assert np.array_equal(A.indptr, K.indptr) and np.array_equal(A.indices, K.indices)
        assert np.array_equal(A.data, K.data)
    # README sizes: 500x500 -> 250000 / 1248000
    A = native((500, 500)); assert A.shape[0] == 250000 and A.nnz == 1248000


@pytest.mark.parametrize("grid", [(20, 17), (9, 10, 11)])
def test_fast_scalar_setup_equals_generic_scipy_path_bitwise(grid):
    """The array-level fast path (host helpers, OpenMP SpGEMM) must round exactly like the
    generic path that calls scipy's sparse products (the reference's arithmetic)."""
    A = poisson(grid)
    sm = ("jacobi", {"omega": 4.0 / 3.0})
    np.random.seed(0)
    fast = smoothed_aggregation_solver(A.copy(), presmoother=sm, postsmoother=sm, max_coarse=10, fast=True)
    np.random.seed(0)
    slow = smoothed_aggregation_solver(A.copy(), presmoother=sm, postsmoother=sm, max_coarse=10, fast=False)
    assert len(fast.levels) == len(slow.levels) >= 3
    for lf, ls in zip(fast.levels, slow.levels):
        for name in ("A", "P", "R"):
            if hasattr(ls, name):
                F, S = getattr(lf, name), getattr(ls, name)
                assert type(F) is type(S) and F.shape == S.shape
                assert np.array_equal(F.indptr, S.indptr), name
                assert np.array_equal(F.indices, S.indices), name      # same stored order
                assert np.array_equal(F.data.ravel(), S.data.ravel()), name


def test_rs_setup_reproduces_reference_hierarchy_and_readme():
    from pyamg_amd.classical import ruge_stuben_solver
    g = golden_io.load_hier("rs_gs_2d")
    ml = ruge_stuben_solver(poisson((40, 40)), max_coarse=40)
    assert len(ml.levels) == g["meta"]["nlevels"]
    for lvl, G in zip(ml.levels, g["levels"]):
        same(lvl.A, G["A"], 1e-14)
        if "P" in G:
            same(lvl.P, G["P"], 1e-14)
            same(lvl.R, G["R"], 1e-14)
            # stored entry order too (it is the SpMV summation order)
            assert np.array_equal(lvl.A.indices, G["A"].indices) and np.array_equal(lvl.A.data, G["A"].data)
    # the README example (README.md:84-94 / BASELINE.md): levels 0-3 as published; the last two
    # differ from the README by <= 3 nnz with today's scipy exactly as the reference itself does here
    from pyamg_amd.aggregation import poisson as native
    ml = ruge_stuben_solver(native((500, 500)))
    sizes = [(l.A.shape[0], l.A.nnz) for l in ml.levels]
    assert sizes[:4] == [(250000, 1248000), (125000, 1121002), (31252, 280662), (7825, 70657)]
    assert sizes[4:] == [(1937, 17971), (483, 4725)]          # reference run in this container
    assert abs(ml.operator_complexity() - 2.198) < 1e-3 and abs(ml.grid_complexity() - 1.666) < 1e-3


@pytest.mark.parametrize("case,sm", [
    ("elas_bgs_2d", ("block_gauss_seidel", {"sweep": "symmetric"})),
    ("bs3_bgs_2d", ("block_gauss_seidel", {"sweep": "symmetric", "blocksize": 3})),
])
def test_block_sa_setup_reproduces_reference_hierarchy(case, sm):
    """BSR operators with several near-null-space candidates (2D elasticity: blocks 2x2 -> 3x3 with the
    three rigid-body modes; a 3-unknowns-per-node diffusion system): block candidate improvement,
    block strength pattern, per-aggregate QR (fit_candidates), BSR Jacobi smoothing and Galerkin product."""
    g = golden_io.load_hier(case)
    np.random.seed(0)
    ml = smoothed_aggregation_solver(g["levels"][0]["A"].copy(), B=g["B0"], presmoother=sm, postsmoother=sm,
                                     max_coarse=10)
    assert len(ml.levels) == g["meta"]["nlevels"]
    for lvl, G in zip(ml.levels, g["levels"]):
        assert type(lvl.A) is type(G["A"]) and lvl.A.blocksize == G["A"].blocksize
        same(lvl.A, G["A"], 1e-12)
        if "P" in G:
            assert lvl.P.blocksize == G["P"].blocksize and lvl.R.blocksize == G["R"].blocksize
            same(lvl.P, G["P"], 1e-12)
            same(lvl.R, G["R"], 1e-12)
            assert lvl.presmoother.desc["name"] == G["pre"]["name"]
            assert np.allclose(np.ravel(lvl.presmoother.desc["Dinv"]), np.ravel(G["pre"]["Dinv"]), rtol=1e-10, atol=1e-14)


# --- our host setup kernels vs the reference's native ones (tests/golden/setup_kernels.npz) -----
def _setup_cases(prefix):
    z = np.load(golden_io.os.path.join(golden_io.GOLDEN, "setup_kernels.npz"), allow_pickle=False)
    for name in z["cases"]:
        name = str(name)
        if name.startswith(prefix):
            yield name, {k[len(name) + 2:]: z[k] for k in z.files if k.startswith(name + "__")}


def test_standard_aggregation_identical_to_reference_kernel():
    from pyamg_amd.aggregation import _ip, host_lib
    n_cases = 0
    for name, c in _setup_cases("standard_aggregation_"):
        n = int(c["n"][0])
        Ap, Aj = np.ascontiguousarray(c["Ap"], np.intc), np.ascontiguousarray(c["Aj"], np.intc)
        agg = np.empty(n, dtype=np.intc); roots = np.empty(n, dtype=np.intc)
        cnt = host_lib().amgsetup_standard_aggregation(n, _ip(Ap), _ip(Aj), _ip(agg), _ip(roots))
        assert cnt == int(c["count"][0]), name
        assert np.array_equal(agg, c["agg"]), name
        assert np.array_equal(roots[:cnt], c["roots"]), name
        n_cases += 1
    assert n_cases >= 5


def test_classical_kernels_identical_to_reference_kernels():
    from pyamg_amd.aggregation import _dp, _ip
    from pyamg_amd.classical import _lib
    L = _lib()
    for name, c in _setup_cases("classical_strength_"):
        Ap, Aj, Ax = (np.ascontiguousarray(c["Ap"], np.intc), np.ascontiguousarray(c["Aj"], np.intc),
                      np.ascontiguousarray(c["Ax"], np.float64))
        n = len(Ap) - 1
        Sp = np.empty_like(Ap); Sj = np.empty_like(Aj); Sx = np.empty_like(Ax)
        nnz = L.amgsetup_classical_strength(n, float(c["theta"][0]), _ip(Ap), _ip(Aj), _dp(Ax), _ip(Sp), _ip(Sj), _dp(Sx))
        assert np.array_equal(Sp, c["Sp"]) and np.array_equal(Sj[:nnz], c["Sj"]) and np.array_equal(Sx[:nnz], c["Sx"]), name
    for name, c in _setup_cases("rs_cf_splitting_"):
        Sp, Sj, Tp, Tj = (np.ascontiguousarray(c[k], np.intc) for k in ("Sp", "Sj", "Tp", "Tj"))
        n = len(Sp) - 1
        spl = np.empty(n, dtype=np.intc)
        L.amgsetup_rs_cf_splitting(n, _ip(Sp), _ip(Sj), _ip(Tp), _ip(Tj), _ip(spl))
        assert np.array_equal(spl, c["splitting"]), name
    for name, c in _setup_cases("rs_direct_interpolation_"):
        Ap, Aj, Cp, Cj, spl = (np.ascontiguousarray(c[k], np.intc) for k in ("Ap", "Aj", "Cp", "Cj", "splitting"))
        Ax, Cx = np.ascontiguousarray(c["Ax"], np.float64), np.ascontiguousarray(c["Cx"], np.float64)
        n = len(Ap) - 1
        Pp = np.empty(n + 1, dtype=np.intc)
        nnz = L.amgsetup_rs_direct_interpolation_pass1(n, _ip(Cp), _ip(Cj), _ip(spl), _ip(Pp))
        Pj = np.empty(nnz, dtype=np.intc); Px = np.empty(nnz, dtype=np.float64)
        L.amgsetup_rs_direct_interpolation_pass2(n, _ip(Ap), _ip(Aj), _dp(Ax), _ip(Cp), _ip(Cj), _dp(Cx), _ip(spl),
                                                 _ip(Pp), _ip(Pj), _dp(Px))
        assert np.array_equal(Pp, c["Pp"]) and np.array_equal(Pj, c["Pj"]), name
        assert np.array_equal(Px, c["Px"], equal_nan=True), name


# --------------------------------------------------------------------------- round 2: block (BSR) setup, configuration C5
def _c5_operator(case):
    """the level-0 operator and candidates the reference was handed (stored in the fixture)"""
    g = golden_io.load_hier(case)
    return g, g["levels"][0]["A"], g.get("B0")


@pytest.mark.parametrize("case,mc", [("c5_diff_p1_cube_bgs", 6), ("c5_elas_p1_cube_bgs", 8), ("bs3_bgs_2d", 10)])
def test_block_sa_setup_reproduces_reference_hierarchy(case, mc):
    """BSR(3,3) operators -- the reference's unit_cube tetrahedral mesh (P1 diffusion with the default 3 candidates,
    P1 elasticity with 6 rigid-body modes) and the Kronecker case -- through our setup, fast path where it applies:
    same level sizes / block sizes / sparsity, operators to rounding, block-diagonal inverses to rounding."""
    g, A, B = _c5_operator(case)
    sm = ("block_gauss_seidel", {"sweep": "symmetric", "blocksize": 3})
    np.random.seed(0)
    ml = smoothed_aggregation_solver(A, B=B, presmoother=sm, postsmoother=sm, max_coarse=mc)
    assert len(ml.levels) == g["meta"]["nlevels"]
    for lvl, G in zip(ml.levels, g["levels"]):
        assert lvl.A.blocksize == G["A"].blocksize
        same(lvl.A, G["A"], 1e-12)
        if "P" in G:
            assert lvl.P.blocksize == G["P"].blocksize
            same(lvl.P, G["P"], 1e-12)
            same(lvl.R, G["R"], 1e-12)
            D, GD = np.ravel(lvl.presmoother.desc["Dinv"]), np.ravel(G["pre"]["Dinv"])
            assert np.abs(D - GD).max() <= 1e-10 * np.abs(GD).max()


@pytest.mark.parametrize("n,bs,ncand", [(12, 3, None), (12, 3, 1), (10, 2, None), (15, 3, None)])
def test_fast_block_setup_equals_generic_scipy_path_bitwise(n, bs, ncand):
    """The block fast path (row-parallel bsr_matmat / bsr_minus_bsr / bsr_transpose restatements in
    csrc/setup_host.cpp) must produce the generic scipy path's operators bit for bit, stored block order
    included (it is the summation order of every later product)."""
    from pyamg_amd.gallery import tet_diffusion
    A = tet_diffusion(n, blocksize=bs)
    B = None if ncand is None else np.ones((A.shape[0], ncand))
    hier = []
    for fast in (True, False):
        np.random.seed(0)
        hier.append(smoothed_aggregation_solver(A.copy(), B=B, presmoother=None, postsmoother=None, max_coarse=5, fast=fast))
    fast, slow = hier
    assert len(fast.levels) == len(slow.levels) >= 3
    for lf, ls in zip(fast.levels, slow.levels):
        assert np.array_equal(np.asarray(lf.B), np.asarray(ls.B))
        for name in ("A", "P", "R"):
            if hasattr(ls, name):
                F, S = getattr(lf, name), getattr(ls, name)
                assert F.shape == S.shape and F.blocksize == S.blocksize
                assert np.array_equal(F.indptr, S.indptr) and np.array_equal(F.indices, S.indices), name
                assert np.array_equal(F.data, S.data), name


def test_native_kuhn_assembler_matches_element_assembly():
    """csrc/setup_host.cpp amgsetup_kuhn_p1_diffusion (row-by-row, for 5*10^7 unknowns) against the element-list
    assembly of gallery.p1_diffusion: same sparsity, entries to rounding (the summation order over elements differs)."""
    from pyamg_amd.gallery import tet_diffusion
    for n in (5, 9):
        A = tet_diffusion(n, native=False)
        N = tet_diffusion(n, native=True)
        assert np.array_equal(A.indptr, N.indptr) and np.array_equal(A.indices, N.indices)
        assert np.abs(A.data - N.data).max() <= 1e-13 * np.abs(A.data).max()
    Nb = tet_diffusion(9, native=True, blocksize=3)
    assert Nb.blocksize == (3, 3) and abs(Nb - tet_diffusion(9, native=False, blocksize=3)).max() <= 1e-13 * abs(Nb).max()


def test_pipelined_candidate_improvement_is_the_sequential_sweep(monkeypatch):
    """aggregation._improve above 10^5 unknowns runs its Gauss-Seidel sweeps with several host threads trailing each
    other chunk by chunk (setup_host.cpp: pipelined_sweep): bit for bit the one-thread sweeps, point and block"""
    import scipy.sparse as sp
    from pyamg_amd import aggregation
    monkeypatch.setenv("AMG_SETUP_DEVICE_GS", "0")            # the host sweeps, also where a GPU would take this size
    A = aggregation.poisson((60, 60, 60))                     # 216 000 rows, bandwidth 3 600
    A.symmetry = "hermitian"
    rng = np.random.RandomState(3)
    B = rng.rand(A.shape[0], 2)
    ran = []
    L = aggregation.host_lib()
    for name in ("amgsetup_gauss_seidel_pipelined", "amgsetup_block_gauss_seidel_pipelined"):
        orig = getattr(L, name)

        def wrapped(*a, _orig=orig, _name=name):
            r = _orig(*a)
            ran.append((_name, r))
            return r
        monkeypatch.setattr(L, name, wrapped)
    for method in (("gauss_seidel", {"sweep": "symmetric", "iterations": 2}),
                   ("gauss_seidel", {"sweep": "backward", "iterations": 1}),
                   ("block_gauss_seidel", {"sweep": "symmetric", "iterations": 1, "blocksize": 1})):
        monkeypatch.setenv("AMG_SETUP_PIPELINED_GS", "0")
        ref = aggregation._improve(method, A, B)
        monkeypatch.setenv("AMG_SETUP_PIPELINED_GS", "1")
        del ran[:]
        out = aggregation._improve(method, A, B)
        assert ran and all(r == 1 for _, r in ran), ran          # the pipelined sweep really ran
        assert np.array_equal(out, ref)
    # 3x3 blocks (the C5 shape): a block operator with the grid's pattern and dense, diagonally dominant blocks
    nb = A.shape[0]
    blocks = rng.rand(A.nnz, 3, 3) * 0.1
    diag = np.flatnonzero(A.indices == np.repeat(np.arange(nb), np.diff(A.indptr)))
    blocks[diag] += 4.0 * np.eye(3)
    Ab = sp.bsr_matrix((blocks, A.indices, A.indptr), shape=(3 * nb, 3 * nb))
    Ab.symmetry = "hermitian"
    Bb = rng.rand(3 * nb, 1)
    method = ("block_gauss_seidel", {"sweep": "symmetric", "iterations": 1})
    monkeypatch.setenv("AMG_SETUP_PIPELINED_GS", "0")
    ref = aggregation._improve(method, Ab, Bb)
    monkeypatch.setenv("AMG_SETUP_PIPELINED_GS", "1")
    del ran[:]
    out = aggregation._improve(method, Ab, Bb)
    assert ran and ran[0] == ("amgsetup_block_gauss_seidel_pipelined", 1), ran
    assert np.array_equal(out, ref)
    # an operator that does not qualify (structurally unsymmetric) falls back to the one-thread loop
    Au = A.tolil(); Au[0, 5000] = -1.0; Au = Au.tocsr(); Au.symmetry = "hermitian"
    del ran[:]
    out = aggregation._improve(("gauss_seidel", {"sweep": "forward", "iterations": 1}), Au, B[:, :1])
    assert ran == [("amgsetup_gauss_seidel_pipelined", 0)]
