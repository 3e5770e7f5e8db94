"""Fused level-0 smoother chains (kernels.hip level0_chain_kernel, hier.hip cycle): the pre-smoother with the
restriction's residual, and the post-smoother with the next norm's residual, each as one tiled sweep.  Where the fused
path is taken it must give the same bits as the separate passes (amg_set_level0_fusion(0)) and as the C oracle;
where it is not taken (other smoothers, variable coefficients, couplings that leave the box, partitioned levels) the
query says so and the results are still the oracle's."""
import os
import socket

import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu

CHEB2 = ("chebyshev", {"degree": 2})


def _lib():
    from pyamg_amd import _lib
    return _lib.lib()


def _solver(A, sm=CHEB2):
    from pyamg_amd.aggregation import smoothed_aggregation_solver
    np.random.seed(0)
    return smoothed_aggregation_solver(A, presmoother=sm, postsmoother=sm)


def _oracle(ml):
    levels = []
    for lvl in ml.levels:
        L = {"A": lvl.A}
        if hasattr(lvl, "P"):
            L.update(P=lvl.P, R=lvl.R, pre=dict(lvl.presmoother.desc), post=dict(lvl.postsmoother.desc))
        levels.append(L)
    kind, M = ml.coarse_solver.device_form(ml.levels[-1].A)
    return oracle_lib.Hierarchy(levels, M)


def _fused(ml):
    return _lib().amg_hier_level0_fused(ml.device_hierarchy().h)


def _both(run):
    """run() with the fused chains and with the separate passes"""
    out = {}
    try:
        for on in (1, 0):
            _lib().amg_set_level0_fusion(on)
            out[on] = run()
    finally:
        _lib().amg_set_level0_fusion(1)
    return out[1], out[0]


def _solve(ml, b, x0, steps, cyc):
    res = []
    x = ml.solve(b, x0=x0, tol=0.0, maxiter=steps, cycle=cyc, residuals=res)
    return x, np.array(res)


@pytest.mark.parametrize("grid", [(33, 33, 33), (40, 41, 42), (130, 97, 75)])
def test_fused_path_taken_and_bit_identical(grid):
    """C3-shaped hierarchies take the fused path: cubic and non-cubic grids, extents that are not multiples of the
    tile interiors (28 and 26 rows), z extents shorter than one z chunk (64 planes) and one with a ragged last chunk.
    1 and 6 steps (the sixth is a graph replay) from x0 = 0 and from a random x0: same iterates and residual
    histories as the separate passes, and the oracle's iterates."""
    from pyamg_amd.aggregation import poisson
    A = poisson(grid)
    ml = _solver(A)
    assert _fused(ml) == 1
    rng = np.random.RandomState(sum(grid))
    b = rng.rand(A.shape[0])
    x0 = rng.rand(A.shape[0])
    H = _oracle(ml)
    for guess in (None, x0):
        for steps in (1, 6):
            (xf, rf), (xu, ru) = _both(lambda: _solve(ml, b, guess, steps, "V"))
            assert np.array_equal(xf, xu), (guess is None, steps)
            assert np.array_equal(rf, ru), (guess is None, steps)
            xo, reso = H.solve(b, x0=(np.zeros_like(b) if guess is None else guess), tol=0.0, maxiter=steps)
            assert np.array_equal(xf, xo), (guess is None, steps)
            assert np.allclose(rf, reso, rtol=1e-12)


@pytest.mark.parametrize("cyc", ["V", "W", "F"])
def test_cycles_keep_and_graphs(cyc):
    """V, W and F cycles, with and without the kept residual and graph replay: the fused path gives the separate
    passes' bits in every combination, and the oracle's iterates."""
    from pyamg_amd.aggregation import poisson
    A = poisson((37, 35, 29))
    ml = _solver(A)
    assert _fused(ml) == 1
    dev = ml.device_hierarchy()
    rng = np.random.RandomState(4)
    b = rng.rand(A.shape[0])
    x0 = rng.rand(A.shape[0])
    H = _oracle(ml)
    try:
        for keep in (1, 0):
            for graphs in (1, 0):
                _lib().amg_hier_keep_residual(dev.h, keep)
                _lib().amg_hier_use_graphs(dev.h, graphs)
                for guess in (None, x0):
                    (xf, rf), (xu, ru) = _both(lambda: _solve(ml, b, guess, 6, cyc))
                    assert np.array_equal(xf, xu) and np.array_equal(rf, ru), (keep, graphs, guess is None)
    finally:
        _lib().amg_hier_keep_residual(dev.h, 1)
        _lib().amg_hier_use_graphs(dev.h, 1)
    xo, _ = H.solve(b, x0=x0, tol=0.0, maxiter=6, cycle=cyc)
    assert np.array_equal(xf, xo)


def test_cycle_without_norm_and_cg():
    """A cycle that no norm follows (amg_hier_cycle: the post chain ends at POLY_LAST), aspreconditioner and
    solve(accel='cg') (its preconditioner is such a cycle from zero)."""
    from pyamg_amd.aggregation import poisson
    A = poisson((31, 30, 45))
    ml = _solver(A)
    assert _fused(ml) == 1
    dev = ml.device_hierarchy()
    rng = np.random.RandomState(9)
    b = rng.rand(A.shape[0])
    x0 = rng.rand(A.shape[0])
    H = _oracle(ml)

    def one_cycle(zero):
        x = np.zeros_like(b) if zero else x0.copy()
        dev.cycle(b, x, "V", x0_zero=zero)
        return x

    for zero in (True, False):
        xf, xu = _both(lambda: one_cycle(zero))
        assert np.array_equal(xf, xu), zero
        xo, _ = H.solve(b, x0=(np.zeros_like(b) if zero else x0), tol=0.0, maxiter=1)
        assert np.array_equal(xf, xo), zero
    M = ml.aspreconditioner()
    yf, yu = _both(lambda: M.matvec(b))
    assert np.array_equal(yf, yu)

    def cg():
        res = []
        x = ml.solve(b, tol=1e-10, maxiter=25, accel="cg", residuals=res)
        return x, np.array(res)

    (xf, rf), (xu, ru) = _both(cg)
    assert np.array_equal(xf, xu) and np.array_equal(rf, ru)


def _check_not_fused_and_oracle(ml, b):
    assert _fused(ml) == 0
    x, res = _solve(ml, b, None, 3, "V")
    xo, reso = _oracle(ml).solve(b, tol=0.0, maxiter=3)
    assert np.array_equal(x, xo)
    assert np.allclose(res, reso, rtol=1e-12)


@pytest.mark.parametrize("sm", [("jacobi", {}), ("gauss_seidel", {"sweep": "symmetric"}),
                                ("multicolor_gauss_seidel", {"sweep": "symmetric"}), ("chebyshev", {"degree": 3})],
                         ids=["jacobi", "sgs", "mcgs", "cheb3"])
def test_other_smoothers_keep_the_separate_passes(sm):
    from pyamg_amd.aggregation import poisson
    A = poisson((20, 21, 22))
    ml = _solver(A, sm)
    _check_not_fused_and_oracle(ml, np.random.RandomState(1).rand(A.shape[0]))


def test_variable_coefficients_keep_the_separate_passes():
    """Too many distinct values for the value index: no codes, no fused chains."""
    import scipy.sparse as sp
    from pyamg_amd.aggregation import poisson
    A = sp.csr_matrix(poisson((20, 21, 22)))
    rng = np.random.RandomState(2)
    A.data = A.data * (1.0 + 0.01 * rng.rand(A.nnz))
    A = sp.csr_matrix(0.5 * (A + A.T))
    A.sort_indices()
    ml = _solver(A)
    assert _lib().amg_hier_value_index(ml.device_hierarchy().h, 0, -1) == 0
    _check_not_fused_and_oracle(ml, rng.rand(A.shape[0]))


def test_wrap_around_coupling_keeps_the_separate_passes():
    """The 7-point offsets, plus one coupling between the end of a grid line and the start of the next (offsets +1
    and -1 of those two rows): the union stencil is unchanged, the box scan rejects it."""
    import scipy.sparse as sp
    from pyamg_amd.aggregation import poisson
    nz, ny, nx = 20, 21, 22
    A = poisson((nz, ny, nx)).tolil()
    i = 5 * nx * ny + 3 * nx + (nx - 1)            # last row of a line
    A[i, i + 1] = -1.0
    A[i + 1, i] = -1.0
    A = sp.csr_matrix(A)
    A.sort_indices()
    ml = _solver(A)
    dev = ml.device_hierarchy()
    assert _lib().amg_hier_operator_form(dev.h, 0) == 2 and _lib().amg_hier_value_index(dev.h, 0, -1) > 0
    _check_not_fused_and_oracle(ml, np.random.RandomState(3).rand(A.shape[0]))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker_partitioned(rank, world, port, grid, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["AMG_DIST_TRANSPORT"] = "peer"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    S = None
    try:
        from pyamg_amd.aggregation import poisson
        from pyamg_amd.distributed import DistributedSolver, HipBackend, split_rows, levels_from_ml
        A = poisson(grid)
        ml = _solver(A)
        b = np.random.RandomState(7).rand(A.shape[0])
        levels, coarse = levels_from_ml(ml)
        S = DistributedSolver(levels, coarse, HipBackend(0), rank, world, replicate_below=600)
        Lb, h, _ = S.native
        fused = Lb.amg_hier_level0_fused(h)
        bnd = split_rows(len(b), world)
        lo, hi = int(bnd[rank]), int(bnd[rank + 1])
        x, res = S.solve(b[lo:hi], None, tol=0.0, maxiter=3, cycle="V", fixed=True)
        np.save(os.path.join(out_dir, "x_%d.npy" % rank), x)
        np.save(os.path.join(out_dir, "fused_%d.npy" % rank), np.array([fused]))
    finally:
        if S is not None:
            S.close()
        dist.destroy_process_group()


def test_partitioned_hierarchy_keeps_the_separate_passes(tmp_path):
    """Two ranks on one GPU: level 0 is row-partitioned, the chains are not used; the iterates are the oracle's."""
    import torch.multiprocessing as mp
    from pyamg_amd.aggregation import poisson
    grid = (25, 24, 23)
    mp.spawn(_worker_partitioned, args=(2, _free_port(), grid, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        assert np.load(tmp_path / ("fused_%d.npy" % r))[0] == 0
    x = np.concatenate([np.load(tmp_path / ("x_%d.npy" % r)) for r in range(2)])
    A = poisson(grid)
    ml = _solver(A)
    b = np.random.RandomState(7).rand(A.shape[0])
    xo, _ = _oracle(ml).solve(b, tol=0.0, maxiter=3)
    assert np.array_equal(x, xo)
