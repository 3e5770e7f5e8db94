"""Level-0 chains whose row sums take an absent slot as a stored zero (kernels.hip coded_row_sum<MODE, true>,
level0_chain_kernel<FR, LR, true>).

Code 255 of a row's code word means "slot not stored".  The chains used to skip such a slot with a compare and two
selects; now the dictionary entry 255 holds +0.0 and the slot is multiplied and added like any other.  The sum starts at
+0.0 and is never -0.0, so its bits do not change for finite operands (tests/test_coded_row_sum_zero_slots.py restates
the argument on the CPU).  Here every case runs three ways -- zero slots on, zero slots off
(amg_set_level0_zero_slots(0), the select form) and the separate passes (amg_set_level0_fusion(0)) -- and the iterates
and residual histories must agree bit for bit after 1, 2 and 6 steps, the sixth being a graph replay, from x0 = 0 (pre
chain <0,1>) and from a given x0 (first pre chain <1,1>).  The zero-slot form runs in the chains with a leading
residual: the post chain <1,1> of every step, the first pre chain from a given x0, and <1,0> in the cycles without a
norm; <0,1> keeps the selects under either setting (it measured slower without them).

Boxes are (nz, ny, nx), 60 000 rows at the most; tile interiors are 26 x 10 lanes for 3 stages and 28 x 12 for 2.

    case        box             purpose
    ragged      (  5, 11, 27)   4 tiles, out-of-box lanes inside a tile on both axes
    two-chunk   (131, 13, 29)   ragged edges and the boundary between two z chunks of 128 planes
    two-rows    (  9,  2, 57)   nearly every lane of a tile is out of the box in y.  The issue asks for one row,
                                (4, 1, 57); that operator has 5 offsets and the chains take only the 7-point stencil
                                (level0_chain_check), and an operator gets its stencil form from 1024 rows on
                                (try_patterns), which two rows of 57 reach at nz = 9: the nearest box the chains run on
    dropped     ( 40, 20, 37)   poisson with about 2 % of the stored couplings dropped in symmetric pairs (seeded):
                                absent slots inside the box, whose operand is live data
    layers      (140, 13, 30)   the scaled operator of tests/test_gpu_level0_plane_reuse.py: several dictionary values
    zeros       ( 40, 20, 37)   the dropped operator with b and x0 that hold +0.0 and -0.0 on about a tenth of the rows:
                                both ends of dropped couplings, rows on the box faces, and rows drawn at random
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

CHEB2 = ("chebyshev", {"degree": 2})
S_VALUES = (1.0, 1.25, 0.75)
LAYER_CHANGES = (1, 64, 65, 127, 128, 129, 139)
DROP_GRID = (40, 20, 37)


def _poisson(grid):
    from pyamg_amd.aggregation import poisson
    A = sp.csr_matrix(poisson(grid))
    A.sort_indices()
    return A


def _layers(grid):
    nz, ny, nx = grid
    which = np.cumsum(np.isin(np.arange(nz), LAYER_CHANGES)) % 3
    S = sp.diags(np.repeat(np.array(S_VALUES)[which], ny * nx))
    B = sp.csr_matrix(S @ _poisson(grid) @ S)
    B.sort_indices()
    return B


@functools.lru_cache(maxsize=None)
def _dropped_pairs():
    """(i, j), i < j: about 2 % of the couplings poisson(DROP_GRID) stores above its diagonal"""
    U = sp.triu(_poisson(DROP_GRID), k=1).tocoo()
    pick = np.random.RandomState(37).rand(U.nnz) < 0.02
    return U.row[pick].copy(), U.col[pick].copy()


def _dropped(grid):
    assert grid == DROP_GRID
    i, j = _dropped_pairs()
    A = _poisson(grid).tolil()
    A[i, j] = 0.0
    A[j, i] = 0.0
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    A.sort_indices()
    return A


# name -> (box, operator, right-hand side and guess with signed zeros)
CASES = {
    "ragged": ((5, 11, 27), _poisson, False),
    "two-chunk": ((131, 13, 29), _poisson, False),
    "two-rows": ((9, 2, 57), _poisson, False),
    "dropped": (DROP_GRID, _dropped, False),
    "layers": ((140, 13, 30), _layers, False),
    "zeros": (DROP_GRID, _dropped, True),
}


@functools.lru_cache(maxsize=None)
def _operator(make, grid):
    return make(grid)


@functools.lru_cache(maxsize=None)
def _solver(make, grid):
    from pyamg_amd.aggregation import smoothed_aggregation_solver
    np.random.seed(0)
    return smoothed_aggregation_solver(_operator(make, grid), presmoother=CHEB2, postsmoother=CHEB2)


def _zero_rows(grid):
    """about a tenth of the rows: both ends of dropped couplings, rows on the six box faces, rows at random"""
    nz, ny, nx = grid
    n = nz * ny * nx
    rng = np.random.RandomState(11)
    i, j = _dropped_pairs()
    p = rng.permutation(len(i))[:500]
    z, y, x = np.unravel_index(np.arange(n), grid)
    face = np.flatnonzero((z == 0) | (z == nz - 1) | (y == 0) | (y == ny - 1) | (x == 0) | (x == nx - 1))
    rows = np.unique(np.concatenate([i[p], j[p], rng.choice(face, 1000, replace=False), rng.choice(n, 1000, replace=False)]))
    return rows


def _vectors(name):
    grid, _, zeros = CASES[name]
    n = int(np.prod(grid))
    rng = np.random.RandomState(sum(grid))
    b, x0 = rng.rand(n), rng.rand(n)
    if zeros:
        rows = _zero_rows(grid)
        assert 0.07 * n < len(rows) < 0.13 * n
        b[rows] = np.where(np.arange(len(rows)) % 2 == 0, 0.0, -0.0)
        x0[rows] = np.where(np.arange(len(rows)) % 3 == 0, 0.0, -0.0)
        assert np.signbit(b[rows]).any() and np.signbit(x0[rows]).any()
    return b, x0


def test_cases_are_what_the_table_says():
    for name, (grid, make, _) in CASES.items():
        assert int(np.prod(grid)) <= 60000, name
    i, j = _dropped_pairs()
    P = _poisson(DROP_GRID)
    A = _operator(_dropped, DROP_GRID)
    stored = (P.nnz - P.shape[0]) // 2
    assert 0.015 * stored < len(i) < 0.025 * stored
    assert A.nnz == P.nnz - 2 * len(i)
    assert (abs(A - A.T)).nnz == 0
    assert np.array_equal(A.diagonal(), P.diagonal())
    assert len(np.unique(_operator(_layers, CASES["layers"][0]).data)) > 6
    _vectors("zeros")


# ---------------------------------------------------------------------------------------------------------- on the GPU
def _lib():
    from pyamg_amd import _lib
    return _lib.lib()


def _three_ways(run):
    """run() with the zero slots, with the select form, and with the separate passes"""
    L = _lib()
    out = []
    try:
        for zero_slots, fusion in ((1, 1), (0, 1), (1, 0)):
            L.amg_set_level0_zero_slots(zero_slots)
            L.amg_set_level0_fusion(fusion)
            out.append(run())
    finally:
        L.amg_set_level0_zero_slots(1)
        L.amg_set_level0_fusion(1)
    return out


def _solve(ml, b, x0, steps):
    res = []
    x = ml.solve(b, x0=x0, tol=0.0, maxiter=steps, cycle="V", residuals=res)
    return x, np.array(res)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_solve_bit_identical_three_ways(name):
    grid, make, _ = CASES[name]
    ml = _solver(make, grid)
    L, h = _lib(), ml.device_hierarchy().h
    assert L.amg_hier_level0_fused(h) == 1
    b, x0 = _vectors(name)
    for guess in (None, x0):
        for steps in (1, 2, 6):
            (xz, rz), (xs, rs), (xu, ru) = _three_ways(lambda: _solve(ml, b, guess, steps))
            assert len(rz) > 1 and np.isfinite(xz).all()
            assert np.array_equal(xz.view(np.int64), xs.view(np.int64)), (guess is None, steps)
            assert np.array_equal(xz.view(np.int64), xu.view(np.int64)), (guess is None, steps)
            assert np.array_equal(rz, rs) and np.array_equal(rz, ru), (guess is None, steps)
    assert L.amg_hier_level0_fused(h) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["two-chunk", "zeros"])
def test_cycle_without_norm_bit_identical_three_ways(name):
    """two consecutive cycles without a norm: the post chain is <1,0>; from zero and from a given x0"""
    grid, make, _ = CASES[name]
    dev = _solver(make, grid).device_hierarchy()
    assert _lib().amg_hier_level0_fused(dev.h) == 1
    b, x0 = _vectors(name)

    def cycles(zero):
        x = np.zeros_like(b) if zero else x0.copy()
        dev.cycle(b, x, "V", x0_zero=zero)
        x1 = x.copy()
        dev.cycle(b, x, "V", x0_zero=False)
        return x1, x

    for zero in (True, False):
        (z1, z2), (s1, s2), (u1, u2) = _three_ways(lambda: cycles(zero))
        for a, c in ((z1, s1), (z1, u1), (z2, s2), (z2, u2)):
            assert np.array_equal(a.view(np.int64), c.view(np.int64)), zero
