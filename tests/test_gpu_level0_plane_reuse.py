"""Level-0 chains that load a column's code word once per run of equal planes (kernels.hip level0_chain_kernel,
Level0ChainArgs::same; hier.hip level0_chain_check).

A setup-time scan flags plane z when every column's code word on it equals the one on plane z - 1.  On a flagged plane
a lane takes its column's word from the register that holds plane z - 1's; the first plane of a z chunk always loads.
Every lane decodes the same word as before, so the iterates and the residual histories are those of the chains with
the switch off (amg_set_level0_plane_reuse(0)) and of the separate passes (amg_set_level0_fusion(0)), bit for bit.

The flag rule restated on the host from the CSR rows: plane z reuses iff every row of plane z has the same
(offset, value) pairs as the row one plane below it.  The host test checks the expected counts without a GPU; the GPU
tests require amg_hier_level0_plane_reuse to return that count.

Boxes are (nz, ny, nx); a workgroup marches over a z chunk of 128 planes.

    case       box             operator                                   flagged planes
    two-chunk  (129, 11, 35)   poisson                                    nz - 3: chunks 128 + 1, the second starts on flagged planes
    nz2        (  2, 24, 24)   poisson                                    0
    nz3        (  3, 20, 20)   poisson                                    0
    nz4        (  4, 20, 20)   poisson                                    1: plane 2 alone
    layers     (140, 13, 30)   S A S, s(z) changes at 1, 64, 65, 127,     the planes z - 1, z, z + 1 of every change clear,
                               128, 129, 139                              next to each other and on both sides of plane 128
    columns    ( 40, 20, 37)   S A S, s drawn per (x, y)                  nz - 3: invariant along z, different in every column
    one-entry  ( 70, 12, 14)   poisson, one diagonal entry of plane 33    nz - 5: planes 33 and 34 clear beyond the box's own
                               set to 7.0
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

CHEB2 = ("chebyshev", {"degree": 2})
S_VALUES = (1.0, 1.25, 0.75)
LAYER_CHANGES = (1, 64, 65, 127, 128, 129, 139)


def _poisson(grid):
    from pyamg_amd.aggregation import poisson
    A = sp.csr_matrix(poisson(grid))
    A.sort_indices()
    return A


def _scaled(A, s):
    S = sp.diags(s)
    B = sp.csr_matrix(S @ A @ S)
    B.sort_indices()
    return B


def _layers(grid):
    nz, ny, nx = grid
    which = np.cumsum(np.isin(np.arange(nz), LAYER_CHANGES)) % 3        # s(z) != s(z - 1) exactly at the listed z
    s = np.repeat(np.array(S_VALUES)[which], ny * nx)
    return _scaled(_poisson(grid), s)


def _columns(grid):
    nz, ny, nx = grid
    s = np.tile(np.array(S_VALUES)[np.random.RandomState(7).randint(0, 3, ny * nx)], nz)
    return _scaled(_poisson(grid), s)


def _one_entry(grid):
    nz, ny, nx = grid
    A = _poisson(grid).tolil()
    i = 33 * ny * nx + 5 * nx + 6
    A[i, i] = 7.0
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


# name -> (box, builder, flagged planes)
CASES = {
    "two-chunk": ((129, 11, 35), _poisson, 129 - 3),
    "nz2": ((2, 24, 24), _poisson, 0),
    "nz3": ((3, 20, 20), _poisson, 0),
    "nz4": ((4, 20, 20), _poisson, 1),
    # A change of s at z clears the flags of z - 1, z and z + 1 and nothing else: {0, 1, 2}, {63 .. 66}, {126 .. 130},
    # {138, 139}, which take in the box's own clear planes 0, 1 and nz - 1.  14 clear planes, so 126 flagged ones (the
    # issue that asked for this case quotes 124, which no s with exactly these changes gives under its own rule).
    "layers": ((140, 13, 30), _layers, 140 - 14),
    "columns": ((40, 20, 37), _columns, 40 - 3),
    "one-entry": ((70, 12, 14), _one_entry, 70 - 5),
}


@functools.lru_cache(maxsize=None)
def _operator(name):
    grid, make, _ = CASES[name]
    return make(grid)


def plane_flags(A, grid):
    """same[z] = 1 iff every row of plane z stores the (offset, value) pairs of the row one plane below it"""
    nz, ny, nx = grid
    P = ny * nx
    assert A.shape[0] == nz * P
    counts = np.diff(A.indptr)
    offsets = A.indices - np.repeat(np.arange(A.shape[0]), counts)
    same = np.zeros(nz, dtype=np.uint8)
    for z in range(1, nz):
        lo, mid, hi = A.indptr[(z - 1) * P], A.indptr[z * P], A.indptr[(z + 1) * P]
        same[z] = (np.array_equal(counts[(z - 1) * P:z * P], counts[z * P:(z + 1) * P]) and
                   np.array_equal(offsets[lo:mid], offsets[mid:hi]) and
                   np.array_equal(A.data[lo:mid].view(np.int64), A.data[mid:hi].view(np.int64)))
    return same


@pytest.mark.parametrize("name", list(CASES))
def test_flag_rule_gives_the_expected_counts(name):
    grid, _, expected = CASES[name]
    assert int(np.prod(grid)) <= 60000
    same = plane_flags(_operator(name), grid)
    assert same[0] == 0
    assert int(same.sum()) == expected


def test_flag_rule_places_the_clear_flags():
    nz = CASES["one-entry"][0][0]
    assert np.flatnonzero(plane_flags(_operator("one-entry"), CASES["one-entry"][0]) == 0).tolist() == [0, 1, 33, 34, nz - 1]
    clear = set(np.flatnonzero(plane_flags(_operator("layers"), CASES["layers"][0]) == 0).tolist())
    assert {127, 128, 129} <= clear and {63, 64, 65, 66} <= clear        # on both sides of the chunk boundary
    assert plane_flags(_operator("columns"), CASES["columns"][0])[2:-1].all()
    w = _operator("columns").diagonal()[:20 * 37]
    assert len(np.unique(w)) == 3                                          # the columns do differ


# ---------------------------------------------------------------------------------------------------------- on the GPU
def _lib():
    from pyamg_amd import _lib
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def _solver(name):
    from pyamg_amd.aggregation import smoothed_aggregation_solver
    np.random.seed(0)
    return smoothed_aggregation_solver(_operator(name), presmoother=CHEB2, postsmoother=CHEB2)


def _three_ways(run):
    """run() with the plane reuse, with every plane loading its words, and with the separate passes"""
    L = _lib()
    out = []
    try:
        for reuse, fusion in ((1, 1), (0, 1), (1, 0)):
            L.amg_set_level0_plane_reuse(reuse)
            L.amg_set_level0_fusion(fusion)
            out.append(run())
    finally:
        L.amg_set_level0_plane_reuse(1)
        L.amg_set_level0_fusion(1)
    return out


def _solve(ml, b, x0, steps):
    res = []
    x = ml.solve(b, x0=x0, tol=0.0, maxiter=steps, cycle="V", residuals=res)
    return x, np.array(res)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_solve_bit_identical_three_ways(name):
    """1, 2 and 6 steps (the sixth is a graph replay) from x0 = 0 (pre chain <0,1>) and from a random x0 (first pre
    chain <1,1>); every step ends in the post chain <1,1>."""
    grid = CASES[name][0]
    A = _operator(name)
    ml = _solver(name)
    L, h = _lib(), ml.device_hierarchy().h
    assert L.amg_hier_level0_fused(h) == 1
    assert L.amg_hier_level0_plane_reuse(h) == int(plane_flags(A, grid).sum())
    try:
        L.amg_set_level0_plane_reuse(0)
        assert L.amg_hier_level0_plane_reuse(h) == 0
    finally:
        L.amg_set_level0_plane_reuse(1)
    rng = np.random.RandomState(sum(grid))
    b = rng.rand(A.shape[0])
    x0 = rng.rand(A.shape[0])
    for guess in (None, x0):
        for steps in (1, 2, 6):
            (xr, rr), (xl, rl), (xu, ru) = _three_ways(lambda: _solve(ml, b, guess, steps))
            assert len(rr) > 1
            assert np.array_equal(xr, xl) and np.array_equal(xr, xu), (guess is None, steps)
            assert np.array_equal(rr, rl) and np.array_equal(rr, ru), (guess is None, steps)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["two-chunk", "layers"])
def test_cycle_without_norm_bit_identical_three_ways(name):
    """two consecutive cycles without a norm: the post chain is <1,0>; from zero and from a random x0"""
    grid = CASES[name][0]
    A = _operator(name)
    ml = _solver(name)
    dev = ml.device_hierarchy()
    assert _lib().amg_hier_level0_fused(dev.h) == 1
    rng = np.random.RandomState(sum(grid) + 1)
    b = rng.rand(A.shape[0])
    x0 = rng.rand(A.shape[0])

    def cycles(zero):
        x = np.zeros_like(b) if zero else x0.copy()
        dev.cycle(b, x, "V", x0_zero=zero)
        x1 = x.copy()
        dev.cycle(b, x, "V", x0_zero=False)
        return x1, x

    for zero in (True, False):
        (r1, r2), (l1, l2), (u1, u2) = _three_ways(lambda: cycles(zero))
        assert np.array_equal(r1, l1) and np.array_equal(r1, u1), zero
        assert np.array_equal(r2, l2) and np.array_equal(r2, u2), zero
