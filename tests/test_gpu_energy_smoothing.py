"""Energy-minimisation prolongation smoothing on the device (csrc/energy.hip): the three flat amg_core entries against
the reference's recorded calls and the sequential models of tests/energy_io.py, the device route against the host
route bit for bit, and one hierarchy built through it."""
import os

import numpy as np
import pytest
import scipy.sparse as sps

import energy_io as eio
import evolution_io as evo
import golden_io
import pyamg_amd
from pyamg_amd import amg_core, smooth
from pyamg_amd.aggregation import fit_candidates, standard_aggregation, symmetric_strength_of_connection
from pyamg_amd.smooth import energy_prolongation_smoother

pytestmark = pytest.mark.gpu

NO = (False, {})


def flat_call(kernel, a):
    """one call through the flat device entry -> the output array"""
    a = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    out = eio.OUTPUT[kernel]
    a[out] = a[out].copy()
    getattr(amg_core, kernel)(*[a[k] for k in eio.ARGS[kernel]])
    return a[out]


def model_call(kernel, a):
    if kernel == "incomplete_mat_mult_bsr":
        return eio.model_incomplete_mat_mult_bsr(*[a[k] for k in eio.ARGS[kernel]])
    if kernel == "satisfy_constraints_helper":
        return eio.model_satisfy_constraints(*[a[k] for k in eio.ARGS[kernel]])
    return eio.model_calc_BtB(a["NullDim"], a["Nnodes"], a["ColsPerBlock"], a["b"], a["BsqCols"], a["Sp"], a["Sj"])


# ---------------------------------------------------------------------------------------------- the flat entries
@pytest.mark.parametrize("name", eio.PROBLEMS)
def test_flat_entries_reproduce_the_recorded_native_calls(name):
    n = 0
    for q, s in enumerate(eio.problem(name)["sets"]):
        for ci, (kernel, args, want) in enumerate(s["calls"]):
            got = flat_call(kernel, args)
            assert np.array_equal(got, want), "%s set %d call %d (%s): worst %g" % (name, q, ci, kernel, np.abs(got - want).max())
            n += 1
    assert n >= len(eio.problem(name)["sets"])


SHAPES = [(1, 1, 1), (2, 2, 3), (3, 3, 6), (2, 3, 1)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sorted_rows,fill", [(False, True), (True, False)])
def test_incomplete_product_against_the_model(shape, sorted_rows, fill):
    """unsorted rows and a pre-filled Sx; an empty row of A, B and S"""
    R, N, Cc = shape
    rng = np.random.RandomState(100 * R + 10 * N + Cc)
    args = eio.pattern_case(rng, 40, 17, R, N, Cc, 300, sorted_rows=sorted_rows, empty_row=11, fill=fill)
    Ap, Bp, Sp = args[0], args[3], args[6]
    assert Ap[12] == Ap[11] and Bp[12] == Bp[11] and Sp[12] == Sp[11]
    a = dict(zip(eio.ARGS["incomplete_mat_mult_bsr"], args))
    got = flat_call("incomplete_mat_mult_bsr", a)
    want = model_call("incomplete_mat_mult_bsr", a)
    assert np.array_equal(got, want)
    assert fill or np.count_nonzero(got) > 0


@pytest.mark.parametrize("n_blocks", [255, 256, 257, 1025])
def test_incomplete_product_at_workgroup_boundaries(n_blocks):
    """1 x 1 blocks: one lane per block, so the last lane of a full workgroup and the first of a new one own a scalar"""
    rng = np.random.RandomState(n_blocks)
    args = eio.pattern_case(rng, 70, 40, 1, 1, 1, n_blocks)
    a = dict(zip(eio.ARGS["incomplete_mat_mult_bsr"], args))
    assert len(a["Sj"]) == n_blocks
    assert np.array_equal(flat_call("incomplete_mat_mult_bsr", a), model_call("incomplete_mat_mult_bsr", a))


def test_incomplete_product_empty_S_and_duplicate_column():
    rng = np.random.RandomState(5)
    args = eio.pattern_case(rng, 10, 6, 2, 2, 3, 0)
    a = dict(zip(eio.ARGS["incomplete_mat_mult_bsr"], args))
    assert flat_call("incomplete_mat_mult_bsr", a).size == 0
    # a row of S that stores a column twice: the later slot receives everything (the reference's behaviour)
    one = np.array([0, 1], dtype=np.intc); z = np.array([0], dtype=np.intc)
    Sx = np.array([5.0, 7.0])
    amg_core.incomplete_mat_mult_bsr(one, z, np.array([2.0]), one, z, np.array([3.0]), np.array([0, 2], dtype=np.intc),
                                     np.array([0, 0], dtype=np.intc), Sx, 1, 1, 1, 1, 1)
    assert np.array_equal(Sx, [5.0, 13.0])


@pytest.mark.parametrize("R,Cc,ND", [(1, 1, 1), (2, 3, 3), (3, 6, 6), (2, 1, 3)])
def test_constraints_and_BtB_against_the_models(R, Cc, ND):
    rng = np.random.RandomState(10 * R + Cc + ND)
    n_brow, n_bcol = 37, 19
    args = eio.pattern_case(rng, n_brow, n_bcol, R, R, Cc, 257)
    Sp, Sj, Sx = args[6], args[7], args[8]
    B = rng.uniform(-1.0, 1.0, n_bcol * Cc * ND)
    a = dict(RowsPerBlock=R, ColsPerBlock=Cc, num_block_rows=n_brow, NullDim=ND, x=B, y=rng.uniform(-1.0, 1.0, n_brow * R * ND),
             z=rng.uniform(-1.0, 1.0, n_brow * ND * ND), Sp=Sp, Sj=Sj, Sx=Sx)
    assert np.array_equal(flat_call("satisfy_constraints_helper", a), model_call("satisfy_constraints_helper", a))
    BsqCols = ND * (ND + 1) // 2
    b = dict(NullDim=ND, Nnodes=n_brow, ColsPerBlock=Cc, b=rng.uniform(-1.0, 1.0, n_bcol * Cc * BsqCols), BsqCols=BsqCols,
             x=np.zeros(n_brow * ND * ND), Sp=Sp, Sj=Sj)
    assert np.array_equal(flat_call("calc_BtB", b), model_call("calc_BtB", b))


def test_argument_errors_are_the_tables_error():
    rng = np.random.RandomState(9)
    good = dict(zip(eio.ARGS["incomplete_mat_mult_bsr"], eio.pattern_case(rng, 10, 6, 2, 2, 3, 20)))
    bad = []
    a = dict(good); a["Sj"] = good["Sj"].copy(); a["Sj"][3] = 6; bad.append(a)                  # column outside S
    a = dict(good); a["Aj"] = good["Aj"].copy(); a["Aj"][0] = -1; bad.append(a)                 # column outside A
    a = dict(good); a["Sp"] = good["Sp"].copy(); a["Sp"][4] = a["Sp"][3] - 1; bad.append(a)     # offsets decrease
    a = dict(good); a["Sx"] = good["Sx"][:-1].copy(); bad.append(a)                             # Sx shorter than blocks need
    a = dict(good); a["Bx"] = good["Bx"][:-1].copy(); bad.append(a)
    a = dict(good); a["bcol_B"] = 0; bad.append(a)
    a = dict(good); a["Ap"] = good["Ap"][:-1].copy(); bad.append(a)
    for a in bad:
        before = a["Sx"].copy()
        with pytest.raises(ValueError):
            getattr(amg_core, "incomplete_mat_mult_bsr")(*[a[k] for k in eio.ARGS["incomplete_mat_mult_bsr"]])
        assert np.array_equal(a["Sx"], before)
    Sp, Sj = good["Sp"], good["Sj"]
    with pytest.raises(ValueError):          # y shorter than the block rows need
        amg_core.satisfy_constraints_helper(2, 3, 10, 3, np.ones(6 * 9), np.ones(10 * 6 - 1), np.ones(10 * 9), Sp, Sj, good["Sx"].copy())
    with pytest.raises(ValueError):          # x holds fewer block columns than Sj names
        amg_core.satisfy_constraints_helper(2, 3, 10, 3, np.ones(1 * 9), np.ones(10 * 6), np.ones(10 * 9), Sp, Sj, good["Sx"].copy())
    with pytest.raises(ValueError):          # BsqCols is not NullDim (NullDim + 1) / 2
        amg_core.calc_BtB(3, 10, 3, np.ones(6 * 3 * 6), 5, np.zeros(90), Sp, Sj)
    with pytest.raises(ValueError):          # x shorter than Nnodes * NullDim^2
        amg_core.calc_BtB(3, 10, 3, np.ones(6 * 3 * 6), 6, np.zeros(89), Sp, Sj)


# ---------------------------------------------------------------------------------------------- the device route
def both_routes(A, T, Atilde, Bc, **opt):
    th, td = [], []
    H = energy_prolongation_smoother(A, T, Atilde, Bc, None, NO, device=False, _trace=th, **opt)
    D = energy_prolongation_smoother(A, T, Atilde, Bc, None, NO, device=True, _trace=td, **opt)
    eio.same_bits(D, H)
    assert td == th, "the two routes took other inner products: %r and %r" % (td, th)
    return H, th


@pytest.mark.parametrize("name,q", eio.all_sets())
def test_device_route_equals_host_route_bit_for_bit(name, q):
    p = eio.problem(name)
    s = p["sets"][q]
    if not smooth._scatter(sps.bsr_matrix(p["T"]), s["Sp"], s["Sj"])[1].all():
        # random_spd_150 with degree 1: the empty row of Atilde leaves a block of T outside the pattern
        assert (name, q) == ("random_spd_150", 1)
        with pytest.raises(NotImplementedError, match="outside the restated setup"):
            energy_prolongation_smoother(p["A"], p["T"], p["Atilde"], p["Bc"], None, NO, device=True, **s["options"])
        return
    H, trace = both_routes(p["A"], p["T"], p["Atilde"], p["Bc"], **s["options"])
    assert len(trace) == len(s["trace"])
    assert np.array_equal(H.indices, s["P"].indices)


def test_device_route_maxiter_zero_and_vanishing_residual():
    p = eio.problem("elasticity_12x12")
    H, trace = both_routes(p["A"], p["T"], p["Atilde"], p["Bc"], maxiter=0)
    assert trace == []
    T = sps.bsr_matrix(p["T"]); T.sort_indices()
    eio.same_bits(H, T)
    # A T = 0 on the pattern: R is all zero at iteration 0
    n = 12
    L1 = sps.diags([-np.ones(n - 1), np.r_[1.0, 2 * np.ones(n - 2), 1.0], -np.ones(n - 1)], [-1, 0, 1], format="csr")
    A = sps.block_diag([L1, L1], format="csr")
    T = sps.csr_matrix(sps.block_diag([np.ones((n, 1)), np.ones((n, 1))]))
    H, trace = both_routes(A, T, None, np.ones((2, 1)) * np.sqrt(n))
    assert len(trace) == 1 and trace[0][0] == 0.0
    eio.same_bits(H, sps.bsr_matrix(T, blocksize=(1, 1)))


@pytest.mark.parametrize("maxiter", [0, 1])
@pytest.mark.parametrize("n", [1, 65])
def test_device_route_on_one_row_and_one_past_a_wave(n, maxiter):
    # arrays of one or two entries and of one row more than a wave: where an upload or the padding behind it can go wrong
    A = sps.diags([-np.ones(n - 1), np.linspace(2.0, 3.0, n), -np.ones(n - 1)], [-1, 0, 1], format="csr")
    B = np.linspace(1.0, 2.0, n).reshape(-1, 1)
    AggOp = sps.csr_matrix((np.ones(n), (np.arange(n), np.arange(n) // 3)), shape=(n, (n + 2) // 3))
    T, Bc = fit_candidates(AggOp, B)
    H, trace = both_routes(A, T, None, Bc, maxiter=maxiter)
    assert len(trace) == maxiter and H.shape == T.shape
    assert np.abs(H * Bc - B).max() <= 1e-12


def test_device_route_refuses_a_prolongator_outside_the_pattern():
    p = eio.problem("aniso_17x23")
    At = sps.lil_matrix(p["Atilde"])
    At[5, :] = 0.0
    At = sps.csr_matrix(At); At.eliminate_zeros()
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        energy_prolongation_smoother(p["A"], p["T"], At, p["Bc"], None, NO, device=True)


def test_device_route_at_working_size():
    """the 480 x 481 grid of tests/evolution_io.py (230 880 rows): every kernel and the inner product's levels span many
    workgroups; the host route, pinned to the reference at small size, is the oracle"""
    A, _ = evo.large_grid()
    B = np.ones((A.shape[0], 1))
    C = symmetric_strength_of_connection(A)
    T, Bc = fit_candidates(standard_aggregation(C)[0], B)
    H, trace = both_routes(A, T, C, Bc, maxiter=4, degree=1, weighting="local")
    assert len(trace) == 4 and H.shape[0] == 230880 and len(H.indices) > 256 * 256
    assert np.abs(H * Bc - B).max() <= 1e-12


# ---------------------------------------------------------------------------------------------- the hierarchy
def test_sa_hierarchy_through_the_device_route_and_resident_solve():
    g = eio.load_hier("sa_evolution_energy_2d")
    A = g["levels"][0]["A"]
    gs = ("block_gauss_seidel", {"sweep": "symmetric"})
    built = []
    for device in (True, False):
        np.random.seed(0)
        built.append(pyamg_amd.smoothed_aggregation_solver(
            A, strength=("evolution", {"k": 2, "epsilon": 4.0}), max_coarse=20, presmoother=gs, postsmoother=gs,
            smooth=("energy", {"krylov": "cg", "maxiter": 4, "degree": 1, "weighting": "local", "device": device})))
    dev, host = built
    assert [lvl.A.shape[0] for lvl in dev.levels] == [1600, 280, 56, 10]
    for a, b in zip(dev.levels, host.levels):
        ops = [("A", a.A, b.A)] + ([("P", a.P, b.P), ("R", a.R, b.R)] if hasattr(b, "P") else [])
        for what, x, y in ops:
            assert type(x) is type(y) and np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices, y.indices) \
                and np.array_equal(x.data, y.data), what
    res = []
    x = dev.solve(g["b"], tol=g["meta"]["tol"], maxiter=g["meta"]["maxiter"], residuals=res)
    assert len(res) == len(g["residuals"]) == 28
    golden_io.assert_history(res, g["residuals"], A, x, g["b"])


def test_elasticity_hierarchy_takes_the_rectangular_blocks_unchanged():
    g = eio.load_hier("elas_energy_2d")
    A = g["levels"][0]["A"]
    B = np.load(os.path.join(eio.ENERGY, "hier_elas_energy_2d.npz"), allow_pickle=False)["B0"]
    gs = ("block_gauss_seidel", {"sweep": "symmetric"})
    built = []
    for device in (True, False):
        np.random.seed(0)
        built.append(pyamg_amd.smoothed_aggregation_solver(
            A, B=B, max_coarse=10, presmoother=gs, postsmoother=gs,
            smooth=("energy", {"krylov": "cg", "maxiter": 4, "degree": 1, "weighting": "local", "device": device})))
    dev, host = built
    assert [lvl.P.blocksize for lvl in dev.levels[:-1]] == [(2, 3), (3, 3)]
    for a, b in zip(dev.levels, host.levels):
        if hasattr(b, "P"):
            eio.same_bits(a.P, b.P)
    res = []
    x = dev.solve(g["b"], tol=g["meta"]["tol"], maxiter=g["meta"]["maxiter"], residuals=res)
    assert len(res) == len(g["residuals"]) == 10
    golden_io.assert_history(res, g["residuals"], A, x, g["b"])
