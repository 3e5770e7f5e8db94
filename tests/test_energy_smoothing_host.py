"""Energy-minimisation prolongation smoothing, host route (pyamg_amd/smooth.py, csrc/setup_host.cpp) against the
reference's fixtures of tests/golden/energy/ -- no device needed."""
import ctypes
import os

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sps

import energy_io as eio
import golden_io
import oracle_lib
import pyamg_amd
from pyamg_amd import _host, aggregation, amg_core, smooth
from pyamg_amd.aggregation import host_lib
from pyamg_amd.smooth import energy_prolongation_smoother

LIB = os.path.join(os.path.dirname(os.path.abspath(pyamg_amd.__file__)), "lib", "libamgcore_hip.so")
FLAT = {"incomplete_mat_mult_bsr": 14, "satisfy_constraints_helper": 10, "calc_BtB": 8}
NATIVE_ARGS = {"incomplete_mat_mult_bsr": 9 * 2 + 5, "satisfy_constraints_helper": 4 + 6 * 2, "calc_BtB": 3 + 2 + 1 + 3 * 2}

# Against the reference the host route agrees to rounding, not bit for bit: the two inner products add in another order
# than scipy's sum, and BtBinv comes from LAPACK's gelss.  Measured on the development machine with the deviation()
# measure (the same() measure of tests/test_setup_golden.py), the largest over all problems and option sets, once per
# OpenBLAS kernel set (OPENBLAS_CORETYPE = Haswell, SkylakeX, Zen, Sandybridge, Nehalem, Prescott): 1.041e-13 for P
# (9.08e-16 with the machine's own kernel set), 3.007e-13 for the operators of the two hierarchies; sparsity identical
# in every run.  Allowed: ten times that.
MEASURED_P = 1.041e-13
MEASURED_HIER = 3.007e-13
RTOL_P = 10 * MEASURED_P
RTOL_HIER = 10 * MEASURED_HIER

ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


# ---------------------------------------------------------------------------------------------- names
def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(LIB)
    from pyamg_amd import _lib
    L = _lib.lib()
    for name, n_args in FLAT.items():
        assert hasattr(raw, "amgcore_%s_f64" % name), name
        assert not hasattr(raw, "amgcore_%s_f32" % name)
        assert name in amg_core.__all__ and callable(getattr(amg_core, name))
        assert name in _lib.FLAT_TABLE and name in _lib.FLAT_F64_ONLY
        kinds, sized = _lib.FLAT_TABLE[name]
        assert len(kinds) == n_args and sized
        assert len(getattr(L, "amgcore_%s_f64" % name).argtypes) == NATIVE_ARGS[name]
    assert hasattr(raw, "amg_energy_smooth_device") and hasattr(raw, "amg_energy_fetch")
    assert len(L.amg_energy_smooth_device.argtypes) == 20 and len(L.amg_energy_fetch.argtypes) == 2
    assert "energy_prolongation_smoother" in aggregation.__all__
    assert aggregation.energy_prolongation_smoother is energy_prolongation_smoother
    assert "jacobi_prolongation_smoother" in aggregation.__all__
    assert smooth.DEVICE_AUTO is False


def test_flat_entries_take_float64_only():
    p = np.array([0, 1], dtype=np.intc); j = np.array([0], dtype=np.intc)
    f = np.ones(1, dtype=np.float32)
    with pytest.raises(NotImplementedError):
        amg_core.incomplete_mat_mult_bsr(p, j, f, p, j, f, p, j, f, 1, 1, 1, 1, 1)
    with pytest.raises(NotImplementedError):
        amg_core.calc_BtB(1, 1, 1, np.ones(1, dtype=np.complex128), 1, np.ones(1, dtype=np.complex128), p, j)
    with pytest.raises(NotImplementedError):
        amg_core.satisfy_constraints_helper(1, 1, 1, 1, np.ones(1), np.ones(1), np.ones(1), p.astype(np.int64), j, np.ones(1))


# ---------------------------------------------------------------------------------------------- the native loops
def host_call(kernel, a):
    """one recorded call through the loops of csrc/setup_host.cpp -> the output array"""
    L = host_lib()
    c = lambda v: np.ascontiguousarray(v)
    if kernel == "incomplete_mat_mult_bsr":
        Sx = a["Sx"].copy()
        L.amgsetup_incomplete_mat_mult_bsr(ip(c(a["Ap"])), ip(c(a["Aj"])), dp(c(a["Ax"])), ip(c(a["Bp"])), ip(c(a["Bj"])), dp(c(a["Bx"])),
                                           ip(c(a["Sp"])), ip(c(a["Sj"])), dp(Sx), a["n_brow"], a["n_bcol"], a["brow_A"], a["bcol_A"],
                                           a["bcol_B"])
        return Sx
    if kernel == "satisfy_constraints_helper":
        Sx = a["Sx"].copy()
        L.amgsetup_satisfy_constraints_helper(a["RowsPerBlock"], a["ColsPerBlock"], a["num_block_rows"], a["NullDim"], dp(c(a["x"])),
                                              dp(c(a["y"])), dp(c(a["z"])), ip(c(a["Sp"])), ip(c(a["Sj"])), dp(Sx))
        return Sx
    x = a["x"].copy()
    L.amgsetup_calc_BtB(a["NullDim"], a["Nnodes"], a["ColsPerBlock"], dp(c(a["b"])), a["BsqCols"], dp(x), ip(c(a["Sp"])), ip(c(a["Sj"])))
    return x


def model_call(kernel, a):
    if kernel == "incomplete_mat_mult_bsr":
        return eio.model_incomplete_mat_mult_bsr(*[a[k] for k in eio.ARGS[kernel]])
    if kernel == "satisfy_constraints_helper":
        return eio.model_satisfy_constraints(*[a[k] for k in eio.ARGS[kernel]])
    return eio.model_calc_BtB(a["NullDim"], a["Nnodes"], a["ColsPerBlock"], a["b"], a["BsqCols"], a["Sp"], a["Sj"])


def test_fixtures_hold_calls_of_all_three_kernels():
    kinds = [eio.problem(n)["sets"][q]["calls"][ci][0] for n, q, ci in eio.recorded_calls()]
    assert len(eio.recorded_calls("calc_BtB")) == len(eio.all_sets())
    assert kinds.count("incomplete_mat_mult_bsr") >= 20 and kinds.count("satisfy_constraints_helper") >= 20
    shapes = set()
    for n, q, ci in eio.recorded_calls("incomplete_mat_mult_bsr"):
        a = eio.problem(n)["sets"][q]["calls"][ci][1]
        shapes.add((a["brow_A"], a["bcol_A"], a["bcol_B"]))
    assert shapes == {(1, 1, 1), (2, 2, 3), (3, 3, 6)}


@pytest.mark.parametrize("name", eio.PROBLEMS)
def test_host_loops_reproduce_every_recorded_call(name):
    n = 0
    for q, s in enumerate(eio.problem(name)["sets"]):
        for ci, (kernel, args, want) in enumerate(s["calls"]):
            got = host_call(kernel, args)
            assert np.array_equal(got, want), "%s set %d call %d (%s): worst %g" % (name, q, ci, kernel, np.abs(got - want).max())
            n += 1
    assert n >= len(eio.problem(name)["sets"])


# the 40 x 40 problems keep calc_BtB only; the sequential models run every recorded call of the other four
@pytest.mark.parametrize("name", eio.PROBLEMS)
def test_python_models_reproduce_the_recorded_calls(name):
    for q, s in enumerate(eio.problem(name)["sets"]):
        for ci, (kernel, args, want) in enumerate(s["calls"]):
            got = model_call(kernel, args)
            assert np.array_equal(got, want), "%s set %d call %d (%s): worst %g" % (name, q, ci, kernel, np.abs(got - want).max())


def test_duplicate_column_in_a_row_of_S_goes_to_the_later_slot():
    one = np.array([0, 1], dtype=np.intc)
    Sp = np.array([0, 2], dtype=np.intc); Sj = np.array([0, 0], dtype=np.intc)
    Sx = np.array([5.0, 7.0])
    host_lib().amgsetup_incomplete_mat_mult_bsr(ip(one), ip(Sj[:1]), dp(np.array([2.0])), ip(one), ip(Sj[:1]), dp(np.array([3.0])),
                                                ip(Sp), ip(Sj), dp(Sx), 1, 1, 1, 1, 1)
    assert np.array_equal(Sx, [5.0, 13.0])
    assert np.array_equal(eio.model_incomplete_mat_mult_bsr(one, Sj[:1], np.array([2.0]), one, Sj[:1], np.array([3.0]), Sp, Sj,
                                                            np.array([5.0, 7.0]), 1, 1, 1, 1, 1), [5.0, 13.0])


@pytest.mark.parametrize("n_brow", [1, 255, 256, 257, 70000])
def test_inner_product_is_the_model_for_any_thread_count(n_brow):
    rng = np.random.RandomState(n_brow)
    counts = rng.randint(0, 4, n_brow)
    Sp = np.concatenate([[0], np.cumsum(counts)]).astype(np.intc)
    X = rng.uniform(-1.0, 1.0, int(Sp[-1]) * 2); Y = rng.uniform(-1.0, 1.0, X.size)
    X[rng.rand(X.size) < 0.2] = 0.0
    want = eio.model_inner_product(n_brow, 2, Sp, X, Y)
    L = host_lib()
    keep = L.amgsetup_num_threads()
    try:
        for threads in (1, 3, keep):
            L.amgsetup_set_num_threads(threads)
            out = np.empty(2)
            L.amgsetup_energy_inner_product(n_brow, 2, ip(Sp), dp(X), dp(Y), dp(out))
            assert (out[0], out[1]) == want
    finally:
        L.amgsetup_set_num_threads(keep)


def test_block_row_product_is_the_model():
    p = eio.problem("c5_elasticity")
    s = p["sets"][0]
    R, Cc = p["T"].blocksize
    ND = p["Bc"].shape[1]
    n_brow = len(s["Sp"]) - 1
    Ux = np.random.RandomState(4).uniform(-1.0, 1.0, len(s["Sj"]) * R * Cc)
    UB = np.empty(n_brow * R * ND)
    Bc = np.ascontiguousarray(p["Bc"]).ravel()
    host_lib().amgsetup_energy_block_row_product(n_brow, R, Cc, ND, ip(s["Sp"]), ip(s["Sj"]), dp(Ux), dp(Bc), dp(UB))
    assert np.array_equal(UB, eio.model_block_row_product(n_brow, R, Cc, ND, s["Sp"], s["Sj"], Ux, Bc))


# ---------------------------------------------------------------------------------------------- the smoother
@pytest.mark.parametrize("name,q", eio.all_sets())
def test_host_route_against_the_reference(name, q):
    p = eio.problem(name)
    s = p["sets"][q]
    A0, T0, B0 = p["A"].copy(), p["T"].copy(), p["Bc"].copy()
    trace = []
    P = energy_prolongation_smoother(p["A"], p["T"], p["Atilde"], p["Bc"], None, (False, {}), device=False, _trace=trace,
                                     **s["options"])
    G = s["P"]
    # pattern and B_i^T B_i bit for bit
    R, Cc = p["T"].blocksize
    Sp, Sj = smooth.sparsity_pattern(sps.bsr_matrix(p["T"]), p["Atilde"], s["options"]["degree"])
    assert np.array_equal(Sp, s["Sp"]) and np.array_equal(Sj, s["Sj"])
    (kernel, args, want), = [c for c in s["calls"] if c[0] == "calc_BtB"]
    assert np.array_equal(smooth.calc_BtB(np.ascontiguousarray(p["Bc"]), Sp, Sj, len(Sp) - 1, Cc).ravel(), want)
    # the result: identical sparsity, values to the measured tolerance, constraints kept
    assert sps.isspmatrix_bsr(P) and P.blocksize == G.blocksize == (R, Cc)
    assert np.array_equal(P.indptr, G.indptr) and np.array_equal(P.indices, G.indices)
    dev = eio.deviation(P, G)
    print("%s %r: deviation %.3e (allowed %.3e)" % (name, s["options"], dev, RTOL_P))
    assert dev <= RTOL_P
    assert np.abs(P * p["Bc"] - p["B"]).max() <= 1e-12 * np.abs(p["B"]).max()
    # the iteration took the reference's course: as many started iterations, the same break
    ref = s["trace"]
    assert len(trace) == len(ref)
    for mine, theirs in zip(trace, ref):
        assert abs(mine[0] - theirs[0]) <= 1e-9 * abs(theirs[0]) + 1e-25
        if not np.isnan(theirs[1]):
            assert abs(mine[0] / mine[1] - theirs[1]) <= 1e-9 * abs(theirs[1])
    # the caller's arrays are untouched
    for M, M0 in ((p["A"], A0), (p["T"], T0)):
        assert np.array_equal(M.data, M0.data) and np.array_equal(M.indices, M0.indices) and np.array_equal(M.indptr, M0.indptr)
    assert np.array_equal(p["Bc"], B0)


def test_early_break_fixture_breaks_at_iteration_two():
    for name in ("aniso_40x40_symmetric", "aniso_40x40_evolution"):
        s = eio.problem(name)["sets"][4]
        assert s["options"]["tol"] == 0.5 and s["options"]["maxiter"] == 6
        assert len(s["trace"]) == 3 and s["trace"][2, 0] < 0.5 < s["trace"][1, 0]


def test_zero_rule_of_the_pseudo_inverse_is_reached():
    s = eio.problem("random_spd_150")["sets"][0]
    (kernel, args, BtB), = [c for c in s["calls"] if c[0] == "calc_BtB"]
    assert np.count_nonzero(BtB == 0.0) > 0 and np.array_equal(s["BtBinv"][BtB == 0.0], np.zeros(np.count_nonzero(BtB == 0.0)))
    At = eio.problem("random_spd_150")["Atilde"]
    assert At.indptr[10] == At.indptr[9]


def test_csr_operands_and_default_strength():
    p = eio.problem("aniso_17x23")
    s = p["sets"][0]
    T = sps.csr_matrix(p["T"])
    P = energy_prolongation_smoother(sps.csr_matrix(p["A"]), T, p["Atilde"], p["Bc"], None, (False, {}), **s["options"])
    Pb = energy_prolongation_smoother(p["A"].tobsr(blocksize=(1, 1)), p["T"], p["Atilde"], p["Bc"], None, (False, {}), **s["options"])
    eio.same_bits(P, Pb)
    assert P.blocksize == (1, 1)
    # Atilde = None: A's own pattern
    Pn = energy_prolongation_smoother(p["A"], p["T"], None, p["Bc"], None, (False, {}), **s["options"])
    ones = sps.csr_matrix((np.ones(p["A"].nnz), p["A"].indices, p["A"].indptr), shape=p["A"].shape)
    eio.same_bits(Pn, energy_prolongation_smoother(p["A"], p["T"], ones, p["Bc"], None, (False, {}), **s["options"]))


def test_maxiter_zero_and_empty_operands_return_the_tentative_prolongator():
    p = eio.problem("aniso_17x23")
    T = sps.bsr_matrix(p["T"])
    P = energy_prolongation_smoother(p["A"], T, p["Atilde"], p["Bc"], None, (False, {}), maxiter=0)
    eio.same_bits(P, T)
    empty = sps.bsr_matrix(T.shape, dtype=np.float64, blocksize=(1, 1))
    P = energy_prolongation_smoother(p["A"], empty, p["Atilde"], p["Bc"], None, (False, {}))
    assert P.nnz == 0 and P.shape == T.shape


def test_vanishing_residual_stops_before_the_first_step():
    # A T = 0 on the pattern: T spans the kernel of a graph Laplacian block by block
    n = 12
    L1 = sps.diags([-np.ones(n - 1), np.r_[1.0, 2 * np.ones(n - 2), 1.0], -np.ones(n - 1)], [-1, 0, 1], format="csr")
    A = sps.block_diag([L1, L1], format="csr")
    T = sps.csr_matrix(sps.block_diag([np.ones((n, 1)), np.ones((n, 1))]))
    Bc = np.ones((2, 1)) * np.sqrt(n)
    trace = []
    P = energy_prolongation_smoother(A, T, None, Bc, None, (False, {}), _trace=trace)
    assert len(trace) == 1 and trace[0][0] == 0.0
    eio.same_bits(P, sps.bsr_matrix(T, blocksize=(1, 1)))


def test_tentative_prolongator_outside_the_pattern_takes_the_host_route(monkeypatch):
    from pyamg_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    p = eio.problem("aniso_17x23")
    At = sps.lil_matrix(p["Atilde"])
    At.setdiag(0.0)
    At[5, :] = 0.0                          # an empty row of Atilde: row 5 of the pattern is empty, row 5 of T is not
    At = sps.csr_matrix(At); At.eliminate_zeros()
    Sp, Sj = smooth.sparsity_pattern(sps.bsr_matrix(p["T"]), At, 1)
    assert Sp[6] == Sp[5]
    monkeypatch.setattr(smooth, "DEVICE_AUTO", True)
    monkeypatch.setattr(_host, "device_present", lambda: True)
    monkeypatch.setattr(_lib, "lib", touched)
    P = energy_prolongation_smoother(p["A"], p["T"], At, p["Bc"], None, (False, {}))
    assert np.abs(P * p["Bc"] - p["B"]).max() <= 1e-12
    # every block of T is still there: the pattern alone would have lost them
    Tn = sps.csr_matrix(p["T"])
    assert np.all(np.asarray(sps.csr_matrix(P)[Tn.nonzero()]).ravel() != 0.0)
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        energy_prolongation_smoother(p["A"], p["T"], At, p["Bc"], None, (False, {}), device=True)


def test_device_none_falls_back_when_the_device_entry_refuses(monkeypatch):
    p = eio.problem("aniso_17x23")
    s = p["sets"][0]

    def refuses(*a, **k):
        raise NotImplementedError("the device entry refuses: outside the restated setup")
    want = energy_prolongation_smoother(p["A"], p["T"], p["Atilde"], p["Bc"], None, (False, {}), device=False, **s["options"])
    monkeypatch.setattr(smooth, "DEVICE_AUTO", True)
    monkeypatch.setattr(_host, "device_present", lambda: True)
    monkeypatch.setattr(smooth, "_cg_device", refuses)
    got = energy_prolongation_smoother(p["A"], p["T"], p["Atilde"], p["Bc"], None, (False, {}), **s["options"])
    eio.same_bits(got, want)
    with pytest.raises(NotImplementedError):
        energy_prolongation_smoother(p["A"], p["T"], p["Atilde"], p["Bc"], None, (False, {}), device=True, **s["options"])


def test_device_none_is_the_host_route(monkeypatch):
    from pyamg_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(_lib, "device_count", touched)
    p = eio.problem("aniso_17x23")
    P = energy_prolongation_smoother(p["A"], p["T"], p["Atilde"], p["Bc"], None, (False, {}))
    assert eio.deviation(P, p["sets"][0]["P"]) <= RTOL_P


# ---------------------------------------------------------------------------------------------- refusals
def _call(**kw):
    p = eio.problem("aniso_17x23")
    a = dict(A=p["A"], T=p["T"], Atilde=p["Atilde"], B=p["Bc"], Bf=None, Cpt_params=(False, {}))
    a.update(kw)
    return energy_prolongation_smoother(a.pop("A"), a.pop("T"), a.pop("Atilde"), a.pop("B"), a.pop("Bf"), a.pop("Cpt_params"), **a)


@pytest.mark.parametrize("kw", [dict(krylov="cgnr"), dict(krylov="gmres"), dict(weighting="block"), dict(prefilter={"theta": 0.1}),
                                dict(postfilter={"k": 3}), dict(Cpt_params=(True, {}))])
def test_refusals_before_any_device_work(kw, monkeypatch):
    from pyamg_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(_lib, "device_count", touched)
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        _call(device=True, **kw)


@pytest.mark.parametrize("case", ["complex_A", "float32_A", "complex_B", "float32_T"])
def test_value_types_outside_the_restated_setup(case):
    p = eio.problem("aniso_17x23")
    kw = {}
    if case == "complex_A":
        kw["A"] = p["A"].astype(np.complex128)
    elif case == "float32_A":
        kw["A"] = p["A"].astype(np.float32)
    elif case == "complex_B":
        kw["B"] = p["Bc"] + 0j
    else:
        kw["T"] = p["T"].astype(np.float32)
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        _call(**kw)


def test_reference_errors():
    p = eio.problem("elasticity_12x12")
    with pytest.raises(ValueError):
        _call(maxiter=-1)
    with pytest.raises(ValueError):
        _call(tol=1.5)
    with pytest.raises(TypeError):
        _call(A=eio.problem("aniso_17x23")["A"].tocsc())
    with pytest.raises(TypeError):
        _call(T=sps.csc_matrix(eio.problem("aniso_17x23")["T"]))
    with pytest.raises(TypeError):
        _call(Atilde=eio.problem("aniso_17x23")["Atilde"].tocsc())
    with pytest.raises(ValueError):          # T row-blocksize should be the same as A blocksize
        _call(A=p["A"], T=sps.bsr_matrix(sps.csr_matrix(p["T"]), blocksize=(1, 3)), Atilde=p["Atilde"], B=p["Bc"])
    with pytest.raises(ValueError):          # num_rows(B) = num_cols(T)
        _call(B=np.ones((3, 1)))
    with pytest.raises(ValueError):
        _call(weighting="rowsum")


# ---------------------------------------------------------------------------------------------- the driver
def test_fast_paths_decline_an_energy_descriptor():
    p = eio.problem("aniso_17x23")
    e = ("energy", {"maxiter": 4})
    assert aggregation._scalar_fast_path_ok(p["A"], np.ones((p["A"].shape[0], 1)), "symmetric", "standard", ("jacobi", {}))
    assert not aggregation._scalar_fast_path_ok(p["A"], np.ones((p["A"].shape[0], 1)), "symmetric", "standard", e)
    assert not aggregation._scalar_fast_path_ok(p["A"], np.ones((p["A"].shape[0], 1)), "symmetric", "standard", "energy")
    Ab = eio.problem("c5_elasticity")["A"]
    assert aggregation._block_fast_path_ok(Ab, None, "symmetric", "standard", ("jacobi", {}))
    assert not aggregation._block_fast_path_ok(Ab, None, "symmetric", "standard", e)


GS = ("block_gauss_seidel", {"sweep": "symmetric"})
ENERGY = ("energy", {"krylov": "cg", "maxiter": 4, "degree": 1, "weighting": "local"})
HIERARCHIES = {"sa_evolution_energy_2d": (dict(strength=("evolution", {"k": 2, "epsilon": 4.0}), max_coarse=20), [1600, 280, 56, 10], 27),
               "elas_energy_2d": (dict(max_coarse=10), [288, 48, 9], 9)}


def build_hierarchy(name, **extra):
    kw, sizes, cycles = HIERARCHIES[name]
    g = eio.load_hier(name)
    kw = dict(kw)
    if name == "elas_energy_2d":
        kw["B"] = np.load(os.path.join(eio.ENERGY, "hier_%s.npz" % name), allow_pickle=False)["B0"]
    smooth_opt = (ENERGY[0], dict(ENERGY[1], **extra))
    np.random.seed(0)
    ml = pyamg_amd.smoothed_aggregation_solver(g["levels"][0]["A"], smooth=smooth_opt, presmoother=GS, postsmoother=GS, **kw)
    return g, ml


@pytest.fixture(scope="module", params=sorted(HIERARCHIES))
def built(request):
    return (request.param,) + build_hierarchy(request.param)


def test_hierarchy_level_sizes_and_block_shapes(built):
    name, g, ml = built
    sizes = HIERARCHIES[name][1]
    assert [lvl.A.shape[0] for lvl in ml.levels] == sizes == [L["A"].shape[0] for L in g["levels"]]
    want = {"sa_evolution_energy_2d": [(1, 1)] * 3, "elas_energy_2d": [(2, 3), (3, 3)]}[name]
    assert [lvl.P.blocksize for lvl in ml.levels[:-1]] == want == [L["P"].blocksize for L in g["levels"][:-1]]


def test_hierarchy_operators(built):
    name, g, ml = built
    worst = 0.0
    for lvl, G in zip(ml.levels, g["levels"]):
        worst = max(worst, eio.deviation(lvl.A, G["A"]))         # asserts identical sparsity
        if "P" in G:
            worst = max(worst, eio.deviation(lvl.P, G["P"]), eio.deviation(lvl.R, G["R"]))
    print("%s: deviation %.3e (allowed %.3e)" % (name, worst, RTOL_HIER))
    assert worst <= RTOL_HIER


def test_hierarchy_solve_history(built):
    name, g, ml = built
    levels = []
    for lvl, G in zip(ml.levels, g["levels"]):
        L = {"A": lvl.A}
        if "P" in G:
            L.update(P=lvl.P, R=lvl.R, pre=G["pre"], post=G["post"])
        levels.append(L)
    pinv = np.ascontiguousarray(scipy.linalg.pinv(ml.levels[-1].A.toarray()))
    H = oracle_lib.Hierarchy(levels, pinv)
    x, res = H.solve(g["b"], tol=g["meta"]["tol"], maxiter=g["meta"]["maxiter"])
    assert len(res) - 1 == len(g["residuals"]) - 1 == HIERARCHIES[name][2]
    golden_io.assert_history(res, g["residuals"], g["levels"][0]["A"], g["x"], g["b"])


def test_other_smoother_names_are_still_refused():
    A = eio.problem("aniso_17x23")["A"]
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        pyamg_amd.smoothed_aggregation_solver(A, smooth="richardson", max_coarse=4)
