"""Root-node smoothed aggregation on the host (pyamg_amd/rootnode.py, the root-node rules of pyamg_amd/smooth.py, the
helpers of pyamg_amd/util.py, csrc/setup_host.cpp) against the reference's fixtures of tests/golden/rootnode/ -- no
device needed."""
import ctypes

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sps

import energy_io as eio
import golden_io
import oracle_lib
import rootnode_io as rio
import pyamg_amd
from pyamg_amd import amg_core, smooth, util
from pyamg_amd.aggregation import host_lib
from pyamg_amd.smooth import energy_prolongation_smoother

# Against the reference the host route agrees to rounding (the inner products add in another order than scipy's sum,
# BtBinv and the root blocks of scale_T come from LAPACK's gelss).  Measured on the development machine with the
# deviation() measure (the same() measure of tests/test_setup_golden.py), the largest over all problems and option sets
# (the fitted T of maxiter=0 included), once per OpenBLAS kernel set; sparsity identical in every run:
#   OPENBLAS_CORETYPE   scale_T      P           operators of the three hierarchies
#   Haswell, Zen        0            1.821e-14   7.990e-14
#   SkylakeX (native)   0            4.996e-16   1.872e-14
#   Sandybridge, Nehalem, Prescott
#                       0            1.882e-14   8.000e-14
# Allowed: ten times the largest.  scale_T came out bit for bit in all six; a measured zero gives no scale, so its bound
# is ten times one unit roundoff, the smallest deviation the measure could have shown.
MEASURED_T = np.finfo(np.float64).eps
MEASURED_P = 1.882e-14
MEASURED_HIER = 8.000e-14
RTOL_T = 10 * MEASURED_T
RTOL_P = 10 * MEASURED_P
RTOL_HIER = 10 * MEASURED_HIER

ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def same_arrays(M, G):
    assert M.shape == G.shape and M.blocksize == G.blocksize
    assert np.array_equal(M.indptr, G.indptr) and np.array_equal(M.indices, G.indices) and np.array_equal(M.data, G.data)


def params_of(p):
    return util.get_Cpt_params(p["A"], p["Cnodes"], p["AggOp"], p["T0"])


def smoothed(p, s, **kw):
    return energy_prolongation_smoother(p["A"], p["T"], p["Atilde"], p["Bc"], p["B"], (True, p["params"]), **dict(s["options"], **kw))


# ---------------------------------------------------------------------------------------------- names
def test_names_exported_and_bound():
    from pyamg_amd import _lib, rootnode
    assert "rootnode_solver" in pyamg_amd.__all__ and pyamg_amd.rootnode_solver is rootnode.rootnode_solver
    for name in ("get_Cpt_params", "scale_T", "filter_operator", "filter_matrix_rows", "truncate_rows"):
        assert name in util.__all__ and callable(getattr(util, name))
    assert "truncate_rows_csr" in amg_core.__all__ and "truncate_rows_csr" in _lib.FLAT_F64_ONLY
    assert _lib.FLAT_TABLE["truncate_rows_csr"] == ("iiIIV", True)
    L = _lib.lib()
    assert len(L.amg_energy_smooth_rootnode_device.argtypes) == 22 and len(L.amg_energy_smooth_device.argtypes) == 20
    assert smooth.DEVICE_AUTO is False


# ---------------------------------------------------------------------------------------------- the helpers
@pytest.mark.parametrize("name", rio.PROBLEMS)
def test_get_Cpt_params_and_scale_T(name):
    p = rio.problem(name)
    par = params_of(p)
    for k in ("P_I", "I_F", "I_C"):
        assert sps.isspmatrix_bsr(par[k])
        same_arrays(par[k], p["params"][k])
    assert par["Cpts"].dtype == np.dtype(int)
    assert np.array_equal(par["Cpts"], p["params"]["Cpts"]) and np.array_equal(par["Fpts"], p["params"]["Fpts"])
    T0 = p["T0"].copy()
    T = util.scale_T(p["T0"], par["P_I"], par["I_F"])
    assert np.array_equal(T.indptr, p["T"].indptr) and np.array_equal(T.indices, p["T"].indices)
    dev = eio.deviation(T, p["T"])
    print("%s: scale_T deviation %.3e (allowed %.3e)" % (name, dev, RTOL_T))
    assert dev <= RTOL_T
    assert rio.rows_are_identity(T, par["Cpts"])
    assert np.array_equal(p["T0"].data, T0.data)


def test_trivial_coarse_grid_has_no_root():
    A = sps.identity(4, format="csr")
    AggOp = sps.csr_matrix((4, 1), dtype=np.int8)
    T = sps.bsr_matrix((4, 1), blocksize=(1, 1), dtype=np.float64)
    par = util.get_Cpt_params(A, np.array([], dtype=np.intc), AggOp, T)
    assert par["P_I"].nnz == 0 and par["P_I"].shape == (4, 1) and par["I_C"].nnz == 0 and par["I_F"].nnz == 4
    assert len(par["Cpts"]) == 0 and np.array_equal(par["Fpts"], np.arange(4))
    assert util.scale_T(T, par["P_I"], par["I_F"]) is T


def test_host_quicksort_reproduces_every_truncation_bit_for_bit():
    L = host_lib()
    cases = [(a["n_row"], a["k"], a["Sp"], a["Sj"], a["Sx"], o["Sj"], o["Sx"]) for a, o in rio.recorded_calls("truncate_rows_csr")]
    assert len(cases) >= 3
    cases += [(len(Sp) - 1, k, Sp, Sj, Sx, wj, wx) for k, Sp, Sj, Sx, wj, wx in rio.crafted_truncations()]
    changed = 0
    for n_row, k, Sp, Sj, Sx, wj, wx in cases:
        j, x = Sj.copy(), Sx.copy()
        L.amgsetup_truncate_rows_csr(n_row, k, ip(Sp), ip(j), dp(x))
        assert np.array_equal(j, wj) and np.array_equal(x, wx)
        mj, mx = rio.model_truncate_rows_csr(n_row, k, Sp, Sj, Sx)
        assert np.array_equal(mj, wj) and np.array_equal(mx, wx)
        changed += int(not np.array_equal(Sj, wj))
        # util.truncate_rows: the same entries, zeros removed
        M = sps.csr_matrix((Sx, Sj, Sp), shape=(n_row, int(Sj.max()) + 1 if len(Sj) else 1))
        F = util.truncate_rows(M, k)
        W = sps.csr_matrix((wx.copy(), wj.copy(), Sp.copy()), shape=M.shape); W.eliminate_zeros(); W.prune()
        assert np.array_equal(F.indptr, W.indptr) and np.array_equal(F.indices, W.indices) and np.array_equal(F.data, W.data)
        assert np.array_equal(M.data, Sx) and np.array_equal(M.indices, Sj) and M.indptr[-1] == len(Sx)
    assert changed >= 4


def test_crafted_truncations_hold_the_tie_cases():
    lengths = set()
    for k, Sp, Sj, Sx, wj, wx in rio.crafted_truncations():
        lengths |= set(np.diff(Sp).tolist())
    assert {0, 1, 4, 5, 65, 300} <= lengths
    k, Sp, Sj, Sx, wj, wx = [c for c in rio.crafted_truncations() if c[0] == 4][0]
    assert any(len(set(np.abs(Sx[Sp[i]:Sp[i + 1]]))) == 1 and Sp[i + 1] - Sp[i] > 4 for i in range(len(Sp) - 1))


def test_filter_matrix_rows_reproduces_the_recorded_strength_calls():
    calls = rio.recorded_calls("classical_strength_of_connection")
    assert len(calls) >= 2
    for a, o in calls:
        n = a["n_row"]
        M = sps.csr_matrix((a["Ax"], a["Aj"] - n, a["Ap"]), shape=(n, int((a["Aj"] - n).max()) + 1))
        F = util.filter_matrix_rows(M, a["theta"])
        nnz = o["Sp"][-1]
        assert np.array_equal(F.indptr, o["Sp"]) and np.array_equal(F.indices, o["Sj"][:nnz] - n) and np.array_equal(F.data, o["Sx"][:nnz])
    with pytest.raises(ValueError):
        util.filter_matrix_rows(M, 1.0)


def test_filter_operator_fits_the_candidates():
    p = rio.problem("elasticity_12x12")
    s = p["sets"][0]
    Sp, Sj, _ = s["passes"][0]
    R, Cc = p["T"].blocksize
    pattern = sps.bsr_matrix((np.ones((len(Sj), R, Cc)), Sj, Sp), shape=p["T"].shape)
    F = util.filter_operator(p["T"], pattern, p["Bc"], p["B"])
    F = sps.bsr_matrix(p["params"]["I_F"] * F + p["params"]["P_I"])
    G = s["fits"][0]
    assert np.array_equal(F.indptr, G.indptr) and np.array_equal(F.indices, G.indices)
    assert eio.deviation(F, G) <= RTOL_P
    # scalar operands in CSR
    A = sps.csr_matrix(np.array([[1.0, 1, 1], [1, 1, 1], [0, 1, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1]]))
    Cm = sps.csr_matrix(np.array([[1.0, 1, 0], [1, 1, 0], [0, 1, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1]]))
    got = util.filter_operator(A, Cm, np.ones((3, 1)), np.ones((6, 1)))
    assert sps.isspmatrix_csr(got)
    assert np.allclose(got.toarray(), [[0.5, 0.5, 0], [0.5, 0.5, 0], [0, 1, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1]], atol=1e-15)


# ---------------------------------------------------------------------------------------------- the smoother
@pytest.mark.parametrize("name,q", rio.all_sets())
def test_host_route_against_the_reference(name, q):
    p = rio.problem(name)
    s = p["sets"][q]
    opt = s["options"]
    A0, T0 = p["A"].copy(), p["T"].copy()
    # the pattern of the first pass, pre-filtered ones included, bit for bit
    R, Cc = p["T"].blocksize
    n_brow, n_bcol = p["T"].shape[0] // R, p["T"].shape[1] // Cc
    root_row, IF, PI = smooth._root_structure(p["params"]["P_I"], p["params"]["I_F"], n_brow, n_bcol, R, Cc)
    Sp, Sj = smooth.sparsity_pattern(sps.bsr_matrix(p["T"]), p["Atilde"], opt["degree"], opt.get("prefilter", {}), (IF, PI))
    assert np.array_equal(Sp, s["passes"][0][0]) and np.array_equal(Sj, s["passes"][0][1])
    assert np.array_equal(np.diff(Sp)[root_row], np.ones(n_bcol)) and np.array_equal(Sj[Sp[root_row]], np.arange(n_bcol))
    trace = []
    P = smoothed(p, s, device=False, _trace=trace)
    G = s["P"]
    assert sps.isspmatrix_bsr(P) and P.blocksize == G.blocksize == (R, Cc)
    assert np.array_equal(P.indptr, G.indptr) and np.array_equal(P.indices, G.indices)
    dev = eio.deviation(P, G)
    print("%s %r: deviation %.3e (allowed %.3e)" % (name, opt, dev, RTOL_P))
    assert dev <= RTOL_P
    assert rio.rows_are_identity(P, p["params"]["Cpts"])
    # the iteration took the reference's course in every pass
    ref = np.concatenate(s["traces"])
    assert len(trace) == len(ref) and len(s["traces"]) == (2 if opt.get("postfilter") else 1)
    for mine, theirs in zip(trace, ref):
        assert abs(mine[0] - theirs[0]) <= 1e-9 * abs(theirs[0]) + 1e-25
        if not np.isnan(theirs[1]):
            assert abs(mine[0] / mine[1] - theirs[1]) <= 1e-9 * abs(theirs[1])
    for M, M0 in ((p["A"], A0), (p["T"], T0)):
        assert np.array_equal(M.data, M0.data) and np.array_equal(M.indices, M0.indices) and np.array_equal(M.indptr, M0.indptr)


@pytest.mark.parametrize("name", ["elasticity_12x12", "c5_elasticity"])
def test_initial_fit_is_the_result_of_maxiter_zero(name):
    p = rio.problem(name)
    s = p["sets"][0]
    assert p["Bc"].shape[1] > p["A"].blocksize[0] and len(s["fits"]) == 1
    P = smoothed(p, s, device=False, maxiter=0)
    G = s["fits"][0].copy(); G.eliminate_zeros()
    assert np.array_equal(P.indptr, G.indptr) and np.array_equal(P.indices, G.indices)
    assert eio.deviation(P, G) <= RTOL_P
    assert rio.rows_are_identity(P, p["params"]["Cpts"])


def test_prefilter_with_both_keys_is_the_union():
    p = rio.problem("aniso_17x23")
    T = sps.bsr_matrix(p["T"])
    k_only = smooth.sparsity_pattern(T, p["Atilde"], 2, {"k": 2})
    th_only = smooth.sparsity_pattern(T, p["Atilde"], 2, {"theta": 0.5})
    both = smooth.sparsity_pattern(T, p["Atilde"], 2, {"k": 2, "theta": 0.5})
    as_set = lambda S: set(zip(np.repeat(np.arange(len(S[0]) - 1), np.diff(S[0])).tolist(), S[1].tolist()))
    assert as_set(both) == as_set(k_only) | as_set(th_only)
    assert len(as_set(both)) > max(len(as_set(k_only)), len(as_set(th_only)))
    P = energy_prolongation_smoother(p["A"], p["T"], p["Atilde"], p["Bc"], p["B"], (True, p["params"]), degree=2,
                                     prefilter={"k": 2, "theta": 0.5})
    assert rio.rows_are_identity(P, p["params"]["Cpts"])
    # degree 0: T's own values are filtered
    P0 = energy_prolongation_smoother(p["A"], p["T"], p["Atilde"], p["Bc"], p["B"], (True, p["params"]), degree=0, prefilter={"k": 1})
    assert rio.rows_are_identity(P0, p["params"]["Cpts"])


# ---------------------------------------------------------------------------------------------- refusals
def _call(**kw):
    p = rio.problem("aniso_17x23")
    a = dict(A=p["A"], T=p["T"], Atilde=p["Atilde"], B=p["Bc"], Bf=p["B"], Cpt_params=(True, p["params"]))
    a.update(kw)
    return energy_prolongation_smoother(a.pop("A"), a.pop("T"), a.pop("Atilde"), a.pop("B"), a.pop("Bf"), a.pop("Cpt_params"), **a)


@pytest.mark.parametrize("kw", [dict(Cpt_params=(True, {})), dict(Cpt_params=(True, {"P_I": None})),
                                dict(prefilter={"k": 3}, Cpt_params=(False, {})), dict(postfilter={"theta": 0.1}, Cpt_params=(False, {})),
                                dict(krylov="cgnr"), dict(krylov="gmres"), dict(weighting="block")])
def test_smoother_refusals_before_any_device_work(kw, monkeypatch):
    from pyamg_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(_lib, "device_count", touched)
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        _call(device=True, **kw)


def test_unknown_filter_keys():
    with pytest.raises(ValueError, match="Unrecognized prefilter option"):
        _call(prefilter={"drop": 0.1})
    with pytest.raises(ValueError, match="Unrecognized prefilter option"):
        _call(prefilter={"k": 3, "tol": 0.1})
    with pytest.raises(ValueError, match="Unrecognized postfilter option"):
        _call(postfilter={"kk": 3})


def test_malformed_root_operators():
    p = rio.problem("aniso_17x23")
    P_I = p["params"]["P_I"].copy()
    P_I.data[0] = 2.0
    with pytest.raises(ValueError):
        _call(Cpt_params=(True, dict(p["params"], P_I=P_I)))
    with pytest.raises(ValueError):
        _call(Cpt_params=(True, dict(p["params"], I_F=sps.identity(p["A"].shape[0], format="csr").tobsr(blocksize=(1, 1)))))
    e = rio.problem("elasticity_12x12")
    with pytest.raises(ValueError):         # the fit needs the fine candidates
        energy_prolongation_smoother(e["A"], e["T"], e["Atilde"], e["Bc"], None, (True, e["params"]))


@pytest.mark.parametrize("kw", [dict(symmetry="nonsymmetric"), dict(diagonal_dominance=True), dict(aggregate="lloyd"),
                                dict(smooth="jacobi"), dict(strength="classical"), dict(smooth=("energy", {"krylov": "gmres"})),
                                dict(aggregate=["standard", "naive"]), "complex"])
def test_solver_refusals_before_any_level(kw, monkeypatch):
    from pyamg_amd import rootnode

    def touched(*a, **k):
        raise AssertionError("a level was built")
    monkeypatch.setattr(rootnode, "extend_hierarchy", touched)
    A = rio.problem("aniso_17x23")["A"]
    if kw == "complex":
        A, kw = A.astype(np.complex128), {}
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        pyamg_amd.rootnode_solver(A, max_coarse=4, **kw)


def test_solver_reference_errors():
    e = rio.problem("elasticity_12x12")
    with pytest.raises(ValueError):         # B.shape[1] < blocksize
        pyamg_amd.rootnode_solver(e["A"], B=np.ones((e["A"].shape[0], 1)))
    with pytest.raises(ValueError):
        pyamg_amd.rootnode_solver(e["A"], B=np.ones((5, 3)))
    with pytest.raises(ValueError):
        pyamg_amd.rootnode_solver(e["A"], symmetry="skew")
    with pytest.raises(ValueError):
        pyamg_amd.rootnode_solver(sps.csr_matrix(np.ones((3, 4))))


# ---------------------------------------------------------------------------------------------- the hierarchies
BUILD, build_hierarchy = rio.BUILD, rio.build_hierarchy


@pytest.fixture(scope="module", params=sorted(BUILD))
def built(request):
    return (request.param,) + build_hierarchy(request.param, keep=request.param == "rootnode_elas")


def test_hierarchy_level_sizes_and_roots(built):
    name, g, ml = built
    sizes = rio.HIERARCHIES[name][0]
    assert [lvl.A.shape[0] for lvl in ml.levels] == sizes == [L["A"].shape[0] for L in g["levels"]]
    for lvl, Cpts in zip(ml.levels[:-1], g["Cpts"]):
        assert np.array_equal(lvl.Cpts, Cpts)
        assert rio.rows_are_identity(lvl.P, lvl.Cpts)
    kept = [hasattr(ml.levels[0], k) for k in ("C", "AggOp", "T", "Fpts", "P_I", "I_F", "I_C")]
    assert all(kept) if name == "rootnode_elas" else not any(kept)


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
    assert len(res) - 1 == len(g["residuals"]) - 1 == rio.HIERARCHIES[name][1]
    golden_io.assert_history(res, g["residuals"], g["levels"][0]["A"], g["x"], g["b"])


def test_smooth_none_keeps_the_scaled_tentative_prolongator():
    A = rio.problem("aniso_17x23")["A"]
    np.random.seed(0)
    ml = pyamg_amd.rootnode_solver(A, smooth=None, max_coarse=40, keep=True)
    lvl = ml.levels[0]
    eio.same_bits(sps.bsr_matrix(lvl.P), sps.bsr_matrix(lvl.T))
    assert rio.rows_are_identity(lvl.P, lvl.Cpts)
    # the coarse candidates are the improved fine candidates injected at the roots
    assert np.array_equal(ml.levels[1].B, lvl.B[lvl.Cpts])


def test_predefined_aggregation_needs_its_root_nodes():
    p = rio.problem("aniso_17x23")
    with pytest.raises(ValueError):
        pyamg_amd.rootnode_solver(p["A"], aggregate=("predefined", {"AggOp": p["AggOp"]}))
    np.random.seed(0)
    ml = pyamg_amd.rootnode_solver(p["A"], aggregate=("predefined", {"AggOp": p["AggOp"], "Cnodes": p["Cnodes"]}), improve_candidates=None)
    assert len(ml.levels) == 2 and ml.levels[1].A.shape[0] == p["AggOp"].shape[1]
    assert eio.deviation(ml.levels[0].P, p["sets"][0]["P"]) <= RTOL_P


# ---------------------------------------------------------------------------------------------- non-interference
# sha256 over indptr, indices and data of the host route's P on tests/golden/energy/aniso_17x23 (one candidate: no LAPACK
# in BtBinv), taken from the commit before root-node smoothing existed
BEFORE = {1: "ba5550ac92d345178e378b79c2e3c5c8c7c6933aa607ca9b425c36c16993f8c9",
          2: "ce89457538a6397075dd35731525488949b8458f62ba08ab20f2ae13051947d3"}


def test_plain_energy_smoothing_and_sa_are_unchanged():
    import hashlib
    p = eio.problem("aniso_17x23")
    for s in p["sets"]:
        P = energy_prolongation_smoother(p["A"], p["T"], p["Atilde"], p["Bc"], None, (False, {}), device=False, **s["options"])
        G = s["P"]
        assert np.array_equal(P.indptr, G.indptr) and np.array_equal(P.indices, G.indices)
        assert eio.deviation(P, G) <= 10 * 1.041e-13           # the tolerance of tests/test_energy_smoothing_host.py
        digest = hashlib.sha256(P.indptr.tobytes() + P.indices.tobytes() + P.data.tobytes()).hexdigest()
        assert digest == BEFORE[s["options"]["degree"]]
    Sp, Sj = smooth.sparsity_pattern(sps.bsr_matrix(p["T"]), p["Atilde"], 1)
    assert np.array_equal(Sp, p["sets"][0]["Sp"]) and np.array_equal(Sj, p["sets"][0]["Sj"])
    # smoothed_aggregation_solver still goes through the plain smoother: no roots, and level 0 is that call's bits
    np.random.seed(0)
    ml = pyamg_amd.smoothed_aggregation_solver(p["A"], max_coarse=20, smooth=("energy", {"maxiter": 4}), keep=True)
    lvl = ml.levels[0]
    assert not hasattr(lvl, "Cpts") and [L.A.shape[0] for L in ml.levels] == [391, 48, 6]
    eio.same_bits(lvl.P, energy_prolongation_smoother(lvl.A, lvl.T, lvl.C, ml.levels[1].B, None, (False, {}), maxiter=4))
    assert not rio.rows_are_identity(lvl.P, rio.problem("aniso_17x23")["params"]["Cpts"])
