"""MIS(2) aggregation on the host (csrc/setup_host.cpp: amgsetup_mis_aggregation) against the definition of DESIGN.md
section 8l, restated in plain Python in tests/mis_cases.py, and aggregate='mis' in the two SA solvers."""
import numpy as np
import pytest
import scipy.sparse as sps

import mis_cases as mc
from pyamg_amd import _host, aggregation, rootnode_solver, smoothed_aggregation_solver
from pyamg_amd.aggregation import mis_aggregation, standard_aggregation
from pyamg_amd.gallery import poisson

SYMMETRIC = mc.symmetric_names()
PROBLEMS = {"poisson_40x40": (40, 40), "poisson_12x12x12": (12, 12, 12)}


def _touched(*a, **k):
    raise AssertionError("the library was touched")


def _untouchable(monkeypatch):
    from pyamg_amd import _lib
    monkeypatch.setattr(_lib, "lib", _touched)
    monkeypatch.setattr(_lib, "device_count", _touched)


@pytest.mark.parametrize("name", SYMMETRIC)
def test_host_route_equals_the_model_of_the_definition(name):
    g = mc.graphs()[name]
    agg, cpts = mc.model_mis_aggregation(g)
    for device in (False, None):
        AggOp, Cpts = mis_aggregation(mc.matrix(g), g["y"], device=device)
        assert sps.isspmatrix_csr(AggOp) and AggOp.dtype == np.int8 and Cpts.dtype == np.intc
        assert AggOp.shape == (g["n"], max(1, len(cpts))) and np.array_equal(Cpts, cpts)
        assert np.array_equal(mc.agg_of(AggOp), agg)
    # the same shapes and types as standard_aggregation's
    Std, StdCpts = standard_aggregation(mc.matrix(g))
    assert (type(Std), Std.dtype, StdCpts.dtype, Std.shape[0]) == (type(AggOp), AggOp.dtype, Cpts.dtype, AggOp.shape[0])
    assert (Std.shape[1] == 1 and Std.nnz == 0) == (len(cpts) == 0)


@pytest.mark.parametrize("name", SYMMETRIC)
def test_properties_of_the_aggregates(name):
    g = mc.graphs()[name]
    n, Ap, Aj = g["n"], g["Ap"], g["Aj"]
    AggOp, Cpts = mis_aggregation(mc.matrix(g), g["y"])
    agg = mc.agg_of(AggOp)
    x = np.zeros(n, dtype=bool)
    x[np.flatnonzero(mc.model_mis_k(g, 2)[0])] = True
    off_diagonal = np.array([np.any(Aj[Ap[i]:Ap[i + 1]] != i) for i in range(n)], dtype=bool)
    # Cpts is the ascending list of the members with an off-diagonal entry, one per aggregate, root a in aggregate a
    assert np.array_equal(Cpts, np.flatnonzero(x & off_diagonal))
    assert np.array_equal(agg[Cpts], np.arange(len(Cpts)))
    # every vertex with an off-diagonal entry is aggregated, the others have zero rows
    assert np.array_equal(agg != -1, off_diagonal)
    # every aggregate is connected through its root within two edges: a member is the root, next to it, or next to
    # a member that is next to it
    for a, root in enumerate(Cpts):
        ring1 = set(int(j) for j in Aj[Ap[root]:Ap[root + 1]] if agg[j] == a)
        for i in np.flatnonzero(agg == a):
            assert i == root or i in ring1 or ring1 & set(int(j) for j in Aj[Ap[i]:Ap[i + 1]]), (name, a, i)


def test_the_pattern_alone_is_read_and_the_weights_are_drawn_here():
    g = mc.graphs()["grid_17x19"]
    M = mc.matrix(g).astype(np.float64)
    M.data[:] = np.random.RandomState(1).randn(M.nnz)
    want = mis_aggregation(mc.matrix(g), g["y"])
    got = mis_aggregation(M, g["y"])
    assert np.array_equal(got[0].toarray(), want[0].toarray()) and np.array_equal(got[1], want[1])
    np.random.seed(5)
    drawn = mis_aggregation(M)
    follow = np.random.rand()
    np.random.seed(5)
    again = mis_aggregation(M, np.random.rand(g["n"]))
    assert np.array_equal(drawn[0].toarray(), again[0].toarray()) and follow == np.random.rand()


def test_refusals_come_before_any_library(monkeypatch):
    u = mc.graphs()["random_unsymmetric_400"]
    g = mc.graphs()["grid_17x19"]
    bad = g["y"].copy()
    bad[3] = np.nan
    want = mis_aggregation(mc.matrix(g), bad, device=False)
    _untouchable(monkeypatch)
    for device in (True, False, None):
        with pytest.raises(ValueError, match="symmetric"):
            mis_aggregation(mc.matrix(u), u["y"], device=device)
        with pytest.raises(ValueError):
            mis_aggregation(sps.csr_matrix((3, 4)), device=device)
        with pytest.raises(TypeError):
            mis_aggregation(mc.matrix(g).tocsc(), device=device)
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        mis_aggregation(mc.matrix(g), bad, device=True)
    # device=None: the host route; with MIS_DEVICE_AUTO and a GPU "present" a refusal is answered by the host route
    assert aggregation.MIS_DEVICE_AUTO is False
    monkeypatch.setattr(aggregation, "MIS_DEVICE_AUTO", True)
    monkeypatch.setattr(_host, "device_present", lambda: True)
    got = mis_aggregation(mc.matrix(g), bad)
    assert np.array_equal(got[0].toarray(), want[0].toarray()) and np.array_equal(got[1], want[1])
    with pytest.raises(AssertionError, match="the library was touched"):    # the route is live
        mis_aggregation(mc.matrix(g), g["y"])


@pytest.mark.parametrize("problem", list(PROBLEMS))
def test_smoothed_aggregation_solver_with_mis(problem):
    A = poisson(PROBLEMS[problem], format="csr")
    built = []
    for _ in range(2):
        np.random.seed(0)
        built.append(smoothed_aggregation_solver(A, aggregate="mis", max_coarse=20, keep=True))
    ml, again = built
    assert len(ml.levels) >= 2 and ml.levels[-1].A.shape[0] <= 20 and len(ml.levels) == len(again.levels)
    for a, b in zip(ml.levels, again.levels):
        for name in ("A", "P", "R"):
            if hasattr(a, name):
                Ma, Mb = getattr(a, name), getattr(b, name)
                assert np.array_equal(Ma.indptr, Mb.indptr) and np.array_equal(Ma.indices, Mb.indices) and np.array_equal(Ma.data, Mb.data)
    # every level's AggOp is mis_aggregation of its strength matrix under the level's draw: rand(n) at the aggregation
    # stage, after strength and before the spectral-radius estimate takes its own
    np.random.seed(0)
    for lvl in ml.levels[:-1]:
        n = lvl.A.shape[0]
        AggOp, _ = mis_aggregation(lvl.C, np.random.rand(n))
        assert AggOp.shape == lvl.AggOp.shape and (AggOp != lvl.AggOp).nnz == 0
        np.random.rand(n, 1)                # approximate_spectral_radius' start vector
    # the tuple form and the per-level list are the same descriptor
    np.random.seed(0)
    other = smoothed_aggregation_solver(A, aggregate=[("mis", {"device": False})], max_coarse=20)
    assert [l.A.shape for l in other.levels] == [l.A.shape for l in ml.levels]
    assert np.array_equal(other.levels[-1].A.data, ml.levels[-1].A.data)


@pytest.mark.parametrize("problem", list(PROBLEMS))
def test_rootnode_solver_with_mis_keeps_the_identity_at_the_roots(problem):
    A = poisson(PROBLEMS[problem], format="csr")
    np.random.seed(0)
    ml = rootnode_solver(A, aggregate="mis", max_coarse=20, keep=True)
    assert len(ml.levels) >= 2 and ml.levels[-1].A.shape[0] <= 20
    for lvl in ml.levels[:-1]:
        Cpts = np.asarray(lvl.Cpts)
        assert len(Cpts) == lvl.P.shape[1] and np.all(np.diff(Cpts) > 0)
        at_roots = sps.csr_matrix(lvl.P)[Cpts]
        assert (at_roots != sps.identity(len(Cpts), format="csr")).nnz == 0
        # the roots are the aggregation's: root a lies in aggregate a
        assert np.array_equal(mc.agg_of(lvl.AggOp)[Cpts], np.arange(len(Cpts)))


def test_other_aggregations_keep_their_refusals():
    A = poisson((10, 10), format="csr")
    for solver in (smoothed_aggregation_solver, rootnode_solver):
        for name in ("lloyd", "naive"):
            with pytest.raises(NotImplementedError, match="outside the restated setup"):
                solver(A, aggregate=name, max_coarse=5)
