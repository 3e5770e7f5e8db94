"""The distance-k independent set and the MIS(2) aggregation on the device (csrc/misagg.hip: amg_mis_k_device,
amg_mis_aggregation_device): the set against the reference's integers (tests/golden/mis_k/cases.npz), the aggregation
and the solvers built on it against the host route, which tests/test_mis_k_host.py and
tests/test_mis_aggregation_host.py pin.  Every comparison is exact equality.

The device route gives every vertex one lane whatever its row length (there is no long-row form and so no threshold):
the 700-entry row of star_700 runs in the same kernels as everything else."""
import ctypes as C

import numpy as np
import pytest

import mis_cases as mc
import prolong_cases as pc
from pyamg_amd import _host, _lib, aggregation, graph, smoothed_aggregation_solver
from pyamg_amd.aggregation import mis_aggregation, symmetric_strength_of_connection
from pyamg_amd.gallery import poisson
from pyamg_amd.graph import maximal_independent_set_k

pytestmark = pytest.mark.gpu


def same_matrix(a, b):
    return a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) \
        and np.array_equal(a.data, b.data)


@pytest.mark.parametrize("name", list(mc.graphs()))
def test_device_set_equals_the_reference(name):
    g = mc.graphs()[name]
    for k, m in mc.runs(name):
        want = mc.reference_x(name, k, m)
        assert np.array_equal(maximal_independent_set_k(mc.matrix(g), k, g["y"], m, device=True), want), (k, m)
        if g["n"] == 0:
            continue
        xd, xh = np.full(g["n"], -7, dtype=np.intc), np.full(g["n"], -7, dtype=np.intc)
        times = []
        rounds_d = graph.mis_k(g["n"], g["Ap"], g["Aj"], k, xd, g["y"], m, device=True, times=times)
        rounds_h = graph.mis_k(g["n"], g["Ap"], g["Aj"], k, xh, g["y"], m, device=False)
        assert np.array_equal(xd, want) and np.array_equal(xh, want)
        assert rounds_d == rounds_h and (m == -1 or rounds_d <= m), (k, m, rounds_d, rounds_h)
        assert len(times) == 3 and min(times) >= 0.0


def _both_routes(Cm, y):
    rounds, times = [], []
    dev = mis_aggregation(Cm, y, device=True, times=times, rounds=rounds)
    host = mis_aggregation(Cm, y, device=False, rounds=rounds)
    assert dev[0].dtype == np.int8 and dev[1].dtype == np.intc
    assert same_matrix(dev[0], host[0]) and np.array_equal(dev[1], host[1])
    assert rounds[0] == rounds[1] and (len(times) == 3 or Cm.shape[0] == 0)
    return dev


@pytest.mark.parametrize("name", mc.symmetric_names())
def test_device_aggregation_equals_the_host_route_on_the_designed_graphs(name):
    g = mc.graphs()[name]
    AggOp, Cpts = _both_routes(mc.matrix(g), g["y"])
    agg, cpts = mc.model_mis_aggregation(g)
    assert np.array_equal(Cpts, cpts) and np.array_equal(mc.agg_of(AggOp), agg)


@pytest.mark.parametrize("grid", [(30, 30), (12, 12, 12)], ids=["poisson_30x30", "poisson_12x12x12"])
def test_device_aggregation_equals_the_host_route_on_strength_patterns(grid):
    Cm = symmetric_strength_of_connection(poisson(grid, format="csr"))
    n = Cm.shape[0]
    for y in (np.random.RandomState(0).rand(n), np.random.RandomState(1).randint(0, 4, n) / 4.0):
        AggOp, Cpts = _both_routes(Cm, y)
        assert AggOp.nnz == n and 0 < len(Cpts) < n / 4


@pytest.mark.parametrize("name", pc.degenerate_graph_names())
def test_device_aggregation_equals_the_host_route_on_degenerate_sizes(name):
    Cm, y = pc.degenerate_graphs()[name]
    live, rounds = _lib.live_buffers(), []
    dev = mis_aggregation(Cm.copy(), y.copy(), device=True, rounds=rounds)
    host = mis_aggregation(Cm.copy(), y.copy(), device=False, rounds=rounds)
    assert pc.same_matrix(dev[0], host[0]) and dev[1].dtype == host[1].dtype and np.array_equal(dev[1], host[1])
    assert dev[0].shape == (Cm.shape[0], 1) and dev[0].nnz == 0 and len(dev[1]) == 0     # no vertex has a neighbour: no root
    assert rounds[0] == rounds[1] and _lib.live_buffers() == live


@pytest.mark.parametrize("grid", [(40, 40), (12, 12, 12)], ids=["poisson_40x40", "poisson_12x12x12"])
def test_solver_levels_are_the_same_bits_by_both_routes_and_solve(grid):
    A = poisson(grid, format="csr")
    b = np.random.RandomState(7).rand(A.shape[0])
    built = {}
    for device in (True, False):
        np.random.seed(0)
        built[device] = smoothed_aggregation_solver(A, aggregate=("mis", {"device": device}), max_coarse=20)
    dev, host = built[True], built[False]
    assert len(dev.levels) == len(host.levels) >= 2
    for ld, lh in zip(dev.levels, host.levels):
        for name in ("A", "P", "R"):
            assert hasattr(ld, name) == hasattr(lh, name)
            if hasattr(ld, name):
                assert same_matrix(getattr(ld, name), getattr(lh, name)), name
    for ml in (dev, host):
        res = []
        ml.solve(b, tol=1e-8, residuals=res)            # from zero, the default maxiter=100
        print("%s aggregate='mis': levels %r, %d cycles" % (grid, [l.A.shape[0] for l in ml.levels], len(res) - 1))
        # the cap only keeps a diverging hierarchy from passing; the counts are in the README table, not asserted
        assert len(res) - 1 <= 100 and res[-1] <= 1e-8 * res[0]


def test_no_vertices_launches_nothing(monkeypatch):
    L = _lib.lib()
    live = _lib.live_buffers()
    rounds, n_agg = C.c_int(-1), C.c_int(-1)
    ms = (C.c_double * 3)(-1.0, -1.0, -1.0)
    _lib.check(L.amg_mis_k_device(0, None, None, 2, None, -1, None, C.byref(rounds), ms))
    assert rounds.value == 0 and list(ms) == [0.0, 0.0, 0.0]
    _lib.check(L.amg_mis_aggregation_device(0, None, None, None, None, None, C.byref(n_agg), C.byref(rounds), ms))
    assert n_agg.value == 0 and rounds.value == 0 and _lib.live_buffers() == live

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    empty = mc.matrix(mc.graphs()["empty"])
    assert maximal_independent_set_k(empty, 2, device=True).shape == (0,)
    AggOp, Cpts = mis_aggregation(empty, device=True)
    assert AggOp.shape == (0, 1) and len(Cpts) == 0


def test_bad_arguments_are_refused_before_any_launch():
    g = mc.graphs()["grid_17x19"]
    x = np.zeros(g["n"], dtype=np.intc)
    L = _lib.lib()
    Aj = np.array(g["Aj"])
    Aj[5] = g["n"]
    for k, cols in ((0, g["Aj"]), (2, Aj)):
        assert L.amg_mis_k_device(g["n"], g["Ap"].ctypes.data, cols.ctypes.data, k, g["y"].ctypes.data, -1, x.ctypes.data, None,
                                  None) == _lib.AMG_EINVAL


def test_a_device_refusal_under_none_falls_back_to_the_host_result(monkeypatch):
    g = mc.graphs()["random_symmetric_1000"]
    y = g["y"].copy()
    y[11] = np.inf
    want_set = maximal_independent_set_k(mc.matrix(g), 2, y, device=False)
    want_agg = mis_aggregation(mc.matrix(g), y, device=False)
    monkeypatch.setattr(graph, "MIS_K_DEVICE_AUTO", True)
    monkeypatch.setattr(aggregation, "MIS_DEVICE_AUTO", True)
    assert _host.device_present()
    assert np.array_equal(maximal_independent_set_k(mc.matrix(g), 2, y), want_set)
    got = mis_aggregation(mc.matrix(g), y)
    assert same_matrix(got[0], want_agg[0]) and np.array_equal(got[1], want_agg[1])
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        mis_aggregation(mc.matrix(g), y, device=True)
    # with finite weights None now takes the device route: its times arrive
    times = []
    mis_aggregation(mc.matrix(g), g["y"], times=times)
    assert len(times) == 3
