"""The distance-k independent set on the host (csrc/setup_host.cpp: amgsetup_mis_k_parallel) against the reference's
integers (tests/golden/mis_k/cases.npz, written by tools/gen_golden_mis_k.py on the designed graphs of
tests/mis_cases.py): every comparison is exact integer equality."""
import numpy as np
import pytest

import mis_cases as mc
from pyamg_amd import _host, amg_core, graph
from pyamg_amd.graph import maximal_independent_set, maximal_independent_set_k

RUNS = mc.all_runs()
IDS = [mc.run_id(*r) for r in RUNS]


def _touched(*a, **k):
    raise AssertionError("the library was touched")


def _untouchable(monkeypatch):
    from pyamg_amd import _lib
    monkeypatch.setattr(_lib, "lib", _touched)
    monkeypatch.setattr(_lib, "device_count", _touched)


def test_the_fixture_holds_every_run_and_nothing_but_arrays():
    f = mc.fixture()
    assert list(f["names"]) == list(mc.graphs())
    assert [tuple(r) for r in f["runs"]] == [(list(mc.graphs()).index(n), k, m) for n, k, m in RUNS]
    assert all(v.dtype.kind in "ifU" for v in f.values())


@pytest.mark.parametrize("name,k,m", RUNS, ids=IDS)
def test_host_route_equals_the_reference(name, k, m):
    g = mc.graphs()[name]
    want = mc.reference_x(name, k, m)
    for device in (False, None):
        got = maximal_independent_set_k(mc.matrix(g), k, g["y"], m, device=device)
        assert got.dtype == np.intc and np.array_equal(got, want)


@pytest.mark.parametrize("name,k,m", RUNS, ids=IDS)
def test_flat_entry_equals_the_reference_in_place(name, k, m):
    g = mc.graphs()[name]
    x = np.full(g["n"], -7, dtype=np.intc)
    ret = amg_core.maximal_independent_set_k_parallel(g["n"], np.array(g["Ap"]), np.array(g["Aj"]), k, x, np.array(g["y"]), m)
    assert ret is None and np.array_equal(x, mc.reference_x(name, k, m))


@pytest.mark.parametrize("name,k,m", RUNS, ids=IDS)
def test_python_model_equals_the_reference(name, k, m):
    x, rounds = mc.model_mis_k(mc.graphs()[name], k, m)
    assert np.array_equal(x, mc.reference_x(name, k, m))
    assert m == -1 or rounds <= m


def test_round_counts_are_the_models():
    for name, k, m in RUNS:
        g = mc.graphs()[name]
        if g["n"] == 0:
            continue
        x = np.empty(g["n"], dtype=np.intc)
        assert graph.mis_k(g["n"], g["Ap"], g["Aj"], k, x, g["y"], m, device=False) == mc.model_mis_k(g, k, m)[1], (name, k, m)
    # the increasing path decides one vertex a round: the retire logic runs many times
    assert mc.model_mis_k(mc.graphs()["path_increasing"], 2)[1] == 67


@pytest.mark.parametrize("name", mc.symmetric_names())
@pytest.mark.parametrize("k", mc.KS)
def test_sets_are_independent_and_maximal_at_distance_k(name, k):
    # independently of the reference: no two members within k edges, every other vertex within k edges of a member
    g = mc.graphs()[name]
    x = maximal_independent_set_k(mc.matrix(g), k, g["y"])
    members = np.flatnonzero(x)
    assert np.all(mc.distances_from(g, members, k) <= k)
    for s in members:
        near = mc.distances_from(g, [s], k) <= k
        near[s] = False
        assert not np.any(x[near]), "members within %d edges of member %d" % (k, s)


def test_weights_are_drawn_where_the_reference_draws_them():
    g = mc.graphs()["grid_17x19"]
    np.random.seed(3)
    drawn = maximal_independent_set_k(mc.matrix(g), 2)
    follow = np.random.rand()
    np.random.seed(3)
    y = np.random.rand(g["n"])
    assert np.array_equal(drawn, maximal_independent_set_k(mc.matrix(g), 2, y)) and follow == np.random.rand()


def test_arguments():
    g = mc.graphs()["grid_17x19"]
    for k in (0, -1):
        with pytest.raises(ValueError):
            maximal_independent_set_k(mc.matrix(g), k, g["y"])
        with pytest.raises(ValueError):
            amg_core.maximal_independent_set_k_parallel(g["n"], np.array(g["Ap"]), np.array(g["Aj"]), k, np.zeros(g["n"], dtype=np.intc),
                                                        np.array(g["y"]), -1)
    with pytest.raises(ValueError):
        maximal_independent_set_k(mc.matrix(g), 2, g["y"][:-1])
    with pytest.raises(NotImplementedError):
        amg_core.maximal_independent_set_k_parallel(g["n"], g["Ap"].astype(np.int64), np.array(g["Aj"]), 2, np.zeros(g["n"], dtype=np.intc),
                                                    np.array(g["y"]), -1)
    assert "maximal_independent_set_k_parallel" in amg_core.__all__
    # max_iters == 0 runs no round
    assert not maximal_independent_set_k(mc.matrix(g), 2, g["y"], 0).any()
    # weights on which the reference's loop does not end: vertex 2 never beats its retired neighbour's -1
    with pytest.raises(ValueError, match="does not end"):
        maximal_independent_set_k(mc.matrix(mc._path(3, [9.0, 0.0, -5.0])), 1, [9.0, 0.0, -5.0])


def test_no_vertices_touches_neither_library(monkeypatch):
    _untouchable(monkeypatch)
    monkeypatch.setattr(graph, "_host", _touched)
    for device in (True, False, None):
        out = maximal_independent_set_k(mc.matrix(mc.graphs()["empty"]), 2, device=device)
        assert out.dtype == np.intc and out.shape == (0,)


def test_device_true_refuses_weights_that_are_not_finite_before_the_library(monkeypatch):
    _untouchable(monkeypatch)
    g = mc.graphs()["grid_17x19"]
    for bad in (np.nan, np.inf, -np.inf):
        y = g["y"].copy()
        y[5] = bad
        with pytest.raises(NotImplementedError, match="outside the restated setup"):
            maximal_independent_set_k(mc.matrix(g), 2, y, device=True)


def test_device_none_is_the_host_route_and_a_refusal_falls_back(monkeypatch):
    g = mc.graphs()["grid_17x19"]
    y = g["y"].copy()
    y[5] = np.inf
    want = maximal_independent_set_k(mc.matrix(g), 2, y, device=False)
    _untouchable(monkeypatch)
    assert graph.MIS_K_DEVICE_AUTO is False
    assert np.array_equal(maximal_independent_set_k(mc.matrix(g), 2, y), want)
    monkeypatch.setattr(graph, "MIS_K_DEVICE_AUTO", True)
    monkeypatch.setattr(_host, "device_present", lambda: True)
    assert np.array_equal(maximal_independent_set_k(mc.matrix(g), 2, y), want)
    with pytest.raises(AssertionError, match="the library was touched"):    # the route is live: finite weights go on
        maximal_independent_set_k(mc.matrix(g), 2, g["y"])


def test_the_old_name_still_refuses_distance_k():
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        maximal_independent_set(mc.matrix(mc.graphs()["grid_17x19"]), k=2)
