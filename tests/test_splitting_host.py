"""The parallel C/F splittings on the host route: the restatements of csrc/setup_host.cpp against every native call
recorded from the reference (tests/golden/splitting/), against sequential Python models on random graphs, and the
public functions of pyamg_amd.graph and pyamg_amd.classical against the recorded results.  No GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sps

import golden_io
import oracle_lib
import splitting_io as sio
import pyamg_amd
from pyamg_amd import _host, classical, graph
from pyamg_amd.classical import CLJP, CLJPc, MIS, PMIS, PMISc, preprocess, ruge_stuben_solver
from pyamg_amd.graph import maximal_independent_set, vertex_coloring
from test_setup_golden import same


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _w(a):
    return np.array(a, copy=True)


def replay(entry, args):
    """one recorded native call on the host restatement -> (outputs, return value)"""
    L = graph._host()
    a = {k: (_w(v) if v.ndim else v.item()) for k, v in args.items()}
    if entry == "maximal_independent_set_parallel":
        ret = L.amgsetup_mis_parallel(a["num_rows"], _ip(a["Ap"]), _ip(a["Aj"]), a["active"], a["C"], a["F"], _ip(a["x"]),
                                      _dp(a["y"]), a["max_iters"])
        return {"x": a["x"]}, ret
    if entry == "maximal_independent_set_serial":
        ret = L.amgsetup_mis_serial(a["num_rows"], _ip(a["Ap"]), _ip(a["Aj"]), a["active"], a["C"], a["F"], _ip(a["x"]))
        return {"x": a["x"]}, ret
    n = a["num_rows"] if "num_rows" in a else a["n"]
    x = np.full(n, -77, dtype=np.intc)
    if entry == "vertex_coloring_mis":
        return {"x": x}, L.amgsetup_vertex_coloring_mis(n, _ip(a["Ap"]), _ip(a["Aj"]), _ip(x))
    if entry == "vertex_coloring_jones_plassmann":
        ret = L.amgsetup_vertex_coloring_jones_plassmann(n, _ip(a["Ap"]), _ip(a["Aj"]), _ip(x), _dp(a["z"]))
        return {"x": x, "z": a["z"]}, ret
    if entry == "vertex_coloring_LDF":
        return {"x": x}, L.amgsetup_vertex_coloring_LDF(n, _ip(a["Ap"]), _ip(a["Aj"]), _ip(x), _dp(a["y"]))
    assert entry == "cljp_naive_splitting"
    L.amgsetup_cljp_naive_splitting(n, _ip(a["Sp"]), _ip(a["Sj"]), _ip(a["Tp"]), _ip(a["Tj"]), _ip(x), a["colorflag"])
    return {"splitting": x}, -1


@pytest.mark.parametrize("name", sio.PROBLEMS)
def test_host_restatements_reproduce_every_recorded_native_call(name):
    p = sio.problem(name)
    seen = set()
    for tag in p["tags"]:
        for entry, args, outs, ret in p["calls"][tag]:
            got, got_ret = replay(entry, args)
            for k, v in outs.items():
                assert got[k].dtype == v.dtype and np.array_equal(got[k], v), (tag, entry, k)
            assert got_ret == ret, (tag, entry, got_ret, ret)
            seen.add(entry)
    assert seen == set(sio.ARGS)


@pytest.mark.parametrize("name", sio.PROBLEMS)
def test_fixture_exercises_the_tie_rule(name):
    ties = 0
    for tag, args, x_out, ret in sio.mis_calls(name):
        n, Ap, Aj, y = int(args["num_rows"]), args["Ap"], args["Aj"], args["y"]
        rows = np.repeat(np.arange(n), np.diff(Ap))
        ties += int(np.count_nonzero((rows != Aj) & (y[rows] == y[Aj])))
    assert ties > 0


RUNS = {"PMIS": lambda S, G, **kw: PMIS(S, **kw),
        "PMISc_JP": lambda S, G, **kw: PMISc(S, method="JP", **kw),
        "PMISc_MIS": lambda S, G, **kw: PMISc(S, method="MIS", **kw),
        "PMISc_LDF": lambda S, G, **kw: PMISc(S, method="LDF", **kw),
        "CLJP": lambda S, G, **kw: CLJP(S, **kw),
        "CLJPc": lambda S, G, **kw: CLJPc(S, **kw),
        "MIS_ones": lambda S, G, **kw: MIS(G, np.ones((G.shape[0], 1)).ravel(), **kw),
        "color_MIS": lambda S, G, **kw: vertex_coloring(G, "MIS", **kw),
        "color_JP": lambda S, G, **kw: vertex_coloring(G, "JP", **kw),
        "color_LDF": lambda S, G, **kw: vertex_coloring(G, "LDF", **kw),
        "mis_serial": lambda S, G, **kw: maximal_independent_set(G, "serial", **kw),
        "mis_parallel": lambda S, G, **kw: maximal_independent_set(G, "parallel", **kw)}


@pytest.mark.parametrize("name", sio.PROBLEMS)
def test_seeded_public_functions_equal_the_fixtures(name):
    p = sio.problem(name)
    assert set(p["tags"]) == set(RUNS)
    for tag in p["tags"]:
        S, G = p["S"].copy(), p["G"].copy()
        np.random.seed(0)
        got = RUNS[tag](S, G)
        assert got.dtype == np.intc and np.array_equal(got, p[tag]), tag
        assert (abs(S - p["S"])).nnz == 0                                   # arguments are left alone
        if tag.startswith("color"):
            sio.assert_proper_coloring(p["G"], got)
        elif tag in ("PMIS", "PMISc_JP", "PMISc_MIS", "PMISc_LDF", "MIS_ones", "mis_serial", "mis_parallel"):
            sio.assert_independent_and_maximal(p["G"], got)
        else:
            assert set(np.unique(got)) <= {0, 1}


@pytest.mark.parametrize("name", sio.PROBLEMS)
def test_recorded_luby_sets_are_the_greedy_sets_by_priority(name):
    # the argument of DESIGN.md for the device route, checked on the reference's own results
    for tag, args, x_out, ret in sio.mis_calls(name):
        if int(args["max_iters"]) != -1 or not np.all(args["x"] == -1):
            continue
        want = sio.model_greedy_mis(int(args["num_rows"]), args["Ap"], args["Aj"], args["y"])
        assert np.array_equal(x_out, want), tag


def test_luby_restatement_equals_the_model_on_random_graphs():
    rng = np.random.RandomState(20)
    L = graph._host()
    for case in range(50):
        n = int(rng.randint(5, 121))
        G = sio.random_graph(rng, n, symmetric=True, diagonal=case % 5 == 0)
        y = sio.random_weights(rng, n, integer=case % 2 == 0)
        x0 = np.full(n, -1, dtype=np.intc)
        if case % 3 == 0:                                   # partly decided on entry, as the colourings call it
            x0[rng.rand(n) < 0.2] = 7
        for max_iters in (1, 2, -1):
            xm, xh = x0.copy(), x0.copy()
            Nm = sio.model_mis_parallel(n, G.indptr, G.indices, -1, 3, -2, xm, y, max_iters)
            Nh = L.amgsetup_mis_parallel(n, _ip(G.indptr), _ip(G.indices), -1, 3, -2, _ip(xh), _dp(y), max_iters)
            assert np.array_equal(xm, xh) and Nm == Nh, (case, max_iters)
        if case % 3 != 0:
            want = sio.model_greedy_mis(n, G.indptr, G.indices, y)
            assert np.array_equal(np.where(xh == 3, 1, 0), want), case
            # the serial greedy set is the same set for the priorities -i
            xs = x0.copy()
            L.amgsetup_mis_serial(n, _ip(G.indptr), _ip(G.indices), -1, 3, -2, _ip(xs))
            assert np.array_equal(np.where(xs == 3, 1, 0), sio.model_greedy_mis(n, G.indptr, G.indices, -np.arange(n, dtype=float))), case


def test_cljp_restatement_equals_the_model_on_random_graphs():
    rng = np.random.RandomState(21)
    L = graph._host()
    for case in range(50):
        n = int(rng.randint(5, 121))
        S = sio.random_graph(rng, n, symmetric=case % 2 == 0, diagonal=case % 5 == 0)
        T = sps.csr_matrix(S.T)
        T.sort_indices()
        Tp, Tj = T.indptr.astype(np.intc), T.indices.astype(np.intc)
        base = sio.random_weights(rng, n, integer=case % 4 < 2)
        if case % 4 < 2:
            base = base / 4.0                               # tied fractions below 1, as colour weights are
        w0 = sio.model_cljp_start_weights(n, S.indptr, S.indices, base)
        wm, wh = w0.copy(), w0.copy()
        want = sio.model_cljp_select(n, S.indptr, S.indices, Tp, Tj, wm)
        got = np.empty(n, dtype=np.intc)
        L.amgsetup_cljp_select(n, _ip(S.indptr), _ip(S.indices), _ip(Tp), _ip(Tj), _dp(wh), _ip(got))
        assert np.array_equal(got, want), case
        assert set(np.unique(got)) <= {0, 1}


def test_cljp_start_weights_are_glibc_rand_plus_in_degree():
    p = sio.problem("unsym_400")
    S = classical.remove_diagonal(p["S"])
    n = S.shape[0]
    Sp, Sj = S.indptr.astype(np.intc), S.indices.astype(np.intc)
    got = np.empty(n)
    graph._host().amgsetup_cljp_weights(n, _ip(Sp), _ip(Sj), 0, _dp(got))
    want = sio.model_cljp_start_weights(n, Sp, Sj, sio.glibc_weights(n))
    assert np.array_equal(got, want)
    T = sps.csr_matrix(S.T)
    T.sort_indices()
    split = sio.model_cljp_select(n, Sp, Sj, T.indptr.astype(np.intc), T.indices.astype(np.intc), want)
    assert np.array_equal(split, p["CLJP"])
    # a vertex nobody depends on starts below 1 and still ends as C: it is only decided by being selected
    lonely = np.flatnonzero(np.bincount(Sj, minlength=n) == 0)
    assert len(lonely) >= 4 and np.all(p["CLJP"][lonely] == 1)


@pytest.mark.parametrize("hier", sorted(sio.HIERARCHIES))
def test_hierarchy_reproduces_the_reference(hier):
    g = sio.load_hier(hier)
    A = sio.poisson2d(40, 40)
    same(A, g["levels"][0]["A"], 0.0)
    np.random.seed(0)
    ml = ruge_stuben_solver(A, CF=sio.HIERARCHIES[hier], max_coarse=20)
    assert [l.A.shape[0] for l in ml.levels] == [L["A"].shape[0] for L in g["levels"]]
    for lvl, G in zip(ml.levels, g["levels"]):
        same(lvl.A, G["A"], 1e-13)
        if "P" in G:
            same(lvl.P, G["P"], 1e-13)
            same(lvl.R, G["R"], 1e-13)
    # the solve on the levels built here, by the sequential oracle (no GPU)
    levels = []
    for lvl, G in zip(ml.levels, g["levels"]):
        L = {"A": lvl.A}
        if "P" in G:
            L.update(P=lvl.P, R=lvl.R, pre=G["pre"], post=G["post"])
        levels.append(L)
    pinv = np.ascontiguousarray(scipy.linalg.pinv(ml.levels[-1].A.toarray()))
    x, res = oracle_lib.Hierarchy(levels, pinv).solve(g["b"], tol=g["meta"]["tol"], maxiter=g["meta"]["maxiter"])
    golden_io.assert_history(res, g["residuals"], g["levels"][0]["A"], g["x"], g["b"])


def _untouchable(monkeypatch):
    from pyamg_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(_lib, "device_count", touched)


def test_distance_k_sets_are_refused():
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        maximal_independent_set(sio.problem("poisson_17x23")["G"], k=2)


def test_device_true_refusals_come_before_the_library_is_touched(monkeypatch):
    _untouchable(monkeypatch)
    p, u = sio.problem("poisson_17x23"), sio.problem("unsym_400")
    w = np.ones(p["n"])
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        MIS(p["G"], w, maxiter=1, device=True)
    Gu = sps.csr_matrix(classical.remove_diagonal(u["S"]))
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        MIS(Gu, np.ones(u["n"]), device=True)
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        maximal_independent_set(Gu, "serial", device=True)
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        maximal_independent_set(Gu, "parallel", device=True)
    for method in ("JP", "LDF"):
        with pytest.raises(NotImplementedError, match="outside the restated setup"):
            vertex_coloring(p["G"], method, device=True)


def test_device_none_is_the_host_route(monkeypatch):
    _untouchable(monkeypatch)
    assert classical.DEVICE_AUTO is False and graph.DEVICE_AUTO is False
    p = sio.problem("poisson_17x23")
    for tag in ("PMIS", "CLJP", "color_MIS", "mis_serial"):
        np.random.seed(0)
        assert np.array_equal(RUNS[tag](p["S"], p["G"], device=None), p[tag])
        np.random.seed(0)
        assert np.array_equal(RUNS[tag](p["S"], p["G"], device=False), p[tag])


def test_device_none_falls_back_when_the_device_entry_refuses(monkeypatch):
    # DEVICE_AUTO set and a GPU "present": what the device route refuses is answered by the host route, never raised.
    # Every refusal here comes from the checks made before the library is reached, so it stays untouched.
    u = sio.problem("unsym_400")
    Gu = sps.csr_matrix(classical.remove_diagonal(u["S"]))
    y = np.random.RandomState(1).rand(u["n"])
    want_limit = MIS(u["G"], y, maxiter=1, device=False)
    want_unsym = MIS(Gu, y, device=False)
    want_serial = maximal_independent_set(Gu, "serial", device=False)
    want_color = vertex_coloring(Gu, "MIS", device=False)
    _untouchable(monkeypatch)
    monkeypatch.setattr(graph, "DEVICE_AUTO", True)
    monkeypatch.setattr(classical, "DEVICE_AUTO", True)
    monkeypatch.setattr(_host, "device_present", lambda: True)
    assert -1 in want_limit and np.array_equal(MIS(u["G"], y, maxiter=1), want_limit)
    assert np.array_equal(MIS(Gu, y), want_unsym)
    assert np.array_equal(maximal_independent_set(Gu, "serial"), want_serial)
    assert np.array_equal(vertex_coloring(Gu, "MIS"), want_color)
    np.random.seed(0)
    assert np.array_equal(vertex_coloring(u["G"], "JP"), u["color_JP"])
    with pytest.raises(AssertionError, match="the library was touched"):    # the route is live: a symmetric graph goes on
        MIS(u["G"], y)


def test_statements_and_error_types_of_the_reference():
    p = sio.problem("poisson_17x23")
    for fn in (PMIS, PMISc, CLJP, CLJPc, preprocess):
        with pytest.raises(TypeError):
            fn(p["S"].tocsc())
    with pytest.raises(TypeError):
        MIS(p["G"].tocsc(), np.ones(p["n"]))
    with pytest.raises(ValueError):
        preprocess(sps.csr_matrix(np.ones((3, 4))))
    with pytest.raises(ValueError):
        MIS(p["G"], np.ones(p["n"]), maxiter=-1)
    with pytest.raises(ValueError):
        maximal_independent_set(p["G"], "bogus")
    with pytest.raises(ValueError):
        vertex_coloring(p["G"], "bogus")
    with pytest.raises(ValueError):
        graph.asgraph(np.ones((3, 4)))
    assert np.all(MIS(p["G"], np.ones(p["n"]), maxiter=0) == -1)
    np.random.seed(0)
    weights, G, S, T = preprocess(classical.remove_diagonal(p["S"]))
    np.random.seed(0)
    assert np.array_equal(weights, np.bincount(S.indices, minlength=p["n"]) + np.random.rand(p["n"]))
    assert (abs(G - p["G"])).nnz == 0 and (abs(T - S.T)).nnz == 0 and np.all(S.data == 1)


def test_other_splittings_are_still_refused():
    A = sio.poisson2d(12, 12)
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        ruge_stuben_solver(A, CF="bogus", max_coarse=10)
    ml = ruge_stuben_solver(A, CF=("CLJP", {"device": False}), max_coarse=10)
    assert len(ml.levels) > 1


def test_exports_and_signatures():
    from pyamg_amd import _lib, amg_core
    for name in ("PMIS", "PMISc", "CLJP", "CLJPc", "MIS", "preprocess", "RS", "ruge_stuben_solver"):
        assert name in classical.__all__ and callable(getattr(classical, name))
    assert graph.__all__ == ["asgraph", "maximal_independent_set", "vertex_coloring"]
    assert pyamg_amd.graph is graph and "graph" in pyamg_amd.__all__
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(PMIS) == ["S", "device"] and sig(PMISc) == ["S", "method", "device"]
    assert sig(CLJP) == ["S", "color", "device"] and sig(CLJPc) == ["S", "device"]
    assert sig(MIS) == ["G", "weights", "maxiter", "device"] and sig(preprocess) == ["S", "coloring_method"]
    assert sig(maximal_independent_set) == ["G", "algo", "k", "device"]
    assert inspect.signature(PMISc).parameters["method"].default == "JP"
    assert sig(amg_core.maximal_independent_set_parallel) == ["num_rows", "Ap", "Aj", "active", "C", "F", "x", "y", "max_iters"]
    assert sig(amg_core.cljp_naive_splitting) == ["n", "Sp", "Sj", "Tp", "Tj", "splitting", "colorflag"]
    for name in ("maximal_independent_set_parallel", "cljp_naive_splitting"):
        assert name in amg_core.__all__ and name not in _lib.FLAT_TABLE


def test_amg_core_entries_check_their_arguments_before_the_library(monkeypatch):
    from pyamg_amd import amg_core
    _untouchable(monkeypatch)
    G = sio.problem("poisson_17x23")["G"]
    n = G.shape[0]
    Ap, Aj = G.indptr.astype(np.intc), G.indices.astype(np.intc)
    x, y = np.full(n, -1, dtype=np.intc), np.ones(n)
    with pytest.raises(NotImplementedError):
        amg_core.maximal_independent_set_parallel(n, Ap, Aj, -1, 1, 0, x, y, 1)
    with pytest.raises(NotImplementedError):
        amg_core.maximal_independent_set_parallel(n, Ap.astype(np.int64), Aj, -1, 1, 0, x, y, -1)
    with pytest.raises(NotImplementedError):
        amg_core.maximal_independent_set_parallel(n, Ap, Aj, -1, 1, 0, x, y.astype(np.float32), -1)
    with pytest.raises(TypeError):
        amg_core.maximal_independent_set_parallel(n, Ap, Aj, -1, 1, 0, np.full(2 * n, -1, dtype=np.intc)[::2], y, -1)
    with pytest.raises(NotImplementedError):
        amg_core.cljp_naive_splitting(n, Ap, Aj, Ap, Aj, np.empty(n, dtype=np.int64), 0)
    with pytest.raises(TypeError):
        amg_core.cljp_naive_splitting(n, Ap, Aj, Ap, Aj, np.empty(2 * n, dtype=np.intc)[::2], 0)
