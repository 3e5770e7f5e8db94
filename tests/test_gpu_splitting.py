"""The parallel C/F splittings on the device (csrc/split.hip: amg_mis_device, amg_cljp_device) against the host route:
every comparison is exact integer equality.  The host route itself is pinned to the reference by
tests/test_splitting_host.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import golden_io
import splitting_io as sio
from pyamg_amd import amg_core, classical, graph
from pyamg_amd.classical import CLJP, CLJPc, MIS, PMIS, PMISc, classical_strength_of_connection, ruge_stuben_solver
from pyamg_amd.graph import maximal_independent_set, vertex_coloring

pytestmark = pytest.mark.gpu


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def csr32(M):
    M = sps.csr_matrix(M)
    M.sort_indices()
    return M, M.indptr.astype(np.intc), M.indices.astype(np.intc)


def luby_both(G, y, x0=None, active=-1, Cv=1, Fv=0):
    """Luby's set on the symmetric graph G by both routes -> (x, vertices that joined, device rounds)"""
    G, Ap, Aj = csr32(G)
    n = G.shape[0]
    y = np.ascontiguousarray(y, dtype=np.float64)
    xh = np.full(n, active, dtype=np.intc) if x0 is None else np.array(x0, dtype=np.intc)
    xd = xh.copy()
    Nh = graph._host().amgsetup_mis_parallel(n, _ip(Ap), _ip(Aj), active, Cv, Fv, _ip(xh), _dp(y), -1)
    Nd, rounds = graph._luby_device(n, Ap, Aj, active, Cv, Fv, xd, y)
    assert np.array_equal(xd, xh), "device and host sets differ at %r" % (np.flatnonzero(xd != xh)[:8],)
    assert Nd == Nh
    return xd, Nd, rounds


def cljp_both(S, weight0):
    """the CLJP selection loop on start weights by both routes -> (splitting, device passes)"""
    S, Sp, Sj = csr32(S)
    T, Tp, Tj = csr32(S.T)
    n = S.shape[0]
    wh = np.array(weight0, dtype=np.float64)
    wd = wh.copy()
    host, dev = np.full(n, -9, dtype=np.intc), np.full(n, -9, dtype=np.intc)
    graph._host().amgsetup_cljp_select(n, _ip(Sp), _ip(Sj), _ip(Tp), _ip(Tj), _dp(wh), _ip(host))
    passes = classical.cljp_device(n, Sp, Sj, Tp, Tj, wd, dev)
    assert np.array_equal(dev, host), "device and host splittings differ at %r" % (np.flatnonzero(dev != host)[:8],)
    assert set(np.unique(dev)) <= {0, 1}
    return dev, passes


def start_weights(S, base):
    """base + in-degree (diagonal skipped), by repeated +1 as the reference adds them"""
    S, Sp, Sj = csr32(S)
    return sio.model_cljp_start_weights(S.shape[0], Sp, Sj, base) if S.shape[0] < 2000 else \
        np.asarray(base, dtype=np.float64) + np.bincount(Sj[np.repeat(np.arange(S.shape[0]), np.diff(Sp)) != Sj], minlength=S.shape[0])


def planted_graph(rng, n=900):
    """a sparse random unsymmetric S with tied start weights and, planted on vertices 0-23: two C candidates 0 and 1
    that depend on each other and carry equal weights, and an edge 2 -> 3 whose ends both depend on 0 and on 1"""
    M = sps.random(n, n, density=0.008, random_state=rng, format="lil")
    M[:24, :] = 0
    M[:, :24] = 0
    M[0, 1] = M[1, 0] = 1
    for c in (0, 1):
        M[2, c] = M[3, c] = 1
        for leaf in range(4 + 10 * c, 14 + 10 * c):
            M[leaf, c] = 1
    M[2, 3] = 1
    M.setdiag(0)
    S = sps.csr_matrix(M)
    S.eliminate_zeros()
    base = rng.randint(0, 2, n) / 2.0
    base[:24] = 0.5
    return S, base


def cljp_cases(S, w0, split):
    """what the first pass of the selection loop meets on (S, w0): adjacent vertices selected together, vertices nobody
    depends on, an edge that two new C points reach in P6"""
    S, Sp, Sj = csr32(S)
    n = S.shape[0]
    pattern = sps.csr_matrix((np.ones(len(Sj)), Sj, Sp), shape=(n, n))
    either = sps.csr_matrix(pattern + pattern.T)
    rows = np.repeat(np.arange(n), np.diff(either.indptr))
    beaten = np.zeros(n, dtype=bool)
    beaten[rows[w0[either.indices] > w0[rows]]] = True
    first = np.flatnonzero(~beaten)
    shared = (pattern[:, first] * pattern[:, first].T).multiply(pattern)         # per edge (j, k): the c's in both rows
    return {"the first pass's set becomes C": bool(np.all(split[first] == 1)),
            "adjacent vertices selected together": pattern[first][:, first].nnz > 0,
            "vertices nobody depends on": bool(np.any(np.bincount(Sj, minlength=n) == 0)),
            "an edge two new C points reach": shared.nnz > 0 and shared.data.max() >= 2}


def grid_graph(nx, ny):
    A = sio.poisson2d(nx, ny)
    return classical.remove_diagonal(A)


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name", sio.PROBLEMS)
def test_recorded_mis_calls_on_the_device(name):
    ran = 0
    for tag, args, x_out, ret in sio.mis_calls(name):
        if int(args["max_iters"]) != -1:
            continue
        n = int(args["num_rows"])
        x = np.array(args["x"], dtype=np.intc)
        N, rounds = graph._luby_device(n, np.array(args["Ap"]), np.array(args["Aj"]), int(args["active"]), int(args["C"]),
                                       int(args["F"]), x, np.array(args["y"]))
        assert np.array_equal(x, x_out), tag
        assert N == ret and rounds >= 1
        ran += 1
    assert ran >= 5


@pytest.mark.parametrize("name", sio.PROBLEMS)
def test_four_splittings_on_the_device_equal_the_fixtures(name):
    p = sio.problem(name)
    runs = {"PMIS": lambda: PMIS(p["S"], device=True), "PMISc_JP": lambda: PMISc(p["S"], device=True),
            "PMISc_MIS": lambda: PMISc(p["S"], method="MIS", device=True),
            "PMISc_LDF": lambda: PMISc(p["S"], method="LDF", device=True),
            "CLJP": lambda: CLJP(p["S"], device=True), "CLJPc": lambda: CLJPc(p["S"], device=True),
            "MIS_ones": lambda: MIS(p["G"], np.ones(p["n"]), device=True),
            "mis_serial": lambda: maximal_independent_set(p["G"], "serial", device=True),
            "mis_parallel": lambda: maximal_independent_set(p["G"], "parallel", device=True),
            "color_MIS": lambda: vertex_coloring(p["G"], "MIS", device=True)}
    for tag, fn in runs.items():
        np.random.seed(0)
        got = fn()
        assert got.dtype == np.intc and np.array_equal(got, p[tag]), tag


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n", [0, 1, 65, 255, 256, 257, 513])
def test_block_edges_for_both_entries(n):
    rng = np.random.RandomState(n)
    G = sio.random_graph(rng, n, symmetric=True) if n > 1 else sps.csr_matrix((n, n))
    for integer in (False, True):
        x, N, rounds = luby_both(G, sio.random_weights(rng, n, integer))
        sio.assert_independent_and_maximal(G, x)
    S = sio.random_graph(rng, n, symmetric=False) if n > 1 else sps.csr_matrix((n, n))
    for integer in (False, True):
        base = sio.random_weights(rng, n, integer) / (4.0 if integer else 1.0)
        cljp_both(S, start_weights(S, base))


def test_graph_without_edges_and_isolated_vertices():
    n = 300
    empty = sps.csr_matrix((n, n))
    x, N, rounds = luby_both(empty, np.arange(n) % 3)
    assert np.all(x == 1) and N == n and rounds == 1
    split, passes = cljp_both(empty, np.linspace(0.0, 0.9, n))
    assert np.all(split == 1)                               # weights below 1, never decremented: selected, never F
    rng = np.random.RandomState(4)
    G = sio.random_graph(rng, n, symmetric=True)
    lonely = np.flatnonzero(np.diff(G.indptr) == 0)
    assert 0 < len(lonely) < n
    x, N, rounds = luby_both(G, rng.rand(n))
    assert np.all(x[lonely] == 1)
    S = sio.random_graph(rng, n, symmetric=False)
    split, passes = cljp_both(S, start_weights(S, rng.rand(n)))
    assert np.all(split[np.flatnonzero((np.diff(S.indptr) == 0) & (np.bincount(S.indices, minlength=n) == 0))] == 1)


def test_all_equal_weights_every_decision_a_tie():
    G = grid_graph(33, 31)
    n = G.shape[0]
    x, N, rounds = luby_both(G, np.ones(n))
    assert np.array_equal(x, sio.model_greedy_mis(n, G.indptr, G.indices, np.ones(n)))
    assert x[n - 1] == 1                                    # the largest index wins every tie it is in
    cljp_both(G, start_weights(G, np.full(n, 0.5)))


def test_path_needs_one_round_per_vertex():
    n = 300
    G = sps.diags([np.ones(n - 1), np.ones(n - 1)], [-1, 1], format="csr")
    x, N, rounds = luby_both(G, np.arange(n, dtype=np.float64))
    assert np.array_equal(x, (np.arange(n) % 2 == (n - 1) % 2).astype(np.intc))
    assert rounds == n // 2                                 # one vertex joins per round: the flag is read after each
    cljp_both(G, start_weights(G, np.arange(n) / float(n)))


@pytest.mark.parametrize("hub", ["max", "min"])
def test_star_with_a_row_of_5000(hub):
    n = 5001
    rows = np.zeros(n - 1, dtype=np.intc)
    cols = np.arange(1, n, dtype=np.intc)
    G = sps.coo_matrix((np.ones(2 * (n - 1)), (np.concatenate([rows, cols]), np.concatenate([cols, rows]))), shape=(n, n)).tocsr()
    y = np.random.RandomState(8).rand(n)
    y[0] = 2.0 if hub == "max" else -1.0
    x, N, rounds = luby_both(G, y)
    assert (x[0] == 1 and N == 1) if hub == "max" else (x[0] == 0 and N == n - 1)
    # CLJP: the leaves depend on the hub (S rows of one entry, T row of 5000), and the other way round
    leaves_on_hub = sps.coo_matrix((np.ones(n - 1), (cols, rows)), shape=(n, n)).tocsr()
    base = y / 4.0 if hub == "max" else (1.0 - y) / 4.0
    for S in (leaves_on_hub, sps.csr_matrix(leaves_on_hub.T), G):
        cljp_both(S, start_weights(S, np.clip(base, 0.0, 0.99)))


def test_amg_core_mis_with_a_stored_diagonal_and_a_partly_decided_state():
    rng = np.random.RandomState(12)
    n = 700
    G = sio.random_graph(rng, n, symmetric=True)
    G = sps.csr_matrix(G + sps.identity(n, format="csr"))
    G, Ap, Aj = csr32(G)
    y = sio.random_weights(rng, n, integer=True)
    x0 = np.full(n, -1, dtype=np.intc)
    decided = rng.rand(n) < 0.3
    x0[decided] = rng.choice([0, 1, 2, 3], int(decided.sum()))      # earlier colours, some of them the new C value
    xh, xd = x0.copy(), x0.copy()
    Nh = graph._host().amgsetup_mis_parallel(n, _ip(Ap), _ip(Aj), -1, 3, -2, _ip(xh), _dp(y), -1)
    Nd = amg_core.maximal_independent_set_parallel(n, Ap, Aj, -1, 3, -2, xd, y, -1)
    assert np.array_equal(xd, xh) and Nd == Nh
    assert np.array_equal(xd[decided], x0[decided]) and not np.any(xd == -1)
    assert Nd == np.count_nonzero(xd == 3) - np.count_nonzero(x0 == 3) > 0
    with pytest.raises(NotImplementedError):
        amg_core.maximal_independent_set_parallel(n, Ap, Aj, -1, 3, -2, x0.copy(), y, 1)


def test_amg_core_cljp_entry():
    p = sio.problem("unsym_400")
    for tag in ("CLJP", "CLJPc"):
        entry, args, outs, ret = p["calls"][tag][0]
        split = np.full(p["n"], -9, dtype=np.intc)
        amg_core.cljp_naive_splitting(int(args["n"]), np.array(args["Sp"]), np.array(args["Sj"]), np.array(args["Tp"]),
                                      np.array(args["Tj"]), split, int(args["colorflag"]))
        assert np.array_equal(split, outs["splitting"]), tag


def test_cljp_on_unsymmetric_graphs_with_tied_weights():
    p = sio.problem("unsym_400")
    S = classical.remove_diagonal(p["S"])
    n = S.shape[0]
    rng = np.random.RandomState(13)
    for base in (sio.glibc_weights(n), rng.randint(0, 3, n) / 3.0, np.zeros(n)):
        cljp_both(S, start_weights(S, base))
    S, base = planted_graph(rng)
    w0 = start_weights(S, base)
    split, passes = cljp_both(S, w0)
    for name, seen in cljp_cases(S, w0, split).items():
        assert seen, name


def test_working_size_poisson_300x300():
    A = sio.poisson2d(300, 300)
    S = classical_strength_of_connection(A, 0.25)
    assert S.shape[0] == 90000 > 65536
    np.random.seed(0)
    host = PMIS(S, device=False)
    np.random.seed(0)
    dev = PMIS(S, device=True)
    assert np.array_equal(dev, host)
    assert np.array_equal(CLJP(S, device=True), CLJP(S, device=False))


# ------------------------------------------------------------------------------------------------ hierarchies
@pytest.mark.parametrize("hier", sorted(sio.HIERARCHIES))
def test_hierarchy_through_the_device_route(hier):
    g = sio.load_hier(hier)
    cf = sio.HIERARCHIES[hier]
    A = sio.poisson2d(40, 40)
    np.random.seed(0)
    host = ruge_stuben_solver(A, CF=(cf, {"device": False}), max_coarse=20)
    np.random.seed(0)
    ml = ruge_stuben_solver(A, CF=(cf, {"device": True}), max_coarse=20)
    assert len(ml.levels) == len(host.levels) == g["meta"]["nlevels"]
    for a, b in zip(ml.levels, host.levels):
        for key in ("A", "P", "R"):
            if hasattr(b, key):
                Ma, Mb = getattr(a, key), getattr(b, key)
                assert np.array_equal(Ma.indptr, Mb.indptr) and np.array_equal(Ma.indices, Mb.indices)
                assert np.array_equal(Ma.data, Mb.data), key
    res = []
    x = ml.solve(g["b"], tol=g["meta"]["tol"], residuals=res)
    golden_io.assert_history(res, g["residuals"], g["levels"][0]["A"], g["x"], g["b"])
