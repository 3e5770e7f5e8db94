"""Designed graphs, fixtures and pure-Python models for the distance-k independent set and the MIS(2) aggregation
(DESIGN.md section 8l).  Shared by tests/test_mis_k_host.py, tests/test_mis_aggregation_host.py,
tests/test_gpu_mis_aggregation.py and tools/gen_golden_mis_k.py, which runs the reference on graphs() and writes
tests/golden/mis_k/cases.npz.

Every graph is a dict: n, Ap, Aj (int32 CSR, as stored: rows may be unsorted and hold a column twice), y (float64),
symmetric (whether the pattern is structurally symmetric) and limits (whether it also runs with max_iters 1 and 2).
"""
import functools
import os

import numpy as np
import scipy.sparse as sps

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mis_k", "cases.npz")
KS = (1, 2, 3)


def _graph(Ap, Aj, y, symmetric=True, limits=False):
    Ap, Aj = np.ascontiguousarray(Ap, dtype=np.intc), np.ascontiguousarray(Aj, dtype=np.intc)
    n = len(Ap) - 1
    y = np.ascontiguousarray(y, dtype=np.float64)
    assert y.shape == (n,) and Ap[0] == 0 and Ap[-1] == len(Aj) and (n == 0 or len(Aj) == 0 or (0 <= Aj.min() and Aj.max() < n))
    return {"n": n, "Ap": Ap, "Aj": Aj, "y": y, "symmetric": symmetric, "limits": limits}


def _from_rows(rows, y, **kw):
    Ap = np.concatenate(([0], np.cumsum([len(r) for r in rows])))
    Aj = np.array([j for r in rows for j in r], dtype=np.intc)
    return _graph(Ap, Aj, y, **kw)


def _from_edges(n, edges, y, **kw):
    rows = [[] for _ in range(n)]
    for a, b in edges:
        rows[a].append(b)
        rows[b].append(a)
    return _from_rows(rows, y, **kw)


def _path(n, y):
    return _from_edges(n, [(i, i + 1) for i in range(n - 1)], y, limits=True)


def _grid(nx, ny):
    """5-point grid with stored diagonals (self loops): n = 323 is no multiple of 64 or 256"""
    idx = np.arange(nx * ny).reshape(nx, ny)
    edges = [(idx[i, j], idx[i + 1, j]) for i in range(nx - 1) for j in range(ny)]
    edges += [(idx[i, j], idx[i, j + 1]) for i in range(nx) for j in range(ny - 1)]
    g = _from_edges(nx * ny, edges, np.random.RandomState(3).rand(nx * ny), limits=True)
    rows = [sorted([i] + list(g["Aj"][g["Ap"][i]:g["Ap"][i + 1]])) for i in range(g["n"])]
    return _from_rows(rows, g["y"], limits=True)


def _star(leaves=700, tail=40):
    """centre 0, leaves 1 .. leaves, and a path of `tail` vertices hanging off the last leaf: one long row.  (The device
    route has no long-row form, so there is no threshold for the leaf count to exceed.)"""
    edges = [(0, i) for i in range(1, leaves + 1)]
    edges += [(leaves + t, leaves + t + 1) for t in range(tail)]
    n = leaves + tail + 1
    return _from_edges(n, edges, np.random.RandomState(4).randint(0, 5, n) / 4.0)


def _degenerate(n=300):
    """two components (0 .. 149 and 150 .. 299) of random edges, then: rows 7, 160, 161 and 299 emptied (with their
    mirrors), rows 20 and 200 left with only their self loop, self loops on every fifth vertex, every row's entries
    reversed or shuffled (unsorted), and a column stored twice in every third non-empty row (its mirror once)."""
    rng = np.random.RandomState(5)
    nbr = [set() for _ in range(n)]
    for lo, hi in ((0, 150), (150, 300)):
        for i in range(lo, hi - 1):
            nbr[i].add(i + 1)
            nbr[i + 1].add(i)
        for _ in range(150):
            a, b = rng.randint(lo, hi, 2)
            if a != b:
                nbr[a].add(b)
                nbr[b].add(a)
    for i in (7, 160, 161, 299, 20, 200):
        for j in nbr[i]:
            nbr[j].discard(i)
        nbr[i] = set()
    rows = []
    for i in range(n):
        r = sorted(nbr[i])
        if i % 5 == 0 and i not in (7, 160, 161, 299):
            r.append(i)
        rng.shuffle(r)
        if i % 3 == 0 and len(r) > 0:
            r.insert(rng.randint(0, len(r) + 1), r[0])
        rows.append(r)
    assert rows[7] == [] and rows[20] == [20] and rows[200] == [200]
    return _from_rows(rows, rng.randint(0, 4, n) / 4.0)


def _random_symmetric(n=1000, per_row=6):
    rng = np.random.RandomState(6)
    M = sps.random(n, n, density=per_row / 2.0 / n, random_state=rng, format="csr")
    M = sps.csr_matrix(M + M.T)
    M.sort_indices()
    return _graph(M.indptr, M.indices, rng.randint(0, 8, n) / 8.0)


def _random_unsymmetric(n=400):
    rng = np.random.RandomState(7)
    M = sps.random(n, n, density=5.0 / n, random_state=rng, format="csr")
    M.sort_indices()
    assert (abs(M - M.T) > 0).nnz > 0
    return _graph(M.indptr, M.indices, rng.randint(0, 8, n) / 8.0, symmetric=False)


@functools.lru_cache(maxsize=None)
def graphs():
    """name -> graph, in a fixed order"""
    out = {}
    out["path_increasing"] = _path(200, np.arange(200) / 200.0)
    out["path_equal"] = _path(200, np.full(200, 0.5))
    out["path_quarters"] = _path(200, np.random.RandomState(2).randint(0, 4, 200) / 4.0)
    out["grid_17x19"] = _grid(17, 19)
    out["star_700"] = _star()
    out["degenerate_300"] = _degenerate()
    out["random_symmetric_1000"] = _random_symmetric()
    out["random_unsymmetric_400"] = _random_unsymmetric()
    out["one_vertex"] = _from_rows([[]], [0.25])
    out["one_vertex_loop"] = _from_rows([[0]], [0.25])
    out["empty"] = _graph([0], [], [])
    for g in out.values():
        for a in ("Ap", "Aj", "y"):
            g[a].setflags(write=False)
    return out


def runs(name):
    """the (k, max_iters) pairs of a graph"""
    limits = (-1, 1, 2) if graphs()[name]["limits"] else (-1,)
    return [(k, m) for k in KS for m in limits]


def all_runs():
    return [(name, k, m) for name in graphs() for k, m in runs(name)]


def symmetric_names():
    return [name for name, g in graphs().items() if g["symmetric"]]


def run_id(name, k, m):
    return "%s-k%d-m%d" % (name, k, m)


def key(name, k, m):
    return "%s__k%d__m%d__x" % (name, k, m)


@functools.lru_cache(maxsize=None)
def fixture():
    """the reference's x of every run, read once; the arrays are read-only"""
    with np.load(FIXTURE) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def reference_x(name, k, m):
    f = fixture()
    g = graphs()[name]
    for a in ("Ap", "Aj", "y"):          # the fixture was made on these very graphs
        assert np.array_equal(f["%s__%s" % (name, a)], g[a]), "tests/golden/mis_k/cases.npz is stale: rerun tools/gen_golden_mis_k.py"
    return f[key(name, k, m)]


def matrix(g):
    """the graph as a scipy CSR matrix that keeps the stored order and the duplicates"""
    return sps.csr_matrix((np.ones(len(g["Aj"]), dtype=np.int8), g["Aj"].copy(), g["Ap"].copy()), shape=(g["n"], g["n"]))


# ------------------------------------------------------------------------------------------------ models
def model_propagate(Ap, Aj, keys, vals):
    """one out-of-place max-propagation: the (value, key) maximum over a vertex and its row, the larger key on equal
    values"""
    n = len(Ap) - 1
    o_keys, o_vals = list(keys), list(vals)
    for i in range(n):
        k_max, v_max = keys[i], vals[i]
        for jj in range(Ap[i], Ap[i + 1]):
            j = Aj[jj]
            k_j, v_j = keys[j], vals[j]
            if k_j == k_max or v_j < v_max:
                continue
            if v_j > v_max or k_j > k_max:
                k_max, v_max = k_j, v_j
        o_keys[i], o_vals[i] = k_max, v_max
    return o_keys, o_vals


def model_mis_k(g, k, max_iters=-1):
    """the algorithm of section 8l in plain Python -> (x, rounds)"""
    n = g["n"]
    Ap, Aj, y = g["Ap"].tolist(), g["Aj"].tolist(), g["y"].tolist()
    x = [0] * n
    active = [True] * n
    keys, vals = list(range(n)), list(y)
    rounds = 0
    while max_iters == -1 or rounds < max_iters:
        rounds += 1
        for _ in range(k):
            keys, vals = model_propagate(Ap, Aj, keys, vals)
        for i in range(n):
            if keys[i] == i and active[i]:
                x[i] = 1
        keys, vals = list(range(n)), [float(v) for v in x]
        for _ in range(k):
            keys, vals = model_propagate(Ap, Aj, keys, vals)
        work_left = False
        for i in range(n):
            if vals[i] == 1:
                active[i] = False
                vals[i] = -1.0
            else:
                vals[i] = y[i]
                work_left = True
        keys = list(range(n))
        if not work_left:
            break
    return np.array(x, dtype=np.intc), rounds


def model_mis_aggregation(g, x=None):
    """the definition of section 8l in plain Python -> (agg with -1 for the vertices of no aggregate, Cpts)"""
    n, Ap, Aj, y = g["n"], g["Ap"], g["Aj"], g["y"]
    if x is None:
        x = model_mis_k(g, 2)[0]
    row = [[int(j) for j in Aj[Ap[i]:Ap[i + 1]] if j != i] for i in range(n)]
    cpts = [i for i in range(n) if x[i] and row[i]]
    number = {r: a for a, r in enumerate(cpts)}
    agg1 = [-1] * n
    for i in range(n):
        if i in number:
            agg1[i] = number[i]
        else:
            roots = {j for j in row[i] if j in number}
            assert len(roots) <= 1, "two roots within two edges of each other"
            if roots:
                agg1[i] = number[roots.pop()]
    agg2 = list(agg1)
    for i in range(n):
        if agg1[i] == -1 and row[i]:
            cand = [(y[cpts[agg1[j]]], cpts[agg1[j]]) for j in row[i] if agg1[j] != -1]
            assert cand, "a vertex with a neighbour was left over"
            agg2[i] = number[max(cand)[1]]
    return np.array(agg2, dtype=np.intc), np.array(cpts, dtype=np.intc)


def agg_of(AggOp):
    """the aggregate of every row of AggOp, -1 for a zero row"""
    AggOp = sps.csr_matrix(AggOp)
    counts = np.diff(AggOp.indptr)
    assert counts.max(initial=0) <= 1 and np.all(AggOp.data == 1)
    agg = np.full(AggOp.shape[0], -1, dtype=np.intc)
    agg[counts == 1] = AggOp.indices
    return agg


def distances_from(g, sources, limit):
    """breadth-first search along the stored entries: hops from the nearest source, limit + 1 where it is further"""
    dist = np.full(g["n"], limit + 1, dtype=np.int64)
    front = [int(s) for s in sources]
    dist[front] = 0
    for d in range(1, limit + 1):
        nxt = []
        for i in front:
            for j in g["Aj"][g["Ap"][i]:g["Ap"][i + 1]]:
                if dist[j] > d:
                    dist[j] = d
                    nxt.append(int(j))
        front = nxt
    return dist
