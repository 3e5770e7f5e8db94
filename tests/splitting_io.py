"""Fixtures of the parallel C/F splittings (tests/golden/splitting/, recorded from the reference by
tools/gen_golden_splitting.py) and plain sequential Python models of the two native loops behind them, written from
the reference's text (amg_core/graph.h:90-156, amg_core/ruge_stuben.h:316-480)."""
import ctypes
import os

import numpy as np
import scipy.sparse as sps

import golden_io

DIR = os.path.join(golden_io.GOLDEN, "splitting")
PROBLEMS = ("poisson_17x23", "poisson_40x40", "aniso_40x40", "unsym_400")
SPLITTINGS = ("PMIS", "PMISc_JP", "PMISc_MIS", "PMISc_LDF", "CLJP", "CLJPc")
HIERARCHIES = {"rs_pmis_2d": "PMIS", "rs_cljp_2d": "CLJP"}
ARGS = {"maximal_independent_set_serial": ("num_rows", "Ap", "Aj", "active", "C", "F", "x"),
        "maximal_independent_set_parallel": ("num_rows", "Ap", "Aj", "active", "C", "F", "x", "y", "max_iters"),
        "vertex_coloring_mis": ("num_rows", "Ap", "Aj", "x"),
        "vertex_coloring_jones_plassmann": ("num_rows", "Ap", "Aj", "x", "z"),
        "vertex_coloring_LDF": ("num_rows", "Ap", "Aj", "x", "y"),
        "cljp_naive_splitting": ("n", "Sp", "Sj", "Tp", "Tj", "splitting", "colorflag")}

_cache = {}


def problem(name):
    """-> dict: S, G (csr), n, one entry per recorded run (its result) and calls[run] = [(entry, args, outputs, ret)]"""
    if name in _cache:
        return _cache[name]
    z = np.load(os.path.join(DIR, "%s.npz" % name), allow_pickle=False)
    n = int(z["n"])
    p = {"n": n,
         "S": sps.csr_matrix((z["S_data"], z["S_indices"], z["S_indptr"]), shape=(n, n)),
         "G": sps.csr_matrix((np.ones(len(z["G_indices"])), z["G_indices"], z["G_indptr"]), shape=(n, n)),
         "calls": {}, "tags": [str(t) for t in z["tags"]]}
    for tag in p["tags"]:
        p[tag] = z[tag]
        calls = []
        for ci, entry in enumerate(z[tag + "__calls"]):
            entry = str(entry)
            pre = "%s__c%d__" % (tag, ci)
            args = {a: z[pre + a] for a in ARGS[entry] if pre + a in z.files}
            outs = {k[len(pre):-4]: z[k] for k in z.files if k.startswith(pre) and k.endswith("_out")}
            calls.append((entry, args, outs, int(z[pre + "ret"])))
        p["calls"][tag] = calls
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[name] = p
    return p


def mis_calls(name):
    """every recorded maximal_independent_set_parallel call of a problem: (run, args, x_out, ret)"""
    p = problem(name)
    return [(tag, args, outs["x"], ret) for tag in p["tags"] for entry, args, outs, ret in p["calls"][tag]
            if entry == "maximal_independent_set_parallel"]


def load_hier(name):
    """golden_io.load_hier for a hier_<name>.npz of tests/golden/splitting/"""
    keep = golden_io.GOLDEN
    golden_io.GOLDEN = DIR
    try:
        return golden_io.load_hier(name)
    finally:
        golden_io.GOLDEN = keep


def poisson2d(nx, ny):
    """the 5-point Laplacian, last axis fastest, sorted int32 CSR (what the fixtures were recorded on)"""
    def lap(n):
        return sps.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")
    A = sps.csr_matrix(sps.kron(lap(nx), sps.identity(ny, format="csr")) + sps.kron(sps.identity(nx, format="csr"), lap(ny)))
    A.sort_indices()
    A.indices = A.indices.astype(np.intc)
    A.indptr = A.indptr.astype(np.intc)
    return A


# ------------------------------------------------------------------------------------------------ properties
def assert_independent_and_maximal(G, mis):
    """mis (1 in the set, 0 beside it) on the graph G, self loops ignored"""
    G = sps.csr_matrix(G)
    n = G.shape[0]
    rows = np.repeat(np.arange(n), np.diff(G.indptr))
    off = rows != G.indices
    rows, cols = rows[off], G.indices[off]
    assert set(np.unique(mis)) <= {0, 1}
    assert not np.any((mis[rows] == 1) & (mis[cols] == 1)), "two adjacent vertices in the set"
    covered = np.zeros(n, dtype=bool)
    covered[rows[mis[cols] == 1]] = True
    assert np.all(covered[mis == 0]), "a vertex outside the set has no neighbour in it"


def assert_proper_coloring(G, colors):
    G = sps.csr_matrix(G)
    rows = np.repeat(np.arange(G.shape[0]), np.diff(G.indptr))
    off = rows != G.indices
    assert colors.min() >= 0
    assert not np.any(colors[rows[off]] == colors[G.indices[off]]), "two adjacent vertices share a colour"


# ------------------------------------------------------------------------------------------------ sequential models
def model_mis_parallel(n, Ap, Aj, active, C, F, x, y, max_iters=-1):
    """graph.h:90-156: in-place sweeps in index order; x is changed; returns the number of vertices that became C"""
    N = 0
    sweeps = 0
    active_nodes = True
    while active_nodes and (max_iters == -1 or sweeps < max_iters):
        active_nodes = False
        sweeps += 1
        for i in range(n):
            if x[i] != active:
                continue
            row = Aj[Ap[i]:Ap[i + 1]]
            selected = True
            for j in row:
                if x[j] == C:
                    x[i] = F
                    selected = False
                    break
                if x[j] == active and (y[j] > y[i] or (y[j] == y[i] and j > i)):
                    selected = False
                    break
            if selected:
                for j in row:
                    if x[j] == active:
                        x[j] = F
                N += 1
                x[i] = C
            else:
                active_nodes = True
    return N


def model_greedy_mis(n, Ap, Aj, y):
    """the set Luby's algorithm run to completion must return on a symmetric graph: vertices taken in descending order
    of (y, index), each joining when no neighbour has joined before it"""
    order = sorted(range(n), key=lambda i: (y[i], i), reverse=True)
    mis = np.zeros(n, dtype=np.intc)
    for i in order:
        if not any(mis[j] == 1 for j in Aj[Ap[i]:Ap[i + 1]] if j != i):
            mis[i] = 1
    return mis


def glibc_weights(n, seed=2448422):
    """rand() / RAND_MAX of the C library after srand(seed), as ruge_stuben.h:357-360 draws them"""
    libc = ctypes.CDLL(None)
    libc.rand.restype = ctypes.c_int
    libc.srand(ctypes.c_uint(seed))
    return np.array([float(libc.rand()) / 2147483647 for _ in range(n)], dtype=np.float64)


def model_cljp_start_weights(n, Sp, Sj, base):
    """ruge_stuben.h:363-370: +1 per vertex that depends on i, one addition at a time"""
    w = np.array(base, dtype=np.float64)
    for i in range(n):
        for j in Sj[Sp[i]:Sp[i + 1]]:
            if i != j:
                w[j] = w[j] + 1.0
    return w


def model_cljp_select(n, Sp, Sj, Tp, Tj, weight):
    """ruge_stuben.h:373-478: the selection loop in the reference's order; weight is changed; returns the splitting"""
    U, Fp, Cp = 2, 0, 1
    splitting = np.full(n, U, dtype=np.intc)
    edgemark = np.ones(Sp[n], dtype=np.intc)
    cache = np.full(n, -1, dtype=np.int64)
    unassigned = n
    while unassigned > 0:
        Dlist = []
        for i in range(n):
            if splitting[i] != U:
                continue
            top = True
            for j in Sj[Sp[i]:Sp[i + 1]]:
                if splitting[j] == U and weight[j] > weight[i]:
                    top = False
                    break
            if top:
                for j in Tj[Tp[i]:Tp[i + 1]]:
                    if splitting[j] == U and weight[j] > weight[i]:
                        top = False
                        break
            if top:
                Dlist.append(i)
                unassigned -= 1
        for c in Dlist:
            splitting[c] = Cp
        for c in Dlist:
            for jj in range(Sp[c], Sp[c + 1]):
                j = Sj[jj]
                if splitting[j] == U and edgemark[jj] != 0:
                    edgemark[jj] = 0
                    weight[j] -= 1.0
                    if weight[j] < 1:
                        splitting[j] = Fp
                        unassigned -= 1
        for c in Dlist:
            for j in Tj[Tp[c]:Tp[c + 1]]:
                if splitting[j] == U:
                    cache[j] = c
            for j in Tj[Tp[c]:Tp[c + 1]]:
                for kk in range(Sp[j], Sp[j + 1]):
                    k = Sj[kk]
                    if splitting[k] == U and edgemark[kk] != 0 and cache[k] == c:
                        edgemark[kk] = 0
                        weight[k] -= 1.0
                        if weight[k] < 1:
                            splitting[k] = Fp
                            unassigned -= 1
    return splitting


# ------------------------------------------------------------------------------------------------ random graphs
def random_graph(rng, n, symmetric, diagonal=False):
    """CSR pattern (int32) of a random graph of n vertices with some isolated ones"""
    density = rng.uniform(0.02, 0.3)
    M = (rng.rand(n, n) < density).astype(np.int8)
    if not diagonal:
        np.fill_diagonal(M, 0)
    lonely = rng.rand(n) < 0.1
    M[lonely, :] = 0
    M[:, lonely] = 0
    if symmetric:
        M = ((M + M.T) > 0).astype(np.int8)
    G = sps.csr_matrix(M)
    G.sort_indices()
    G.indices = G.indices.astype(np.intc)
    G.indptr = G.indptr.astype(np.intc)
    return G


def random_weights(rng, n, integer):
    """integer-valued weights make ties frequent"""
    return rng.randint(0, 4, n).astype(np.float64) if integer else rng.rand(n)
