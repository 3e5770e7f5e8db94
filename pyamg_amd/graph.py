"""Graph algorithms of the classical setup (pyamg/graph.py of the reference): maximal independent sets and vertex
colourings, by one of two routes that return the same integers:

  host    the reference's sequential sweeps restated in csrc/setup_host.cpp (amg_core/graph.h:34-327, :455-589);
  device  Luby's rounds run to completion in HBM (csrc/split.hip, amg_mis_device), and the rounds of the distance-k
          set (csrc/misagg.hip, amg_mis_k_device).

The device route takes what has ONE answer whatever the sweep order: Luby's algorithm without a
sweep limit on a structurally symmetric graph, which also covers the greedy serial set (priority -i) and the 'MIS'
colouring built from it.  The Jones-Plassmann and largest-degree-first colourings call ONE in-place sweep per colour,
whose result depends on the order of the sweep: they stay on the host.

The distance-k set lives in maximal_independent_set_k: every pass of its algorithm is written out of place, so it has
one answer on any pattern, with or without a round limit, and the device route refuses only
weights that are not finite.  maximal_independent_set(G, k=...) keeps refusing.

The global numpy RNG is drawn exactly where the reference draws it: rand(N) for algo='parallel', for the distance-k set,
for 'JP' and for 'LDF'.
"""
import ctypes as C

import numpy as np
from scipy import sparse

from ._host import attempt, dp as _dp, f64 as _f64, host_lib as _host, i32 as _i32, ip as _ip, outside as _outside, route

# the reference's names (tests/test_splitting_host.py pins this list); maximal_independent_set_k is public beside them
__all__ = ["asgraph", "maximal_independent_set", "vertex_coloring"]

# What device=None does when a GPU is present: the host route until the measurement in profiles/r16_splitting.txt says
# otherwise.
DEVICE_AUTO = False
# The same for the distance-k set (profiles/r21_mis_aggregation.txt).
MIS_K_DEVICE_AUTO = False


def _pattern_symmetric(n, Ap, Aj):
    return bool(_host().amgsetup_pattern_symmetric(n, _ip(Ap), _ip(Aj)))


def _luby_device(n, Ap, Aj, active, Cval, Fval, x, y, max_iters=-1, times=None):
    """amg_mis_device on a structurally symmetric graph (checked here, before anything is uploaded); x in place.
    Returns (vertices that joined, rounds).  times: a list that receives (upload, rounds, fetch) in milliseconds."""
    if max_iters != -1:
        raise _outside("the device route of an independent set with a sweep limit")
    if not _pattern_symmetric(n, Ap, Aj):
        raise _outside("the device route of an independent set on a structurally unsymmetric graph")
    from . import _lib
    before = int(np.count_nonzero(x == Cval))
    rounds = C.c_int(0)
    ms = (C.c_double * 3)()
    _lib.check(_lib.lib().amg_mis_device(n, Ap.ctypes.data, Aj.ctypes.data, y.ctypes.data, int(active), int(Cval), int(Fval),
                                         x.ctypes.data, C.byref(rounds), ms))
    if times is not None:
        times.extend([ms[0], ms[1], ms[2]])
    return int(np.count_nonzero(x == Cval)) - before, rounds.value


def luby(n, Ap, Aj, active, Cval, Fval, x, y, max_iters=-1, device=None, auto=None, times=None):
    """maximal_independent_set_parallel (graph.h:90-156) on int32 CSR arrays; x (int32) in place.  Returns the number of
    vertices that joined the set."""
    return attempt(route(device, DEVICE_AUTO if auto is None else auto),
                   lambda: _luby_device(n, Ap, Aj, active, Cval, Fval, x, y, max_iters, times)[0],
                   lambda: _host().amgsetup_mis_parallel(n, _ip(Ap), _ip(Aj), int(active), int(Cval), int(Fval), _ip(x), _dp(y),
                                                         int(max_iters)))


def asgraph(G):
    """pyamg/graph.py:23-30"""
    if not (sparse.isspmatrix_csr(G) or sparse.isspmatrix_csc(G)):
        G = sparse.csr_matrix(G)
    if G.shape[0] != G.shape[1]:
        raise ValueError("expected square matrix")
    return G


def maximal_independent_set(G, algo="serial", k=None, device=None):
    """Compute a maximal independent vertex set of a graph (pyamg/graph.py:33-81).

    G : symmetric sparse matrix whose non-zeros are the edges; self loops are ignored.
    algo : 'serial' (greedy in index order) or 'parallel' (Luby's algorithm on rand(N) weights).
    device : True = the device route (symmetric graphs only), False = the host route, None = the host route unless
    DEVICE_AUTO and a GPU.
    Returns an int32 array: 1 for the vertices of the set, 0 for the others."""
    G = asgraph(G)
    N = G.shape[0]
    if k is not None:
        raise _outside("the distance-k independent set (k=%r)" % (k,))
    if algo not in ("serial", "parallel"):
        raise ValueError("unknown algorithm (%s)" % algo)
    mis = np.full(N, -1, dtype=np.intc)
    Ap, Aj = _i32(G.indptr), _i32(G.indices)
    if algo == "parallel":
        luby(N, Ap, Aj, -1, 1, 0, mis, _f64(np.random.rand(N)), -1, device)
        return mis

    def on_host():
        mis[:] = -1
        _host().amgsetup_mis_serial(N, _ip(Ap), _ip(Aj), -1, 1, 0, _ip(mis))

    # the greedy set in index order is Luby's set for the priorities -i
    attempt(route(device, DEVICE_AUTO), lambda: _luby_device(N, Ap, Aj, -1, 1, 0, mis, -np.arange(N, dtype=np.float64)), on_host)
    return mis


def _finite_weights(y):
    if not np.all(np.isfinite(y)):
        raise _outside("the device route of the distance-k independent set on weights that are not finite")


def _mis_k_device(n, Ap, Aj, k, x, y, max_iters, times=None):
    """amg_mis_k_device; x in place.  Returns the rounds run.  times as in _luby_device."""
    _finite_weights(y)
    from . import _lib
    rounds = C.c_int(0)
    ms = (C.c_double * 3)()
    _lib.check(_lib.lib().amg_mis_k_device(n, Ap.ctypes.data, Aj.ctypes.data, int(k), y.ctypes.data, int(max_iters), x.ctypes.data,
                                           C.byref(rounds), ms))
    if times is not None:
        times.extend([ms[0], ms[1], ms[2]])
    return rounds.value


def _no_end(rounds):
    if rounds < 0:
        raise ValueError("the distance-k independent set does not end on these weights (an active weight at or below -1)")
    return rounds


def mis_k(n, Ap, Aj, k, x, y, max_iters=-1, device=None, times=None):
    """maximal_independent_set_k_parallel (graph.h:501-589) on int32 CSR arrays; x (int32) is written: 1 for the members,
    0 for the others.  Returns the number of rounds run."""
    return attempt(route(device, MIS_K_DEVICE_AUTO),
                   lambda: _mis_k_device(n, Ap, Aj, k, x, y, max_iters, times),
                   lambda: _no_end(_host().amgsetup_mis_k_parallel(n, _ip(Ap), _ip(Aj), int(k), _ip(x), _dp(y), int(max_iters))))


def maximal_independent_set_k(G, k, y=None, max_iters=-1, device=None):
    """Compute a distance-k maximal independent set: no two members within k edges of each other, every other vertex
    within k edges of a member (what pyamg/graph.py's maximal_independent_set(G, k=k) computes).

    G : sparse matrix whose non-zeros are the edges; self loops, duplicate entries, empty rows and unsymmetric patterns
    are taken as they are (edges are then followed from a row to its columns).
    y : the weights, the larger index winning a tie; None draws np.random.rand(N) where the reference draws it.
    max_iters : rounds to run, -1 = until no vertex is active (only then is the set maximal).
    device : True = the device route (finite weights only), False = the host route, None = the host route unless
    MIS_K_DEVICE_AUTO and a GPU.
    Returns an int32 array: 1 for the vertices of the set, 0 for the others."""
    G = asgraph(G)
    N = G.shape[0]
    if int(k) < 1:
        raise ValueError("k must be at least 1")
    if N == 0:
        return np.empty(0, dtype=np.intc)
    y = _f64(np.random.rand(N) if y is None else y)
    if y.shape != (N,):
        raise ValueError("expected one weight per vertex")
    mis = np.empty(N, dtype=np.intc)
    mis_k(N, _i32(G.indptr), _i32(G.indices), k, mis, y, max_iters, device)
    return mis


def vertex_coloring(G, method="MIS", device=None):
    """Compute a vertex colouring of a graph (pyamg/graph.py:84-125).

    method : 'MIS' (colour K is a greedy independent set of what is left), 'JP' (Jones-Plassmann) or 'LDF'
    (largest degree first); the last two draw rand(N).
    device : True = 'MIS' by the device route (one Luby run per colour; 'JP' and 'LDF' are refused), False = the host
    route, None = the host route unless DEVICE_AUTO and a GPU.
    Returns an int32 array of colours from 0 up."""
    G = asgraph(G)
    N = G.shape[0]
    if method not in ("MIS", "JP", "LDF"):
        raise ValueError("unknown method (%s)" % method)
    if device is True and method != "MIS":
        raise _outside("the device route of the %r colouring" % method)
    coloring = np.empty(N, dtype=np.intc)
    Ap, Aj = _i32(G.indptr), _i32(G.indices)
    L = _host()
    if method == "MIS":
        def on_device():
            coloring[:] = -1
            y = -np.arange(N, dtype=np.float64)
            done, K = 0, 0
            while done < N:
                done += _luby_device(N, Ap, Aj, -1 - K, K, -2 - K, coloring, y)[0]
                K += 1

        attempt(route(device, DEVICE_AUTO), on_device, lambda: L.amgsetup_vertex_coloring_mis(N, _ip(Ap), _ip(Aj), _ip(coloring)))
    elif method == "JP":
        z = _f64(np.random.rand(N))
        L.amgsetup_vertex_coloring_jones_plassmann(N, _ip(Ap), _ip(Aj), _ip(coloring), _dp(z))
    else:
        y = _f64(np.random.rand(N))
        L.amgsetup_vertex_coloring_LDF(N, _ip(Ap), _ip(Aj), _ip(coloring), _dp(y))
    return coloring
