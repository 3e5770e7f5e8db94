"""Designed operands of the device transpose (csrc/transpose.hip), a pure-Python model of its
definition -- a walk over P's stored arrays that appends every entry to the list of its column -- and the operators of
the classical chain's hierarchies with the sizes the host route gives them.

A case is (P, forms): P a scipy CSR matrix built from raw arrays (nothing sorted, summed or pruned) and forms the set
of forms ('lane', 'lds', 'hbm') its rows of R were designed to reach; no form at all for the cases without a launch."""
import numpy as np
import scipy.sparse as sps

import extended_io as xio
import splitting_io as sio

LANE_MAX, LDS_MAX = 32, 2048            # TR_LANE_MAX, TR_LDS_MAX of csrc/transpose.hip (_lib.TRANSPOSE_*_MAX)
_cache = {}


def raw(n_row, n_col, rows):
    """rows: per row of P a list of (column, value) in stored order"""
    Pp = np.zeros(n_row + 1, dtype=np.intc)
    Pp[1:] = np.cumsum([len(r) for r in rows])
    Pj = np.array([c for r in rows for c, _ in r], dtype=np.intc)
    Px = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return sps.csr_matrix((Px, Pj, Pp), shape=(n_row, n_col))


def model(P):
    """(Rp, Rj, Rx) by the definition: per column the entries in the order in which a walk over P's arrays meets them"""
    n_row, n_col = P.shape
    columns = [[] for _ in range(n_col)]
    for i in range(n_row):
        for k in range(P.indptr[i], P.indptr[i + 1]):
            columns[P.indices[k]].append((i, k))
    Rp = np.zeros(n_col + 1, dtype=np.intc)
    Rp[1:] = np.cumsum([len(c) for c in columns])
    Rj = np.array([i for c in columns for i, _ in c], dtype=np.intc)
    at = np.array([k for c in columns for _, k in c], dtype=np.int64)
    return Rp, Rj, np.ascontiguousarray(P.data[at], dtype=np.float64)


def forms_of(P):
    """rows of R per form, as _lib.transpose_last_route() reports them: (lane_rows, lds_rows, hbm_rows)"""
    length = np.bincount(P.indices, minlength=P.shape[1])
    return int(np.sum(length <= LANE_MAX)), int(np.sum((length > LANE_MAX) & (length <= LDS_MAX))), int(np.sum(length > LDS_MAX))


def _random(n_row, n_col, per_row, seed, order):
    rng = np.random.RandomState(seed)
    rows = []
    for _ in range(n_row):
        cols = rng.choice(n_col, size=min(per_row, n_col), replace=False)
        cols = {"descending": lambda c: np.sort(c)[::-1], "shuffled": lambda c: c, "ascending": np.sort}[order](cols)
        rows.append([(int(c), float(rng.randn())) for c in cols])
    return raw(n_row, n_col, rows)


def _hub(length, where):
    """one column that receives every one of `length` rows, first, last or between short columns (8 entries or fewer)"""
    n_col = 5
    hub = {"first": 0, "last": n_col - 1, "between": 2}[where]
    others = [c for c in range(n_col) if c != hub]
    rows = []
    for i in range(length):
        row = [(hub, float(i + 1))]
        if i < 8:
            row.append((others[i % 4], -float(i + 1)))
        rows.append(row[::-1] if i % 2 else row)
    return raw(length, n_col, rows)


def _value_bits():
    bits = np.array([0x8000000000000000, 0x0000000000000000, 0x7ff8000000001234, 0xfff8000000000abc, 0x7ff0000000000001,
                     0x7ff0000000000000, 0xfff0000000000000, 0x0000000000000001, 0x800fffffffffffff], dtype=np.uint64)
    vals = bits.view(np.float64)
    P = raw(3, 4, [[(3, 0.0), (0, 0.0), (1, 0.0)], [(1, 0.0), (3, 0.0), (2, 0.0)], [(0, 0.0), (1, 0.0), (3, 0.0)]])
    P.data[:] = vals
    assert P.data.view(np.uint64).tolist() == bits.tolist()
    return P


def cases():
    """name -> (P, forms)"""
    if "cases" in _cache:
        return _cache["cases"]
    out = {
        "no_rows": (raw(0, 5, []), set()),
        "no_entries": (raw(4, 3, [[], [], [], []]), set()),
        "one_by_one": (raw(1, 1, [[(0, 2.5)]]), {"lane"}),
        "single_row": (raw(1, 7, [[(5, 1.0), (1, 2.0), (3, 3.0)]]), {"lane"}),
        "single_column": (raw(9, 1, [[(0, float(i))] for i in range(9)]), {"lane"}),
        "empty_columns": (raw(6, 8, [[(2, 1.0), (5, 2.0)], [(6, 3.0)], [], [(3, 4.0), (2, 5.0)], [(5, 6.0)], [(6, 7.0), (3, 8.0)]]),
                          {"lane"}),
        "wide": (_random(5, 40, 6, 1, "shuffled"), {"lane"}),
        "tall": (_random(40, 5, 3, 2, "shuffled"), {"lane"}),
        "descending": (_random(50, 20, 7, 3, "descending"), {"lane"}),
        "shuffled": (_random(50, 20, 7, 4, "shuffled"), {"lane"}),
        "duplicates": (raw(4, 5, [[(2, 1.0), (0, 2.0), (2, -1.0)], [(3, 3.0), (3, 4.0), (1, 5.0), (3, -6.0)], [(2, 7.0)],
                                  [(3, 8.0), (2, 9.0), (2, 9.5)]]), {"lane"}),
        "value_bits": (_value_bits(), {"lane"}),
        "interleaved": (_random(5000, 300, 8, 5, "shuffled"), {"lds"}),
    }
    perm = np.random.RandomState(6).permutation(70000)
    out["many_columns"] = (sps.csr_matrix((np.arange(70000, dtype=np.float64) + 1.0, perm.astype(np.intc),
                                           np.arange(70001, dtype=np.intc)), shape=(70000, 70000)), {"lane"})
    for threshold, below, above in ((LANE_MAX, "lane", "lds"), (LDS_MAX, "lds", "hbm")):
        for length in (threshold - 1, threshold, threshold + 1):
            for where in ("first", "last", "between"):
                out["hub_%d_%s" % (length, where)] = (_hub(length, where), {"lane", below if length <= threshold else above})
    _cache["cases"] = out
    return out


# ------------------------------------------------------------------------------------------------ hierarchies
def star(leaves):
    """hub 0 joined to `leaves` leaves: off-diagonals -1, hub diagonal `leaves`, leaf diagonals 1.5"""
    n = leaves + 1
    rows = [[(0, float(leaves))] + [(j, -1.0) for j in range(1, n)]] + [[(0, -1.0), (j, 1.5)] for j in range(1, n)]
    A = raw(n, n, rows)
    assert A.has_canonical_format
    return A


def poisson1d(n):
    A = sps.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")
    A.indices, A.indptr = A.indices.astype(np.intc), A.indptr.astype(np.intc)
    return A


def diagonal(n):
    return raw(n, n, [[(i, float(i + 1))] for i in range(n)])


EXTENDED_4 = ("extended_i", {"max_per_row": 4})
# name -> (operator, options of ruge_stuben_solver, level sizes of the host hierarchy, coarse row order: True where
# every coarse product has sorted rows, False where every one is unsorted, None where the table does not say)
HIERARCHIES = {
    "poisson_pmis": (lambda: sio.poisson2d(40, 40), dict(CF="PMIS", max_coarse=20), [1600, 593, 148, 34, 9], False),
    "poisson_cljp": (lambda: sio.poisson2d(40, 40), dict(CF="CLJP", max_coarse=20), [1600, 978, 338, 122, 44, 17], False),
    "line_pmis": (lambda: poisson1d(50), dict(CF="PMIS", max_coarse=5), [50, 21, 11, 5], True),
    "diagonal_pmis": (lambda: diagonal(30), dict(CF="PMIS", max_coarse=5, max_levels=4), [30, 30, 30, 30], True),
    "star_pmis": (lambda: star(300), dict(CF="PMIS", max_coarse=5), [301, 1], None),
    "star_cljp": (lambda: star(300), dict(CF="CLJP", max_coarse=5), [301, 1], None),
    "poisson_pmis_ext": (lambda: sio.poisson2d(40, 40), dict(CF="PMIS", max_coarse=20, interpolation="extended_i"),
                         [1600, 593, 136, 26, 7], None),
    "poisson_pmis_ext4": (lambda: sio.poisson2d(40, 40), dict(CF="PMIS", max_coarse=20, interpolation=EXTENDED_4),
                          [1600, 593, 136, 28, 8], None),
    "poisson_cljp_ext": (lambda: sio.poisson2d(40, 40), dict(CF="CLJP", max_coarse=20, interpolation="extended_i"), None, None),
    "poisson_cljp_ext4": (lambda: sio.poisson2d(40, 40), dict(CF="CLJP", max_coarse=20, interpolation=EXTENDED_4), None, None),
    "poisson3d_pmis_ext": (lambda: xio.poisson3d(12), dict(CF="PMIS", max_coarse=20, interpolation="extended_i"), None, None),
    "aniso_pmis": (xio.aniso, dict(CF="PMIS", max_coarse=20), None, None),
    "big_star_pmis": (lambda: star(3000), dict(CF="PMIS", max_coarse=5), [3001, 1], None),
}


def host_hierarchy(name, keep=True):
    """the hierarchy of HIERARCHIES[name] by the host route from seed 0, built once and shared"""
    from pyamg_amd.classical import ruge_stuben_solver
    key = ("host", name, keep)
    if key not in _cache:
        make, options, _, _ = HIERARCHIES[name]
        np.random.seed(0)
        _cache[key] = ruge_stuben_solver(make(), keep=keep, device=False, **options)
    return _cache[key]


def rows_sorted(A):
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return not np.any((rows[1:] == rows[:-1]) & (np.diff(A.indices.astype(np.int64)) <= 0))
