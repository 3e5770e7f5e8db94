"""TEST INFRASTRUCTURE: the designed operators, operands and NumPy models that pin the multi-RHS engine
(csrc/hier_multi.hip, amg_hierm_*): tests/test_multi_cases_host.py on the CPU, tests/test_gpu_multi_forms.py on the
device.  tests/c128_cases.py builds the complex128 engine's cases on the same patterns.

Everything is built on operator_cases.irregular(), whose content rules stay: explicit zeros and unsorted even rows;
rows with no diagonal, a 0.0 diagonal or a doubled diagonal; doubled off-diagonal entries; the diagonal stored last in
long even rows.  Nothing here needs a GPU."""
import numpy as np

import operator_cases as oc

# RESTATEMENTS of csrc/hier_multi.hip (kept in step by reading; test_multi_cases_host asserts what the families claim
# under these values): Shape<KP>::ROWS, the rows of one workgroup of csr_rows_multi / csr_rows_direct at the layout
# width KP; CHUNK, the entries staged in LDS at a time; DIRECT_MAX_ROW, apply_rows takes csr_rows_direct when
# nnz <= DIRECT_MAX_ROW * nrows; the fixed grid of norm_partial_multi / norm_final_multi is restated in vector_models.
ROWS = {1: 256, 2: 256, 4: 128, 8: 64}
CHUNK = 2048
DIRECT_MAX_ROW = 12
WIDTHS = (1, 2, 4, 8)

N1 = 37                                  # coarse size of the transfer cycles
KS = (1, 2, 3, 4, 5, 8)                  # columns per call, each on a handle created for exactly that many
KMAX_PAIRS = [(k, k) for k in KS] + [(8, 3)]       # (kmax of amg_hierm_create, k of the call)
ZERO_COLUMN = 2                          # the all-zero column of B and X (calls of three columns or more have it)
GUARD = -8.765e201                       # the guard row behind row n - 1 of every host B and X

LONG_LENGTHS = oc.LONG_LENGTHS


def width_of(k):
    """RESTATEMENT of hier_multi.hip width_of: the layout width k columns run at"""
    return 1 if k <= 1 else 2 if k <= 2 else 4 if k <= 4 else 8


def kernel_of(csr):
    """'direct' or 'staged': the side of apply_rows' rule an operator is on ('none': no rows, no launch)"""
    n, nnz = csr[0], int(csr[2][-1])
    if n == 0:
        return "none"
    return "direct" if nnz <= DIRECT_MAX_ROW * n else "staged"


# ---------------------------------------------------------------------------------------------- square operators
def _irregular(seed, nrows, ncols, lengths):
    """operator_cases.irregular, which needs three columns or more (column 0 and the row's own are never drawn)"""
    lengths = np.minimum(np.asarray(lengths, dtype=np.int64), max(ncols - 2, 0))
    if ncols < 3 or nrows == 0:
        return oc.empty(nrows, ncols)
    return oc.irregular(seed, nrows, ncols, lengths)


def short(n):
    """row lengths 0..12 (fewer where n - 2 is less), first and last rows empty, a run of 40 empty rows; n = 1: the one
    entry a 1 x 1 operator can hold, a diagonal"""
    if n == 1:
        return 1, 1, np.array([0, 1], dtype=np.intc), np.zeros(1, dtype=np.intc), np.array([0.75])
    rng = np.random.RandomState(2000 + n)
    lengths = rng.randint(0, 13, size=n)
    lengths[0] = lengths[-1] = 0
    if n > 120:
        lengths[60:100] = 0
    return _irregular(13 + n, n, n, lengths)


SHORT_STAGED_LONG_ROWS = (5, 130, 131, 255, 256, 290, 900, 901, 1023, 1099)


def short_staged():
    """n = 1100, lengths 0..12; rows 300..811 are empty, so at every width a whole workgroup has e0 == e1 (rows 512..767
    at 256 rows per workgroup, 384..511 at 128, 320..383 at 64); ten rows of 900..1090 entries (a row of 1100 columns
    holds no more distinct ones) put the operator on the staged side and rows across chunk boundaries"""
    rng = np.random.RandomState(2301)
    lengths = rng.randint(0, 13, size=1100)
    lengths[list(SHORT_STAGED_LONG_ROWS)] = rng.randint(900, 1091, size=len(SHORT_STAGED_LONG_ROWS))
    lengths[300:812] = 0
    return _irregular(2302, 1100, 1100, lengths)


LONG_N = 6200


def long_rows(lo, hi, seed):
    """n = 6200: the first twelve rows have LONG_LENGTHS (one chunk less one, exactly one, one more, two and three
    chunks), every other row lo..hi entries"""
    rng = np.random.RandomState(seed)
    lengths = rng.randint(lo, hi + 1, size=LONG_N)
    lengths[:len(LONG_LENGTHS)] = LONG_LENGTHS
    return _irregular(seed + 1, LONG_N, LONG_N, lengths)


def threshold_pair():
    """(at, over): one matrix of n = 200 rows with nnz == 12 n exactly, and the same matrix with one more entry behind
    the last row's"""
    n = 200
    rng = np.random.RandomState(2401)
    lengths = rng.randint(4, 21, size=n)
    i = 0
    while lengths.sum() != DIRECT_MAX_ROW * n:            # one entry at a time, row after row
        step = 1 if lengths.sum() < DIRECT_MAX_ROW * n else -1
        if 1 <= lengths[i % n] + step <= 24:
            lengths[i % n] += step
        i += 1
    at = _irregular(2402, n, n, lengths)
    Ap = at[2].copy()
    Ap[-1] += 1
    over = (n, n, Ap, np.append(at[3], np.intc(7)).astype(np.intc), np.append(at[4], 0.3125))
    return at, over


def dominant(csr):
    """The same operator with every off-diagonal value of row i scaled by 0.4 / len(row i).  The stored diagonals have
    magnitude 0.5 to 1.5 and the drawn values lie in (-1, 1), so every row with a usable diagonal is strictly
    dominant (off-diagonal sum below 0.4) and the iterates of every smoother stay finite."""
    n, nc, Ap, Aj, Ax = csr
    Ax = Ax.copy()
    for i in range(n):
        s, e = int(Ap[i]), int(Ap[i + 1])
        if e > s:
            off = Aj[s:e] != i
            Ax[s:e][off] = Ax[s:e][off] * (0.4 / (e - s))
    return n, nc, Ap, Aj, Ax


# ---------------------------------------------------------------------------------------------- transfer operators
def restriction(n0, seed, with_long):
    """R (N1 x n0) with long rows: lengths 0..700 (0..n0 - 2 where that is less), two empty rows; with_long: its first
    twelve rows have LONG_LENGTHS"""
    rng = np.random.RandomState(seed)
    lengths = rng.randint(0, 701, size=N1)
    lengths[[3, 20]] = 0
    if with_long:
        lengths[:len(LONG_LENGTHS)] = LONG_LENGTHS
    return _irregular(seed + 1, N1, n0, lengths)


def prolongation(n0, seed, sparse_rows):
    """P (n0 x N1) with row lengths 0..30 and runs of empty rows: rows n0/5 .. n0/5 + 40, and with sparse_rows the
    middle third as well (which puts P on the direct side)"""
    rng = np.random.RandomState(seed)
    lengths = rng.randint(0, 31, size=n0)
    lengths[n0 // 5:n0 // 5 + 40] = 0
    if sparse_rows:
        lengths[n0 // 3:n0 // 3 + (2 * n0) // 5] = 0
    return _irregular(seed + 1, n0, N1, lengths)


def coarse_identity(n):
    return n, n, np.arange(n + 1, dtype=np.intc), np.arange(n, dtype=np.intc), np.ones(n)


# ---------------------------------------------------------------------------------------------- cases
class Case(object):
    """One square operator A with everything its two kinds of cycle need.
    A: as built; Ad: dominant(A), what the smoother cycles run on; kernel: the side of the nnz <= 12 n rule.
    R, P, A1 (identity), M (dense N1 x N1): the transfer cycle.  B8, X8: (n + 1, 8) right-hand sides and starting
    iterates, row n the guard row; a call of k columns takes the first k."""

    def __init__(self, name, csr, kernel, with_long=False):
        self.name = name
        self.A = csr
        self.n = csr[0]
        self.nnz = int(csr[2][-1])
        self.kernel = kernel
        self.Ad = dominant(csr)
        seed = 5000 + sum(map(ord, name))
        self.R = restriction(self.n, seed, with_long)
        self.P = prolongation(self.n, seed + 2, sparse_rows=(kernel != "staged"))
        self.A1 = coarse_identity(N1)
        rng = np.random.RandomState(seed + 4)
        self.M = rng.uniform(-1.0, 1.0, size=(N1, N1))
        self.B8 = columns(rng, self.n)
        self.X8 = columns(rng, self.n)
        for arr in self.A[2:] + self.Ad[2:] + self.R[2:] + self.P[2:] + (self.M, self.B8, self.X8):
            arr.setflags(write=False)                 # shared by every test: nobody sorts or sums them in place

    def __repr__(self):
        return self.name


def columns(rng, n, kcols=8):
    """(n + 1, kcols): uniform values in (-1, 1) with some -0.0; column j scaled by 10 ** (3 j - 9), so that a mixed-up
    column is off by orders of magnitude; column ZERO_COLUMN all zero; row n is the guard row"""
    V = rng.uniform(-1.0, 1.0, size=(n + 1, kcols))
    V[rng.rand(n + 1, kcols) < 0.03] = -0.0
    V = V * (10.0 ** (3.0 * np.arange(kcols) - 9.0))
    V[:, ZERO_COLUMN] = 0.0
    V[n, :] = GUARD
    return np.ascontiguousarray(V)


def take(V8, cols):
    """a host array of the given columns of V8, guard row included, C-contiguous"""
    return np.ascontiguousarray(V8[:, list(cols)])


_CACHE = {}


def cases():
    """every family of square operators"""
    if "cases" not in _CACHE:
        out = [Case("short_%d" % n, short(n), "direct") for n in (1, 63, 64, 65, 127, 129, 255, 256, 257)]
        out.append(Case("short_769", short(769), "direct"))
        out.append(Case("short_staged_1100", short_staged(), "staged"))
        out.append(Case("medium", oc.medium(), "staged"))
        out.append(Case("long_staged", long_rows(8, 24, 2501), "staged", with_long=True))
        out.append(Case("long_direct", long_rows(0, 6, 2503), "direct", with_long=True))
        at, over = threshold_pair()
        out.append(Case("threshold_at", at, "direct"))
        out.append(Case("threshold_over", over, "staged"))
        out.append(Case("empty_300", oc.empty(300, 300), "direct"))       # no entries: 0 <= 12 n, and nothing to read
        _CACHE["cases"] = out
    return _CACHE["cases"]


def by_name():
    return dict((c.name, c) for c in cases())


LONG_FAMILIES = ("long_staged", "long_direct")

# the smoother settings of the smoother cycles (pre and post alike), as oracle_lib / golden_io descriptors
SMOOTHERS = [
    ("jacobi", {"name": "jacobi", "omega": 0.7, "iterations": 2}),
    ("gs_forward", {"name": "gauss_seidel", "sweep": "forward", "iterations": 2}),
    ("gs_backward", {"name": "gauss_seidel", "sweep": "backward", "iterations": 2}),
    ("gs_symmetric", {"name": "gauss_seidel", "sweep": "symmetric", "iterations": 2}),
    ("sor", {"name": "sor", "omega": 1.3, "sweep": "symmetric", "iterations": 1}),
    ("poly1", {"name": "polynomial", "coefficients": [0.6], "iterations": 1}),
    ("poly3", {"name": "polynomial", "coefficients": [0.3, -0.2, 0.45], "iterations": 2}),
]
NONE = {"name": None}


# ---------------------------------------------------------------------------------------------- shape properties
def workgroup_entries(csr, rows):
    """[(r0, r1, e0, e1)] of every workgroup of `rows` rows"""
    n, Ap = csr[0], csr[2]
    return [(r0, min(n, r0 + rows), int(Ap[r0]), int(Ap[min(n, r0 + rows)])) for r0 in range(0, n, rows)]


def straddling_rows(csr, rows, chunk=CHUNK):
    """rows that hold entries of two chunks or more of their workgroup's slice (chunks count from the slice's start)"""
    Ap = csr[2]
    out = []
    for r0, r1, e0, e1 in workgroup_entries(csr, rows):
        for i in range(r0, r1):
            s, e = int(Ap[i]), int(Ap[i + 1])
            if e > s and (s - e0) // chunk != (e - 1 - e0) // chunk:
                out.append(i)
    return out


def late_diagonal_rows(csr, rows, chunk=CHUNK):
    """rows whose last stored entry is their diagonal and lies in a chunk after the one the row starts in"""
    Ap, Aj = csr[2], csr[3]
    out = []
    for r0, r1, e0, e1 in workgroup_entries(csr, rows):
        for i in range(r0, r1):
            s, e = int(Ap[i]), int(Ap[i + 1])
            if e > s and Aj[e - 1] == i and (e - 1 - e0) // chunk > (s - e0) // chunk:
                out.append(i)
    return out


def empty_workgroups(csr, rows):
    """first rows of the FULL workgroups with e0 == e1"""
    return [r0 for r0, r1, e0, e1 in workgroup_entries(csr, rows) if e0 == e1 and r1 - r0 == rows]


def unusable_diagonal_rows(csr):
    """rows the relaxations leave alone: no stored diagonal, or the last stored one is 0.0"""
    n, _, Ap, Aj, Ax = csr
    out = []
    for i in range(n):
        d = Ax[Ap[i]:Ap[i + 1]][Aj[Ap[i]:Ap[i + 1]] == i]
        if len(d) == 0 or d[-1] == 0.0:
            out.append(i)
    return out


# ---------------------------------------------------------------------------------------------- the model
# A plain NumPy / Python model of hier_multi.hip.  Vectors are (rows, k) arrays; every operation acts on a column
# element by element, so a column's arithmetic never sees another column.  Every product and every sum is a ufunc call
# of its own (one rounding each: the library builds with -ffp-contract=off), and np.add.accumulate /
# np.subtract.accumulate run strictly left to right.
ROW_SUM, ROW_OFFDIAG, ROW_BSR1 = 0, 1, 2


def row_sum(csr, i, V, mode, b_i=None):
    """(acc, diag) of row i as csr_rows_multi / csr_rows_direct / gs_level_multi form them, in stored order.
    ROW_SUM: from 0.0, every entry's product added.  ROW_OFFDIAG: entries of column i are left out, the last one
    stored is the diagonal.  ROW_BSR1: the same, from b_i, each product passed through 0.0 + p and subtracted."""
    _, _, Ap, Aj, Ax = csr
    s, e = int(Ap[i]), int(Ap[i + 1])
    cols, vals = Aj[s:e], Ax[s:e]
    diag = 0.0
    if mode != ROW_SUM:
        on = cols == i
        if on.any():
            diag = float(vals[on][-1])
        cols, vals = cols[~on], vals[~on]
    prod = np.multiply(vals[:, None], V[cols])
    if mode == ROW_BSR1:
        loc = np.add(0.0, prod)
        return np.subtract.accumulate(np.vstack((b_i[None, :], loc)), axis=0)[-1], diag
    start = np.zeros((1, V.shape[1]))
    return np.add.accumulate(np.vstack((start, prod)), axis=0)[-1], diag


def rows_through(csr, V, mode=ROW_SUM, B=None):
    """(acc (n, k), diag (n,)) of every row"""
    n, k = csr[0], V.shape[1]
    acc, diag = np.zeros((n, k)), np.zeros(n)
    for i in range(n):
        acc[i], diag[i] = row_sum(csr, i, V, mode, None if B is None else B[i])
    return acc, diag


def epi_store(acc):                                   # EpiStore
    return acc.copy()


def epi_resid(b, acc):                                # EpiResid: b - (A v)
    return np.subtract(b, acc)


def epi_add(x, acc):                                  # EpiAdd: x + (A v)
    return np.add(x, acc)


def epi_poly0(b, acc, c0):                            # EpiPoly0: r = b - acc; h = c0 * r
    r = np.subtract(b, acc)
    return r, np.multiply(c0, r)


def epi_poly_step(r, acc, cf):                        # EpiPolyStep: h = (cf * r) + acc
    return np.add(np.multiply(cf, r), acc)


def epi_jacobi(temp, b, acc, diag, w):                # EpiJacobi: (1 - w) temp + w ((b - acc) / diag); diag == 0: left alone
    out = temp.copy()
    ok = diag != 0.0
    q = np.divide(np.subtract(b[ok], acc[ok]), diag[ok, None])
    out[ok] = np.add(np.multiply(1.0 - w, temp[ok]), np.multiply(w, q))
    return out


def epi_jacobi_bsr1(temp, acc, diag, w):              # EpiJacobiBsr1: (1 - w) temp + (w acc) / diag
    out = temp.copy()
    ok = diag != 0.0
    out[ok] = np.add(np.multiply(1.0 - w, temp[ok]), np.divide(np.multiply(w, acc[ok]), diag[ok, None]))
    return out


def gs_sweep(csr, x, b, bsr, backward):
    """one sequential Gauss-Seidel sweep in place: CSR x_i = (b_i - rsum) / diag, BSR 1 x 1 x_i = (b_i - p1 - p2 ..) / diag"""
    n = csr[0]
    for i in (range(n - 1, -1, -1) if backward else range(n)):
        acc, diag = row_sum(csr, i, x, ROW_BSR1 if bsr else ROW_OFFDIAG, b[i])
        if diag != 0.0:
            x[i] = np.divide(acc, diag) if bsr else np.divide(np.subtract(b[i], acc), diag)


def relax(csr, desc, x, b, bsr=False):
    """one application of a smoother descriptor, in place (hier_multi.hip relax<KP>)"""
    name = desc.get("name")
    if name is None or csr[0] == 0:
        return
    its = int(desc.get("iterations", 1))
    sweep = desc.get("sweep", "forward")

    def sweeps():
        if sweep != "backward":
            gs_sweep(csr, x, b, bsr, False)
        if sweep != "forward":
            gs_sweep(csr, x, b, bsr, True)
    for _ in range(its):
        if name == "gauss_seidel":
            sweeps()
        elif name == "sor":
            w = desc["omega"]
            old = x.copy()
            sweeps()
            x[:] = np.add(np.multiply(x, w), np.multiply(old, 1.0 - w))          # sor_blend_multi
        elif name == "jacobi":
            w = desc["omega"]
            temp = x.copy()
            if bsr:
                acc, diag = rows_through(csr, temp, ROW_BSR1, b)
                x[:] = epi_jacobi_bsr1(temp, acc, diag, w)
            else:
                acc, diag = rows_through(csr, temp, ROW_OFFDIAG)
                x[:] = epi_jacobi(temp, b, acc, diag, w)
        elif name == "polynomial":
            co = desc["coefficients"]
            r, h = epi_poly0(b, rows_through(csr, x)[0], co[0])
            if len(co) == 1:
                x[:] = np.add(x, h)                                              # add_to_multi
            for c, cf in enumerate(co[1:], 1):
                h = epi_poly_step(r, rows_through(csr, h)[0], cf)
                if c == len(co) - 1:
                    x[:] = np.add(x, h)
        else:
            raise KeyError(name)


def dense_apply(M, b):
    """dense_apply_multi: s = s + M[i][k] * b[k] from 0.0, k left to right"""
    s = np.zeros((M.shape[0], b.shape[1]))
    for k in range(M.shape[1]):
        s = np.add(s, np.multiply(M[:, k][:, None], b[k][None, :]))
    return s


def two_level_cycle(A, R, P, M, B, X, pre=NONE, post=NONE, bsr=False):
    """one cycle of a two-level hierarchy with a dense coarse operator on (n, k) arrays; returns the new iterate"""
    x = np.array(X, dtype=np.float64)
    b = np.asarray(B, dtype=np.float64)
    relax(A, pre, x, b, bsr)
    r = epi_resid(b, rows_through(A, x)[0])
    bc = epi_store(rows_through(R, r)[0])
    xc = dense_apply(M, bc)
    x = epi_add(x, rows_through(P, xc)[0])
    relax(A, post, x, b, bsr)
    return x


# ---------------------------------------------------------------------------------------------- the oracle
def as_scipy(csr, bsr=False):
    """the stored arrays as a scipy matrix, nothing sorted, summed or dropped; bsr: 1 x 1 blocks"""
    import scipy.sparse as sps
    n, nc, Ap, Aj, Ax = csr
    if bsr:
        return sps.bsr_matrix((Ax.reshape(-1, 1, 1).copy(), Aj.copy(), Ap.copy()), shape=(n, nc))
    return sps.csr_matrix((Ax.copy(), Aj.copy(), Ap.copy()), shape=(n, nc))


def transfer_levels(case):
    """(levels, coarse dense operator) of the smoother-free transfer cycle, for oracle_lib.Hierarchy"""
    levels = [{"A": as_scipy(case.A), "P": as_scipy(case.P), "R": as_scipy(case.R), "pre": NONE, "post": NONE},
              {"A": as_scipy(case.A1)}]
    return levels, case.M


SMOOTHER_A1 = (1, 1, np.array([0, 1], dtype=np.intc), np.zeros(1, dtype=np.intc), np.ones(1))
SMOOTHER_M = np.zeros((1, 1))


def smoother_transfers(n):
    """(R, P) with no entries for a coarse level of one unknown"""
    return oc.empty(1, n), oc.empty(n, 1)


def smoother_levels(case, desc, bsr):
    R, P = smoother_transfers(case.n)
    levels = [{"A": as_scipy(case.Ad, bsr), "P": as_scipy(P), "R": as_scipy(R), "pre": desc, "post": desc},
              {"A": as_scipy(SMOOTHER_A1)}]
    return levels, SMOOTHER_M


def oracle_cycle(levels, M, B, X):
    """one V cycle of every column through oracle_lib.Hierarchy; B, X (n, k); returns the new (n, k) iterate"""
    import oracle_lib
    H = oracle_lib.Hierarchy(levels, M)
    out = np.empty_like(X)
    for j in range(X.shape[1]):
        x = np.ascontiguousarray(X[:, j], dtype=np.float64).copy()
        b = np.ascontiguousarray(B[:, j], dtype=np.float64)
        if len(x):
            H.cycle(x, b)
        out[:, j] = x
    return out


_ORACLE = {}


def oracle_transfer(case):
    """the oracle's transfer cycle of all eight columns (computed once, shared, never written)"""
    key = (case.name, "transfer")
    if key not in _ORACLE:
        levels, M = transfer_levels(case)
        out = oracle_cycle(levels, M, case.B8[:-1], case.X8[:-1])
        out.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def oracle_smoother(case, label, bsr):
    key = (case.name, label, bool(bsr))
    if key not in _ORACLE:
        levels, M = smoother_levels(case, dict(SMOOTHERS)[label], bsr)
        out = oracle_cycle(levels, M, case.B8[:-1], case.X8[:-1])
        out.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def bit_mismatches(a, b):
    return oc.bit_mismatches(np.ravel(a), np.ravel(b))
