"""TEST INFRASTRUCTURE: the operand pairs that pin every route of the device sparse product (csrc/spgemm.hip matmat())
to scipy's csr_matmat, bit for bit -- tests/test_spgemm_cases_host.py on the CPU, tests/test_gpu_spgemm_routes.py on
the device.

Three things live here and none of them needs a GPU:
  * route(): a plain-Python RESTATEMENT of matmat()'s policy.  It predicts the record amg_spgemm_last_route returns:
    the lane-group width tried first, the width that produced the result, where the tables lived, table entries per
    row, workgroups, rows of the per-thread second tier.  Its constants are compared with the source text by the host
    test.
  * reference_matmat(): csr_matmat restated per row with a dict of sums and a first-touch list, multiply and add
    separate, output in reverse first-touch order, results that are == 0 dropped.
  * cases(dtype): named pairs, each the smallest shape that still reaches the code it is named for.  Every builder is
    deterministic (the seed is the case's name)."""
import functools
import zlib

import numpy as np
import scipy.sparse as sps

F64, C128 = "f64", "c128"
DTYPES = (F64, C128)
NP_DTYPE = {F64: np.float64, C128: np.complex128}
WIDTHS = {F64: (8, 16, 32, 64), C128: (16, 32, 64)}       # lane-group widths matmat() can try first

# ---- constants of csrc/spgemm.hip (test_spgemm_cases_host.py reads them from the source as text)
WAVE_CAP = {F64: 4096, C128: 2048}    # wave_cap<V>: LDS table entries per wave
ENTRY = {F64: 16, C128: 24}           # bytes of a table entry: key, place in the order list, sum
LB = 64                               # left-hand entries staged per batch and row
PD = 4                                # right-hand first chunks requested ahead of use
GRID_CAP = 256 * 2 * 8                # workgroups of the LDS launches at most
HBM_BLOCK_CAP = 1024                  # workgroups (= tables) of the HBM wave launches at most
HASH = 2654435761
LDS_PRODUCTS = 1024                   # rows of more products than this may move their table to HBM ...
HBM_WAVE_PRODUCTS = 1 << 22           # ... up to this many
TABLE_BUDGET = 4 << 30                # bytes the HBM tables of a product may take
FIRST_TIER = 256                      # per-thread tables: entries of the first tier
AMG_EINVAL = -1


# =============================================================================================== the route policy
def first_width(B, dtype):
    """lanes per output row from the right-hand operand's mean row length; complex128 one step wider"""
    avg = float(B.nnz) / float(B.shape[0]) if B.shape[0] > 0 else 1.0
    g = 8 if avg <= 10.0 else (16 if avg <= 20.0 else (32 if avg <= 40.0 else 64))
    return min(64, 2 * g) if dtype == C128 else g


def table_entries(G, dtype):
    """LDS table entries of a row that G lanes work on"""
    return WAVE_CAP[dtype] * G // 64


def slot(c, entries):
    """home slot of column c in a table of `entries` entries"""
    return ((int(c) * HASH) & 0xFFFFFFFF) & (entries - 1)


def row_products(A, B):
    """products of every output row (spgemm_upper_kernel)"""
    per_entry = np.diff(B.indptr).astype(np.int64)[A.indices]
    cs = np.concatenate([[0], np.cumsum(per_entry)])
    return cs[A.indptr[1:]] - cs[A.indptr[:-1]]


def row_distinct(A, B, i):
    cols = set()
    for j in A.indices[A.indptr[i]:A.indptr[i + 1]]:
        cols.update(B.indices[B.indptr[j]:B.indptr[j + 1]].tolist())
    return len(cols)


def row_outgrows(A, B, i, G, entries):
    """The group kernel's walk over output row i: left-hand entries in order, the right-hand row each selects in chunks
    of G.  A chunk that starts with n_ins + G > entries / 2 sends the row on -- whether or not it would have brought a
    new column."""
    seen = set()
    for j in A.indices[A.indptr[i]:A.indptr[i + 1]]:
        b0, b1 = int(B.indptr[j]), int(B.indptr[j + 1])
        for kb in range(b0, b1, G):
            if len(seen) + G > entries // 2:
                return True
            seen.update(B.indices[kb:min(kb + G, b1)].tolist())
    return False


def outgrown_rows(A, B, G, entries, products=None):
    """rows the G-lane kernel sends on.  (n_ins never exceeds the row's products, so a row of at most entries / 2 - G
    products cannot be one and is not walked.)"""
    products = row_products(A, B) if products is None else products
    return [int(i) for i in np.nonzero(products > entries // 2 - G)[0] if row_outgrows(A, B, i, G, entries)]


def table_threads(want):
    """tables of a per-thread launch: whole workgroups of 256, at least one"""
    return (max(256, want) + 255) // 256 * 256


def route(A, B, dtype):
    """(return code, route record) of matmat() for C = A * B"""
    rec = dict(complex=int(dtype == C128), lanes_first=0, lanes=0, tables="refused", entries=0, blocks=0,
               second_tier_rows=0)
    if A.shape[1] != B.shape[0]:
        return AMG_EINVAL, rec
    n = A.shape[0]
    if n == 0:
        rec["tables"] = "none"
        return 0, rec
    products = row_products(A, B)
    max_upper = int(min(products.max(), 2 ** 31 - 1))
    cap = 64
    while cap < 2 * max_upper and cap < (1 << 30):
        cap <<= 1
    G0 = first_width(B, dtype)
    rec["lanes_first"] = G0
    for G in ((G0,) if G0 == 64 else (G0, 64)):                 # the preferred width, then the whole wave per row
        entries = table_entries(G, dtype)
        if not outgrown_rows(A, B, G, entries, products):
            rec.update(lanes=G, tables="lds", entries=entries, blocks=min(-(-n // (64 // G)), GRID_CAP))
            return 0, rec
    if LDS_PRODUCTS < max_upper <= HBM_WAVE_PRODUCTS:           # whole wave per row, the row's table in HBM
        bound = min(max_upper, B.shape[1])
        gcap = 1024
        while gcap < 2 * bound + 256:
            gcap <<= 1
        assert not outgrown_rows(A, B, 64, gcap, products)      # 2 * distinct + 256 entries: no row outgrows these
        rec.update(lanes=64, tables="hbm_wave", entries=gcap,
                   blocks=max(1, min(n, HBM_BLOCK_CAP, TABLE_BUDGET // (gcap * ENTRY[dtype]))))
        return 0, rec
    # one thread per row: the guard counts both tiers as Tables::make would allocate them if every row went on
    small = min(cap, FIRST_TIER)
    t2 = min(256 * 512, (3 << 30) // (cap * ENTRY[dtype]))
    table_bytes = (table_threads(min(65536, n)) * small + table_threads(min(t2, n)) * cap) * ENTRY[dtype]
    if table_bytes > TABLE_BUDGET:
        rec["entries"] = cap
        return AMG_EINVAL, rec
    big = sum(1 for i in range(n) if products[i] > small // 2 and row_distinct(A, B, i) > small // 2)
    rec.update(lanes=1, tables="hbm_thread", entries=small, blocks=table_threads(min(65536, n)) // 256,
               second_tier_rows=big)
    return 0, rec


# =============================================================================================== the reference
def reference_matmat(A, B, dtype):
    """csr_matmat restated: (indptr int64, indices intc, data) of A * B"""
    Ap, Aj, Bp, Bj = A.indptr.tolist(), A.indices.tolist(), B.indptr.tolist(), B.indices.tolist()
    cplx = dtype == C128
    if cplx:
        Ar, Ai = A.data.real.tolist(), A.data.imag.tolist()
        Br, Bi = B.data.real.tolist(), B.data.imag.tolist()
    else:
        Ar, Br = A.data.tolist(), B.data.tolist()
    Cp, Cj, Cr, Ci = [0], [], [], []
    for i in range(A.shape[0]):
        sums, order = {}, []
        for jj in range(Ap[i], Ap[i + 1]):
            j = Aj[jj]
            for kk in range(Bp[j], Bp[j + 1]):
                c = Bj[kk]
                if c not in sums:
                    sums[c] = [0.0, 0.0]
                    order.append(c)
                s = sums[c]
                if cplx:
                    pr = Ar[jj] * Br[kk] - Ai[jj] * Bi[kk]
                    pi = Ar[jj] * Bi[kk] + Ai[jj] * Br[kk]
                    s[0] = s[0] + pr
                    s[1] = s[1] + pi
                else:
                    p = Ar[jj] * Br[kk]
                    s[0] = s[0] + p
        for c in reversed(order):
            s = sums[c]
            if s[0] != 0 or (cplx and s[1] != 0):
                Cj.append(c)
                Cr.append(s[0])
                Ci.append(s[1])
        Cp.append(len(Cj))
    if cplx:
        data = np.empty(len(Cr), dtype=np.complex128)
        data.real, data.imag = Cr, Ci                           # part by part: the sign of a zero part survives
    else:
        data = np.array(Cr, dtype=np.float64)
    return np.array(Cp, dtype=np.int64), np.array(Cj, dtype=np.intc), data


# =============================================================================================== the cases
class Case(object):
    """name, dtype, A, B (scipy CSR, stored exactly as built: unsorted, duplicates and explicit zeros kept);
    intent = (tables, lanes_first, lanes) the case is built for; props: what its name claims, checked on the CPU;
    device: False for operands outside the device entry's contract (duplicate columns in a right-hand row);
    nan: the reference holds NaNs; big: no reference is formed (the product is refused)."""

    def __init__(self, name, dtype, A, B, intent, props=None, device=True, nan=False, big=False):
        self.name, self.dtype, self.A, self.B, self.intent = name, dtype, A, B, intent
        self.props = props or {}
        self.device, self.nan, self.big = device, nan, big

    def __repr__(self):
        return "Case(%s, %s)" % (self.name, self.dtype)


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def _values(rng, n, dtype):
    v = rng.randn(n)
    return v + 1j * rng.randn(n) if dtype == C128 else v


def _csr(rows, n_col, dtype, rng, values=None):
    """CSR matrix with exactly these rows (lists of columns, kept in the given order, repeats kept)"""
    lens = [len(r) for r in rows]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.intc)
    indices = np.array([c for r in rows for c in r], dtype=np.intc)
    data = _values(rng, len(indices), dtype) if values is None else np.asarray(values, dtype=NP_DTYPE[dtype])
    assert len(data) == len(indices) and (len(indices) == 0 or (indices.min() >= 0 and indices.max() < n_col))
    return sps.csr_matrix((data, indices, indptr), shape=(len(rows), n_col))


def _distinct(rng, n_col, length):
    return rng.choice(n_col, size=length, replace=False).tolist()


def _rnd(rng, n, m, k, dtype):
    """k draws per row, duplicates summed (the operands of the older product tests)"""
    rows = np.repeat(np.arange(n), k)
    cols = rng.randint(0, m, size=n * k)
    M = sps.csr_matrix((_values(rng, n * k, dtype), (rows, cols)), shape=(n, m))
    M.sum_duplicates()
    return M


def _mean_interval(G, dtype):
    """(lo, hi, filler): right-hand mean row lengths in (lo, hi] select width G; filler lies inside"""
    g = G if dtype == F64 else G // 2
    if dtype == C128 and G == 64:
        return 20.0, np.inf, 30
    return {8: (-1.0, 10.0, 5), 16: (10.0, 20.0, 15), 32: (20.0, 40.0, 30), 64: (40.0, np.inf, 60)}[g]


def _fill_to_width(rows, n_col, G, dtype, rng):
    """append filler rows until the mean row length selects width G"""
    lo, hi, f = _mean_interval(G, dtype)
    rows = list(rows)
    for _ in range(400):
        mean = sum(len(r) for r in rows) / float(len(rows))
        if lo < mean <= hi:
            return rows
        rows.append(_distinct(rng, n_col, min(f, n_col)))
    raise AssertionError("no filler count selects width %d" % G)


def mixed_lengths(G, dtype):
    """right-hand row lengths 0, 1, G-1, G, G+1, 2G+1 and what keeps their mean selecting width G"""
    base = [0, 1, G - 1, G, G + 1, 2 * G + 1]
    if dtype == C128 and G == 16:
        return base + [1] * 6
    if dtype == C128 and G == 32:
        return base + [3] * 6
    return base


LEFT_BATCH_LENGTHS = [63, 0, 64, 0, 65, 0, 128, 129, 0, 0, 129, 64, 1, 0, 63, 65]


def _mixed_right(rng, G, dtype, n_inner):
    lens = mixed_lengths(G, dtype)
    n_col = 8 * G                       # at most 8 G distinct columns per output row: no table is outgrown
    rows = [_distinct(rng, n_col, lens[k % len(lens)]) for k in range(n_inner)]
    return _csr(rows, n_col, dtype, rng)


def _width_cases(dtype, G):
    out = []
    NG = 64 // G
    # a few hundred rows; left rows of 0 to 9 entries (the prefetch ring of 4), right rows of every length around G
    name = "mixed_%d" % G
    rng = _rng(name + dtype)
    n_inner = 4 * len(mixed_lengths(G, dtype))
    B = _mixed_right(rng, G, dtype, n_inner)
    A = _csr([_distinct(rng, n_inner, i % 10) for i in range(300)], n_inner, dtype, rng)
    out.append(Case(name, dtype, A, B, ("lds", G, G),
                    dict(left_lengths=set(range(10)), right_lengths=set([0, 1, G - 1, G, G + 1, 2 * G + 1]), rows=300)))
    # the staging batch of 64 left-hand entries: rows of 63, 64, 65, 128, 129 entries beside empty ones in one wave
    name = "batches_%d" % G
    rng = _rng(name + dtype)
    B = _mixed_right(rng, G, dtype, 160)
    A = _csr([_distinct(rng, 160, L) for L in LEFT_BATCH_LENGTHS], 160, dtype, rng)
    out.append(Case(name, dtype, A, B, ("lds", G, G),
                    dict(left_lengths=set(LEFT_BATCH_LENGTHS), rows=len(LEFT_BATCH_LENGTHS))))
    # the last, partly filled wave
    for n in sorted(set([1, NG - 1, NG + 1]) - set([0])):
        name = "rows%d_%d" % (n, G)
        rng = _rng(name + dtype)
        B = _mixed_right(rng, G, dtype, n_inner)
        A = _csr([_distinct(rng, n_inner, 1 + i % 9) for i in range(n)], n_inner, dtype, rng)
        out.append(Case(name, dtype, A, B, ("lds", G, G), dict(rows=n, blocks=-(-n // NG))))
    return out


def _boundary_parts(dtype, G, rng):
    """Right-hand rows for the overflow boundary of the G-lane table: K rows that hold disjoint blocks of r columns
    (K r = D = entries / 2 - G distinct columns in all, every row one chunk) and row K = X, which holds the new column D
    and r - 1 of the old ones."""
    entries = table_entries(G, dtype)
    r = G if dtype == F64 else G // 2               # the row length that selects width G
    D = entries // 2 - G
    K = D // r
    assert K * r == D
    rows = [rng.permutation(np.arange(k * r, (k + 1) * r)).tolist() for k in range(K)]
    rows.append([D] + list(range(1, r)))
    return rows, D + 8, K, D, r


def _boundary_cases(dtype, G):
    out = []
    name = "stay_%d" % G
    rng = _rng(name + dtype)
    rows, n_col, K, D, r = _boundary_parts(dtype, G, rng)
    B = _csr(rows, n_col, dtype, rng)
    # row 0: D distinct columns, then two chunks of repeats; row 1: the column D + 1 arrives with the last chunk
    A = _csr([list(range(K)) + [0, 1], list(range(K)) + [K], [K]], K + 1, dtype, rng)
    out.append(Case(name, dtype, A, B, ("lds", G, G), dict(distinct={0: D, 1: D + 1}, entries=table_entries(G, dtype))))
    if G < 64:
        name = "go_%d" % G
        rng = _rng(name + dtype)
        rows, n_col, K, D, r = _boundary_parts(dtype, G, rng)
        B = _csr(rows, n_col, dtype, rng)
        # row 0: D + 1 distinct columns before a further chunk (of repeats)
        A = _csr([list(range(K)) + [K, 0], [2]], K + 1, dtype, rng)
        out.append(Case(name, dtype, A, B, ("lds", G, 64),
                        dict(distinct={0: D + 1}, entries=WAVE_CAP[dtype], outgrown={G: [0]})))
    else:
        # the 64-lane LDS table against the HBM wave tables: 1030 rows, the long rows 3 and 1027 share workgroup 3 of
        # 1024 (the second one finds the table the first one cleared), every other row holds one entry
        name = "go_64_hbm"
        rng = _rng(name + dtype)
        rows, n_col, K, D, r = _boundary_parts(dtype, G, rng)
        B = _csr(rows, n_col, dtype, rng)
        long_row = list(range(K)) + [K, 0, 1]
        A = _csr([long_row if i in (3, 1027) else [i % (K + 1)] for i in range(1030)], K + 1, dtype, rng)
        out.append(Case(name, dtype, A, B, ("hbm_wave", 64, 64),
                        dict(distinct={3: D + 1, 1027: D + 1}, rows=1030, blocks=1024, outgrown={64: [3, 1027]},
                             longest=D + 3 * r)))
    return out


def _per_thread_case(dtype):
    """Rows of at most 1024 products with 961 to 1024 distinct columns beside short rows.  complex128: the wave's table
    is outgrown and no row has more than 1024 products, so one thread per row -- rows of at most 128 distinct columns in
    the 256-entry tables, the others redone in the second tier.  float64: the 64-lane table holds them all."""
    name = "long_rows"
    rng = _rng(name + dtype)
    rows = [rng.permutation(np.arange(32 * k, 32 * k + 32)).tolist() for k in range(32)]              # 0..31
    rows += [rng.permutation(np.arange(1024 + 64 * k, 1088 + 64 * k)).tolist() for k in range(16)]   # 32..47
    rows += [[1024 + 960], [1024]]                                                                   # 48 new, 49 old
    B = _csr(rows, 2048 + 8, dtype, rng)
    left = [list(range(32)),                                # 1024 products, 1024 distinct
            list(range(32, 47)) + [48, 49],                 # 962 products, 961 distinct: one too many at the last chunk
            [3, 9, 20, 31],                                 # 128 distinct: the first tier's last fit
            [3, 9, 20, 31, 5],                              # 160 distinct: second tier
            []]
    left += [_distinct(rng, 32, 1 + i % 3) for i in range(34)]
    left += [list(range(31))]                               # 992 distinct
    A = _csr(left, len(rows), dtype, rng)
    intent = ("hbm_thread", 64, 1) if dtype == C128 else ("lds", 64, 64)
    props = dict(distinct={0: 1024, 1: 961, 2: 128, 3: 160, len(left) - 1: 992}, longest=1024, rows=len(left))
    if dtype == C128:
        # (the row of 992 distinct columns alone would have stayed in LDS: its 31 chunks start with at most 960)
        props.update(second_tier_rows=4, entries=FIRST_TIER, blocks=1, outgrown={64: [0, 1]})
    return Case(name, dtype, A, B, intent, props)


def _columns_with_slot(s, entries, count, n_col=1 << 20, skip=()):
    """the first `count` columns below n_col whose home slot is s"""
    out = []
    for c in range(n_col):
        if slot(c, entries) == s and c not in skip:
            out.append(c)
            if len(out) == count:
                return out
    raise AssertionError("no %d columns with slot %d" % (count, s))


def _hash_case(dtype, G):
    """Probe chains: a right-hand row whose G columns share one home slot (every lane's atomicCAS meets the same slot in
    one step), columns whose home is one of the last two slots (the chains wrap to slot 0), a later left-hand entry that
    finds the wrapped columns again, and columns whose own home slots 0 and 1 the wrapped ones took."""
    name = "hash_%d" % G
    rng = _rng(name + dtype)
    entries = table_entries(G, dtype)
    n_col = 1 << 20
    S = _columns_with_slot(5, entries, G + 1)
    W1 = _columns_with_slot(entries - 1, entries, 3)
    W2 = _columns_with_slot(entries - 2, entries, 3)
    Z = _columns_with_slot(0, entries, 1) + _columns_with_slot(1, entries, 1)
    wrap = [W2[0], W1[0], W2[1], W1[1], W2[2], W1[2]]
    rows = [S[:G], wrap, Z + wrap[::-1], S[::-1]]
    rows = _fill_to_width(rows, 4096, G, dtype, rng)
    B = _csr(rows, n_col, dtype, rng)
    A = _csr([[0], [1, 4 % len(rows), 2], [0, 3, 1, 2, 0], [2, 1], []], len(rows), dtype, rng)
    return Case(name, dtype, A, B, ("lds", G, G),
                dict(slots={5: S, entries - 1: W1, entries - 2: W2, 0: Z[:1], 1: Z[1:]}, entries=entries))


def _value_cases(dtype):
    out = []
    G0 = WIDTHS[dtype][0]
    z = NP_DTYPE[dtype]

    def case(name, A, B, intent=("lds", G0, G0), **kw):
        out.append(Case(name, dtype, A, B, intent, **kw))
    # a column first touched by a zero product keeps its place: row 0 touches 5 (0.0 * 2), then 7 and 5 -> 7, 5
    rng = _rng("zero_first_touch" + dtype)
    B = _csr([[5], [7, 5], [2]], 9, dtype, rng, [2.0, 3.0, 4.0, 0.0])
    A = _csr([[0, 1], [0], [2, 1], [0, 2]], 3, dtype, rng, [0.0, 1.5, -0.0, 1.0, -0.0, -0.0, 7.0])
    case("zero_first_touch", A, B, props=dict(first_row=[7, 5]))
    # stored 0.0 and -0.0 in either operand
    rng = _rng("stored_zeros" + dtype)
    A = _rnd(rng, 60, 40, 4, dtype)
    A.data[::3] = z(-0.0)
    A.data[1::5] = z(0.0)
    B = _rnd(rng, 40, 30, 3, dtype)
    B.data[1::4] = z(-0.0) if dtype == F64 else complex(-0.0, 0.0)
    B.data[2::7] = z(0.0)
    case("stored_zeros", A, B, props=dict(stored_zeros=True))
    # exact cancellation: (1, -1) against equal rows
    A = sps.csr_matrix(np.array([[1.0, -1.0, 0.0], [2.0, 0.0, 1.0]], dtype=z))
    W = np.array([[3.0, 4.0], [3.0, 4.0], [0.0, 5.0]], dtype=z)
    if dtype == C128:
        W = W * (1.0 + 2.0j)
    case("cancel", A, sps.csr_matrix(W), props=dict(empty_result_rows=[0]))
    if dtype == C128:
        # one part cancels, the other does not: the result stays, its zero part as computed (scipy's complex != 0)
        W = np.array([[3.0 + 4.0j, 4.0 + 2.0j, 1.0], [3.0 + 5.0j, 5.0 + 2.0j, 1.0], [0.0, 5.0, 2.0j]])
        case("cancel_one_part", A, sps.csr_matrix(W), props=dict(one_part_zero=True))
    # inf, nan and inf * 0; inf - inf; a NaN sum is a result like any other
    rng = _rng("nonfinite" + dtype)
    j = 1j if dtype == C128 else 0.0
    B = _csr([[0, 1, 2], [1, 2, 3], [4]], 5, dtype, rng, [0.0, 2.0, -1.0 + j, 1.0, 1.0 - j, np.nan, np.inf])
    A = _csr([[0, 1], [0, 1], [0, 1], [2, 0], [2]], 3, dtype, rng,
             [np.inf, 1.0 + j, 1.0, 1.0, np.inf, -np.inf, 0.0, 3.0, -2.0 + j])
    case("nonfinite", A, B, nan=True, props=dict(nan_results=True))
    rng = _rng("shapes" + dtype)
    case("rectangular", _rnd(rng, 37, 23, 3, dtype), _rnd(rng, 23, 301, 4, dtype))
    case("no_entries_left", sps.csr_matrix((5, 7), dtype=z), _rnd(rng, 7, 3, 2, dtype))
    case("no_entries_right", _rnd(rng, 6, 7, 2, dtype), sps.csr_matrix((7, 4), dtype=z))
    case("no_rows", sps.csr_matrix((0, 7), dtype=z), _rnd(rng, 7, 3, 2, dtype), intent=("none", 0, 0))
    U = _rnd(rng, 40, 30, 6, dtype) @ _rnd(rng, 30, 35, 5, dtype)          # unsorted, as scipy's product leaves it
    case("unsorted_left", U, _rnd(rng, 35, 20, 4, dtype), props=dict(unsorted_left=True))
    # duplicate columns.  In a left-hand row they are taken one after the other like any two entries.
    rng = _rng("duplicates" + dtype)
    B = _rnd(rng, 12, 40, 5, dtype)
    A = _csr([[2, 2, 5, 2], [7], [3, 4, 3]], 12, dtype, rng)
    case("dup_left", A, B, props=dict(noncanonical="A"))
    # In a right-hand row two lanes of one chunk would add to one sum in one step: outside the device entry's contract
    rows = [_distinct(rng, 40, 5) for _ in range(12)]
    rows[4] = [9, 9, 3, 17, 3]
    case("dup_right_adjacent", _rnd(rng, 10, 12, 3, dtype), _csr(rows, 40, dtype, rng), device=False,
         props=dict(noncanonical="B"))
    rows = [_distinct(rng, 40, 5) for _ in range(12)]
    rows[4] = [9] + list(range(20, 20 + G0 + 1)) + [9, 38]                  # the two 9s lie more than G apart
    case("dup_right_far", _rnd(rng, 10, 12, 3, dtype), _csr(rows, 40, dtype, rng), device=False,
         props=dict(noncanonical="B"))
    return out


def _second_round_cases(dtype):
    out = []
    # more workgroups than the grid holds, one row per wave
    name = "second_round_64"
    rng = _rng(name + dtype)
    B = _csr([_distinct(rng, 128, int(L)) for L in rng.randint(44, 65, size=32)], 128, dtype, rng)
    A = _csr([_distinct(rng, 32, 1 + i % 2) for i in range(4100)], 32, dtype, rng)
    out.append(Case(name, dtype, A, B, ("lds", 64, 64), dict(rows=4100, blocks=GRID_CAP)))
    # and at the narrowest width: NG * 4096 + 5 rows of at most two entries
    G = WIDTHS[dtype][0]
    NG = 64 // G
    name = "second_round_%d" % G
    rng = _rng(name + dtype)
    B = _csr([_distinct(rng, 32, int(L)) for L in rng.randint(2, 7, size=16)], 32, dtype, rng)
    A = _csr([_distinct(rng, 16, i % 3) for i in range(NG * GRID_CAP + 5)], 16, dtype, rng)
    out.append(Case(name, dtype, A, B, ("lds", G, G), dict(rows=NG * GRID_CAP + 5, blocks=GRID_CAP)))
    return out


def _refusal_case(dtype):
    """One left row of 2100 entries against 2100 right-hand rows of 2048 entries over 4096 columns: 4.3 M products, past
    the gate of the HBM wave tables, so only per-thread tables of 2^24 entries are left -- 256 of them at the least.
    The memory guard refuses that on the host."""
    k = np.arange(2048, dtype=np.int64)
    indices = ((2 * k)[None, :] + (7 * np.arange(2100, dtype=np.int64))[:, None]) % 4096
    B = sps.csr_matrix((np.ones(indices.size, dtype=NP_DTYPE[dtype]), indices.ravel().astype(np.intc),
                        (2048 * np.arange(2101)).astype(np.intc)), shape=(2100, 4096))
    A = sps.csr_matrix((np.ones(2100, dtype=NP_DTYPE[dtype]), np.arange(2100, dtype=np.intc),
                        np.array([0, 2100], dtype=np.intc)), shape=(1, 2100))
    return Case("guard_refusal", dtype, A, B, ("refused", 64, 0),
                dict(longest=2100 * 2048, entries=1 << 24, rows=1, outgrown={64: [0]}), big=True)


@functools.lru_cache(maxsize=None)
def cases(dtype):
    """name -> Case, in a fixed order"""
    out = []
    for G in WIDTHS[dtype]:
        out += _width_cases(dtype, G)
        out += _boundary_cases(dtype, G)
        out.append(_hash_case(dtype, G))
    out += _second_round_cases(dtype)
    out.append(_per_thread_case(dtype))
    out += _value_cases(dtype)
    out.append(_refusal_case(dtype))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return dict((c.name, c) for c in out)


def case_ids():
    return [(dtype, name) for dtype in DTYPES for name in cases(dtype)]


@functools.lru_cache(maxsize=None)
def reference(dtype, name):
    """the restatement's product of a case, formed once and shared (read-only arrays)"""
    c = cases(dtype)[name]
    assert not c.big
    out = reference_matmat(c.A, c.B, dtype)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def predicted(dtype, name):
    c = cases(dtype)[name]
    return route(c.A, c.B, dtype)
