"""TEST INFRASTRUCTURE: the operators and operands that pin every apply mode of every operator kernel form
(tests/test_operator_cases_host.py on the CPU, tests/test_gpu_operator_modes.py on the device).

Every builder is deterministic (fixed seeds) and returns (nrows, ncols, Ap, Aj, Ax) as intc / intc / float64.  The
shapes are the smallest at which the kernels' indexing can go wrong: rows longer than one LDS tile, row blocks that
span two tiles, empty row blocks, entry counts that leave a scalar tail behind the 16-byte loads, more row blocks than
the persistent grid, block counts that leave remainders in the block -> XCD map, missing / zero / doubled diagonals.
Nothing here needs a GPU."""
import numpy as np

from pyamg_amd.distributed import (JACOBI, JACOBI_BSR1, MATVEC, MATVEC_ACC, POLY_FIRST, POLY_LAST, POLY_STEP,
                                   RESIDUAL)

WG = 256                 # kernels.hip: threads = rows per workgroup at most
TILE = 2048              # kernels.hip: products staged in LDS per pass
ALL_MODES = (MATVEC, MATVEC_ACC, RESIDUAL, POLY_FIRST, POLY_STEP, POLY_LAST, JACOBI, JACOBI_BSR1)
NON_JACOBI = ALL_MODES[:6]
SENTINEL = -8.765e201    # pre-fill of every output: a finite value no case computes
C0 = 0.7                 # coefficient / omega of the modes that take one
GSCALE = 0.375           # the on-the-fly operand scaling modes 0..5 also run with


def rows_per_wg_for(nnz, rows, tile_target=2048):
    """RESTATEMENT of kernels.hip rows_per_wg_for (kept in step by test_operator_cases_host and, on the device, by the
    coded case, whose codes exist only for the row blocking the library chose): the largest power of two
    <= tile_target / max(average row length, 1), at most 256; 256 for an empty matrix."""
    if rows <= 0 or nnz <= 0:
        return WG
    avg = float(nnz) / float(rows)
    r = int(tile_target / (avg if avg > 1.0 else 1.0))
    p = 1
    while p * 2 <= r and p < WG:
        p *= 2
    return p


def remap_block(b, nb, chunk):
    """RESTATEMENT of kernels.hip remap_block (logical block -> row block), for the host test's remainder claims."""
    if chunk <= 0:
        return b
    gsz = 8 * chunk
    base = (b // gsz) * gsz
    n_g = min(gsz, nb - base)
    l = b - base
    xcd, j = l & 7, l >> 3
    q, r = n_g >> 3, n_g & 7
    return base + xcd * q + min(xcd, r) + j


# ---------------------------------------------------------------------------------------------- irregular rows
def irregular(seed, nrows, ncols, lengths):
    """Rows of the given lengths with the content every irregular family shares:
    about 2 % explicit zero values; odd rows sorted by column, even rows left in drawn order; every third row (i % 3
    == 0) stores no diagonal; rows with i % 17 == 1 store a diagonal of exactly 0.0; rows with i % 11 == 5 store one
    off-diagonal column twice with different values; the first row with i % 3 == 2 and four entries or more stores
    its diagonal twice with the same value; an even row of more than 1024 entries stores its diagonal last (in a
    tile after the first when the row spans several: the Jacobi modes must drop that product there too).  Column 0 is referenced by nobody (row 0 stores no diagonal), so that
    x[0] can carry a NaN: the kernels' padded quads gather it."""
    rng = np.random.RandomState(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    assert len(lengths) == nrows and (lengths.max() if nrows else 0) < ncols - 1
    Ap = np.zeros(nrows + 1, dtype=np.intc)
    Ap[1:] = np.cumsum(lengths)
    Aj = np.zeros(int(Ap[-1]), dtype=np.intc)
    Ax = np.zeros(int(Ap[-1]), dtype=np.float64)
    twice = True
    for i in range(nrows):
        L = int(lengths[i])
        if L == 0:
            continue
        diag = (i % 3 != 0) and i < ncols
        ndiag = 0
        if diag:
            ndiag = 1
            if twice and i % 3 == 2 and L >= 4:
                ndiag, twice = 2, False
        noff = L - ndiag
        # off-diagonal columns: distinct, never 0, never i
        if noff * 4 > ncols:
            pool = rng.permutation(np.arange(1, ncols))
            pool = pool[pool != i][:noff]
        else:
            pool = np.zeros(0, dtype=np.int64)
            while len(pool) < noff:
                extra = rng.randint(1, ncols, size=2 * noff + 4)
                pool = np.concatenate((pool, extra[extra != i]))
                _, first = np.unique(pool, return_index=True)
                pool = pool[np.sort(first)]
            pool = pool[:noff]
        cols = np.asarray(pool, dtype=np.int64)
        if i % 11 == 5 and noff >= 3:
            cols[1] = cols[0]                                   # a duplicated off-diagonal entry, two values
        vals = rng.uniform(-1.0, 1.0, size=L)
        vals[rng.rand(L) < 0.02] = 0.0
        if diag:
            cols = np.concatenate((cols, [i] * ndiag))
            order = rng.permutation(L)
            cols = cols[order]
            dpos = np.nonzero(cols == i)[0]
            vals[dpos] = 0.0 if i % 17 == 1 else (0.5 + rng.rand()) * (1.0 if i % 2 else -1.0)
            if i % 2 == 0 and L > TILE // 2:
                cols[[dpos[-1], L - 1]] = cols[[L - 1, dpos[-1]]]      # a long unsorted row: the diagonal comes last,
                vals[[dpos[-1], L - 1]] = vals[[L - 1, dpos[-1]]]      # in the row's last tile
        if i % 2 == 1:
            order = np.argsort(cols, kind="stable")
            cols, vals = cols[order], vals[order]
        Aj[Ap[i]:Ap[i + 1]] = cols
        Ax[Ap[i]:Ap[i + 1]] = vals
    return nrows, ncols, Ap, Aj, Ax


def short(n, residue=None):
    """rpb 256: row lengths 0..12, a run of 40 empty rows, empty first and last rows.  residue (n = 769): the last
    stored row is trimmed until nnz % 4 == residue (the scalar tail behind the 16-byte loads)."""
    rng = np.random.RandomState(1000 + n)
    lengths = rng.randint(0, 13, size=n)
    lengths[0] = lengths[-1] = 0
    if n > 120:
        lengths[60:100] = 0
    if residue is not None:
        last = n - 2
        lengths[last] = 12
        lengths[last] -= (int(lengths.sum()) - residue) % 4
    return irregular(11 + n, n, max(n, 16), lengths)


def medium(nrows=300, ncols=300, seed=21):
    """rpb 16 or 32: lengths 0..200, rows 100..139 empty (more than one row block)."""
    rng = np.random.RandomState(seed)
    lengths = rng.randint(0, 201, size=nrows)
    lengths[100:140] = 0
    lengths = np.minimum(lengths, ncols - 2)
    return irregular(seed + 1, nrows, ncols, lengths)


def skewed_pair():
    """rpb 64: short rows, and rows 70 and 71 of ~1500 entries side by side in the block of rows 64..127: row 71
    straddles the block's tile boundary and rows 72.. lie wholly in its second tile."""
    rng = np.random.RandomState(31)
    lengths = rng.randint(0, 7, size=200)
    lengths[70], lengths[71] = 1500, 1490
    return irregular(32, 200, 2000, lengths)


def skewed_two():
    """rpb 2: lengths 300..900 and one row of 2500."""
    rng = np.random.RandomState(33)
    lengths = rng.randint(300, 901, size=40)
    lengths[16] = 2500            # row 17 then lies wholly in the block's second tile
    return irregular(34, 40, 3000, lengths)


LONG_LENGTHS = (0, 2047, 1, 2048, 0, 2049, 4100, 3, 6145, 0, 4096, 5)


def long_rows():
    """rpb 1: one tile exactly, one entry over, three tiles."""
    return irregular(41, len(LONG_LENGTHS), 7000, LONG_LENGTHS)


def empty(nrows, ncols):
    return nrows, ncols, np.zeros(nrows + 1, dtype=np.intc), np.zeros(0, dtype=np.intc), np.zeros(0, dtype=np.float64)


def many_blocks():
    """3003 rows of 0..16 entries: created with rows-per-workgroup 1 it has more row blocks than the persistent grid,
    and 3003 leaves a remainder modulo 8 * chunk and modulo 8."""
    rng = np.random.RandomState(51)
    lengths = rng.randint(0, 17, size=3003)
    return irregular(52, 3003, 3003, lengths)


def tile_target_for(csr, rpb):
    """an amg_set_tile_target value under which rows_per_wg_for gives `rpb` for this matrix"""
    n, nnz = csr[0], int(csr[2][-1])
    avg = max(float(nnz) / n, 1.0)
    t = int(np.ceil(avg * rpb)) + 1
    assert rows_per_wg_for(nnz, n, t) == rpb, (t, rpb)
    return t


CODED_ROWS, CODED_COLS, CODED_LEN = 8300, 80000, 8


def coded():
    """The smallest matrix build_index16 accepts (nnz >= 65536, ncols >= 8192), rpb 256.  Even row blocks are banded
    (their columns fit 16 windows of 4096), odd ones scatter over all 20 windows and keep plain indices.  Same row
    content rules as irregular()."""
    rng = np.random.RandomState(61)
    n, nc, L = CODED_ROWS, CODED_COLS, CODED_LEN
    Ap = (np.arange(n + 1) * L).astype(np.intc)
    Aj = np.zeros(n * L, dtype=np.intc)
    Ax = rng.uniform(-1.0, 1.0, size=n * L)
    Ax[rng.rand(n * L) < 0.02] = 0.0
    for i in range(n):
        diag = i % 3 != 0
        noff = L - (1 if diag else 0)
        if (i // WG) % 2 == 0:
            centre = 3000 + int(i * ((nc - 6000.0) / n))
            lo, hi = centre - 2500, centre + 2500
        else:
            lo, hi = 1, nc
        cols = np.zeros(0, dtype=np.int64)
        while len(cols) < noff:
            extra = rng.randint(lo, hi, size=2 * noff)
            cols = np.concatenate((cols, extra[extra != i]))
            _, first = np.unique(cols, return_index=True)
            cols = cols[np.sort(first)]
        cols = cols[:noff]
        if i % 11 == 5:
            cols[1] = cols[0]
        if diag:
            cols = np.concatenate((cols, [i]))[rng.permutation(L)]
            k = Ap[i] + int(np.nonzero(cols == i)[0][0])
            Ax[k] = 0.0 if i % 17 == 1 else 0.5 + rng.rand()
        if i % 2 == 1:
            order = np.argsort(cols, kind="stable")
            cols = cols[order]
            Ax[Ap[i]:Ap[i + 1]] = Ax[Ap[i]:Ap[i + 1]][order]
        Aj[Ap[i]:Ap[i + 1]] = cols
    return n, nc, Ap, Aj, Ax


# ---------------------------------------------------------------------------------------------- structured grids
def structured(dims, reach, halo, seed, drop_entries=True):
    """A stencil operator on a grid (the last axis runs fastest): offsets within `reach` along every axis (reach 1 on
    all three axes: 27 points; `reach` may also be the string "star": 7 points), every coefficient a different value,
    rows sorted.  Two in five rows lose one entry: rows with i % 5 == 1 their diagonal, rows with i % 5 == 2 one of
    three other offsets in turn -- 2 .. 8 % of the entries, chosen by the row number so that the rows keep few
    distinct offset patterns (the pattern dictionary holds 255 patterns and 2048 offsets) and the slots of the
    stencil form stay at least 80 % full (try_stencil's acceptance rule).  Rows with i % 17 == 1 that keep their
    diagonal store exactly 0.0 there.  halo: rows 0..23 and 50..59 also reference one column >= nrows each
    ([owned | halo], a rank's local operator); the stencil form leaves rows 0..59 to the pattern kernel."""
    rng = np.random.RandomState(seed)
    dims = tuple(dims)
    n = int(np.prod(dims))
    nd = len(dims)
    strides = [int(np.prod(dims[a + 1:])) for a in range(nd)]
    if reach == "star":
        offs = [tuple(0 for _ in range(nd))]
        for a in range(nd):
            for s in (-1, 1):
                offs.append(tuple(s if k == a else 0 for k in range(nd)))
    else:
        offs = [()]
        for a in range(nd):
            offs = [o + (d,) for o in offs for d in range(-reach[a], reach[a] + 1)]
    offs.sort(key=lambda o: sum(o[a] * strides[a] for a in range(nd)))
    lin = [sum(o[a] * strides[a] for a in range(nd)) for o in offs]
    dropped = [lin.index(0)] + [k for k in (1, len(offs) // 2 + 1, len(offs) - 2, len(offs) // 3) if lin[k] != 0][:3]
    coords = np.array(np.unravel_index(np.arange(n), dims)).T
    ncols = n + (24 if halo else 0)
    Ap, Aj, Ax = [0], [], []
    for i in range(n):
        drop = dropped[0] if i % 5 == 1 else (dropped[1 + (i // 5) % 3] if i % 5 == 2 else -1)
        if not drop_entries:
            drop = -1
        for k, o in enumerate(offs):
            if k == drop:
                continue
            c = coords[i] + np.array(o)
            if np.all(c >= 0) and np.all(c < np.array(dims)):
                Aj.append(i + lin[k])
                Ax.append(0.0 if (lin[k] == 0 and i % 17 == 1) else rng.uniform(-1.0, 1.0))
        if halo and i < 24:
            Aj.append(n + i)
            Ax.append(rng.uniform(-1.0, 1.0))
        elif halo and 50 <= i < 60:
            Aj.append(n + i - 50)
            Ax.append(rng.uniform(-1.0, 1.0))
        Ap.append(len(Aj))
    return n, ncols, np.array(Ap, dtype=np.intc), np.array(Aj, dtype=np.intc), np.array(Ax, dtype=np.float64)


# ---------------------------------------------------------------------------------------------- cases
class Case(object):
    """One operator with its operands.  x (ncols + 1), b, v2, acc0 (nrows + 1): uniform in (-1, 1) with some -0.0;
    x holds a NaN at every column no entry references; each array ends with a NaN guard one past its end (the
    kernels must neither read it into a result nor write it).  acc0 is what MATVEC_ACC accumulates into."""

    def __init__(self, name, csr, rpb=None, tile_target=2048, modes=None, form=0):
        self.name = name
        self.csr = csr
        self.n, self.nc = csr[0], csr[1]
        self.nnz = int(csr[2][-1])
        self.tile_target = tile_target
        self.rpb = rows_per_wg_for(self.nnz, self.n, tile_target) if rpb is None else rpb
        self.modes = modes if modes is not None else (ALL_MODES if self.nc >= self.n else NON_JACOBI)
        self.form = form                      # amg_mat_form with every switch at its default
        rng = np.random.RandomState(sum(map(ord, name)) + 7 * self.n)

        def vec(m):
            v = rng.uniform(-1.0, 1.0, size=m + 1)
            v[rng.rand(m + 1) < 0.03] = -0.0
            v[m] = np.nan
            return v
        self.x = vec(self.nc)
        ref = np.zeros(self.nc + 1, dtype=bool)
        ref[csr[3]] = True
        ref[self.nc] = True
        self.unreferenced = np.nonzero(~ref)[0]
        self.x[self.unreferenced] = np.nan
        self.b = vec(self.n)
        self.v2 = vec(self.n)
        self.acc0 = vec(self.n)

    def __repr__(self):
        return self.name

    def blocks(self):
        return (self.n + self.rpb - 1) // self.rpb

    def block_entries(self, blk):
        Ap = self.csr[2]
        r0 = blk * self.rpb
        return int(Ap[min(r0 + self.rpb, self.n)] - Ap[r0])

    def row_ranges(self):
        """[0,0), [0,1), [n-1,n), [1,n) and a range whose two ends lie inside row blocks"""
        n, rpb = self.n, self.rpb
        if n == 0:
            return [(0, 0)]
        out = [(0, 0), (0, 1), (n - 1, n), (1, n)]
        lo = rpb + rpb // 2 if n > 2 * rpb else n // 3
        hi = n - 1 - (rpb // 3 if n > 3 * rpb else 0)
        if rpb == 1:
            lo, hi = min(2, n - 1), n - 2
        if hi > lo:
            out.append((lo, hi))
        return out


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def irregular_cases():
    """every irregular family except the coded one and the many-blocks re-blockings"""
    def make():
        cases = [Case("short_%d" % n, short(n)) for n in (1, 255, 256, 257)]
        cases += [Case("short_769_tail%d" % r, short(769, r)) for r in range(4)]
        cases.append(Case("medium", medium()))
        cases.append(Case("skewed_pair", skewed_pair()))
        cases.append(Case("skewed_two", skewed_two()))
        cases.append(Case("long", long_rows()))
        cases.append(Case("empty_300", empty(300, 300)))
        cases.append(Case("empty_0", empty(0, 5)))
        cases.append(Case("rect_wide", medium(150, 420, 71)))
        cases.append(Case("rect_tall", medium(300, 120, 73)))
        return cases
    return _cached("irregular", make)


def many_blocks_cases():
    """the many-blocks matrix under the four row blockings (the first is the one with more blocks than the grid)"""
    def make():
        csr = many_blocks()
        return [Case("many_blocks_rpb%d" % rpb, csr, rpb=rpb, tile_target=tile_target_for(csr, rpb))
                for rpb in (1, 2, 32, 256)]
    return _cached("many", make)


def coded_case():
    return _cached("coded", lambda: Case("coded", coded()))


def coded_block_flags(case):
    """which row blocks of the coded case fit 16 windows of 4096 columns (index16_build_kernel's rule)"""
    n, _, Ap, Aj, _ = case.csr
    flags = []
    for r0 in range(0, n, case.rpb):
        cols = Aj[Ap[r0]:Ap[min(r0 + case.rpb, n)]]
        flags.append(len(np.unique(cols >> 12)) <= 16)
    return np.array(flags)


def structured_cases():
    """form 2 (stencil) unless said otherwise.  The 27-point operator on the 33 x 7 x 5 grid stays in the
    offset-pattern form (1): its boundary rows leave the slots of a 27-offset stencil less than 80 % full, which
    try_stencil refuses, so the same operator is also built with the 7-point star, which it accepts."""
    def make():
        cases = []
        for halo in (False, True):
            h = "_halo" if halo else ""
            for name, dims, reach, seed, form in (("grid27", (33, 7, 5), (1, 1, 1), 81, 1), ("grid7", (33, 7, 5), "star", 82, 2),
                                                  ("line5", (1200,), (2,), 83, 2)):
                case = Case(name + h, structured(dims, reach, halo, seed), form=form)
                case.complete_nnz = int(structured(dims, reach, halo, seed, drop_entries=False)[2][-1])
                cases.append(case)
        return cases
    return _cached("structured", make)


# ---------------------------------------------------------------------------------------------- running a mode
def variants(mode):
    """(label, gscale, in_place) a mode runs with: modes 0..5 plain and with the operand scaling; POLY_LAST also
    writes over v2 (x += h); the Jacobi modes gather the iterate they relax (xg is v2)"""
    if mode in (JACOBI, JACOBI_BSR1):
        return [("xg_is_v2", 1.0, False)]
    out = [("plain", 1.0, False), ("gscale", GSCALE, False)]
    if mode == POLY_LAST:
        out.append(("gscale_inplace", GSCALE, True))
    return out


def run_mode(be, hm, case, mode, gscale=1.0, in_place=False, rows=None, call=None):
    """One application through a backend (HipBackend or OracleBackend: same signatures).  Returns every array the
    launch could have touched, as host arrays including the guard entry: out, out2, x, b, v2."""
    import torch
    n = case.n
    like = be.vec(1)

    def put(a):
        return torch.from_numpy(np.array(a, dtype=np.float64)).to(like.device)

    def fresh():
        v = np.full(n + 1, SENTINEL)
        v[n] = np.nan
        return v
    x, b, v2 = put(case.x), put(case.b), put(case.v2)
    out = put(case.acc0 if mode == MATVEC_ACC else fresh())
    out2 = put(fresh())
    xg = x
    if mode in (JACOBI, JACOBI_BSR1):
        v2 = x                                  # the iterate: gathered and relaxed
    if in_place:
        out = v2
    args = (xg, b, v2, out, out2, C0, gscale)
    if call is not None:
        rc = call(hm, mode, args)
    elif rows is None:
        rc = be.apply(hm, mode, *args)
    else:
        rc = be.apply_rows(hm, mode, rows[0], rows[1], *args)
    be.synchronize()
    res = {"out": out, "out2": out2, "x": x, "b": b, "v2": v2}
    res = dict((k, v.cpu().numpy().copy()) for k, v in res.items())
    res["rc"] = rc
    return res


def untouched(case, mode, in_place=False, rows=None):
    """what every array holds where the launch must not write: name -> (expected array, mask of those entries)"""
    n = case.n
    lo, hi = (0, n) if rows is None else rows
    outside = np.ones(n + 1, dtype=bool)
    outside[lo:hi] = False
    allx = np.ones(case.nc + 1, dtype=bool)
    alln = np.ones(n + 1, dtype=bool)
    sent = np.full(n + 1, SENTINEL)
    sent[n] = np.nan
    exp = {"x": (case.x, allx), "b": (case.b, alln)}
    exp["v2"] = (case.x, allx) if mode in (JACOBI, JACOBI_BSR1) else (case.v2, outside if in_place else alln)
    exp["out2"] = (sent, outside if mode == POLY_FIRST else alln)
    if in_place:
        exp["out"] = (case.v2, outside)
    else:
        exp["out"] = (case.acc0 if mode == MATVEC_ACC else sent, outside)
    return exp


def bit_mismatches(a, b):
    """entries whose bits differ, so that -0.0 is not +0.0; a NaN matches any NaN (vector_models.bit_mismatches)"""
    a = np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64)
    b = np.ascontiguousarray(np.atleast_1d(b), dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int(np.count_nonzero((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))))


def check_untouched(case, res, mode, in_place=False, rows=None):
    """names of the arrays that changed where the launch must not write (guard entries included)"""
    bad = []
    for name, (want, mask) in untouched(case, mode, in_place, rows).items():
        got = res[name]
        if got.shape != want.shape or bit_mismatches(got[mask], want[mask]):
            bad.append(name)
    return bad
