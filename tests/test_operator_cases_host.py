"""The operator cases of tests/operator_cases.py have the properties they are built for, and the model the device
test compares against (cpu_backend.OracleBackend on oracle/amg_oracle.c) equals a plain Python restatement of the
eight apply modes, bit for bit.  No GPU."""
import numpy as np
import pytest

import operator_cases as oc
from cpu_backend import OracleBackend
from operator_cases import (ALL_MODES, C0, GSCALE, JACOBI, JACOBI_BSR1, MATVEC, MATVEC_ACC, POLY_FIRST, POLY_LAST,
                            POLY_STEP, RESIDUAL, TILE, bit_mismatches)


def by_name(cases):
    return dict((c.name, c) for c in cases)


def all_cases():
    return oc.irregular_cases() + oc.many_blocks_cases() + [oc.coded_case()] + oc.structured_cases()


def diag_census(case):
    """rows by what they store on the diagonal: none, one or more all 0.0, the same non-zero value twice"""
    n, nc, Ap, Aj, Ax = case.csr
    none, zero, twice = [], [], []
    for i in range(n):
        d = Ax[Ap[i]:Ap[i + 1]][Aj[Ap[i]:Ap[i + 1]] == i]
        if len(d) == 0:
            none.append(i)
        elif np.all(d == 0.0):
            zero.append(i)
        if len(d) == 2 and d[0] == d[1]:
            twice.append(i)
    return none, zero, twice


# ------------------------------------------------------------------------------------------------ properties
def test_rows_per_workgroup_of_every_family():
    c = by_name(all_cases())
    for name in ("short_1", "short_255", "short_256", "short_257", "short_769_tail0", "short_769_tail3", "empty_300",
                 "empty_0", "coded"):
        assert c[name].rpb == 256, name
    assert c["medium"].rpb in (16, 32)
    assert c["rect_wide"].rpb in (16, 32) and c["rect_tall"].rpb in (16, 32)
    assert c["skewed_pair"].rpb >= 2 and c["skewed_two"].rpb == 2
    assert c["long"].rpb == 1
    for rpb in (1, 2, 32, 256):
        m = c["many_blocks_rpb%d" % rpb]
        assert m.rpb == rpb == oc.rows_per_wg_for(m.nnz, m.n, m.tile_target) and m.tile_target != 2048
    for case in all_cases():          # the value a case claims is the restated rule's, at the tile target it is created under
        assert case.rpb == oc.rows_per_wg_for(case.nnz, case.n, case.tile_target), case.name


def test_common_row_content():
    """explicit zeros, sorted odd rows and unsorted even rows, duplicated off-diagonal entries with two values, a
    diagonal stored twice with one value, rows without a diagonal, diagonals of exactly 0.0"""
    c = by_name(all_cases())
    for name in ("short_257", "short_769_tail1", "medium", "skewed_pair", "skewed_two", "long", "rect_wide",
                 "many_blocks_rpb1", "coded"):
        n, nc, Ap, Aj, Ax = c[name].csr
        frac0 = np.count_nonzero(Ax == 0.0) / float(len(Ax))
        assert 0.005 < frac0 < 0.06, (name, frac0)
        unsorted_even = dup = 0
        for i in range(n):
            cols = Aj[Ap[i]:Ap[i + 1]]
            if i % 2 == 1:
                assert np.all(np.diff(cols) >= 0), (name, i)
            elif np.any(np.diff(cols) < 0):
                unsorted_even += 1
            off = cols[cols != i]
            if len(np.unique(off)) < len(off):
                dup += 1
        assert unsorted_even > 0, name
        none, zero, twice = diag_census(c[name])
        assert dup >= 1, name
        assert len(none) >= n // 3, name
        assert len(zero) >= 1, name
        if name != "coded":
            assert len(twice) == 1, (name, twice)
    # the duplicated entries carry different values
    n, nc, Ap, Aj, Ax = c["medium"].csr
    found = False
    for i in range(5, n, 11):
        cols, vals = Aj[Ap[i]:Ap[i + 1]], Ax[Ap[i]:Ap[i + 1]]
        for col in np.unique(cols[cols != i]):
            v = vals[cols == col]
            if len(v) == 2 and v[0] != v[1]:
                found = True
    assert found


def test_short_family_shapes():
    c = by_name(oc.irregular_cases())
    for name in ("short_255", "short_256", "short_257", "short_769_tail0"):
        n, nc, Ap, Aj, Ax = c[name].csr
        L = np.diff(Ap)
        assert L[0] == 0 and L[-1] == 0 and L.max() <= 12
        assert np.all(L[60:100] == 0)
    assert sorted(c["short_769_tail%d" % r].nnz % 4 for r in range(4)) == [0, 1, 2, 3]
    for r in range(4):
        assert c["short_769_tail%d" % r].nnz % 4 == r
    assert c["short_1"].n == 1 and c["short_769_tail2"].n == 769
    # 769 rows: three full blocks and a block of one row
    assert c["short_769_tail0"].blocks() == 4


def test_medium_has_an_empty_row_block():
    for case in oc.irregular_cases():
        if case.name not in ("medium", "rect_wide", "rect_tall"):
            continue
        L = np.diff(case.csr[2])
        assert L.max() > 100 and np.all(L[100:140] == 0)
        assert 40 > case.rpb
        assert any(case.block_entries(k) == 0 for k in range(case.blocks())), case.name
    c = by_name(oc.irregular_cases())
    assert c["rect_wide"].nc > c["rect_wide"].n and c["rect_tall"].nc < c["rect_tall"].n
    assert c["rect_tall"].modes == ALL_MODES[:6] and c["rect_wide"].modes == ALL_MODES


def straddle(case):
    """(blocks over one tile, rows straddling a tile boundary of their block, rows that start in a later tile).
    Tiles of a block start at its first entry rounded down to a multiple of 4 (the 16-byte loads)."""
    n, nc, Ap, Aj, Ax = case.csr
    big, cross, later = [], [], []
    for k in range(case.blocks()):
        r0, r1 = k * case.rpb, min((k + 1) * case.rpb, n)
        origin = int(Ap[r0]) & ~3
        if int(Ap[r1]) - origin <= TILE:
            continue
        big.append(k)
        for i in range(r0, r1):
            s, e = int(Ap[i]) - origin, int(Ap[i + 1]) - origin
            if e > s and s // TILE != (e - 1) // TILE:
                cross.append(i)
            if e > s and s // TILE >= 1:
                later.append(i)
    return big, cross, later


def test_skewed_and_long_rows_cross_tiles():
    c = by_name(oc.irregular_cases())
    big, cross, later = straddle(c["skewed_pair"])
    assert c["skewed_pair"].rpb >= 2 and big == [70 // c["skewed_pair"].rpb]
    assert 71 in cross and len([i for i in later if i > 71]) >= 3       # whole rows in the second tile
    big, cross, later = straddle(c["skewed_two"])
    assert big == [8] and cross == [16] and later == [17]
    assert np.diff(c["skewed_two"].csr[2]).min() >= 300 and np.diff(c["skewed_two"].csr[2]).max() == 2500
    L = c["long"]
    assert tuple(np.diff(L.csr[2])) == oc.LONG_LENGTHS and L.nc == 7000
    big, cross, later = straddle(L)
    assert big == [5, 6, 8, 10] and cross == big          # rows 1 and 3 fill one tile at most; the rest need 2 .. 4
    n, nc, Ap, Aj, Ax = L.csr
    for i in (8, 10):                                     # a diagonal in the last tile of a multi-tile row
        assert Aj[Ap[i + 1] - 1] == i and Ax[Ap[i + 1] - 1] != 0.0
    for name, i in (("skewed_pair", 70), ("skewed_two", 16)):
        Ap2, Aj2 = c[name].csr[2], c[name].csr[3]
        assert Aj2[Ap2[i + 1] - 1] == i
    assert int(Ap[3]) % 4 == 0 and sorted(set(int(Ap[i]) % 4 for i in big)) != [0]     # aligned and unaligned origins


def test_empty_cases():
    c = by_name(oc.irregular_cases())
    assert c["empty_300"].n == 300 and c["empty_300"].nnz == 0
    assert c["empty_0"].n == 0 and c["empty_0"].nnz == 0


def test_many_blocks_remainders():
    m = oc.many_blocks_cases()[0]
    assert m.n == 3003 and m.blocks() == 3003 and np.diff(m.csr[2]).max() <= 16
    assert any(m.block_entries(k) == 0 for k in range(m.blocks()))
    for chunk in (5, 32):
        assert 3003 % (8 * chunk) != 0
        assert min(8 * chunk, 3003 % (8 * chunk)) % 8 != 0           # the last group's XCD shares are unequal
    # the restated map is a permutation of the blocks for every chunk the device test sets
    for nb in (3003, 1502, 94, 12):
        for chunk in (0, 5, 32):
            assert sorted(oc.remap_block(b, nb, chunk) for b in range(nb)) == list(range(nb)), (nb, chunk)


def test_coded_case_is_the_smallest_coded_matrix():
    case = oc.coded_case()
    assert 65536 <= case.nnz <= 70000 and case.nc >= 8192 and case.n <= case.nc
    flags = oc.coded_block_flags(case)
    half = len(flags) // 2
    assert half - 1 <= np.count_nonzero(flags) <= half + 1 and flags[0] and not flags[1]
    n, nc, Ap, Aj, Ax = case.csr
    coded_entries = sum(case.block_entries(k) for k in range(case.blocks()) if flags[k])
    assert coded_entries >= 0.3 * case.nnz                              # build_index16 keeps the codes
    # irregular enough that the offset-pattern analysis gives up (more than 255 distinct rows patterns)
    pats = set(tuple(Aj[Ap[i]:Ap[i + 1]] - i) for i in range(2000))
    assert len(pats) > 255


def test_structured_cases_fit_the_pattern_dictionary():
    for case in oc.structured_cases():
        n, nc, Ap, Aj, Ax = case.csr
        assert n >= 1024
        pats = set(tuple(Aj[Ap[i]:Ap[i + 1]] - i) for i in range(n))
        assert len(pats) <= 255 and sum(len(p) for p in pats) <= 2048, (case.name, len(pats))
        assert len(np.unique(Ax[Ax != 0.0])) == np.count_nonzero(Ax)    # every coefficient a different value
        none, zero, twice = diag_census(case)
        assert len(none) >= n // 6 and len(zero) >= 10, case.name
        full = {"grid27": 27, "grid7": 7, "line5": 5}[case.name.split("_")[0]]
        dropped = 1.0 - case.nnz / float(case.complete_nnz)
        assert 0.01 < dropped < 0.09, (case.name, dropped)
        assert np.diff(Ap).max() <= full + 1
        assert (case.nc > n) == case.name.endswith("_halo")
    for case in oc.irregular_cases() + oc.many_blocks_cases():
        n, nc, Ap, Aj, Ax = case.csr
        if n >= 1024 and n <= nc:                                       # these must stay in the CSR form
            assert len(set(tuple(Aj[Ap[i]:Ap[i + 1]] - i) for i in range(n))) > 255, case.name


def test_operands():
    for case in all_cases():
        n, nc, Ap, Aj, Ax = case.csr
        ref = np.zeros(nc + 1, dtype=bool)
        ref[Aj] = True
        assert np.all(np.isnan(case.x[:nc]) == ~ref[:nc]), case.name
        assert np.isnan(case.x[nc]) and len(case.x) == nc + 1
        for v in (case.b, case.v2, case.acc0):
            assert len(v) == n + 1 and np.isnan(v[n]) and not np.any(np.isnan(v[:n]))
            assert np.all(np.abs(v[:n]) < 1.0)
        if n >= 255:
            assert np.any(np.signbit(case.b[:n]) & (case.b[:n] == 0.0))
        if case.form == 0 and nc > 0:
            assert np.isnan(case.x[0]), case.name                       # column 0: gathered by padded quads only


# ------------------------------------------------------------------------------------------------ the model
def python_rows(csr, x, gscale, skip_diagonal, start, subtract):
    """strict left-to-right row sums in plain Python floats: separate multiply and add, the product is
    a * (gscale * x); with skip_diagonal every stored diagonal entry is left out and the last one returned as d"""
    n, nc, Ap, Aj, Ax = csr
    Ap, Aj, Ax, x = Ap.tolist(), Aj.tolist(), Ax.tolist(), x.tolist()
    sums, diag = [], []
    for i in range(n):
        s = start[i] if start is not None else 0.0
        d = 0.0
        for k in range(Ap[i], Ap[i + 1]):
            j = Aj[k]
            if skip_diagonal and j == i:
                d = Ax[k]
                continue
            p = Ax[k] * (gscale * x[j])
            s = s - p if subtract else s + p
        sums.append(s)
        diag.append(d)
    return sums, diag


def python_apply(case, mode, gscale, in_place):
    """the eight modes of include/amgcore_hip.h, written out: (out, out2) over the rows, None where not written"""
    n = case.n
    x, b, v2, acc0 = case.x, case.b.tolist(), case.v2.tolist(), case.acc0.tolist()
    if mode in (JACOBI, JACOBI_BSR1):
        old = x.tolist()                                  # the iterate: xg is v2
        if mode == JACOBI:
            s, d = python_rows(case.csr, x, 1.0, True, None, False)
            out = [old[i] if d[i] == 0.0 else (1.0 - C0) * old[i] + C0 * ((b[i] - s[i]) / d[i]) for i in range(n)]
        else:
            s, d = python_rows(case.csr, x, 1.0, True, b, True)      # starts from b and subtracts
            out = [old[i] if d[i] == 0.0 else (1.0 - C0) * old[i] + (C0 * s[i]) / d[i] for i in range(n)]
        return out, None
    s, _ = python_rows(case.csr, x, gscale, False, None, False)
    if mode == MATVEC:
        return s, None
    if mode == MATVEC_ACC:
        return [acc0[i] + s[i] for i in range(n)], None
    if mode == RESIDUAL:
        return [b[i] - s[i] for i in range(n)], None
    if mode == POLY_FIRST:
        r = [b[i] - s[i] for i in range(n)]
        return r, [C0 * r[i] for i in range(n)]
    if mode == POLY_STEP:
        return [C0 * b[i] + s[i] for i in range(n)], None
    assert mode == POLY_LAST
    return [v2[i] + (C0 * b[i] + s[i]) for i in range(n)], None


@pytest.fixture(scope="module")
def backend():
    return OracleBackend()


SMALL = [c for c in all_cases() if c.name != "coded"]


@pytest.mark.parametrize("case", SMALL, ids=repr)
def test_oracle_backend_equals_plain_python(backend, case):
    hm = backend.mat(*case.csr)
    n = case.n
    for mode in case.modes:
        for label, gscale, in_place in oc.variants(mode):
            res = oc.run_mode(backend, hm, case, mode, gscale, in_place)
            out, out2 = python_apply(case, mode, gscale, in_place)
            assert bit_mismatches(res["out"][:n], np.array(out, dtype=np.float64)) == 0, (case.name, mode, label)
            if out2 is not None:
                assert bit_mismatches(res["out2"][:n], np.array(out2, dtype=np.float64)) == 0, (case.name, mode, label)
            assert oc.check_untouched(case, res, mode, in_place) == [], (case.name, mode, label)
            assert not np.any(res["out"][:n] == oc.SENTINEL)


def test_oracle_backend_on_the_coded_case_equals_scipy(backend):
    import scipy.sparse as sp
    case = oc.coded_case()
    n, nc, Ap, Aj, Ax = case.csr
    hm = backend.mat(*case.csr)
    A = sp.csr_matrix((Ax, Aj, Ap), shape=(n, nc))
    for gscale in (1.0, GSCALE):
        xs = gscale * case.x[:nc]
        s = A * np.where(np.isnan(xs), 0.0, xs)        # unreferenced columns: scipy never reads them either
        want = {MATVEC: s, MATVEC_ACC: case.acc0[:n] + s, RESIDUAL: case.b[:n] - s}
        for mode in (MATVEC, MATVEC_ACC, RESIDUAL):
            res = oc.run_mode(backend, hm, case, mode, gscale)
            assert bit_mismatches(res["out"][:n], want[mode]) == 0, (mode, gscale)
            assert oc.check_untouched(case, res, mode) == []


@pytest.mark.parametrize("case", [c for c in SMALL if c.name in ("short_257", "medium", "long", "rect_tall", "empty_300",
                                                                 "empty_0", "line5_halo")], ids=repr)
def test_oracle_backend_apply_rows_stays_inside_the_range(backend, case):
    hm = backend.mat(*case.csr)
    for mode in case.modes:
        label, gscale, in_place = oc.variants(mode)[-1]
        full = oc.run_mode(backend, hm, case, mode, gscale, in_place)
        for lo, hi in case.row_ranges():
            res = oc.run_mode(backend, hm, case, mode, gscale, in_place, rows=(lo, hi))
            assert oc.check_untouched(case, res, mode, in_place, rows=(lo, hi)) == [], (case.name, mode, lo, hi)
            assert bit_mismatches(res["out"][lo:hi], full["out"][lo:hi]) == 0, (case.name, mode, lo, hi)
            if mode == POLY_FIRST:
                assert bit_mismatches(res["out2"][lo:hi], full["out2"][lo:hi]) == 0
