"""The cases of tests/spgemm_cases.py, proven on the CPU: the plain restatement of csr_matmat, scipy and the host product
agree on every pair, bit for bit; every case has the property its name claims; the model of csrc/spgemm.hip's route
policy sends every case down the route it is built for (a case that drifts off its route fails here, not silently on
the GPU); and the model's constants are the ones the source declares."""
import os
import re

import numpy as np
import pytest

import spgemm_cases as sc

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyamg_amd", "csrc", "spgemm.hip")
IDS = sc.case_ids()
SMALL = [(d, n) for d, n in IDS if not sc.cases(d)[n].big]


def _arrays64(M):
    return (np.ascontiguousarray(M.indptr, dtype=np.int64), np.ascontiguousarray(M.indices, dtype=np.intc),
            np.ascontiguousarray(M.data, dtype=np.float64))


@pytest.mark.parametrize("dtype,name", SMALL)
def test_restatement_scipy_and_host_product_agree(dtype, name):
    """row pointer and columns equal, values equal as bytes (NaNs included: all three run on this processor);
    aggregation._matmat is float64, complex pairs are held against scipy alone; duplicate columns included"""
    c = sc.cases(dtype)[name]
    Cp, Cj, Cx = sc.reference(dtype, name)
    S = c.A @ c.B
    assert S.dtype == sc.NP_DTYPE[dtype] and S.shape == (c.A.shape[0], c.B.shape[1])
    assert np.array_equal(Cp, S.indptr) and np.array_equal(Cj, S.indices)
    assert Cx.tobytes() == np.ascontiguousarray(S.data).tobytes()
    assert c.nan == bool(np.isnan(Cx.view(np.float64)).any())
    if dtype == sc.F64:
        from pyamg_amd.aggregation import _matmat
        Hp, Hj, Hx = _matmat(_arrays64(c.A), _arrays64(c.B), S.shape)
        assert np.array_equal(Hp, Cp) and np.array_equal(Hj, Cj) and Hx.tobytes() == Cx.tobytes()


def _has_repeat(M):
    return any(len(set(r)) < len(r) for r in (M.indices[M.indptr[i]:M.indptr[i + 1]].tolist() for i in range(M.shape[0])))


@pytest.mark.parametrize("dtype,name", IDS)
def test_case_has_the_property_its_name_claims(dtype, name):
    c = sc.cases(dtype)[name]
    p = c.props
    A, B = c.A, c.B
    assert A.dtype == B.dtype == sc.NP_DTYPE[dtype] and A.shape[1] == B.shape[0]
    assert A.nnz == len(A.data) and B.nnz == len(B.data)
    if c.intent[1]:
        assert sc.first_width(B, dtype) == c.intent[1]            # the mean right-hand row length selects the width
    if name not in ("dup_right_adjacent", "dup_right_far"):
        assert not _has_repeat(B) and c.device                     # the device entry's contract
    else:
        assert _has_repeat(B) and not B.has_canonical_format and not c.device
    if "rows" in p:
        assert A.shape[0] == p["rows"]
    if "left_lengths" in p:
        assert p["left_lengths"] <= set(np.diff(A.indptr).tolist())
    if "right_lengths" in p:
        assert p["right_lengths"] <= set(np.diff(B.indptr).tolist())
        # an empty right-hand row is selected by a left-hand entry, not merely stored
        assert (np.diff(B.indptr)[A.indices] == 0).any()
    for i, d in p.get("distinct", {}).items():
        assert sc.row_distinct(A, B, i) == d, i
    if "longest" in p:
        assert int(sc.row_products(A, B).max()) == p["longest"]
    for G, rows in p.get("outgrown", {}).items():
        assert sc.outgrown_rows(A, B, G, sc.table_entries(G, dtype)) == rows
    m = re.match(r"(stay|go)_(\d+)", name)
    if m:
        G = int(m.group(2))
        D = sc.table_entries(G, dtype) // 2 - G                    # what a table takes before a further chunk
        assert p["distinct"][min(p["distinct"])] == (D if m.group(1) == "stay" else D + 1)
        assert int(sc.row_products(A, B).max()) > D + 1            # ... and further chunks follow
        if m.group(1) == "stay":
            assert sc.outgrown_rows(A, B, G, sc.table_entries(G, dtype)) == [] and p["distinct"][1] == D + 1
    if name == "go_64_hbm":
        assert int(sc.row_products(A, B).max()) > sc.LDS_PRODUCTS and (1027 - 3) % sc.HBM_BLOCK_CAP == 0
    if name == "long_rows":
        assert int(sc.row_products(A, B).max()) == sc.LDS_PRODUCTS
        assert 961 <= p["distinct"][1] < p["distinct"][0] <= 1024 and p["distinct"][2] == sc.FIRST_TIER // 2
    if "slots" in p:
        for s, cols in p["slots"].items():
            assert len(set(cols)) == len(cols) and all(sc.slot(col, p["entries"]) == s for col in cols)
        G = c.intent[1]
        row0 = B.indices[B.indptr[0]:B.indptr[1]]
        assert len(row0) == G and len(set(sc.slot(col, p["entries"]) for col in row0)) == 1     # one chunk, one slot
        last = [col for s in (p["entries"] - 2, p["entries"] - 1) for col in p["slots"][s]]
        row1 = B.indices[B.indptr[1]:B.indptr[2]].tolist()
        assert sorted(row1) == sorted(last) and len(last) > 2       # more columns than slots before the wrap
        row2 = B.indices[B.indptr[2]:B.indptr[3]].tolist()
        assert set(row1) < set(row2) and A.indices[A.indptr[2]:A.indptr[3]].tolist() == [0, 3, 1, 2, 0]
        assert max(max(cols) for cols in p["slots"].values()) < (1 << 20)
    if p.get("noncanonical") == "A":
        assert _has_repeat(A) and not A.has_canonical_format
    if p.get("unsorted_left"):
        assert not A.has_sorted_indices
    if p.get("stored_zeros"):
        for M in (A, B):
            parts = M.data.view(np.float64)
            assert (parts == 0).any() and np.signbit(parts[parts == 0]).any() and not np.signbit(parts[parts == 0]).all()
    if not c.big:
        Cp, Cj, Cx = sc.reference(dtype, name)
        if "first_row" in p:
            assert Cj[Cp[0]:Cp[1]].tolist() == p["first_row"]
        for i in p.get("empty_result_rows", []):
            assert Cp[i] == Cp[i + 1] and sc.row_products(A, B)[i] > 0
        if p.get("one_part_zero"):
            assert ((Cx.real == 0) & (Cx.imag != 0)).any() and ((Cx.imag == 0) & (Cx.real != 0)).any()
            assert Cp[1] - Cp[0] == 2                           # the third column cancels in both parts and is dropped
        if p.get("nan_results"):
            assert np.isnan(Cx.view(np.float64)).any() and np.isinf(Cx.view(np.float64)).any()


@pytest.mark.parametrize("dtype,name", IDS)
def test_model_sends_the_case_down_its_route(dtype, name):
    c = sc.cases(dtype)[name]
    rc, rec = sc.predicted(dtype, name)
    assert (rec["tables"], rec["lanes_first"], rec["lanes"]) == c.intent
    assert rc == (sc.AMG_EINVAL if c.intent[0] == "refused" else 0)
    assert rec["complex"] == int(dtype == sc.C128)
    for key in ("entries", "blocks", "second_tier_rows"):
        if key in c.props:
            assert rec[key] == c.props[key], key
    if rec["tables"] == "lds":
        assert rec["entries"] == sc.table_entries(rec["lanes"], dtype)


@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_every_route_is_reached(dtype):
    """each first width on its own, each narrower width outgrown and redone by the whole wave, the HBM wave tables, the
    refusal, the product without rows; one thread per row with both tiers in complex128 -- float64 cannot reach that
    kernel at any size, which the model shows for the refusal case"""
    seen = set()
    for name in sc.cases(dtype):
        rc, rec = sc.predicted(dtype, name)
        seen.add((rec["tables"], rec["lanes_first"], rec["lanes"]))
    want = set([("none", 0, 0), ("hbm_wave", 64, 64), ("refused", 64, 0)])
    want |= set(("lds", G, G) for G in sc.WIDTHS[dtype])
    want |= set(("lds", G, 64) for G in sc.WIDTHS[dtype] if G < 64)
    if dtype == sc.C128:
        want.add(("hbm_thread", 64, 1))
        rc, rec = sc.predicted(dtype, "long_rows")
        assert 0 < rec["second_tier_rows"] < sc.cases(dtype)["long_rows"].A.shape[0]
    assert seen == want


def test_second_grid_round_and_table_reuse_are_reached():
    for dtype in sc.DTYPES:
        NG = 64 // sc.WIDTHS[dtype][0]
        for name, per_wave in (("second_round_64", 1), ("second_round_%d" % sc.WIDTHS[dtype][0], NG)):
            c = sc.cases(dtype)[name]
            assert c.A.shape[0] > per_wave * sc.GRID_CAP and int(np.diff(c.A.indptr).max()) <= 2
        assert sc.cases(dtype)["go_64_hbm"].A.shape[0] > sc.HBM_BLOCK_CAP


def test_float64_never_reaches_the_per_thread_kernel():
    """A 64-lane LDS table takes every float64 row of at most 1984 distinct columns, so a row that outgrows it has more
    than 1024 products; up to 2^22 products the HBM wave tables take it and cannot be outgrown; beyond, the second tier
    would hold 256 tables of at least 2^24 entries -- the guard's refusal, whatever the number of rows."""
    assert sc.table_entries(64, sc.F64) // 2 - 64 >= sc.LDS_PRODUCTS
    cap = 64
    while cap < 2 * (sc.HBM_WAVE_PRODUCTS + 1):
        cap <<= 1
    assert cap == 1 << 24 and sc.table_threads(1) * cap * sc.ENTRY[sc.F64] > sc.TABLE_BUDGET
    # and every product of at most 1024 products per row passes the guard (complex128: the only one to get there)
    worst = (sc.table_threads(65536) * sc.FIRST_TIER + sc.table_threads(min(256 * 512, (3 << 30) // (2048 * 24))) * 2048) * 24
    assert worst <= sc.TABLE_BUDGET


def test_model_constants_are_the_sources():
    with open(SRC) as f:
        text = f.read()
    assert re.search(r"template <class V> struct wave_cap \{ static constexpr int value = (\d+); \};", text).group(1) == \
        str(sc.WAVE_CAP[sc.F64])
    assert re.search(r"template <> struct wave_cap<c128> \{ static constexpr int value = (\d+); \};", text).group(1) == \
        str(sc.WAVE_CAP[sc.C128])
    assert re.search(r"constexpr int LB = (\d+);", text).group(1) == str(sc.LB)
    assert re.search(r"constexpr int PD = (\d+);", text).group(1) == str(sc.PD)
    assert "constexpr long ENTRY = 8 + (long)sizeof(V);" in text and sc.ENTRY == {sc.F64: 8 + 8, sc.C128: 8 + 16}
    m = re.search(r"rows_per_wave - 1\) / rows_per_wave, (\d+)L \* (\d+) \* (\d+)\);", text)
    assert int(m.group(1)) * int(m.group(2)) * int(m.group(3)) == sc.GRID_CAP == 4096
    m = re.search(r"std::min<long>\(std::min<long>\(n, (\d+)\), \((\d+)L << (\d+)\) / \(\(long\)gcap \* ENTRY\)\)", text)
    assert int(m.group(1)) == sc.HBM_BLOCK_CAP == 1024 and int(m.group(2)) << int(m.group(3)) == sc.TABLE_BUDGET
    assert "table_bytes > (double)(4L << 30)" in text
    hashes = re.findall(r"\(unsigned\)c \* (\d+)u\) & mask", text)
    assert len(hashes) == 2 and set(hashes) == set([str(sc.HASH)])           # both kernels, one hash
    assert "avgB <= 10.0 ? 8 : (avgB <= 20.0 ? 16 : (avgB <= 40.0 ? 32 : 64))" in text
    assert "CPLX ? std::min(64, 2 * G0r) : G0r" in text
    assert "if (n_ins + G > CAP / 2) bad = true;" in text
    m = re.search(r"if \(max_upper > (\d+) && max_upper <= \(1 << (\d+)\)\)", text)
    assert int(m.group(1)) == sc.LDS_PRODUCTS and 1 << int(m.group(2)) == sc.HBM_WAVE_PRODUCTS
    assert "while (gcap < 2 * distinct_bound + 256) gcap <<= 1;" in text
    assert "const int small_cap = std::min(cap, %d);" % sc.FIRST_TIER in text
    assert "std::min<long>(256L * 512L, (3L << 30) / ((long)cap * ENTRY))" in text
    assert "return (std::max<long>(256, want) + 255) / 256 * 256;" in text
    assert "T1.cap / 2" in text and "T2.cap / 2" in text                    # a tier takes half its entries


def test_callers_keep_operators_with_duplicate_columns_off_the_device():
    """aggregation._columns_once is what the Galerkin call sites ask before they hand an operator over (sorted rows:
    scipy's own check; unsorted rows: the pattern sorted in a copy; BSR(1,1) alike), and the strength measure's device
    pipeline -- whose squarings use the same product -- declines such an operator before it touches the library"""
    import scipy.sparse as sps
    from pyamg_amd import aggregation, strength
    for dtype in sc.DTYPES:
        cs = sc.cases(dtype)
        for name in ("dup_right_adjacent", "dup_right_far"):
            assert not aggregation._columns_once(cs[name].B)             # unsorted rows, neighbours or far apart
            S = cs[name].B.copy()
            S.sort_indices()
            assert S.has_sorted_indices and not aggregation._columns_once(S)
        U = cs["unsorted_left"].A
        assert not U.has_sorted_indices and aggregation._columns_once(U)
        before = (U.indptr.tobytes(), U.indices.tobytes(), U.data.tobytes())
        assert aggregation._columns_once(U) and before == (U.indptr.tobytes(), U.indices.tobytes(), U.data.tobytes())
        assert aggregation._columns_once(cs["mixed_%d" % sc.WIDTHS[dtype][0]].B)
    D = sps.csr_matrix((np.array([2.0, 1.0, -1.0, 3.0]), np.array([0, 0, 1, 1], dtype=np.intc),
                        np.array([0, 3, 4], dtype=np.intc)), shape=(2, 2))
    assert not aggregation._columns_once(D)
    assert not aggregation._columns_once(sps.bsr_matrix((D.data.reshape(-1, 1, 1), D.indices, D.indptr), shape=(2, 2)))
    D._amg_columns_once = True              # (what the package's own products say of themselves is taken at its word)
    assert aggregation._columns_once(D)
    del D._amg_columns_once
    assert strength._device_measure(D, np.ones(2), 1.0, 4.0, 4, True) is None


def test_reference_restatement_on_a_product_worked_by_hand():
    """[[0 a, 1 b]] * [[5: 2], [7: 3, 5: 4]] with a = 0: column 5 is touched first, by a zero product, then 7, then 5
    again -> out in reverse first-touch order 7, 5; the other rows hold products of stored zeros only and come out empty"""
    Cp, Cj, Cx = sc.reference(sc.F64, "zero_first_touch")
    assert Cp.tolist() == [0, 2, 2, 2, 2]
    assert Cj.tolist() == [7, 5]
    assert Cx.tolist() == [1.5 * 3.0, 0.0 * 2.0 + 1.5 * 4.0]
