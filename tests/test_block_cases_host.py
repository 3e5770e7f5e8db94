"""The designed block cases of tests/block_cases.py, pinned on the host: the restated build_levels returns the designed
level widths, every property a case states holds (the dataflow form each is meant for among them), the C oracle equals
the plain-Python model bit for bit for all four kinds, nine sweeps stay finite, and the comparison the device tests make
is sensitive -- a row sum over the blocks in reversed order, one running sum across the blocks, a stale operand from
the neighbouring level, Dinv applied transposed, the diagonal block left in the sum, ascending rows inside a block in a
backward point sweep, or the first instead of the last stored diagonal block each change at least one bit."""
import numpy as np
import pytest

import block_cases as bc

CASES = bc.all_cases()
SMALL = [c for c in CASES if not c.vectorised]


def widths_of(level_ptr):
    return [level_ptr[l + 1] - level_ptr[l] for l in range(len(level_ptr) - 1)]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_designed_levels_and_stated_properties(case):
    level_ptr, order = case.levels()
    assert widths_of(level_ptr) == case.widths
    assert sorted(order) == list(range(case.nb))
    assert case.family == "sliced" or (case.nb <= 5000 and len(case.Ax) <= 200000)
    if case.longest is not None:
        assert case.longest_offdiag() == case.longest
    info = case.info()
    assert set(case.expect) <= set(bc.INFO_FIELDS) and case.expect
    assert {k: info[k] for k in case.expect} == case.expect
    assert info["scheduled"] == case.nb and info["bs"] == case.bs
    if info["flow"]:
        assert (info["seg"], info["lpr"]) == bc.form_for(case.longest_offdiag())
        assert info["rows_per_chunk"] == 64 // (case.bs * info["lpr"]) >= 1
        assert info["nchunks"] == len(info["chunk_slots"]) and info["slot_rows"] == sum(info["chunk_slots"])
        assert info["level_copy"] == 0 and info["slices"] == 0
    # values are non-dyadic: no stored entry but an explicit zero is a short binary fraction
    nz = case.Ax[case.Ax != 0.0][:4000]
    assert np.all(nz * 1024.0 != np.round(nz * 1024.0))
    # the last stored diagonal block dominates its scalar rows unless the case planted a zero on its diagonal
    bs, A = case.bs, case.Ax.reshape(-1, case.bs, case.bs)
    for i in range(0, case.nb, max(1, case.nb // 40)):
        blocks = range(case.Ap[i], case.Ap[i + 1])
        d = [jj for jj in blocks if case.Aj[jj] == i]
        if d and np.all(np.diag(A[d[-1]]) != 0.0):
            off = sum(np.abs(A[jj]).sum(axis=1) for jj in blocks if jj not in d) + np.abs(A[d[-1]]).sum(axis=1)
            assert np.all(2.0 * np.abs(np.diag(A[d[-1]])) > off + 0.0 * bs)


def test_families_forms_and_block_sizes_are_all_present():
    fam = {}
    for c in CASES:
        fam.setdefault(c.family, []).append(c)
    assert set(fam) == {"bflow_lpr", "bflow_grid", "bflow_gate", "stream", "sliced", "oddities"}
    for bs in (2, 3):
        got = [(c.longest, (c.info()["seg"], c.info()["lpr"]) if c.info()["flow"] else None)
               for c in fam["bflow_lpr"] if c.bs == bs]
        assert got == list(zip(bc.LPR_LONGEST, bc.LPR_FORMS))
    # all twelve instantiations of bgs_flow_kernel<BS, SEG, LPR>
    forms = {(c.bs, c.info()["seg"], c.info()["lpr"]) for c in CASES if c.info()["flow"]}
    assert forms == {(bs, seg, lpr) for bs in (2, 3) for seg, lpr in bc.FLOW_FORMS.values()}
    rpc = {(c.bs, c.info()["lpr"]): c.info()["rows_per_chunk"] for c in CASES if c.info()["flow"]}
    assert rpc == {(2, 1): 32, (2, 2): 16, (2, 3): 10, (2, 4): 8, (2, 8): 4, (2, 16): 2,
                   (3, 1): 21, (3, 2): 10, (3, 3): 7, (3, 4): 5, (3, 8): 2, (3, 16): 1}
    assert sorted(c.bs for c in fam["stream"]) == sorted(bc.STREAM_BS) == [2, 3, 4, 5, 6, 7, 16]
    assert sorted(c.bs for c in fam["sliced"]) == [2, 3] and len(fam["sliced"]) <= 2


@pytest.mark.parametrize("case", [c for c in CASES if c.family == "bflow_lpr" and c.longest > 0], ids=repr)
def test_bflow_lpr_shapes(case):
    R = case.props["R"]
    level_ptr, order = case.levels()
    cnt = case.offdiag_counts()
    assert {R - 1, R, R + 1} - {0} <= set(case.widths)
    start = np.concatenate(([0], np.cumsum(case.widths)))
    for l, p in case.props["long_rows"]:
        assert cnt[start[l] + p] == case.longest
    l0 = case.props["long_rows"][0][0]
    assert case.widths[l0] == R and case.props["long_rows"][1][0] == len(case.widths) - 2
    # the last level holds diagonal-only block rows: the form's last chunk has no slots and reads the padding slot row
    assert np.all(cnt[start[-2]:] == 0)
    info = case.info()
    if info["flow"]:
        assert info["chunk_slots"][-1] == 0
        # slot counts differ inside a level, and the per-level sort is not the identity
        lpr = info["lpr"]
        differ = unsorted = False
        for l in range(len(case.widths)):
            s = [-(-int(cnt[i]) // lpr) for i in order[level_ptr[l]:level_ptr[l + 1]]]
            differ |= len(set(s)) > 1
            unsorted |= s != sorted(s, reverse=True)
        assert differ and unsorted


def test_bflow_grid_shapes():
    grid = [c for c in CASES if c.family == "bflow_grid"]
    assert min(c.nb for c in grid) == 1
    chunks = sorted(c.info()["nchunks"] for c in grid)
    assert chunks[:4] == [1, 1, 3, 3] and {31, 32, 33} <= set(chunks)
    wide = [c for c in grid if c.info()["nchunks"] >= 144]
    assert {c.bs for c in wide} == {2, 3}
    for c in wide:
        R = c.info()["rows_per_chunk"]
        assert all((w + R - 1) // R >= 12 for w in c.widths)
        # look-ahead 50, four sweeps: max(50 * chunks per level, 32) waves, at most 4 * nchunks, cut to a multiple of 512
        nl, nch = c.info()["levels"], c.info()["nchunks"]
        nw = min(max(50 * ((nch + nl - 1) // nl), 32), 4 * nch)
        assert nw >= 512 and (nw - nw % 512) % 512 == 0


def test_bflow_gate_shapes():
    gate = [c for c in CASES if c.family == "bflow_gate"]
    for c in gate:
        lev = c.level_of()
        rows = np.repeat(np.arange(c.nb), np.diff(c.Ap))
        off = c.Aj != rows
        dist = lev[rows[off]] - lev[c.Aj[off]]              # > 0: an operand from an earlier level
        back = {}
        for i, dd in zip(rows[off], dist):
            back.setdefault(int(i), []).append(int(dd))
        kinds = set()
        for i, dd in back.items():
            e = sorted(x for x in dd if x > 0)
            kinds.add("one" if e == [1] else "two" if e and e[0] == 2 else "many" if e and e[0] >= 5 else
                      "later" if not e else "mixed")
        assert kinds == {"one", "two", "many", "later", "mixed"}, (c.name, kinds)
    R = {c.name: c.info()["rows_per_chunk"] for c in gate}
    # narrow levels (less than a chunk) and wide ones (several chunks each)
    assert any(max(c.widths) < R[c.name] for c in gate) and any(min(c.widths) > R[c.name] for c in gate)


@pytest.mark.parametrize("case", [c for c in CASES if c.family == "stream"], ids=repr)
def test_stream_shapes(case):
    bs, w = case.bs, 256 // case.bs
    T = (bc.TILE - 1) // (bs * bs)
    assert case.props["tile_blocks"] == T
    assert {w - 1, w, w + 1, 1} <= set(case.widths)
    start = np.concatenate(([0], np.cumsum(case.widths)))
    where = set()
    for l, p in case.props["long_rows"]:
        i = int(start[l] + p)
        cols = case.Aj[case.Ap[i]:case.Ap[i + 1]]
        assert len(cols) == T + 2                           # two tiles of whole blocks
        assert p == 0                                       # the first block row of its level: a workgroup's tiles start with it
        (at,) = np.nonzero(cols == i)[0]
        where.add(int(at))
    assert where == {0, T - 1, T, T + 1}                    # first in a tile, last in one, first of the second tile, last of it
    empty = case.props["empty_row"]
    assert case.Ap[empty] == case.Ap[empty + 1]
    if bs % 2:                                              # a level of the level-ordered copy starts at an odd block offset
        assert any(int(case.Ap[s]) % 2 for s in start[1:-1])
    assert not case.info()["flow"]


def test_sliced_shapes():
    for c in (k for k in CASES if k.family == "sliced"):
        assert c.nb == 1 << 15 and c.bs in (2, 3)
        n = np.diff(c.Ap)
        assert n.min() >= 4 and n.max() <= 12 and {8, 9} <= set(n.tolist())
        assert 8 // bc.BSL_PASS == 1 and -(-9 // bc.BSL_PASS) == 2
        win = c.props["window"]
        assert win == bc.BSL_WIN * (64 // c.bs) and min(c.widths) < win and len(c.widths) <= 6
        assert any(w % win for w in c.widths)               # a final partial window
        # forced level slices and the operator's own slices exist; by default the levels are too narrow for slices
        assert c.info(flow_mode=0, sell_levels=True)["slices"] == sum(-(-w // win) for w in c.widths) * bc.BSL_WIN
        assert c.info(flow_mode=0)["slices"] == 0
        assert c.info("block_jacobi")["slices"] == -(-c.nb // win) * bc.BSL_WIN
    m1 = bc.sliced_minus_one()
    assert m1.nb == (1 << 15) - 1
    assert m1.info(flow_mode=0, sell_levels=True)["slices"] == 0 and m1.info("block_jacobi")["slices"] == 0


def test_oddities_and_flat_ranges():
    odd = {c.name: c for c in CASES if c.family == "oddities"}
    names = ("plain", "descending", "duplicates", "zeros", "diag_twice", "missing_diag", "zero_in_diag", "dinv_not_inverse")
    assert set(odd) == {"odd_%s_%s" % (b, n) for b in ("short", "long") for n in names}
    for base, form in (("short", (8, 1)), ("long", (8, 4))):
        for n in names:
            c = odd["odd_%s_%s" % (base, n)]
            assert (c.info()["seg"], c.info()["lpr"]) == form, c.name
        c = odd["odd_%s_descending" % base]
        assert all(np.all(np.diff(c.Aj[c.Ap[i]:c.Ap[i + 1]]) <= 0) for i in range(c.nb))
        c = odd["odd_%s_duplicates" % base]
        assert any(len(set(c.Aj[c.Ap[i]:c.Ap[i + 1]].tolist()) - {i}) < np.count_nonzero(c.Aj[c.Ap[i]:c.Ap[i + 1]] != i) for i in range(c.nb))
        c = odd["odd_%s_zeros" % base]
        assert np.any(np.all(c.Ax.reshape(-1, c.bs * c.bs) == 0.0, axis=1))
        c = odd["odd_%s_diag_twice" % base]
        assert all(np.count_nonzero(c.Aj[c.Ap[i]:c.Ap[i + 1]] == i) == 2 for i in range(c.nb))
        c = odd["odd_%s_missing_diag" % base]
        assert sum(1 for i in range(c.nb) if not np.any(c.Aj[c.Ap[i]:c.Ap[i + 1]] == i)) == 3
        c = odd["odd_%s_zero_in_diag" % base]
        A = c.Ax.reshape(-1, c.bs, c.bs)
        assert sum(1 for jj in range(c.nblocks) if np.any(np.diag(A[jj]) == 0.0) and np.any(A[jj] != 0.0)) == 3
        # Dinv is the inverse of the last stored diagonal block -- except where the case says it is not
        for n in ("plain", "dinv_not_inverse"):
            c = odd["odd_%s_%s" % (base, n)]
            A, D = c.Ax.reshape(-1, c.bs, c.bs), c.Dinv.reshape(-1, c.bs, c.bs)
            i = 7
            last = [jj for jj in range(c.Ap[i], c.Ap[i + 1]) if c.Aj[jj] == i][-1]
            assert np.allclose(D[i] @ A[last], np.eye(c.bs), atol=1e-12) == (n == "plain")
        # a sub-range, a stride and a backward range list other block rows than all: the dataflow form declines
        c = odd["odd_%s_plain" % base]
        for nm, (lo, hi, st) in bc.flat_ranges(c.nb).items():
            tasks = list(range(lo, hi, st))
            sel = bc.selection(c, "block_gauss_seidel", 2, tasks=tasks)
            assert sel["flow"] == int(nm == "all_fwd" or nm == "all_bwd"), nm
            assert sel["scheduled"] == len(tasks)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_oracle_equals_the_plain_python_model(case):
    for kind in bc.KINDS:
        for seq in bc.SEQS[kind]:
            want = bc.model(case, kind, seq, case.x, case.b)
            got = bc.oracle(case, kind, seq, case.x, case.b)
            assert np.all(np.isfinite(want))
            assert bc.bit_mismatches(got, want) == 0, (case.name, kind, seq)


@pytest.mark.parametrize("name", ["odd_short_diag_twice", "odd_long_missing_diag", "odd_short_zero_in_diag", "bflow_lpr_bs2_17"])
def test_level_model_equals_the_plain_model(name):
    """the numpy model the sliced cases use, against the plain one where both can run -- mutations included"""
    case = next(c for c in CASES if c.name == name)
    for kind in bc.KINDS:
        for mutate in (None,) + bc.SENSITIVITY:
            if mutate is not None and kind not in bc.MUTATION_KINDS[mutate]:
                continue
            seq = bc.SEQS[kind][-1]
            a = bc.model(case, kind, seq, case.x, case.b, mutate)
            b = bc.model_by_levels(case, kind, seq, case.x, case.b, mutate)
            assert bc.bit_mismatches(a, b) == 0, (kind, mutate)


def test_sub_range_sweeps_of_the_model():
    """the model over (start, stop, step) triples, as the flat entries sweep them"""
    case = next(c for c in CASES if c.name == "odd_short_plain")
    for nm, rng3 in bc.flat_ranges(case.nb).items():
        for kind in bc.KINDS:
            if kind == "bsr_jacobi" and rng3[2] < 0:
                continue
            if kind.endswith("jacobi") and not nm.startswith("all"):
                continue                                    # (the model's temp is all of x; the oracle's only the swept rows)
            want = bc.model(case, kind, [rng3], case.x, case.b)
            assert bc.bit_mismatches(bc.oracle(case, kind, [rng3], case.x, case.b), want) == 0, (nm, kind)


def test_nine_sweeps_stay_finite():
    for case in CASES:
        for kind in bc.KINDS:
            seq = [0] * 9 if kind == "bsr_jacobi" else bc.NINE
            assert np.all(np.isfinite(bc.oracle(case, kind, seq, case.x, case.b))), (case.name, kind)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_the_comparison_is_sensitive(case):
    base = {}
    for check in bc.SENSITIVITY:
        if check in case.exempt:
            continue
        changed = 0
        for kind in bc.MUTATION_KINDS[check]:
            seq = bc.SEQS[kind][-1]
            if kind not in base:
                base[kind] = bc.model(case, kind, seq, case.x, case.b)
            changed += bc.bit_mismatches(base[kind], bc.model(case, kind, seq, case.x, case.b, mutate=check))
        assert changed > 0, check


def test_at_most_one_case_in_ten_exempts_a_check():
    for check in bc.SENSITIVITY:
        exempt = [c.name for c in CASES if check in c.exempt]
        assert 10 * len(exempt) <= len(CASES), (check, exempt)
    assert all(c.exempt <= set(bc.SENSITIVITY) for c in CASES)
