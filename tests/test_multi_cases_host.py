"""The multi-RHS cases of tests/multi_cases.py have the shapes they are built for, the inputs are a fair test, and the
plain NumPy model of hier_multi.hip equals the oracle (oracle_lib.Hierarchy on oracle/amg_oracle.c) bit for bit on
every family and every smoother setting tests/test_gpu_multi_forms.py runs.  No GPU."""
import ctypes
import math

import numpy as np
import pytest

import multi_cases as mc
import oracle_lib
import vector_models as vm
from multi_cases import CHUNK, DIRECT_MAX_ROW, ROWS, WIDTHS

CASES = mc.cases()
NAMES = [c.name for c in CASES]
C = mc.by_name()
LABELS = [label for label, _ in mc.SMOOTHERS]


def model_columns(case):
    """the long families run the Python model on three columns (the smallest, the zero one, the largest): the model
    is per column, and all eight would take minutes"""
    return [0, mc.ZERO_COLUMN, 7] if case.name in mc.LONG_FAMILIES else list(range(8))


# ------------------------------------------------------------------------------------------------ shapes
def test_restated_constants():
    assert ROWS == {1: 256, 2: 256, 4: 128, 8: 64} and CHUNK == 2048 and DIRECT_MAX_ROW == 12
    assert [mc.width_of(k) for k in range(1, 9)] == [1, 2, 4, 4, 8, 8, 8, 8]
    assert NAMES == ["short_%d" % n for n in (1, 63, 64, 65, 127, 129, 255, 256, 257)] + [
        "short_769", "short_staged_1100", "medium", "long_staged", "long_direct", "threshold_at", "threshold_over",
        "empty_300"]


@pytest.mark.parametrize("name", NAMES)
def test_family_is_on_the_stated_side_of_the_rule(name):
    case = C[name]
    n, nc, Ap, Aj, Ax = case.A
    assert n == nc == case.n and len(Ap) == n + 1 and Ap[0] == 0 and Ap[-1] == len(Aj) == len(Ax) == case.nnz
    assert Ap.dtype == np.intc and Aj.dtype == np.intc and Ax.dtype == np.float64
    assert mc.kernel_of(case.A) == case.kernel == mc.kernel_of(case.Ad)
    assert (case.nnz <= DIRECT_MAX_ROW * n) == (case.kernel == "direct")
    if case.nnz:
        assert Aj.min() >= 0 and Aj.max() < n


def test_threshold_pair_sits_on_the_rule():
    at, over = C["threshold_at"], C["threshold_over"]
    assert at.nnz == DIRECT_MAX_ROW * at.n and over.nnz == at.nnz + 1 and over.n == at.n
    assert np.array_equal(over.A[3][:-1], at.A[3]) and np.array_equal(over.A[4][:-1], at.A[4])
    assert np.array_equal(over.A[2][:-1], at.A[2][:-1])


def test_short_families():
    for n in (63, 64, 65, 127, 129, 255, 256, 257, 769):
        L = np.diff(C["short_%d" % n].A[2])
        assert len(L) == n and 10 <= L.max() <= 12 and L[0] == 0 and L[-1] == 0
    assert C["short_1"].nnz == 1
    # one below, at and one above a multiple of ROWS for every width
    have = set(c.n for c in CASES)
    for rows in set(ROWS.values()):
        assert any({m - 1, m, m + 1} <= have for m in range(rows, 1024, rows)), rows
    assert {63, 64, 65} <= have and {127, 129} <= have
    assert 769 % 256 == 1 and 769 % 128 == 1 and 769 % 64 == 1


def test_long_rows_reach_both_kernels():
    for name, kernel in (("long_staged", "staged"), ("long_direct", "direct")):
        L = np.diff(C[name].A[2])
        assert tuple(L[:12]) == mc.LONG_LENGTHS and C[name].kernel == kernel and C[name].n == 6200
        assert L[12:].max() <= (24 if kernel == "staged" else 6)
        assert tuple(np.diff(C[name].R[2])[:12]) == mc.LONG_LENGTHS
    assert set(mc.LONG_LENGTHS) >= {CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 3 * CHUNK + 1}
    L = np.diff(C["short_staged_1100"].A[2])
    assert np.all(L[300:812] == 0) and np.count_nonzero(L >= 900) >= 4 and L.max() <= 1098
    assert np.all(np.delete(L, np.nonzero(L >= 900)[0]) <= 12)


@pytest.mark.parametrize("kp", WIDTHS)
def test_chunk_boundaries_empty_workgroups_and_late_diagonals(kp):
    rows = ROWS[kp]
    for name in ("short_staged_1100", "medium", "long_staged"):
        case = C[name]
        assert case.kernel == "staged"
        assert mc.straddling_rows(case.A, rows), (name, kp)
        assert mc.straddling_rows(case.Ad, rows) == mc.straddling_rows(case.A, rows)
        spans = [(e1 - e0 + CHUNK - 1) // CHUNK for _, _, e0, e1 in mc.workgroup_entries(case.A, rows)]
        assert max(spans) >= 2, (name, kp, spans)
    spans = [(e1 - e0 + CHUNK - 1) // CHUNK for _, _, e0, e1 in mc.workgroup_entries(C["medium"].A, rows)]
    assert max(spans) >= (10 if rows == 256 else 3)
    # a row longer than a chunk, and a diagonal ROW_OFFDIAG / ROW_BSR1 must skip and remember in a later chunk
    assert np.diff(C["long_staged"].A[2]).max() > 3 * CHUNK
    late = mc.late_diagonal_rows(C["long_staged"].Ad, rows)
    assert late, kp
    n, _, Ap, Aj, Ax = C["long_staged"].Ad
    assert any(Ax[Ap[i + 1] - 1] != 0.0 for i in late)           # one of them usable: the row is relaxed
    # a whole workgroup with e0 == e1, in a staged operator and in the empty one
    assert mc.empty_workgroups(C["short_staged_1100"].A, rows), kp
    assert mc.empty_workgroups(C["empty_300"].A, rows), kp
    # the transfer operators: R's rows cross chunks too, P has both kernels and empty runs
    assert mc.straddling_rows(C["long_staged"].R, rows) and mc.straddling_rows(C["medium"].R, rows)


def test_transfer_operators():
    kinds = set()
    for case in CASES:
        assert case.R[0] == mc.N1 and case.R[1] == case.n and case.P[0] == case.n and case.P[1] == mc.N1
        L = np.diff(case.P[2])
        assert L.max() <= 30 if case.n else True
        if case.n >= 200:
            assert np.all(L[case.n // 5:case.n // 5 + 40] == 0) and L.max() >= 25
        kinds.add(mc.kernel_of(case.P))
        if case.n > 2:
            assert mc.kernel_of(case.R) == "staged"
    assert kinds == {"direct", "staged"}
    assert mc.kernel_of(mc.smoother_transfers(300)[0]) == "direct"          # EpiStore through the direct kernel


def test_content_rules_survive():
    """what operator_cases.irregular promises, on the families that are large enough to show all of it, before and
    after the dominance scaling (which moves no entry and leaves the diagonals alone)"""
    for name in ("short_257", "short_769", "short_staged_1100", "medium", "long_staged", "long_direct", "threshold_at"):
        for csr in (C[name].A, C[name].Ad):
            n, _, Ap, Aj, Ax = csr
            none = zero = twice = dup = unsorted_even = 0
            for i in range(n):
                cols, vals = Aj[Ap[i]:Ap[i + 1]], Ax[Ap[i]:Ap[i + 1]]
                d = vals[cols == i]
                none += len(d) == 0 and len(cols) > 0
                zero += len(d) > 0 and d[-1] == 0.0
                twice += len(d) == 2
                off = cols[cols != i]
                dup += len(np.unique(off)) < len(off)
                if i % 2 == 1:
                    assert np.all(np.diff(cols) >= 0)
                else:
                    unsorted_even += bool(np.any(np.diff(cols) < 0))
                if len(d) and d[-1] != 0.0:
                    assert 0.5 <= abs(d[-1]) <= 1.5
            assert none and zero and twice == 1 and dup and unsorted_even, name
            assert np.count_nonzero(Ax == 0.0) > 0


def test_operands():
    for case in CASES:
        for V in (case.B8, case.X8):
            assert V.shape == (case.n + 1, 8) and V.flags.c_contiguous
            assert np.all(V[-1] == mc.GUARD)
            assert not np.any(V[:-1, mc.ZERO_COLUMN])
            if case.n >= 63:
                body = V[:-1]
                assert np.any(np.signbit(body) & (body == 0.0))              # some -0.0
                mags = np.abs(body).max(axis=0)
                for j in range(8):
                    if j != mc.ZERO_COLUMN:
                        assert 0.5 * 10.0 ** (3 * j - 9) < mags[j] <= 10.0 ** (3 * j - 9)
    V = mc.take(CASES[3].B8, [4, 1])
    assert V.flags.c_contiguous and np.array_equal(V[:, 0], CASES[3].B8[:, 4]) and V[-1, 1] == mc.GUARD


# ------------------------------------------------------------------------------------------------ dominance
def oracle_relax(csr, desc, x, b):
    lib = oracle_lib.load()
    keep = []
    A = mc.as_scipy(csr)
    M = oracle_lib.make_mat(A, keep)
    s = oracle_lib.make_smoother(desc, A, keep)
    lib.oracle_relax(ctypes.byref(M), ctypes.byref(s), oracle_lib.dp(x), oracle_lib.dp(b))


DOMINANCE_SMOOTHERS = [
    {"name": "jacobi", "omega": 0.7, "iterations": 2},
    {"name": "gauss_seidel", "sweep": "symmetric", "iterations": 2},
    {"name": "sor", "omega": 1.3, "sweep": "symmetric", "iterations": 2},
    {"name": "polynomial", "coefficients": [0.3, -0.2, 0.45], "iterations": 2},
]


@pytest.mark.parametrize("name", NAMES)
def test_dominance_scaling_keeps_the_iterates_finite(name):
    case = C[name]
    n, _, Ap, Aj, Ax = case.Ad
    for i in range(n):
        cols, vals = Aj[Ap[i]:Ap[i + 1]], Ax[Ap[i]:Ap[i + 1]]
        d = vals[cols == i]
        if len(d) and d[-1] != 0.0:
            assert np.abs(vals[cols != i]).sum() < 0.4 < 0.5 <= abs(d[-1])
    rng = np.random.RandomState(77 + n)
    for desc in DOMINANCE_SMOOTHERS:
        x = rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n)           # no zeros among the inputs
        b = rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n)
        oracle_relax(case.Ad, desc, x, b)
        assert np.all(np.isfinite(x)) and np.abs(x).max() < 1e5, (name, desc["name"], np.abs(x).max())
        assert not np.any(x == 0.0), (name, desc["name"])


# ------------------------------------------------------------------------------------------------ model = oracle
@pytest.mark.parametrize("name", NAMES)
def test_transfer_model_equals_the_oracle(name):
    case = C[name]
    want = mc.oracle_transfer(case)
    assert np.all(np.isfinite(want))
    got = mc.two_level_cycle(case.A, case.R, case.P, case.M, case.B8[:-1], case.X8[:-1])
    assert mc.bit_mismatches(got, want) == 0
    # the correction reaches the rows: P has entries in most of them
    changed = np.any(want.view(np.int64) != case.X8[:-1].view(np.int64), axis=1)
    stored = np.diff(case.P[2]) > 0
    if case.n >= 63:
        assert stored.sum() >= 20 and changed[stored].mean() >= 0.95


@pytest.mark.parametrize("bsr", [False, True], ids=["csr", "bsr1"])
@pytest.mark.parametrize("label", LABELS)
@pytest.mark.parametrize("name", NAMES)
def test_smoother_model_equals_the_oracle(name, label, bsr):
    case = C[name]
    desc = dict(mc.SMOOTHERS)[label]
    want = mc.oracle_smoother(case, label, bsr)
    cols = model_columns(case)
    R, P = mc.smoother_transfers(case.n)
    got = mc.two_level_cycle(case.Ad, R, P, mc.SMOOTHER_M, case.B8[:-1][:, cols], case.X8[:-1][:, cols], desc, desc, bsr)
    assert mc.bit_mismatches(got, want[:, cols]) == 0


# ------------------------------------------------------------------------------------------------ the inputs are fair
@pytest.mark.parametrize("label", LABELS)
@pytest.mark.parametrize("name", NAMES)
def test_conditions_on_the_inputs(name, label):
    """On the oracle alone.  Every output is finite.  Every row with a usable diagonal changes, and so do 60 % of all
    rows wherever the family's content allows that many: irregular() leaves a third of the rows without a diagonal,
    and the runs of empty rows the families are built with (rows 300..811 of short_staged_1100, all of empty_300) have
    nothing to relax, so a Jacobi or Gauss-Seidel sweep cannot reach 60 % there; the polynomial reaches every row.
    A row without a usable diagonal is left alone by Jacobi and Gauss-Seidel, bit for bit (its -0.0 entries become
    +0.0 in the cycle's x + P e)."""
    case = C[name]
    n = case.n
    x0 = case.X8[:-1]
    unusable = np.zeros(n, dtype=bool)
    unusable[mc.unusable_diagonal_rows(case.Ad)] = True
    for bsr in (False, True):
        out = mc.oracle_smoother(case, label, bsr)
        assert np.all(np.isfinite(out))
        changed = np.any(out.view(np.int64) != x0.view(np.int64), axis=1)
        assert np.all(changed[~unusable]), (name, label)
        if label.startswith("poly") or (~unusable).mean() >= 0.6:
            assert changed.mean() >= 0.6, (name, label, changed.mean())
        if label in ("jacobi", "gs_forward", "gs_backward", "gs_symmetric") and unusable.any():
            live = ~(np.signbit(x0) & (x0 == 0.0))
            same = (out.view(np.int64) == x0.view(np.int64)) | ~live
            kept = unusable & np.all(same, axis=1) & np.any(x0 != 0.0, axis=1)
            assert kept.any(), (name, label)
            assert np.array_equal(kept, unusable & np.any(x0 != 0.0, axis=1))


@pytest.mark.parametrize("label", ["jacobi", "gs_forward"])
def test_bsr_and_csr_roundings_differ_on_medium(label):
    a = mc.oracle_smoother(C["medium"], label, False)
    b = mc.oracle_smoother(C["medium"], label, True)
    assert mc.bit_mismatches(a, b) > 0
    assert np.allclose(a, b, rtol=1e-9, atol=0.0)


def test_columns_are_independent_in_the_oracle_and_scaled_apart():
    """a column's oracle result does not depend on its neighbours (it is computed alone), and two columns differ by
    orders of magnitude, so a mixed-up column cannot pass"""
    out = mc.oracle_transfer(C["medium"])
    mags = np.abs(out).max(axis=0)
    live = [j for j in range(8) if j != mc.ZERO_COLUMN]
    for a, b in zip(live[:-1], live[1:]):
        assert mags[b] > 100.0 * mags[a]
    assert not np.any(out[:, mc.ZERO_COLUMN])


# ------------------------------------------------------------------------------------------------ the norm tree
def test_multi_norm_model():
    G = vm.MULTI_NORM_GRID
    assert G == 2048 * 256 == 524288
    assert vm.multi_norm_model([3.0]) == 3.0 and vm.multi_norm_model([]) == 0.0
    SMALL = math.sqrt(0.7 * 2.0 ** -52)      # its square is 0.7 ulp of 1.0: two added one by one give 2 ulp, as a pair 1 ulp
    # one entry above the grid: lane 0 of workgroup 0 adds rows 0 and G, in that order, before any tree
    v = np.zeros(G + 1)
    v[0], v[1], v[G] = 1.0, SMALL, SMALL
    q = v * v
    assert (q[0] + q[G]) + q[1] == 1.0 + 2.0 ** -51 and q[0] + (q[G] + q[1]) == 1.0 + 2.0 ** -52
    assert vm.multi_norm_model(v) == math.sqrt(1.0 + 2.0 ** -51) > 1.0 == math.sqrt(1.0 + 2.0 ** -52)
    # lanes t and t + 128 meet first: lanes 0 and 128, then lane 1 -- one by one
    v = np.zeros(G)
    v[0], v[128], v[1] = 1.0, SMALL, SMALL
    assert vm.multi_norm_model(v) == math.sqrt(1.0 + 2.0 ** -51)
    v[128], v[129] = 0.0, SMALL                # lanes 1 and 129 meet before either meets lane 0: as a pair
    assert vm.multi_norm_model(v) == 1.0
    # workgroups w and w + 256 meet in one lane of the second stage, in order: one by one again
    v[129], v[256 * 256 + 1] = 0.0, SMALL
    assert vm.multi_norm_model(v) == math.sqrt(1.0 + 2.0 ** -51)
    rng = np.random.RandomState(9)
    for n in (1, 257, G, G + 1, 2 * G + 3):
        v = rng.uniform(-1.0, 1.0, n)
        exact = math.sqrt(math.fsum(v * v))
        # 2 rounds of a lane + 8 levels, 8 partial sums + 8 levels, one rounding per square, two roots
        assert abs(vm.multi_norm_model(v) - exact) <= 40 * vm.U * exact
