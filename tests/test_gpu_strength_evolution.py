"""Evolution strength of connection on the device (csrc/strength.hip): the four flat entries against the reference's
recorded native calls and against sequential models, the pipeline against the host path and the reference's C."""
import numpy as np
import pytest
import scipy.sparse as sps

import evolution_io as eio
import golden_io
import pyamg_amd
from pyamg_amd import amg_core, strength, util
from pyamg_amd.gallery import poisson
from pyamg_amd.strength import evolution_strength_of_connection

pytestmark = pytest.mark.gpu

ic = lambda a: np.ascontiguousarray(a, dtype=np.intc)


# ---------------------------------------------------------------------------------------------- recorded native calls
@pytest.mark.parametrize("name", eio.PROBLEMS)
def test_flat_kernels_reproduce_the_recorded_native_calls(name):
    p = eio.problem(name)
    seen = set()
    for k in eio.KS:
        for kernel, a, expect in p[k]["calls"]:
            seen.add(kernel)
            Sx = a["Sx"].copy()
            if kernel == "incomplete_mat_mult_csr":
                amg_core.incomplete_mat_mult_csr(a["Ap"], a["Aj"], a["Ax"], a["Bp"], a["Bj"], a["Bx"], a["Sp"], a["Sj"], Sx,
                                                 int(a["dimen"]))
            else:
                amg_core.apply_distance_filter(int(a["n_row"]), float(a["epsilon"]), a["Sp"], a["Sj"], Sx)
            assert np.array_equal(Sx, expect), (name, k, kernel, np.abs(Sx - expect).max())
    assert seen == {"incomplete_mat_mult_csr", "apply_distance_filter"}


def test_min_blocks_and_absolute_filter_reproduce_the_recorded_native_calls():
    z = eio.flat_kernels()
    Tx = np.zeros(int(z["min_blocks__n_blocks"]))
    amg_core.min_blocks(int(z["min_blocks__n_blocks"]), int(z["min_blocks__blocksize"]), z["min_blocks__Sx"], Tx)
    assert np.array_equal(Tx, z["min_blocks__Tx_out"])
    assert Tx[2] == eio.DBL_MAX                                 # the block without a non-zero value
    Sx = z["absfilter__Sx"].copy()
    amg_core.apply_absolute_distance_filter(int(z["absfilter__n_row"]), float(z["absfilter__epsilon"]), z["absfilter__Sp"],
                                            z["absfilter__Sj"], Sx)
    assert np.array_equal(Sx, z["absfilter__Sx_out"])


# ---------------------------------------------------------------------------------------------- sequential models
def rand_csr(n, nnz, rng, empty_rows=()):
    """n x n sorted CSR with exactly nnz entries, none in the rows listed"""
    rows = [i for i in range(n) if i not in empty_rows]
    cells = np.array([(i, j) for i in rows for j in range(n)])
    pick = cells[np.sort(rng.choice(len(cells), nnz, replace=False))]
    M = sps.csr_matrix((rng.uniform(-1.0, 1.0, nnz), (pick[:, 0], pick[:, 1])), shape=(n, n))
    M.sort_indices()
    assert M.nnz == nnz
    return M


def run_incomplete(A, Bcsc, S):
    Sx = np.full(S.nnz, np.nan)
    amg_core.incomplete_mat_mult_csr(ic(A.indptr), ic(A.indices), A.data, ic(Bcsc.indptr), ic(Bcsc.indices), Bcsc.data,
                                     ic(S.indptr), ic(S.indices), Sx, A.shape[0])
    model = eio.model_incomplete_mat_mult(A.indptr, A.indices, A.data, Bcsc.indptr, Bcsc.indices, Bcsc.data, S.indptr,
                                          S.indices, A.shape[0])
    assert np.array_equal(Sx, model)
    return Sx


@pytest.mark.parametrize("nnz", [63, 64, 65, 255, 257])
def test_kernels_against_sequential_models(nnz):
    rng = np.random.RandomState(nnz)
    n = 20
    A = rand_csr(n, 150, rng, empty_rows=(4,))
    B = rand_csr(n, 140, rng, empty_rows=(9,)).tocsc()
    B.sort_indices()
    S = rand_csr(n, nnz, rng, empty_rows=(0, 7, 19))
    run_incomplete(A, B, S)
    # the filters on the same pattern, positive "distances"
    Sx0 = rng.uniform(0.1, 2.0, nnz)
    for absolute, fn in ((False, amg_core.apply_distance_filter), (True, amg_core.apply_absolute_distance_filter)):
        Sx = Sx0.copy()
        fn(n, 1.5, ic(S.indptr), ic(S.indices), Sx)
        with np.errstate(over="ignore"):
            assert np.array_equal(Sx, eio.model_distance_filter(n, 1.5, S.indptr, S.indices, Sx0, absolute))
    # nnz blocks of 3 values, a third of them zero
    blocks = rng.uniform(-1.0, 1.0, nnz * 3)
    blocks[rng.rand(nnz * 3) < 0.34] = 0.0
    blocks[:3] = 0.0
    Tx = np.zeros(nnz)
    amg_core.min_blocks(nnz, 3, blocks, Tx)
    assert np.array_equal(Tx, eio.model_min_blocks(nnz, 3, blocks)) and Tx[0] == eio.DBL_MAX


def test_kernels_on_one_row():
    one = sps.csr_matrix(np.array([[3.0]]))
    assert run_incomplete(one, one.tocsc(), one)[0] == 9.0
    Sx = np.array([0.25])
    amg_core.apply_distance_filter(1, 4.0, ic(one.indptr), ic(one.indices), Sx)
    assert Sx[0] == 1.0
    Tx = np.zeros(1)
    amg_core.min_blocks(1, 1, np.array([-2.0]), Tx)
    assert Tx[0] == -2.0
    # no rows, no entries: nothing to do
    e = np.zeros(0)
    amg_core.incomplete_mat_mult_csr(ic([0]), ic([]), e, ic([0]), ic([]), e, ic([0]), ic([]), e.copy(), 0)
    amg_core.min_blocks(0, 4, e, e.copy())


def test_incomplete_product_with_a_long_row():
    p = eio.problem("unsym_400")
    A = p["A"].copy()
    A.eliminate_zeros()
    assert np.diff(A.indptr).max() >= 290 and np.diff(A.indptr).min() == 0
    B = A.tocsc()
    B.sort_indices()
    run_incomplete(A, B, A)


def test_incomplete_product_whose_merges_never_match():
    rng = np.random.RandomState(1)
    n = 24
    even = sps.csr_matrix(rng.rand(n, n) * (np.arange(n) % 2 == 0)[None, :])        # A: even columns only
    odd = sps.csc_matrix(rng.rand(n, n) * (np.arange(n) % 2 == 1)[:, None])         # B: odd rows only
    even.sort_indices(); odd.sort_indices()
    S = rand_csr(n, 100, rng)
    Sx = run_incomplete(even, odd, S)
    assert np.all(Sx == 0.0) and not np.any(np.signbit(Sx))


def test_bad_arguments_are_value_errors():
    Sp, Sj = ic([0, 1]), ic([5])
    with pytest.raises(ValueError):
        amg_core.incomplete_mat_mult_csr(Sp, ic([0]), np.ones(1), Sp, ic([0]), np.ones(1), Sp, Sj, np.ones(1), 1)
    with pytest.raises(ValueError):
        amg_core.apply_distance_filter(3, 2.0, Sp, ic([0]), np.ones(1))
    with pytest.raises(ValueError):
        amg_core.min_blocks(4, 4, np.ones(8), np.ones(4))


# ---------------------------------------------------------------------------------------------- the pipeline
VARIANTS = [(sym, eps) for sym in (True, False) for eps in (1.5, 4.0, np.inf)]


@pytest.mark.parametrize("k", eio.KS)
@pytest.mark.parametrize("name", eio.PROBLEMS)
def test_pipeline_equals_host_path_bit_for_bit(name, k):
    p = eio.problem(name)
    for sym, eps in VARIANTS:
        kw = dict(epsilon=eps, k=k, symmetrize_measure=sym, rho=p[k]["rho"])
        H = evolution_strength_of_connection(p["A"], p["B"], device=False, **kw)
        D = evolution_strength_of_connection(p["A"], p["B"], device=True, **kw)
        eio.same_bits(D, H)


@pytest.mark.parametrize("k", eio.KS)
@pytest.mark.parametrize("name", eio.PROBLEMS)
def test_pipeline_with_recorded_rho_is_the_reference_bit_for_bit(name, k):
    p = eio.problem(name)
    D = evolution_strength_of_connection(p["A"], p["B"], epsilon=p["epsilon"], k=k, device=True, rho=p[k]["rho"])
    eio.same_bits(D, p[k]["C"])
    Ab = sps.bsr_matrix((p["A"].data.reshape(-1, 1, 1), p["A"].indices, p["A"].indptr), shape=p["A"].shape)
    eio.same_bits(evolution_strength_of_connection(Ab, p["B"], epsilon=p["epsilon"], k=k, device=True, rho=p[k]["rho"]),
                  p[k]["C"])


def test_pipeline_k8_squares_on_the_device():
    p = eio.problem("aniso_17x23")
    kw = dict(epsilon=4.0, k=8, rho=p[4]["rho"])
    eio.same_bits(evolution_strength_of_connection(p["A"], device=True, **kw),
                  evolution_strength_of_connection(p["A"], device=False, **kw))


def test_pipeline_row_that_loses_every_off_diagonal():
    # one candidate entry of the other sign: every ratio that involves node 14 has the wrong angle
    A = poisson((6, 6), format="csr")
    B = np.ones(36)
    B[14] = -1.0
    for sym in (True, False):
        kw = dict(epsilon=4.0, k=2, symmetrize_measure=sym, rho=1.9)
        H = evolution_strength_of_connection(A, B, device=False, **kw)
        D = evolution_strength_of_connection(A, B, device=True, **kw)
        eio.same_bits(D, H)
        assert D.indptr[15] - D.indptr[14] == 1 and D.indices[D.indptr[14]] == 14


def test_pipeline_products_that_cancel_exactly():
    # unit diagonal, rho = 1: M = I - A has no diagonal; (M^T M^T)[3, 0] = 1 * 1 + 1 * (-1) = 0 on A's pattern
    A = np.eye(5)
    A[0, 1] = A[0, 2] = A[1, 3] = -1.0
    A[2, 3] = 1.0
    A[0, 3] = A[3, 0] = -0.5
    A[3, 4] = A[4, 3] = A[1, 0] = A[2, 0] = -0.25
    Mt = (np.eye(5) - A).T
    P = Mt @ Mt
    assert np.any((P == 0.0) & (A != 0.0) & ~np.eye(5, dtype=bool))
    A = sps.csr_matrix(A)
    for k in (2, 4):
        for sym, eps in VARIANTS:
            kw = dict(epsilon=eps, k=k, symmetrize_measure=sym, rho=1.0)
            H = evolution_strength_of_connection(A, device=False, **kw)
            D = evolution_strength_of_connection(A, device=True, **kw)
            eio.same_bits(D, H)


# ---------------------------------------------------------------------------------------------- working size
# evolution_io.large_grid / large_unsym hold more than 2^20 entries and more than 65 536 rows (asserted where they are
# built; the rocPRIM limits they are chosen against are named there, read from rocprim/device/device_radix_sort.hpp and
# device_radix_sort_config.hpp).  Every transpose and row sort of their Jacobi step (and the k = 4 square of about
# 5.7 M entries on the grid) is therefore sorted by onesweep over all 64 key bits with row bits above bit 48 set, and
# every count/scan/fill stage scans n + 1 > 150 000 counts with the multi-block look-back scan.
_host_large = {}


def host_large(name, k, sym=True, eps=eio.LARGE_EPSILON):
    """the host result, pinned to the reference's digests by tests/test_strength_evolution_host.py; computed once"""
    key = (name, k, sym, eps)
    if key not in _host_large:
        A, B = eio.large_problem(name)
        _host_large[key] = evolution_strength_of_connection(A, B, epsilon=eps, k=k, symmetrize_measure=sym, device=False,
                                                            rho=eio.large_digests()[name][k]["rho"])
    return _host_large[key]


@pytest.mark.parametrize("k", eio.KS)
@pytest.mark.parametrize("name", eio.LARGE)
def test_pipeline_reproduces_the_reference_digests_at_working_size(name, k):
    A, B = eio.large_problem(name)
    d = eio.large_digests()[name]
    assert eio.digests(A) == d["A"] and eio.sha(B, "<f8") == d["B"], "the builder did not rebuild the recorded input"
    D = evolution_strength_of_connection(A, B, epsilon=eio.LARGE_EPSILON, k=k, device=True, rho=d[k]["rho"])
    try:
        eio.assert_large_digests(D, d[k], "%s k=%d, device pipeline" % (name, k))
    except AssertionError:
        eio.same_bits(D, host_large(name, k))               # names the first array and position that differ
        raise


@pytest.mark.parametrize("sym,eps", VARIANTS)
def test_pipeline_variants_equal_the_host_path_at_working_size(sym, eps):
    A, B = eio.large_grid()
    H = host_large("large_grid", 2, sym, eps)
    if (sym, eps) in ((True, 4.0), (False, np.inf)):        # 1 151 520 and 1 610 398 entries: the later sorts are onesweep too
        assert H.nnz > eio.SORT_MERGE_LIMIT
    D = evolution_strength_of_connection(A, B, epsilon=eps, k=2, symmetrize_measure=sym, device=True,
                                         rho=eio.large_digests()["large_grid"][2]["rho"])
    eio.same_bits(D, H)


def test_incomplete_product_at_working_size_on_sampled_entries():
    """the flat entry on the large unsymmetric operator, its CSC form and its own pattern, against the sequential model on
    4096 entries: every entry of the 3000-entry row 23, every entry of column 23, the rest drawn"""
    A, _ = eio.large_unsym()
    Bc = A.tocsc()
    Bc.sort_indices()
    Sx = np.full(A.nnz, np.nan)
    amg_core.incomplete_mat_mult_csr(ic(A.indptr), ic(A.indices), A.data, ic(Bc.indptr), ic(Bc.indices), Bc.data,
                                     ic(A.indptr), ic(A.indices), Sx, A.shape[0])
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    special = np.flatnonzero((rows == 23) | (A.indices == 23))
    assert 3000 <= special.size < 4096 and np.count_nonzero(A.indices[special] == 23) > 1
    rest = np.setdiff1d(np.arange(A.nnz), special)
    pick = np.sort(np.concatenate([special, np.random.RandomState(0).choice(rest, 4096 - special.size, replace=False)]))
    model = eio.model_incomplete_entries(A.indptr, A.indices, A.data, Bc.indptr, Bc.indices, Bc.data, rows[pick], A.indices[pick])
    assert not np.any(np.isnan(Sx))
    assert np.array_equal(Sx[pick], model), np.flatnonzero(Sx[pick] != model)[:5]


# ---------------------------------------------------------------------------------------------- block boundaries
def boundary_operator(n, seed, entries=None):
    """random unsymmetric n x n operator, about 7 entries per row, with the row kinds of unsym_400: row 7 stores no
    diagonal, row 11 a stored zero diagonal, row 19 is empty.  entries: every row keeps a non-zero diagonal instead and
    the operator holds exactly that many entries, none zero (its Jacobi step then holds as many: 1 - x / rho and
    0 - x / rho are not zero for the rho of the test)."""
    rng = np.random.RandomState(seed)
    M = sps.random(n, n, density=6.0 / n, random_state=rng, format="lil", data_rvs=lambda s: rng.uniform(-1.0, 1.0, s))
    for i in range(n):
        M[i, i] = 4.0 + rng.rand()
    if entries is None:
        M[19, :] = 0.0
        M[7, 7] = 0.0
    A = sps.csr_matrix(M)
    A.eliminate_zeros()
    A.sort_indices()
    if entries is None:
        A[11, 11] = 0.0                                     # stays stored
        assert A.nnz == np.count_nonzero(A.data) + 1 and A.indptr[20] == A.indptr[19] and A[7, 7] == 0.0
    else:
        off = np.flatnonzero(A.indices != np.repeat(np.arange(n), np.diff(A.indptr)))
        A.data[rng.choice(off, A.nnz - entries, replace=False)] = 0.0
        A.eliminate_zeros()
        assert A.nnz == entries and np.all(A.diagonal() != 0.0)
    B = rng.uniform(0.5, 1.5, n)
    B[::9] *= -1.0
    B[[3, 23, 50]] = 0.0
    return A, B


# n or n + 1 a multiple of the 256-thread block: the lane i == n that writes count[n] = 0 is the last of a full block
# (n = 255, 511), the first of a block of its own (n = 256, 512) or the second (257).  1024 = 256 x 4 items is the
# largest array rocPRIM's radix_sort_pairs sorts with one block; 1025 is the smallest it merge-sorts.
BOUNDARY = [(65, None), (255, None), (256, None), (257, None), (511, None), (512, None), (160, eio.SORT_ONE_BLOCK),
            (160, eio.SORT_ONE_BLOCK + 1)]
BOUNDARY_RHO = 1.3


@pytest.mark.parametrize("k", eio.KS)
@pytest.mark.parametrize("n,entries", BOUNDARY)
def test_pipeline_equals_host_path_at_block_boundaries(n, entries, k):
    A, B = boundary_operator(n, n + (entries or 0), entries)
    for sym, eps in VARIANTS:
        kw = dict(epsilon=eps, k=k, symmetrize_measure=sym, rho=BOUNDARY_RHO)
        H = evolution_strength_of_connection(A, B, device=False, **kw)
        D = evolution_strength_of_connection(A, B, device=True, **kw)
        eio.same_bits(D, H)


@pytest.mark.parametrize("k", (1, 2))
@pytest.mark.parametrize("case", ["no_rows", "one_by_one", "one_by_one_cancelled", "empty_rows", "diagonal_only"])
def test_pipeline_equals_host_path_on_degenerate_operators(case, k):
    rho = 2.0
    if case == "no_rows":
        A = sps.csr_matrix((0, 0), dtype=np.float64)
    elif case.startswith("one_by_one"):
        A = sps.csr_matrix(np.array([[3.0]]))
        rho = 1.0 if case.endswith("cancelled") else 2.0        # rho = 1: the Jacobi step 1 - 1 / rho stores nothing
    elif case == "empty_rows":
        A = sps.csr_matrix((5, 5), dtype=np.float64)
    else:
        A = sps.diags([np.arange(2.0, 9.0)], [0], format="csr")
    for sym, eps in VARIANTS:
        kw = dict(epsilon=eps, k=k, symmetrize_measure=sym, rho=rho)
        H = evolution_strength_of_connection(A, device=False, **kw)
        D = evolution_strength_of_connection(A, device=True, **kw)
        eio.same_bits(D, H)
    if case == "empty_rows":
        eio.same_bits(H, sps.identity(5, format="csr"))


# ---------------------------------------------------------------------------------------------- the gate
def test_device_none_above_the_gate_takes_the_device_path(monkeypatch):
    monkeypatch.setattr(strength, "DEVICE_AUTO", True)
    monkeypatch.setattr(util, "DEVICE_RHO_MIN_ROWS", 1000)
    taken = []
    real = strength._device_measure

    def wrapped(A, b, rho, epsilon, k, symmetrize_measure, *more):
        taken.append(k)
        return real(A, b, rho, epsilon, k, symmetrize_measure, *more)
    monkeypatch.setattr(strength, "_device_measure", wrapped)
    p = eio.problem("aniso_40x40")
    C = evolution_strength_of_connection(p["A"], p["B"], epsilon=p["epsilon"], k=2, rho=p[2]["rho"])
    assert taken == [2]
    eio.same_bits(C, evolution_strength_of_connection(p["A"], p["B"], epsilon=p["epsilon"], k=2, rho=p[2]["rho"], device=False))
    eio.same_bits(C, p[2]["C"])
    # k = 3 is no power of two: the host path, not a refusal
    with pytest.warns(UserWarning):
        C3 = evolution_strength_of_connection(p["A"], p["B"], epsilon=p["epsilon"], k=3, rho=p[2]["rho"])
    assert taken == [2]
    with pytest.warns(UserWarning):
        eio.same_bits(C3, evolution_strength_of_connection(p["A"], p["B"], epsilon=p["epsilon"], k=3, rho=p[2]["rho"], device=False))


def test_pipeline_refuses_what_the_entry_cannot_take():
    A = poisson((4, 4), format="csr")
    with pytest.raises(NotImplementedError):
        evolution_strength_of_connection(A, k=3, device=True)


# ---------------------------------------------------------------------------------------------- the hierarchy
def test_sa_hierarchy_through_the_pipeline_and_resident_solve():
    g = eio.load_hier("sa_evolution_2d")
    A = g["levels"][0]["A"]
    gs = ("block_gauss_seidel", {"sweep": "symmetric"})
    built = []
    for device in (True, False):
        np.random.seed(0)
        built.append(pyamg_amd.smoothed_aggregation_solver(
            A, strength=("evolution", {"k": 2, "epsilon": 4.0, "device": device}), max_coarse=20, presmoother=gs,
            postsmoother=gs))
    dev, host = built
    assert [lvl.A.shape[0] for lvl in dev.levels] == [1600, 280, 76, 10]
    for a, b in zip(dev.levels, host.levels):
        ops = [("A", a.A, b.A)] + ([("P", a.P, b.P), ("R", a.R, b.R)] if hasattr(b, "P") else [])
        for what, x, y in ops:
            assert type(x) is type(y) and np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices, y.indices) \
                and np.array_equal(x.data, y.data), what
    res = []
    x = dev.solve(g["b"], tol=g["meta"]["tol"], maxiter=g["meta"]["maxiter"], residuals=res)
    assert len(res) == len(g["residuals"])
    golden_io.assert_history(res, g["residuals"], A, x, g["b"])
