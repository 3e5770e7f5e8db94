"""The host side of the resident smoothed-aggregation chain: which levels it takes, what the three
strength modes and the row sort have to compute, and what a host build records.  No GPU is needed."""
import numpy as np
import pytest
import scipy.sparse as sps

import sa_chain_cases as sc
from pyamg_amd import _lib, aggregation
from pyamg_amd.aggregation import poisson, symmetric_strength_of_connection

A_CSR = poisson((6, 6), format="csr")
A_BSR = sps.bsr_matrix(A_CSR, blocksize=(1, 1))
ONE = np.ones((36, 1))
ON = {"device": True}
SYM, MIS, JAC = ("symmetric", dict(ON)), ("mis", dict(ON)), ("jacobi", dict(ON, omega=4.0 / 3.0))


def _options(A=A_CSR, B=ONE, strength=SYM, aggregate=MIS, smooth=JAC, device=True):
    return aggregation._chain_options(A, B, strength, aggregate, smooth, device)


def test_chain_takes_the_levels_it_is_for():
    assert _options() == (0, 4.0 / 3.0, 1, "diagonal")
    assert _options(A=A_BSR, strength=("symmetric", dict(ON, theta=0.25))) == (0.25, 4.0 / 3.0, 1, "diagonal")
    assert _options(smooth=("jacobi", dict(ON, weighting="local", degree=2, omega=1.0))) == (0, 1.0, 2, "local")
    assert _options(smooth=("jacobi", dict(ON, weighting="block"))) == (0, 4.0 / 3.0, 1, "diagonal")
    assert _options(smooth=("jacobi", dict(ON, filter=False))) is not None


@pytest.mark.parametrize("change", [
    {"strength": ("symmetric", {"device": False})},
    {"strength": "symmetric"},                                  # device=None: SYMMETRIC_STRENGTH_DEVICE_AUTO is off
    {"strength": ("symmetric", dict(ON, theta=-1.0))},
    {"strength": ("evolution", dict(ON))},
    {"strength": None},
    {"aggregate": ("mis", {"device": False})},
    {"aggregate": "mis"},
    {"aggregate": ("mis", dict(ON, y=np.zeros(36)))},
    {"aggregate": ("standard", {})},
    {"smooth": ("jacobi", {"device": False})},
    {"smooth": "jacobi"},
    {"smooth": ("jacobi", dict(ON, filter=True))},
    {"smooth": ("jacobi", dict(ON, weighting="other"))},
    {"smooth": ("jacobi", dict(ON, degree=0))},
    {"smooth": ("energy", dict(ON))},
    {"smooth": None},
    {"device": False},
    {"device": None},
    {"B": np.ones((36, 2))},
    {"B": np.ones((36, 1), dtype=np.complex128)},
    {"A": A_CSR.astype(np.complex128)},
    {"A": A_CSR.astype(np.float32)},
    {"A": sps.bsr_matrix(A_CSR, blocksize=(2, 2))},
], ids=lambda c: "-".join(c))
def test_chain_leaves_every_other_level_where_it_goes_today(change):
    assert _options(**change) is None


def test_strength_mode_follows_the_format_of_the_host_operator():
    assert aggregation._chain_strength_mode(A_CSR, 0) == _lib.SA_STRENGTH_CSR
    assert aggregation._chain_strength_mode(A_CSR, 0.25) == _lib.SA_STRENGTH_CSR
    assert aggregation._chain_strength_mode(A_BSR, 0) == _lib.SA_STRENGTH_ONES
    assert aggregation._chain_strength_mode(A_BSR, 0.25) == _lib.SA_STRENGTH_SQUARED


def _unsorted_operator():
    """60 rows of mixed sign in a shuffled stored order, a row without a diagonal, a row of stored zeros, an empty row"""
    rng = np.random.RandomState(3)
    M = sps.random(60, 60, density=0.15, random_state=rng, format="lil")
    M.setdiag(rng.rand(60) + 0.5)
    M[7, 7] = 0.0
    M = sps.csr_matrix(M + M.T)
    M.data *= rng.choice([-1.0, 1.0], size=len(M.data))
    rows = []
    for i in range(60):
        lo, hi = M.indptr[i], M.indptr[i + 1]
        order = rng.permutation(hi - lo)
        row = [(M.indices[lo + k], M.data[lo + k]) for k in order]
        if i == 11:
            row = [(j, 0.0) for j, _ in row]
        if i == 13:
            row = []
        rows.append(row)
    Ap = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.intc)
    Aj = np.array([j for r in rows for j, _ in r], dtype=np.intc)
    Ax = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return Ap, Aj, Ax


@pytest.mark.parametrize("theta", [0.0, 0.02, 0.25, 0.6])
def test_strength_models_equal_the_host_route(theta):
    Ap, Aj, Ax = _unsorted_operator()
    csr = sps.csr_matrix((Ax, Aj, Ap), shape=(60, 60))
    bsr = sps.bsr_matrix((Ax.reshape(-1, 1, 1), Aj, Ap), shape=(60, 60))
    for A, mode in ((csr, _lib.SA_STRENGTH_CSR), (bsr, aggregation._chain_strength_mode(bsr, theta))):
        assert mode == aggregation._chain_strength_mode(A, theta)
        want = symmetric_strength_of_connection(A, theta, device=False)
        Sp, Sj, Sx = sc.strength_model(Ap, Aj, Ax, theta, mode)
        assert want.format == "csr" and np.array_equal(want.indptr, Sp) and np.array_equal(want.indices, Sj)
        assert np.array_equal(want.data, Sx)
    assert not np.array_equal(Ap, symmetric_strength_of_connection(csr, 0.6, device=False).indptr)      # (entries are dropped)


def test_row_sort_model_equals_scipy():
    Ap, Aj, Ax = _unsorted_operator()
    A = sps.csr_matrix((Ax.copy(), Aj.copy(), Ap.copy()), shape=(60, 60))
    assert not A.has_sorted_indices
    A.sort_indices()
    Oj, Ox = sc.sorted_rows_model(Ap, Aj, Ax)
    assert np.array_equal(A.indices, Oj) and np.array_equal(A.data, Ox)


def test_host_build_records_no_chained_level_and_no_upload():
    aggregation.LAST_BUILD["uploads"] = -1
    ml = sc.build("poisson_30x30", device=False, fast=False)
    sizes = tuple(lvl.A.shape[0] for lvl in ml.levels)
    assert sizes == sc.cases()["poisson_30x30"][2]
    assert aggregation.LAST_BUILD["uploads"] == 0
    assert len(aggregation.LAST_BUILD["levels"]) == len(sizes) - 1
    assert not any(rec["chained"] or rec["resident"] for rec in aggregation.LAST_BUILD["levels"])
    assert aggregation._RESIDENT_CHAIN is True and aggregation.CHAIN_STAGES[0] == "upload" and aggregation.CHAIN_STAGES[-1] == "fetch"


@pytest.mark.parametrize("name", [n for n, c in sc.cases().items() if c[2] is not None])
def test_cases_have_the_levels_they_are_named_for(name):
    ml = sc.build(name, device=False, fast=False, keep=True)
    assert tuple(lvl.A.shape[0] for lvl in ml.levels) == sc.cases()[name][2]
    if name == "no_aggregate":
        assert ml.levels[1].P.shape == (130, 1) and ml.levels[1].P.nnz == 0
    if name in ("poisson_30x30", "poisson_12x12x12"):
        Cm = ml.levels[1].C                 # level 1 is BSR(1,1) on the host: all ones, in the product's order
        assert np.all(Cm.data == 1.0) and not sps.csr_matrix((Cm.data, Cm.indices, Cm.indptr), shape=Cm.shape).has_sorted_indices
    if name == "poisson_30x30_theta":
        kept = sum(lvl.C.nnz for lvl in ml.levels[1:-1])
        stored = sum(len(lvl.A.indices) for lvl in ml.levels[1:-1])
        assert kept < stored                # levels 1 and 2 drop entries: the squared mode runs


def test_one_sided_case_is_refused_on_the_host():
    with pytest.raises(ValueError, match="expected a structurally symmetric pattern"):
        sc.build("one_sided", device=False, fast=False)
