"""No GPU: the designed operands of the device transpose (transpose_cases) -- the pure-Python model of the definition
against scipy's P.T.tocsr() on every case, and every case against the row lengths it was designed for."""
import numpy as np
import pytest

import classical_io as cio
import transpose_cases as tc


@pytest.mark.parametrize("name", sorted(tc.cases()))
def test_model_equals_scipy(name):
    P, _ = tc.cases()[name]
    R = P.T.tocsr()
    Rp, Rj, Rx = tc.model(P)
    assert R.shape == (P.shape[1], P.shape[0]) and R.nnz == P.nnz
    assert cio.same_bits(Rp, R.indptr.astype(np.intc)) and cio.same_bits(Rj, R.indices.astype(np.intc))
    assert cio.same_bits(Rx, R.data)


@pytest.mark.parametrize("name", sorted(tc.cases()))
def test_cases_reach_the_forms_they_were_designed_for(name):
    P, forms = tc.cases()[name]
    lane, lds, hbm = tc.forms_of(P)
    assert lane + lds + hbm == P.shape[1]
    if not forms:
        assert P.nnz == 0
        return
    assert {form for form, rows in (("lane", lane), ("lds", lds), ("hbm", hbm)) if rows > 0} == forms


def test_thresholds_are_crossed_from_both_sides():
    longest = lambda name: int(np.bincount(tc.cases()[name][0].indices).max())
    for threshold in (tc.LANE_MAX, tc.LDS_MAX):
        for where in ("first", "last", "between"):
            assert [longest("hub_%d_%s" % (n, where)) for n in (threshold - 1, threshold, threshold + 1)] == \
                [threshold - 1, threshold, threshold + 1]
    P = tc.cases()["hub_%d_between" % tc.LDS_MAX][0]
    assert np.bincount(P.indices, minlength=5).tolist() == [2, 2, tc.LDS_MAX, 2, 2]


def test_designed_properties():
    c = tc.cases()
    assert np.bincount(c["empty_columns"][0].indices, minlength=8).tolist() == [0, 0, 2, 2, 0, 2, 2, 0]
    D = c["duplicates"][0]
    assert D.indices[D.indptr[0]:D.indptr[1]].tolist() == [2, 0, 2] and D.indices[D.indptr[1]:D.indptr[2]].tolist() == [3, 3, 1, 3]
    for name, step in (("descending", -1), ("shuffled", 0)):
        P = c[name][0]
        rows = [P.indices[P.indptr[i]:P.indptr[i + 1]] for i in range(P.shape[0])]
        if step:
            assert all(np.all(np.diff(r) < 0) for r in rows)
        else:
            assert any(np.any(np.diff(r) < 0) for r in rows) and any(np.any(np.diff(r) > 0) for r in rows)
    M = c["many_columns"][0]
    assert M.shape[1] == 70000 and np.all(np.bincount(M.indices, minlength=70000) == 1)
    V = c["value_bits"][0].data
    assert np.signbit(V[0]) and V[0] == 0 and np.isnan(V[2]) and np.isinf(V[5]) and 0 < V[7] < np.finfo(np.float64).tiny
    I = c["interleaved"][0]
    assert I.shape == (5000, 300) and I.nnz == 40000
