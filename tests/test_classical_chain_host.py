"""No GPU: the host side of the classical chain -- classical.transpose(device=False) against the model of
transpose_cases, the host hierarchies against the sizes and row orders the chain's GPU tests rely on, the route record of
a host build, and the refusals of the new paths, which are raised before the device library is touched."""
import numpy as np
import pytest

import classical_io as cio
import transpose_cases as tc
from pyamg_amd import _lib, classical
from pyamg_amd.classical import ruge_stuben_solver


def touched(*a, **k):
    raise AssertionError("the device library was touched")


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(_lib, "device_count", touched)


@pytest.mark.parametrize("name", sorted(tc.cases()))
def test_host_transpose_equals_the_model(name, no_device):
    P, _ = tc.cases()[name]
    for device in (False, None):                # None: DEVICE_AUTO is off
        R = classical.transpose(P, device=device)
        Rp, Rj, Rx = tc.model(P)
        assert R.shape == (P.shape[1], P.shape[0])
        assert cio.same_bits(R.indptr.astype(np.intc), Rp) and cio.same_bits(R.indices.astype(np.intc), Rj)
        assert cio.same_bits(R.data, Rx)


def test_transpose_refuses_before_the_library(no_device):
    P, _ = tc.cases()["shuffled"]
    with pytest.raises(TypeError):
        classical.transpose(P.toarray())
    with pytest.raises(TypeError):
        classical.transpose(P.tocsc(), device=True)
    for bad in (P.astype(np.float32), P.astype(np.complex128)):
        with pytest.raises(NotImplementedError, match="not float64"):
            classical.transpose(bad, device=True)
    assert cio.same_csr(classical.transpose(P.astype(np.float32), device=False), P.astype(np.float32).T.tocsr())


@pytest.mark.parametrize("name", sorted(n for n, h in tc.HIERARCHIES.items() if h[2] is not None))
def test_host_hierarchies_have_the_sizes_and_orders_of_the_table(name, no_device):
    _, _, sizes, coarse_sorted = tc.HIERARCHIES[name]
    ml = tc.host_hierarchy(name)
    assert [lvl.A.shape[0] for lvl in ml.levels] == sizes
    if coarse_sorted is not None:
        assert [tc.rows_sorted(lvl.A) for lvl in ml.levels[1:]] == [coarse_sorted] * (len(sizes) - 1)
    for lvl in ml.levels[:-1]:
        assert cio.same_csr(lvl.R, lvl.P.T.tocsr()) and cio.same_csr(ml.levels[ml.levels.index(lvl) + 1].A, lvl.R * lvl.A * lvl.P)


def test_stars_reach_the_long_rows_they_were_sized_for(no_device):
    for name, form in (("star_pmis", (0, 1, 0)), ("star_cljp", (0, 1, 0)), ("big_star_pmis", (0, 0, 1))):
        lvl = tc.host_hierarchy(name).levels[0]
        assert tc.forms_of(lvl.P) == form and lvl.R.shape[0] == 1
        products = int(np.diff(lvl.A.indptr)[lvl.R.indices].sum())          # of the one row of R * A
        assert (products > 1024) == (name == "big_star_pmis")


def test_host_build_records_its_route(no_device):
    make, options, sizes, _ = tc.HIERARCHIES["line_pmis"]
    for device in (False, None):
        np.random.seed(0)
        ml = ruge_stuben_solver(make(), device=device, **options)
        assert [lvl.A.shape[0] for lvl in ml.levels] == sizes
        assert classical.LAST_BUILD["uploads"] == 0 and len(classical.LAST_BUILD["levels"]) == len(sizes) - 1
        assert all(not r["chained"] and not r["resident"] and r["reversed"] is None for r in classical.LAST_BUILD["levels"])


def test_chain_refuses_what_operator_order_refuses_before_the_library(no_device):
    import scipy.sparse as sps
    A = tc.HIERARCHIES["line_pmis"][0]()
    zero = A.copy(); zero.data[3] = 0.0
    nan = A.copy(); nan.data[5] = np.nan
    twice = sps.csr_matrix((np.array([2.0, -1.0, -1.0, 2.0, 1.0]), np.array([0, 1, 0, 1, 1], dtype=np.intc),
                            np.array([0, 2, 5], dtype=np.intc)), shape=(2, 2))
    state = np.random.get_state()
    for bad, what in ((zero, "stored zeros or non-finite"), (nan, "stored zeros or non-finite"), (twice, "duplicated columns")):
        with pytest.raises(NotImplementedError, match=what):
            ruge_stuben_solver(bad, CF="PMIS", max_coarse=1, device=True)
        assert classical.LAST_BUILD == {"uploads": 0, "levels": []}
    with pytest.raises(NotImplementedError, match="interpolation"):
        ruge_stuben_solver(A, CF="PMIS", max_coarse=1, device=True, interpolation="standard")
    with pytest.raises(ValueError, match="theta"):
        ruge_stuben_solver(A, strength=("classical", {"theta": 1.5}), CF="CLJP", max_coarse=1, device=True)
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state()[1:3], state[1:3]))     # nothing was drawn
