"""The resident smoothed-aggregation chain against the per-stage device route and the host route:
the same hierarchy bit for bit -- formats, index dtypes, entry order, candidates, residual histories and the position of
numpy's global RNG -- from one upload."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import scipy.sparse as sps

import prolong_cases as pc
import sa_chain_cases as sc
from pyamg_amd import _lib, aggregation

pytestmark = pytest.mark.gpu


def _live():
    """the library's live device buffers once the collector has run: a solver frees its resident hierarchy when it goes,
    and what earlier tests left for the collector must not count for or against this one"""
    gc.collect()
    return _lib.live_buffers()


def _solve(ml):
    b = np.random.RandomState(2).rand(ml.levels[0].A.shape[0])
    res = []
    ml.solve(b, tol=1e-10, residuals=res)
    return res


def _built(name, keep, **route):
    ml = sc.build(name, keep=keep, **route)
    state = np.random.get_state()
    return ml, state, [dict(rec) for rec in aggregation.LAST_BUILD["levels"]], aggregation.LAST_BUILD["uploads"]


@functools.lru_cache(maxsize=None)
def _host(name, keep):
    """the reference of a case, built once: (hierarchy, RNG state, residual history)"""
    ml, state, _, _ = _built(name, keep, device=False, fast=False)
    return ml, state, _solve(ml)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _same_hierarchy(got, want, keep):
    assert len(got.levels) == len(want.levels)
    for lg, lw in zip(got.levels, want.levels):
        for what in ("A", "P", "R") + (("C", "AggOp", "T") if keep else ()):
            assert hasattr(lg, what) == hasattr(lw, what), what
            if hasattr(lg, what):
                assert pc.same_matrix(getattr(lg, what), getattr(lw, what)), what
        assert lg.B.dtype == lw.B.dtype and lg.B.shape == lw.B.shape and np.array_equal(lg.B, lw.B)
    assert got.levels[-1].A.symmetry == want.levels[-1].A.symmetry


@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep"])
@pytest.mark.parametrize("name", sc.MULTI_LEVEL)
def test_chain_equals_the_stage_route_and_the_host(name, keep, monkeypatch):
    host, host_state, host_res = _host(name, keep)
    live = _live()                          # (the cached reference keeps its solver's buffers)
    assert tuple(lvl.A.shape[0] for lvl in host.levels) == sc.cases()[name][2]
    chain, chain_state, records, uploads = _built(name, keep, device=True)
    assert uploads == 1 and len(records) == len(host.levels) - 1
    assert all(rec["chained"] and rec["resident"] and rec["stopped"] is None for rec in records), records
    theta = dict(sc.cases()[name][1].get("strength", ("symmetric", {}))[1]).get("theta", 0)
    later = _lib.SA_STRENGTH_SQUARED if theta else _lib.SA_STRENGTH_ONES
    assert [rec["strength_mode"] for rec in records] == [_lib.SA_STRENGTH_CSR] + [later] * (len(records) - 1)
    assert all(set(rec["times"]) == set(aggregation.CHAIN_STAGES) and min(rec["times"].values()) >= 0.0 for rec in records)
    # the sort runs where the rows are not sorted: level 0 of the reversed case only, and level 1, whose operator is in
    # the order its product left it (rows of 42 and 78 entries in the two 12^3 cases: the wave form of the sort)
    assert (records[0]["times"]["sort"] > 0.0) == (name == "reversed_rows")
    assert records[1]["times"]["sort"] > 0.0
    monkeypatch.setattr(aggregation, "_RESIDENT_CHAIN", False)
    stage, stage_state, stage_records, stage_uploads = _built(name, keep, device=True)
    assert stage_uploads == 0 and not any(rec["chained"] or rec["resident"] for rec in stage_records)
    _same_hierarchy(chain, host, keep)
    _same_hierarchy(stage, host, keep)
    assert _same_state(chain_state, host_state) and _same_state(stage_state, host_state)
    assert _solve(chain) == host_res and _solve(stage) == host_res and len(host_res) > 2
    del chain, stage
    assert _live() == live


@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep"])
def test_level_without_an_aggregate_goes_to_the_stage_route(keep):
    host, host_state, host_res = _host("no_aggregate", keep)
    live = _live()                          # (the cached reference keeps its solver's buffers)
    assert tuple(lvl.A.shape[0] for lvl in host.levels) == (900, 130, 1)
    assert host.levels[1].P.shape == (130, 1) and host.levels[1].P.nnz == 0
    chain, chain_state, records, uploads = _built("no_aggregate", keep, device=True)
    assert uploads == 1
    assert [(rec["chained"], rec["stopped"]) for rec in records] == [(True, None), (False, "no aggregate")]
    _same_hierarchy(chain, host, keep)
    assert _same_state(chain_state, host_state)             # nothing was drawn twice
    assert _solve(chain) == host_res
    del chain
    assert _live() == live


@pytest.mark.parametrize("name", ["poisson_30x30_theta", "reversed_rows"])
def test_refused_product_is_finished_on_the_host(name, monkeypatch):
    host, host_state, host_res = _host(name, True)
    live = _live()                          # (the cached reference keeps its solver's buffers)
    real = aggregation._chain_level_call
    calls = []

    def refusing(handle, *args):
        rc = real(handle, *args)
        calls.append(rc)
        return _lib.CHAIN_PRODUCT_REFUSED if len(calls) == 1 else rc

    monkeypatch.setattr(aggregation, "_chain_level_call", refusing)
    chain, chain_state, records, uploads = _built(name, True, device=True)
    # the first level's product came from the host and ended its chain; the next level began another
    assert calls[0] == 0 and uploads == 2
    assert [(rec["chained"], rec["resident"]) for rec in records] == [(False, True)] + [(True, True)] * (len(records) - 1)
    _same_hierarchy(chain, host, True)
    assert _same_state(chain_state, host_state)
    assert _solve(chain) == host_res
    del chain
    assert _live() == live


OFF = {"device": False}
JACOBI = ("jacobi", {"omega": 4.0 / 3.0})


@pytest.mark.parametrize("change", [
    {"aggregate": ["mis", ("mis", OFF), "mis"]},
    {"smooth": [JACOBI, ("jacobi", dict(JACOBI[1], **OFF)), JACOBI]},
    {"strength": [("symmetric", {"theta": 0.02}), ("symmetric", dict(OFF, theta=0.02)), ("symmetric", {"theta": 0.02})]},
], ids=lambda c: "-".join(c))
def test_level_taken_off_the_chain_ends_it_and_the_next_begins_another(change, monkeypatch):
    """per-level options that send a stage of level 1 to the host: level 0 is chained, level 1 is built by the stage
    routes, and level 2 must not run on the operator the first chain left in HBM (A_1, 130 rows, where the host has A_2
    with 24)"""
    A, options, sizes = sc.cases()["poisson_30x30_theta"]
    assert len(sizes) == 4
    options = dict({"aggregate": "mis"}, **options)
    options.update(change)

    def built(**route):
        np.random.seed(sc.SEED)
        ml = aggregation.smoothed_aggregation_solver(A.copy(), max_coarse=sc.MAX_COARSE, keep=True, **options, **route)
        return ml, np.random.get_state(), [dict(rec) for rec in aggregation.LAST_BUILD["levels"]], aggregation.LAST_BUILD["uploads"]

    host, host_state, _, _ = built(device=False, fast=False)
    assert tuple(lvl.A.shape[0] for lvl in host.levels) == sizes
    host_res = _solve(host)
    live = _live()
    chain, chain_state, records, uploads = built(device=True)
    assert uploads == 2
    assert [(rec["chained"], rec["resident"]) for rec in records] == [(True, True), (False, False), (True, True)]
    assert records[2]["strength_mode"] == _lib.SA_STRENGTH_SQUARED
    monkeypatch.setattr(aggregation, "_RESIDENT_CHAIN", False)
    stage, stage_state, _, stage_uploads = built(device=True)
    assert stage_uploads == 0
    _same_hierarchy(chain, stage, True)
    _same_hierarchy(chain, host, True)
    assert _same_state(chain_state, stage_state) and _same_state(chain_state, host_state)
    assert _solve(chain) == host_res == _solve(stage)
    del chain, stage
    assert _live() == live


def test_unsymmetric_pattern_raises_on_both_device_routes(monkeypatch):
    live = _live()
    with pytest.raises(ValueError, match="expected a structurally symmetric pattern"):
        sc.build("one_sided", device=True)
    assert aggregation.LAST_BUILD["uploads"] == 1           # (it was the chain that raised)
    monkeypatch.setattr(aggregation, "_RESIDENT_CHAIN", False)
    with pytest.raises(ValueError, match="expected a structurally symmetric pattern"):
        sc.build("one_sided", device=True)
    assert aggregation.LAST_BUILD["uploads"] == 0
    assert _live() == live


def test_column_twice_is_answered_by_the_stage_route(monkeypatch):
    """a chain refusal before anything is drawn: the level goes where it goes today -- whatever that route returns or
    raises -- and the next one is chained"""
    A = sc.cases()["poisson_30x30"][0]
    # row 0 holds column 1 twice, the second time as a stored zero: the pattern stays symmetric
    Ap = A.indptr.copy()
    Ap[1:] += 1
    twice = sps.csr_matrix((np.insert(A.data, 2, 0.0), np.insert(A.indices, 2, 1), Ap), shape=A.shape)
    live = _live()

    def build():
        np.random.seed(sc.SEED)
        try:
            ml = aggregation.smoothed_aggregation_solver(twice.copy(), aggregate="mis", max_coarse=sc.MAX_COARSE, device=True)
            return ml, None, np.random.get_state()
        except Exception as e:      # noqa: BLE001 -- compared below
            return None, (type(e), str(e)), None

    got = build()
    records = [dict(rec) for rec in aggregation.LAST_BUILD["levels"]]
    monkeypatch.setattr(aggregation, "_RESIDENT_CHAIN", False)
    want = build()
    assert (got[0] is None) == (want[0] is None) and got[1] == want[1]
    if got[0] is not None:
        _same_hierarchy(got[0], want[0], False)
        assert _same_state(got[2], want[2])
        assert not records[0]["chained"] and all(rec["chained"] for rec in records[1:])
    del got, want
    assert _live() == live


def test_second_level_call_without_a_fetch_is_a_state_error():
    live = _live()
    A = sc.cases()["poisson_30x30"][0]
    n = A.shape[0]
    L = _lib.lib()
    B = np.ones(n)
    y = np.random.RandomState(1).rand(n)
    dinv = 1.0 / A.diagonal()
    handle = C.c_void_p()
    _lib.check(L.amg_sa_chain_begin(n, A.indptr.ctypes.data, A.indices.ctypes.data, A.data.ctypes.data, B.ctypes.data, C.byref(handle)))
    try:
        sizes, flags = (C.c_long * 5)(), (C.c_int * _lib.SA_CHAIN_FLAG_FIELDS)()

        def level(rows=n):
            return L.amg_sa_chain_level(handle, rows, 0.0, _lib.SA_STRENGTH_CSR, y.ctypes.data, dinv.ctypes.data, 0.5, 1, None, 1e-10, sizes,
                                        flags, None, None)
        assert L.amg_sa_chain_fetch(handle, *([None] * 15), None) == _lib.AMG_ESTATE        # nothing built yet
        assert level() == 0
        first = [int(v) for v in sizes]
        assert level() == _lib.AMG_ESTATE
        assert level(n - 1) == _lib.AMG_EINVAL      # another size than the resident operator's: nothing is read
        assert L.amg_sa_chain_fetch(handle, *([None] * 15), None) == _lib.AMG_EINVAL        # a fetch without arrays drops the level
        assert level() == 0 and [int(v) for v in sizes] == first                            # ... and keeps the operator
        assert 0 < first[4] < n and first[0] == A.nnz and first[1] == n and flags[2] == 1 and flags[3] == 0
    finally:
        L.amg_sa_chain_free(handle)
    assert _live() == live
