"""GPU: classical hierarchies built end to end in HBM (amg_classical_chain_*) --
ruge_stuben_solver(device=True) against device=False from the same seed on the hierarchies of transpose_cases, level by
level on the raw bytes; what classical.LAST_BUILD records about the route; the refusals (a refused product, a coarse
operator with a non-finite value); and the device allocations, which every path leaves where they were."""
import numpy as np
import pytest

import classical_io as cio
import transpose_cases as tc
from pyamg_amd import _lib, classical
from pyamg_amd.classical import ruge_stuben_solver

pytestmark = pytest.mark.gpu


def build(name, keep=True, device=True, **change):
    make, options, _, _ = tc.HIERARCHIES[name]
    np.random.seed(0)
    return ruge_stuben_solver(make(), keep=keep, device=device, **dict(options, **change))


def same_objects(ml, ref):
    """what same_hierarchy does not look at: index dtypes, shapes and the declared format flags of every operator"""
    for a, b in zip(ml.levels, ref.levels):
        for key in ("A", "P", "R"):
            if not hasattr(b, key):
                assert not hasattr(a, key)
                continue
            M, G = getattr(a, key), getattr(b, key)
            assert M.shape == G.shape and M.dtype == G.dtype
            assert M.indices.dtype == G.indices.dtype and M.indptr.dtype == G.indptr.dtype
            assert M.has_sorted_indices == G.has_sorted_indices and M.has_canonical_format == G.has_canonical_format


@pytest.mark.parametrize("name", sorted(tc.HIERARCHIES))
def test_chained_hierarchy_equals_the_host_hierarchy(name):
    _, _, sizes, coarse_sorted = tc.HIERARCHIES[name]
    host = tc.host_hierarchy(name)
    if sizes is not None:
        assert [lvl.A.shape[0] for lvl in host.levels] == sizes
    before = _lib.live_buffers()
    ml = build(name)
    record = {"uploads": classical.LAST_BUILD["uploads"], "levels": list(classical.LAST_BUILD["levels"])}
    assert _lib.live_buffers() == before
    cio.same_hierarchy(ml, host)
    same_objects(ml, host)
    built = len(host.levels) - 1
    assert record["uploads"] == 1 and len(record["levels"]) == built
    assert all(r["chained"] and r["resident"] for r in record["levels"])
    assert all(set(r["times"]) == set(classical.CHAIN_STAGES) and all(t >= 0 for t in r["times"].values()) for r in record["levels"])
    assert [r["reversed"] for r in record["levels"]] == [int(not tc.rows_sorted(lvl.A)) for lvl in host.levels[:-1]]
    if coarse_sorted is not None:
        assert [r["reversed"] for r in record["levels"]] == [0] + [int(not coarse_sorted)] * (built - 1)
    for r, lvl in zip(record["levels"], host.levels):
        t = r["transpose"]
        assert (t["lane_rows"], t["lds_rows"], t["hbm_rows"]) == tc.forms_of(lvl.P) and t["launched"] == 1
        assert all(p in ("lds", "hbm_wave", "hbm_thread") for p in r["products"])


def test_star_takes_the_long_row_forms():
    for name, form, product in (("star_pmis", "lds_rows", "lds"), ("star_cljp", "lds_rows", "lds"), ("big_star_pmis", "hbm_rows", "hbm_wave")):
        host = tc.host_hierarchy(name)
        assert host.levels[0].R.shape[0] == 1 and host.levels[0].R.nnz == host.levels[0].A.shape[0]
        ml = build(name)
        cio.same_hierarchy(ml, host)
        (record,) = classical.LAST_BUILD["levels"]
        assert record["transpose"][form] == 1 and record["transpose"]["lane_rows"] == 0
        assert record["products"][0] == product, record["products"]
    # the product the big star was sized for: its one row of R * A has more than 1024 products
    A = tc.host_hierarchy("big_star_pmis").levels[0].A
    assert A.nnz > 1024 and tc.host_hierarchy("star_pmis").levels[0].A.nnz <= 1024


@pytest.mark.parametrize("name", ["poisson_pmis", "poisson_cljp_ext4"])
def test_keep_does_not_change_the_operators(name):
    kept, plain = build(name, keep=True), build(name, keep=False)
    cio.same_hierarchy(plain, kept, keys=("A", "P", "R"))
    assert not hasattr(plain.levels[0], "C") and not hasattr(plain.levels[0], "splitting")
    cio.same_hierarchy(plain, tc.host_hierarchy(name, keep=False))


def test_per_level_route_is_still_reachable_and_equal(monkeypatch):
    monkeypatch.setattr(classical, "_RESIDENT_CHAIN", False)
    ml = build("poisson_pmis_ext")
    record = classical.LAST_BUILD
    assert record["uploads"] == len(ml.levels) - 1
    assert all(r["resident"] and not r["chained"] for r in record["levels"])
    cio.same_hierarchy(ml, tc.host_hierarchy("poisson_pmis_ext"))


def test_other_configurations_keep_their_routes():
    A = tc.HIERARCHIES["poisson_pmis"][0]()
    for options in (dict(CF="RS"), dict(CF="PMISc"), dict(CF=("PMIS", {"device": False})), dict(CF="CLJPc")):
        np.random.seed(0)
        ml = ruge_stuben_solver(A, max_coarse=20, device=True, **options)
        assert classical.LAST_BUILD["uploads"] == 0 and len(classical.LAST_BUILD["levels"]) == len(ml.levels) - 1
        assert not any(r["chained"] or r["resident"] for r in classical.LAST_BUILD["levels"])
        np.random.seed(0)
        cio.same_hierarchy(ml, ruge_stuben_solver(A, max_coarse=20, device=False, **options), keys=("A", "P", "R"))


@pytest.mark.parametrize("how", ["return_state", "entries_limit"])
def test_refused_product_finishes_the_level_on_the_host(monkeypatch, how):
    host = tc.host_hierarchy("poisson_pmis_ext")
    draws, calls = [], []
    rand = np.random.rand

    def counted(*shape):
        draws.append(shape)
        return rand(*shape)

    if how == "return_state":
        inner = classical._chain_level_call

        def refused_once(handle, *args):
            rc = inner(handle, *args)
            calls.append(rc)
            return _lib.CHAIN_PRODUCT_REFUSED if len(calls) == 2 else rc
        monkeypatch.setattr(classical, "_chain_level_call", refused_once)
        refused_levels = [1]
    else:
        # every coarse operator of more than 2000 entries counts as too large for the host's index arrays
        monkeypatch.setattr(classical, "_PRODUCT_ENTRIES_LIMIT", 2000)
        refused_levels = [k for k, lvl in enumerate(host.levels[1:]) if lvl.A.nnz >= 2000]
        assert refused_levels and len(refused_levels) < len(host.levels) - 1
    monkeypatch.setattr(np.random, "rand", counted)
    before = _lib.live_buffers()
    ml = build("poisson_pmis_ext")
    monkeypatch.setattr(np.random, "rand", rand)
    assert _lib.live_buffers() == before
    cio.same_hierarchy(ml, host)
    assert draws == [(lvl.A.shape[0],) for lvl in host.levels[:-1]]         # one draw per level, the refused one included
    record = classical.LAST_BUILD
    assert [k for k, r in enumerate(record["levels"]) if not r["chained"]] == refused_levels
    assert all(r["resident"] for r in record["levels"])
    # a new chain, and with it an upload, after every refused level that is not the last
    assert record["uploads"] == 1 + sum(1 for k in refused_levels if k + 1 < len(record["levels"]))


def test_non_finite_coarse_operator_is_refused_before_the_next_draw(monkeypatch):
    A = tc.HIERARCHIES["poisson_pmis"][0]()
    A = A * 4e307                      # 1.6e308 on the diagonal: finite, and the first coarse operator (entries up to 12 s) is not
    assert np.all(np.isfinite(A.data))
    np.random.seed(0)
    host = ruge_stuben_solver(A, CF="PMIS", max_coarse=20, device=False, max_levels=2)
    assert not np.all(np.isfinite(host.levels[1].A.data))
    draws = []
    rand = np.random.rand

    def counted(*shape):
        draws.append(shape)
        return rand(*shape)

    monkeypatch.setattr(np.random, "rand", counted)
    before = _lib.live_buffers()
    np.random.seed(0)
    with pytest.raises(NotImplementedError, match="stored zeros or non-finite values is outside the restated setup"):
        ruge_stuben_solver(A, CF="PMIS", max_coarse=20, device=True)
    assert draws == [(A.shape[0],)] and _lib.live_buffers() == before
    assert len(classical.LAST_BUILD["levels"]) == 1 and classical.LAST_BUILD["levels"][0]["chained"]
    # the level that produced the value is no error: with two levels the hierarchy is the host's
    np.random.seed(0)
    ml = ruge_stuben_solver(A, CF="PMIS", max_coarse=20, device=True, max_levels=2)
    monkeypatch.setattr(np.random, "rand", rand)
    cio.same_hierarchy(ml, host, keys=("A", "P", "R"))
    assert _lib.live_buffers() == before


def test_automatic_route_continues_on_the_host_after_a_non_finite_product(monkeypatch):
    monkeypatch.setattr(classical, "DEVICE_AUTO", True)
    A = tc.HIERARCHIES["poisson_pmis"][0]() * 4e307
    np.random.seed(0)
    with np.errstate(all="ignore"):
        host = ruge_stuben_solver(A, CF="PMIS", max_coarse=20, device=False, max_levels=3)
        before = _lib.live_buffers()
        np.random.seed(0)
        ml = ruge_stuben_solver(A, CF="PMIS", max_coarse=20, device=None, max_levels=3)
    assert _lib.live_buffers() == before
    cio.same_hierarchy(ml, host, keys=("A", "P", "R"))
    assert [r["chained"] for r in classical.LAST_BUILD["levels"]] == [True, False]


def test_exception_between_level_and_fetch_releases_the_chain(monkeypatch):
    inner = classical._chain_level_call

    def fails_after(handle, *args):
        inner(handle, *args)
        raise RuntimeError("between the level and its fetch")

    monkeypatch.setattr(classical, "_chain_level_call", fails_after)
    before = _lib.live_buffers()
    with pytest.raises(RuntimeError, match="between the level"):
        build("poisson_pmis")
    assert _lib.live_buffers() == before


def test_c_entries_refuse_bad_arguments_and_release_everything():
    import ctypes as C
    L = _lib.lib()
    A = tc.HIERARCHIES["line_pmis"][0]()
    n = A.shape[0]
    Ap, Aj, Ax = A.indptr.astype(np.intc), A.indices.astype(np.intc), A.data.astype(np.float64)
    before = _lib.live_buffers()
    handle = C.c_void_p()
    bad_j = Aj.copy(); bad_j[3] = n
    twice = Aj.copy(); twice[1] = twice[0]
    for cols in (bad_j, twice):
        assert L.amg_classical_chain_begin(n, Ap.ctypes.data, cols.ctypes.data, Ax.ctypes.data, 0, C.byref(handle)) == _lib.AMG_EINVAL
        assert not handle.value and _lib.live_buffers() == before
    assert L.amg_classical_chain_begin(0, Ap.ctypes.data, Aj.ctypes.data, Ax.ctypes.data, 0, C.byref(handle)) == _lib.AMG_EINVAL
    assert L.amg_classical_chain_begin(n, Ap.ctypes.data, Aj.ctypes.data, Ax.ctypes.data, 0, C.byref(handle)) == 0 and handle.value
    sizes, flags, r = (C.c_long * 5)(), (C.c_int * _lib.CHAIN_FLAG_FIELDS)(), np.random.RandomState(0).rand(n)
    held = _lib.live_buffers()
    assert held > before
    for theta, kind, interp, q in ((1.5, 0, 0, 0), (0.25, 2, 0, 0), (0.25, 0, 2, 0), (0.25, 0, 0, 3), (0.25, 0, 1, -1)):
        assert L.amg_classical_chain_level(handle, theta, kind, r.ctypes.data, interp, q, sizes, flags, None, None) == _lib.AMG_EINVAL
        assert _lib.live_buffers() == held
    nothing = [None] * 13
    assert L.amg_classical_chain_fetch(handle, *nothing, None) == _lib.AMG_ESTATE          # no level built yet
    assert L.amg_classical_chain_level(handle, 0.25, 0, r.ctypes.data, 0, 0, sizes, flags, None, None) == 0
    assert _lib.live_buffers() > held and sizes[4] == 21 and flags[0] == 1 and flags[1] == 1
    assert L.amg_classical_chain_level(handle, 0.25, 0, r.ctypes.data, 0, 0, sizes, flags, None, None) == _lib.AMG_ESTATE
    assert L.amg_classical_chain_fetch(handle, *nothing, None) == _lib.AMG_EINVAL          # null arrays: the level is released
    assert _lib.live_buffers() == held
    L.amg_classical_chain_free(handle)
    L.amg_classical_chain_free(None)
    assert _lib.live_buffers() == before


def test_chained_solver_solves_like_the_host_built_one():
    host, ml = tc.host_hierarchy("poisson_pmis_ext"), build("poisson_pmis_ext")
    b = np.random.RandomState(3).rand(host.levels[0].A.shape[0])
    res_host, res = [], []
    x_host = host.solve(b, tol=1e-8, residuals=res_host)
    x = ml.solve(b, tol=1e-8, residuals=res)
    assert len(res) == len(res_host) and res[-1] <= 1e-8 * res[0]
    assert cio.same_bits(x, x_host) and cio.same_bits(np.array(res), np.array(res_host))
