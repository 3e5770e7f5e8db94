"""GPU: extended+i interpolation on the device (csrc/classical.hip) -- the device route against the
host route and the model on every designed case of extended_io, with and without truncation; PMIS hierarchies built with
device=True against device=False; the level chained in HBM against the stages one by one; and the argument errors of
the C entry.  Everything is compared on the raw bytes."""
import ctypes as C

import numpy as np
import pytest

import classical_io as cio
import extended_io as xio
import splitting_io as sio
from pyamg_amd import _lib, classical
from pyamg_amd.classical import extended_interpolation, ruge_stuben_solver

pytestmark = pytest.mark.gpu

POISON_I = -77
INTERPOLATIONS = {"full": "extended_i", "4_per_row": ("extended_i", {"max_per_row": 4})}


@pytest.mark.parametrize("name", sorted(xio.CASES))
def test_device_route_equals_host_route_and_model(name):
    A, S, spl, check, want, trace = xio.case(name)
    check(trace)
    before = _lib.live_buffers()
    for q in xio.QS:
        host = extended_interpolation(A, S, spl, max_per_row=q, device=False)
        dev = extended_interpolation(A, S, spl, max_per_row=q, device=True)
        assert dev.shape == host.shape
        assert xio.same_arrays(xio.arrays_of(dev), xio.arrays_of(host)), (name, q)
        assert xio.same_arrays(xio.arrays_of(dev), want[q]), (name, q)
    assert _lib.live_buffers() == before


def test_the_workspace_path_is_taken():
    """what the wide cases are for: F rows with more candidate slots than the LDS path holds, beside rows below it"""
    for name in ("wide", "wide_full"):
        A, S, spl, *_ = xio.case(name)
        rows = [xio.slots(S, spl, i) for i in range(A.shape[0]) if spl[i] == 0]
        assert max(rows) > 256
    A, S, spl, *_ = xio.case("wide")
    assert min(xio.slots(S, spl, i) for i in range(A.shape[0]) if spl[i] == 0) <= 256


@pytest.mark.parametrize("kind", sorted(INTERPOLATIONS))
@pytest.mark.parametrize("problem", ["poisson_40x40", "aniso_40x40"])
def test_pmis_hierarchy_on_the_device_equals_the_host_hierarchy(problem, kind):
    A = sio.poisson2d(40, 40) if problem == "poisson_40x40" else xio.aniso()
    np.random.seed(0)
    host = ruge_stuben_solver(A, CF="PMIS", max_coarse=20, keep=True, device=False, interpolation=INTERPOLATIONS[kind])
    before = _lib.live_buffers()
    np.random.seed(0)
    ml = ruge_stuben_solver(A, CF="PMIS", max_coarse=20, keep=True, device=True, interpolation=INTERPOLATIONS[kind])
    assert _lib.live_buffers() == before
    assert len(ml.levels) > 3
    cio.same_hierarchy(ml, host)


@pytest.mark.parametrize("q", [None, 4])
def test_chained_level_equals_the_stages(q):
    """levels 0 and 1 of the Poisson hierarchy (sorted rows, and rows as the Galerkin product leaves them): the level
    chained in HBM, the stages one by one on the device, and the host"""
    choice = "extended_i" if q is None else ("extended_i", {"max_per_row": q})
    np.random.seed(0)
    host = ruge_stuben_solver(sio.poisson2d(40, 40), CF="PMIS", max_coarse=20, keep=True, device=False, interpolation=choice)
    for lvl in host.levels[:2]:
        np.random.seed(5)
        splitting, P, S = classical.classical_level_device(lvl.A, 0.25, "PMIS", keep=True, product_order=True, interpolation=choice)
        np.random.seed(5)
        Cm, spl2, P2 = classical._stages(lvl.A, ("classical", {"theta": 0.25}), ("PMIS", {"device": True}), True, choice)
        assert cio.same_bits(splitting, spl2) and cio.same_csr(S, Cm)
        assert P.shape == P2.shape and cio.same_csr(P, P2)
        assert cio.same_csr(P, extended_interpolation(lvl.A, Cm, splitting, max_per_row=q, device=False))


def test_argument_errors_of_the_c_entry_leave_the_outputs_untouched():
    A, S, spl, *_ = xio.case("signs")
    n = A.shape[0]
    i32 = lambda a: np.array(a, dtype=np.intc)
    good = dict(Ap=i32(A.indptr), Aj=i32(A.indices), Ax=np.array(A.data, dtype=np.float64), Sp=i32(S.indptr), Sj=i32(S.indices),
                spl=i32(spl), q=0)

    def call(**change):
        a = dict(good, **change)
        Pp = np.full(n + 1, POISON_I, dtype=np.intc)
        handle = C.c_void_p()
        rc = _lib.lib().amg_extended_interpolation_device(n, a["Ap"].ctypes.data, a["Aj"].ctypes.data, a["Ax"].ctypes.data,
                                                          a["Sp"].ctypes.data, a["Sj"].ctypes.data, a["spl"].ctypes.data, a["q"],
                                                          Pp.ctypes.data, C.byref(handle), None)
        return rc, Pp, handle

    def edited(a, at, value):
        a = a.copy()
        a[at] = value
        return a

    before = _lib.live_buffers()
    down = edited(good["Ap"], 2, good["Ap"][1] - 1)
    twice_A, twice_S = edited(good["Aj"], 1, good["Aj"][0]), edited(good["Sj"], 1, good["Sj"][0])
    for change, what in ((dict(Ap=down), "decrease"), (dict(Sp=edited(good["Sp"], 2, good["Sp"][1] - 1)), "decrease"),
                         (dict(Aj=edited(good["Aj"], 3, n)), "outside"), (dict(Sj=edited(good["Sj"], 3, n)), "outside"),
                         (dict(spl=edited(good["spl"], 2, 2)), "other than 0 and 1"), (dict(Aj=twice_A), "twice"),
                         (dict(Sj=twice_S), "twice"), (dict(q=-1), "max_per_row")):
        rc, Pp, handle = call(**change)
        assert rc == _lib.AMG_EINVAL and not handle.value and np.all(Pp == POISON_I), what
        with pytest.raises(ValueError, match=what):
            _lib.check(rc)
    assert _lib.live_buffers() == before
    rc, Pp, handle = call()
    assert rc == 0 and handle.value and Pp[0] == 0
    Pj, Px = np.empty(Pp[-1], dtype=np.intc), np.empty(Pp[-1])
    assert _lib.lib().amg_extended_interpolation_fetch(handle, Pj.ctypes.data, Px.ctypes.data) == 0
    assert xio.same_arrays((Pp, Pj, Px), xio.case("signs")[4][None])
    assert _lib.live_buffers() == before
    # the chained entry refuses a column stored twice when it is asked for extended+i
    sizes, r = (C.c_long * 2)(), np.zeros(n)
    rc = _lib.lib().amg_classical_level_build(n, good["Ap"].ctypes.data, twice_A.ctypes.data, good["Ax"].ctypes.data, 0.25, 0, 0,
                                              r.ctypes.data, 1, 0, C.byref(handle), sizes, None, None)
    assert rc == _lib.AMG_EINVAL and not handle.value and _lib.live_buffers() == before
