"""GPU: classical strength of connection and direct interpolation on the device (csrc/classical.hip) -- the flat
amg_core entries against every recorded native call of the reference, the device routes of pyamg_amd.classical against
its host routes, and whole PMIS / CLJP levels built in HBM against the host hierarchy and the reference's.  Everything
is compared on the raw bytes."""
import ctypes as C

import numpy as np
import pytest

import classical_io as cio
import golden_io
import splitting_io as sio
from pyamg_amd import _lib, amg_core, classical
from pyamg_amd.classical import ruge_stuben_solver

pytestmark = pytest.mark.gpu

POISON_I, POISON_X = -77, -7.5          # what the output arrays hold before a call


def _i(a):
    return np.array(a, dtype=np.intc)      # a writable contiguous copy


def _x(a):
    return np.array(a, dtype=np.float64)


class Device(object):
    """the flat entries behind the interface of classical_io.Model"""

    @staticmethod
    def strength(n, theta, Ap, Aj, Ax):
        Ap, Aj, Ax = _i(Ap), _i(Aj), _x(Ax)
        Sp, Sj, Sx = np.full(n + 1, POISON_I, dtype=np.intc), np.full(len(Aj), POISON_I, dtype=np.intc), np.full(len(Ax), POISON_X)
        amg_core.classical_strength_of_connection(n, theta, Ap, Aj, Ax, Sp, Sj, Sx)
        nnz = Sp[n]
        assert np.all(Sj[nnz:] == POISON_I) and np.all(Sx[nnz:] == POISON_X)         # nothing past the last entry
        return Sp, Sj[:nnz], Sx[:nnz]

    @staticmethod
    def maximum(n, Ap, Aj, Ax):
        x = np.full(n, POISON_X)
        amg_core.maximum_row_value(n, x, _i(Ap), _i(Aj), _x(Ax))
        return x

    @staticmethod
    def pass1(n, Sp, Sj, splitting):
        Bp = np.full(n + 1, POISON_I, dtype=np.intc)
        amg_core.rs_direct_interpolation_pass1(n, _i(Sp), _i(Sj), _i(splitting), Bp)
        return Bp

    @staticmethod
    def pass2(n, Ap, Aj, Ax, Sp, Sj, Sx, splitting, Bp):
        Bj, Bx = np.full(Bp[n], POISON_I, dtype=np.intc), np.full(Bp[n], POISON_X)
        amg_core.rs_direct_interpolation_pass2(n, _i(Ap), _i(Aj), _x(Ax), _i(Sp), _i(Sj), _x(Sx), _i(splitting), _i(Bp), Bj, Bx)
        return Bj, Bx


# ------------------------------------------------------------------------------------------------ flat entries
def test_flat_strength_and_row_maximum_on_the_recorded_cases():
    cio.check_setup_strength(Device, also_maximum=cio.Model)


def test_flat_interpolation_on_the_recorded_cases():
    cio.check_setup_interpolation(Device)


@pytest.mark.parametrize("case", cio.CASES)
def test_flat_entries_on_the_crafted_operators(case):
    assert cio.check_crafted(case, Device) == {"classical_strength_of_connection", "maximum_row_value",
                                               "rs_direct_interpolation_pass1", "rs_direct_interpolation_pass2"}


def test_no_rows_and_a_single_row():
    empty_i, empty_x = np.zeros(0, dtype=np.intc), np.zeros(0)
    Sp, Sj, Sx = Device.strength(0, 0.25, [0], empty_i, empty_x)
    assert cio.same_bits(Sp, np.zeros(1, dtype=np.intc)) and len(Sj) == 0 and len(Sx) == 0
    assert len(Device.maximum(0, [0], empty_i, empty_x)) == 0
    assert cio.same_bits(Device.pass1(0, [0], empty_i, empty_i), np.zeros(1, dtype=np.intc))
    Bj, Bx = Device.pass2(0, [0], empty_i, empty_x, [0], empty_i, empty_x, empty_i, [0])
    assert len(Bj) == 0 and len(Bx) == 0
    for Ap, Aj, Ax in (([0, 1], [0], [-0.0]), ([0, 0], [], []), ([0, 2], [0, 0], [3.0, -1.0])):
        for theta in (0.0, 1.0):
            for got, want in zip(Device.strength(1, theta, Ap, Aj, Ax), cio.Model.strength(1, theta, _i(Ap), _i(Aj), _x(Ax))):
                assert cio.same_bits(got, want), (Ap, theta)
        assert cio.same_bits(Device.maximum(1, Ap, Aj, Ax), cio.Model.maximum(1, _i(Ap), _i(Aj), _x(Ax)))
        for spl in ([0], [1]):
            Bp = Device.pass1(1, Ap, Aj, spl)
            assert cio.same_bits(Bp, cio.Model.pass1(1, _i(Ap), _i(Aj), _i(spl)))
            for got, want in zip(Device.pass2(1, Ap, Aj, Ax, Ap, Aj, Ax, spl, Bp),
                                 cio.Model.pass2(1, _i(Ap), _i(Aj), _x(Ax), _i(Ap), _i(Aj), _x(Ax), _i(spl), Bp)):
                assert cio.same_bits(got, want), (Ap, spl)


def test_bad_arrays_are_invalid_arguments():
    A = sio.poisson2d(5, 4)
    n = A.shape[0]
    Ap, Aj, Ax = _i(A.indptr), _i(A.indices), _x(A.data)
    ones = np.ones(n, dtype=np.intc)
    Bp = Device.pass1(n, Ap, Aj, ones)
    two = ones.copy()
    two[3] = 2
    down = Ap.copy()
    down[4] = down[3] - 1
    far = Aj.copy()
    far[7] = n
    late = Ap.copy()
    late[0] = 1
    before = _lib.live_buffers()
    with pytest.raises(ValueError, match="other than 0 and 1"):
        Device.pass1(n, Ap, Aj, two)
    with pytest.raises(ValueError, match="other than 0 and 1"):
        Device.pass2(n, Ap, Aj, Ax, Ap, Aj, Ax, two, Bp)
    for p, j, what in ((down, Aj, "decrease"), (Ap, far, "outside"), (late, Aj, "start at 0")):
        with pytest.raises(ValueError, match=what):
            Device.strength(n, 0.25, p, j, Ax)
        with pytest.raises(ValueError, match=what):
            Device.pass1(n, p, j, ones)
        with pytest.raises(ValueError, match=what):
            Device.pass2(n, p, j, Ax, Ap, Aj, Ax, ones, Bp)
        with pytest.raises(ValueError, match=what):
            Device.pass2(n, Ap, Aj, Ax, p, j, Ax, ones, Bp)
    with pytest.raises(ValueError, match=r"decrease|start at 0"):
        Device.maximum(n, down, Aj, Ax)
    with pytest.raises(ValueError, match="pass 1"):
        Device.pass2(n, Ap, Aj, Ax, Ap, Aj, Ax, ones, 2 * np.arange(n + 1))
    assert _lib.live_buffers() == before


# ------------------------------------------------------------------------------------------------ the two routes
def _splittings(name, S):
    """the recorded PMIS and CLJP splittings where the fixtures have them, the host route's otherwise, and RS"""
    if name in sio.PROBLEMS:
        p = sio.problem(name)
        out = {"PMIS": p["PMIS"], "CLJP": p["CLJP"]}
    else:
        np.random.seed(0)
        out = {"PMIS": classical.PMIS(S, device=False), "CLJP": classical.CLJP(S, device=False)}
    out["RS"] = classical.RS(S)
    return out


@pytest.mark.parametrize("name", ["poisson_17x23", "aniso_40x40", "wide_257c"])
def test_device_routes_equal_host_routes(name):
    A = cio.operator(name)
    for theta in (0.0, 0.25):
        host = classical.classical_strength_of_connection(A, theta, device=False)
        assert cio.same_csr(classical.classical_strength_of_connection(A, theta, device=True), host), theta
    S = classical.classical_strength_of_connection(A, 0.25, device=False)
    if name in sio.PROBLEMS:
        assert cio.same_csr(S, sio.problem(name)["S"])
    for tag, splitting in _splittings(name, S).items():
        assert 0 < splitting.sum() < len(splitting)
        host = classical.direct_interpolation(A, S, splitting, device=False)
        assert cio.same_csr(classical.direct_interpolation(A, S, splitting, device=True), host), tag


# ------------------------------------------------------------------------------------------------ whole levels
SIZES = {"PMIS": [1600, 593, 148, 34, 9], "CLJP": [1600, 978, 338, 122, 44, 17]}


@pytest.mark.parametrize("hier", sorted(sio.HIERARCHIES))
def test_levels_built_in_hbm_equal_the_host_hierarchy_and_the_reference(hier):
    g = sio.load_hier(hier)
    cf = sio.HIERARCHIES[hier]
    A = sio.poisson2d(40, 40)
    np.random.seed(0)
    host = ruge_stuben_solver(A, CF=cf, max_coarse=20, keep=True, device=False)
    before = _lib.live_buffers()
    np.random.seed(0)
    ml = ruge_stuben_solver(A, CF=cf, max_coarse=20, keep=True, device=True)
    assert _lib.live_buffers() == before
    assert [l.A.shape[0] for l in ml.levels] == SIZES[cf] and len(ml.levels) == g["meta"]["nlevels"]
    cio.same_hierarchy(ml, host)
    res = []
    ml.solve(g["b"], tol=g["meta"]["tol"], residuals=res)
    golden_io.assert_history(res, g["residuals"], g["levels"][0]["A"], g["x"], g["b"])


def test_a_single_level_with_and_without_the_strength_matrix():
    A = cio.operator("aniso_40x40")
    p = sio.problem("aniso_40x40")
    for cf in ("PMIS", "CLJP"):
        for keep in (False, True):
            times = []
            np.random.seed(0)
            splitting, P, S = classical.classical_level_device(A, 0.25, cf, keep=keep, times=times)
            assert cio.same_bits(splitting, p[cf])
            assert cio.same_csr(P, classical.direct_interpolation(A, p["S"], p[cf], device=False))
            assert (S is None) if not keep else cio.same_csr(S, p["S"])
            assert len(times) == len(classical.LEVEL_STAGES) and all(t >= 0 for t in times)


def test_rs_hierarchy_with_the_stages_on_the_device():
    A = sio.poisson2d(40, 40)
    host = ruge_stuben_solver(A, CF="RS", max_coarse=20, keep=True, device=False)
    ml = ruge_stuben_solver(A, CF="RS", max_coarse=20, keep=True, device=True)
    assert [l.A.shape[0] for l in ml.levels] == [1600, 800, 202, 52, 13]
    cio.same_hierarchy(ml, host)


def test_no_device_buffer_outlives_a_build_or_a_refusal():
    A = sio.poisson2d(12, 11)
    before = _lib.live_buffers()
    for cf in ("PMIS", "CLJP"):
        ruge_stuben_solver(A, CF=cf, max_coarse=10, device=True)
        assert _lib.live_buffers() == before
    zero = A.copy()
    zero.data[5] = 0.0
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        ruge_stuben_solver(zero, CF="PMIS", max_coarse=10, device=True)
    with pytest.raises(ValueError):
        classical.classical_level_device(A, 1.5, "CLJP")
    h = _lib.lib()
    handle, sizes = C.c_void_p(), (C.c_long * 2)()
    Ap, Aj, Ax = _i(A.indptr), _i(A.indices), _x(A.data)
    Aj[3] = A.shape[0]                     # refused by the library itself: nothing is left behind
    r = np.zeros(A.shape[0])
    rc = h.amg_classical_level_device(A.shape[0], Ap.ctypes.data, Aj.ctypes.data, Ax.ctypes.data, 0.25, 0, 0, r.ctypes.data,
                                      C.byref(handle), sizes, None, None)
    assert rc == _lib.AMG_EINVAL and not handle.value
    assert _lib.live_buffers() == before
