"""CPU: the classical setup stages with a device route (pyamg_amd.classical, pyamg_amd.amg_core): names and argument
lists, the checks made before the device library is touched, the host routes against today's results, the equality
the device route of interpolation rests on, and the numpy models of the two kernels (classical_io.Model) against every
recorded native call of the reference."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sps

import classical_io as cio
import splitting_io as sio
from pyamg_amd import _host, amg_core, classical
from pyamg_amd._host import dp as _dp, ip as _ip

FLAT = {"classical_strength_of_connection": ["n_row", "theta", "Ap", "Aj", "Ax", "Sp", "Sj", "Sx"],
        "maximum_row_value": ["n_row", "x", "Ap", "Aj", "Ax"],
        "rs_direct_interpolation_pass1": ["n_nodes", "Sp", "Sj", "splitting", "Bp"],
        "rs_direct_interpolation_pass2": ["n_nodes", "Ap", "Aj", "Ax", "Sp", "Sj", "Sx", "splitting", "Bp", "Bj", "Bx"]}


class Host(object):
    """the host restatements of csrc/setup_host.cpp behind the interface of classical_io.Model"""

    @staticmethod
    def strength(n, theta, Ap, Aj, Ax):
        Ap, Aj, Ax = np.ascontiguousarray(Ap, np.intc), np.ascontiguousarray(Aj, np.intc), np.ascontiguousarray(Ax, np.float64)
        Sp = np.empty(n + 1, dtype=np.intc); Sj = np.empty_like(Aj); Sx = np.empty_like(Ax)
        nnz = _host.host_lib().amgsetup_classical_strength(n, float(theta), _ip(Ap), _ip(Aj), _dp(Ax), _ip(Sp), _ip(Sj), _dp(Sx))
        return Sp, Sj[:nnz], Sx[:nnz]

    @staticmethod
    def pass1(n, Sp, Sj, splitting):
        Sp, Sj, splitting = (np.ascontiguousarray(a, np.intc) for a in (Sp, Sj, splitting))
        Bp = np.empty(n + 1, dtype=np.intc)
        _host.host_lib().amgsetup_rs_direct_interpolation_pass1(n, _ip(Sp), _ip(Sj), _ip(splitting), _ip(Bp))
        return Bp

    @staticmethod
    def pass2(n, Ap, Aj, Ax, Sp, Sj, Sx, splitting, Bp):
        Ap, Aj, Sp, Sj, splitting, Bp = (np.ascontiguousarray(a, np.intc) for a in (Ap, Aj, Sp, Sj, splitting, Bp))
        Ax, Sx = np.ascontiguousarray(Ax, np.float64), np.ascontiguousarray(Sx, np.float64)
        Bj = np.empty(Bp[n], dtype=np.intc); Bx = np.empty(Bp[n], dtype=np.float64)
        _host.host_lib().amgsetup_rs_direct_interpolation_pass2(n, _ip(Ap), _ip(Aj), _dp(Ax), _ip(Sp), _ip(Sj), _dp(Sx),
                                                                _ip(splitting), _ip(Bp), _ip(Bj), _dp(Bx))
        return Bj, Bx

    maximum = staticmethod(cio.Model.maximum)       # the host library has no maximum_row_value


def _untouchable(monkeypatch):
    from pyamg_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(_lib, "device_count", touched)


def test_the_four_entries_are_in_the_table_with_the_reference_argument_lists():
    from pyamg_amd import _lib
    for name, args in FLAT.items():
        assert name in amg_core.__all__ and name in _lib.FLAT_TABLE and name in _lib.FLAT_F64_ONLY
        assert list(inspect.signature(getattr(amg_core, name)).parameters) == args
        assert len(_lib.FLAT_TABLE[name][0]) == len(args) and _lib.FLAT_TABLE[name][1] is True
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(classical.classical_strength_of_connection) == ["A", "theta", "device"]
    assert sig(classical.direct_interpolation) == ["A", "Cm", "splitting", "device"]
    assert inspect.signature(classical.ruge_stuben_solver).parameters["device"].default is None
    assert classical.DEVICE_AUTO is False
    assert "run on the host.  Other" not in classical.__doc__


def test_flat_entries_check_dtypes_and_layout_before_the_library(monkeypatch):
    _untouchable(monkeypatch)
    A = sio.poisson2d(5, 4)
    n = A.shape[0]
    Ap, Aj, Ax = A.indptr, A.indices, A.data.astype(np.float64)
    Sp, Sj, Sx = np.empty_like(Ap), np.empty_like(Aj), np.empty_like(Ax)
    spl, x = np.ones(n, dtype=np.intc), np.empty(n)
    good = {"classical_strength_of_connection": [n, 0.25, Ap, Aj, Ax, Sp, Sj, Sx],
            "maximum_row_value": [n, x, Ap, Aj, Ax],
            "rs_direct_interpolation_pass1": [n, Ap, Aj, spl, Sp],
            "rs_direct_interpolation_pass2": [n, Ap, Aj, Ax, Ap, Aj, Ax, spl, Sp, Sj, Sx]}
    for name, args in good.items():
        fn = getattr(amg_core, name)
        arrays = [k for k, a in enumerate(args) if isinstance(a, np.ndarray)]
        for k in arrays:
            wide = list(args)
            if args[k].dtype == np.intc:
                wide[k] = args[k].astype(np.int64)
                with pytest.raises(NotImplementedError, match="overloaded function"):
                    fn(*wide)
            else:
                wide[k] = args[k].astype(np.float32)
                with pytest.raises(NotImplementedError, match="overloaded function"):
                    fn(*wide)
            strided = list(args)
            strided[k] = np.repeat(args[k], 2)[::2]
            assert not strided[k].flags.c_contiguous
            with pytest.raises(TypeError, match="contiguous"):
                fn(*strided)
        with pytest.raises(TypeError):
            fn(*args[:-1])


def _refused(A):
    S = classical.classical_strength_of_connection(sps.csr_matrix(A), 0.25, device=False)
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        classical.classical_strength_of_connection(A, 0.25, device=True)
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        classical.direct_interpolation(A, S, np.ones(A.shape[0], dtype=np.intc), device=True)
    with pytest.raises(NotImplementedError, match="outside the restated setup"):
        classical.classical_level_device(A, 0.25, "PMIS")
    for cf in ("PMIS", "CLJP", "RS"):
        with pytest.raises(NotImplementedError, match="outside the restated setup"):
            classical.ruge_stuben_solver(A, CF=cf, max_coarse=5, device=True)


def test_device_true_refuses_before_the_library_is_touched(monkeypatch):
    import warnings
    _untouchable(monkeypatch)
    A = sio.poisson2d(6, 7)
    unsorted = A.copy()
    lo, hi = unsorted.indptr[3], unsorted.indptr[4]
    unsorted.indices[lo:hi] = unsorted.indices[lo:hi][::-1].copy()
    unsorted.data[lo:hi] = unsorted.data[lo:hi][::-1].copy()
    unsorted = sps.csr_matrix((unsorted.data, unsorted.indices, unsorted.indptr), shape=A.shape)
    assert not unsorted.has_sorted_indices
    doubled = sps.csr_matrix((np.r_[A.data, 1.0], np.r_[A.indices, A.indices[-1]].astype(np.intc),
                              np.r_[A.indptr[:-1], A.indptr[-1] + 1].astype(np.intc)), shape=A.shape)
    zero = A.copy()
    zero.data[1] = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for bad in (unsorted, doubled, zero):
            if bad is unsorted:                  # rows that are not sorted are the solver's own coarse operators
                with pytest.raises(NotImplementedError, match="outside the restated setup"):
                    classical.classical_strength_of_connection(bad, 0.25, device=True)
                with pytest.raises(NotImplementedError, match="outside the restated setup"):
                    classical.direct_interpolation(bad, bad, np.ones(bad.shape[0], dtype=np.intc), device=True)
                with pytest.raises(NotImplementedError, match="outside the restated setup"):
                    classical.classical_level_device(bad, 0.25, "CLJP")
            else:
                _refused(bad)
        for fmt in ("csc", "coo"):
            with pytest.raises(NotImplementedError, match="outside the restated setup"):
                classical.classical_strength_of_connection(A.asformat(fmt), 0.25, device=True)
            with pytest.raises(NotImplementedError, match="outside the restated setup"):
                classical.direct_interpolation(A.asformat(fmt), A, np.ones(A.shape[0], dtype=np.intc), device=True)
    with pytest.raises(ValueError, match="theta"):
        classical.classical_strength_of_connection(A, 1.5, device=False)


def _todays_interpolation(A, Cm, splitting):
    """direct_interpolation as it stood before it had routes"""
    Cm = Cm.copy()
    Cm.data[:] = 1.0
    Cm = sps.csr_matrix(Cm.multiply(A))
    n = A.shape[0]
    Pp = Host.pass1(n, Cm.indptr, Cm.indices, splitting)
    Pj, Px = Host.pass2(n, A.indptr, A.indices, A.data, Cm.indptr, Cm.indices, Cm.data, splitting, Pp)
    return sps.csr_matrix((Px, Pj, Pp))


@pytest.mark.parametrize("name", ["poisson_17x23", "aniso_40x40"])
def test_host_routes_return_todays_results(name, monkeypatch):
    from pyamg_amd import _lib
    A = cio.operator(name)
    p = sio.problem(name)
    S0 = classical.classical_strength_of_connection(A, 0.25)
    assert cio.same_csr(S0, p["S"])                         # the recorded strength matrix of the reference
    Sp, Sj, Sx = cio.strength_of(A, 0.25, Host)
    assert cio.same_bits(S0.indptr, Sp) and cio.same_bits(S0.indices, Sj)
    assert cio.same_bits(S0.data, np.abs(Sx) / np.repeat(np.maximum.reduceat(np.abs(Sx), Sp[:-1]), np.diff(Sp)))
    monkeypatch.setattr(classical, "DEVICE_AUTO", True)
    monkeypatch.setattr(_lib, "device_count", lambda: 0)    # device=None without a GPU

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    for device in (False, None):
        assert cio.same_csr(classical.classical_strength_of_connection(A, 0.25, device=device), S0)
        for tag in ("PMIS", "CLJP"):
            want = _todays_interpolation(A, S0, p[tag])
            assert cio.same_csr(classical.direct_interpolation(A, S0, p[tag], device=device), want), (device, tag)
        rs = classical.RS(S0)
        assert cio.same_csr(classical.direct_interpolation(A, S0, rs, device=device), _todays_interpolation(A, S0, rs))


@pytest.mark.parametrize("name", ["poisson_17x23", "aniso_40x40", "wide_257c"])
def test_values_on_the_pattern_equal_the_elementwise_product(name):
    """what the device route of interpolation rests on: for a canonical A, A's values at S's positions in S's order are
    C.multiply(A); for the rows scipy's product leaves unsorted, each row of S reversed"""
    A = cio.operator(name)
    S = classical.classical_strength_of_connection(A, 0.25)
    ones = S.copy()
    ones.data[:] = 1.0
    M = sps.csr_matrix(ones.multiply(A))
    Sp, Sj, Sx = cio.strength_of(A, 0.25, Host)              # the raw values the strength kernel writes
    assert cio.same_bits(M.indptr.astype(np.intc), Sp) and cio.same_bits(M.indices.astype(np.intc), Sj)
    assert cio.same_bits(M.data, Sx)
    assert classical._operator_order(A, "x") is False
    Cp, Cj, Cx = classical.pattern_values(A, S)
    assert cio.same_bits(Cp, Sp) and cio.same_bits(Cj, Sj) and cio.same_bits(Cx, Sx)


def test_coarse_operators_meet_S_in_reverse():
    np.random.seed(0)
    ml = classical.ruge_stuben_solver(sio.poisson2d(40, 40), CF="PMIS", max_coarse=20, keep=True)
    assert len(ml.levels) == 5
    for lvl in ml.levels[1:-1]:
        A, S = lvl.A, lvl.C
        assert classical._operator_order(A, "x", product_order=True) is True
        with pytest.raises(NotImplementedError):
            classical._operator_order(A, "x")
        ones = S.copy()
        ones.data[:] = 1.0
        M = sps.csr_matrix(ones.multiply(A))
        Cp, Cj, Cx = classical.pattern_values(A, S, reverse=True)
        assert cio.same_bits(Cp, M.indptr.astype(np.intc)) and cio.same_bits(Cj, M.indices.astype(np.intc))
        assert cio.same_bits(Cx, M.data)
        Sp, Sj, Sx = cio.strength_of(A, 0.25, Host)
        for i in range(A.shape[0]):
            assert cio.same_bits(Cx[Cp[i]:Cp[i + 1]], Sx[Sp[i]:Sp[i + 1]][::-1])


@pytest.mark.parametrize("cf", ["RS", "PMIS", "CLJP"])
def test_solver_with_device_false_equals_the_call_without_the_keyword(cf):
    A = sio.poisson2d(40, 40)
    np.random.seed(0)
    plain = classical.ruge_stuben_solver(A, CF=cf, max_coarse=20, keep=True)
    np.random.seed(0)
    ml = classical.ruge_stuben_solver(A, CF=cf, max_coarse=20, keep=True, device=False)
    cio.same_hierarchy(ml, plain)


def test_cljp_random_entry_is_the_glibc_stream():
    r = np.empty(50)
    _host.host_lib().amgsetup_cljp_random(50, _dp(r))
    assert cio.same_bits(r, sio.glibc_weights(50))
    assert "amgsetup_cljp_random" in _host._signatures()


@pytest.mark.parametrize("impl", [cio.Model, Host], ids=["model", "host"])
def test_every_recorded_call(impl):
    cio.check_setup_strength(impl)
    cio.check_setup_interpolation(impl)
    seen = set()
    for case in cio.CASES:
        seen |= cio.check_crafted(case, impl)
    assert seen == set(FLAT)
