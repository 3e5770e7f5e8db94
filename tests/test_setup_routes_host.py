"""pyamg_amd/_host.py: the route policy every setup stage reads its ``device`` argument through, and the signature
table of the CPU-side setup library.  No GPU: which route a stage took is seen by whether the device library was
reached."""
import ctypes
import os
import re

import numpy as np
import pytest

import energy_io
import evolution_io
import splitting_io
import pyamg_amd
from pyamg_amd import _host, _lib, classical, graph, smooth, strength, util
from pyamg_amd.smooth import energy_prolongation_smoother
from pyamg_amd.strength import evolution_strength_of_connection

CSRC = os.path.join(os.path.dirname(os.path.abspath(pyamg_amd.__file__)), "csrc", "setup_host.cpp")


def _touched(*a, **k):
    raise AssertionError("the library was touched")


# ---------------------------------------------------------------------------------------------- route(device, auto)
@pytest.mark.parametrize("present", [True, False])
@pytest.mark.parametrize("auto", [True, False])
@pytest.mark.parametrize("device", [True, False, None])
def test_route_table(monkeypatch, device, auto, present):
    calls = []

    def device_count():
        calls.append(1)
        return 1 if present else 0
    monkeypatch.setattr(_lib, "lib", _touched)
    monkeypatch.setattr(_lib, "device_count", device_count)
    want = device if device is not None else (None if (auto and present) else False)
    got = _host.route(device, auto)
    assert got is want
    # the library is asked for a device only where the answer decides the route
    assert len(calls) == (1 if (device is None and auto) else 0)


def test_route_reads_device_present_through_the_modules_own_global(monkeypatch):
    monkeypatch.setattr(_lib, "device_count", _touched)
    monkeypatch.setattr(_host, "device_present", lambda: True)
    assert _host.route(None, True) is None
    monkeypatch.setattr(_host, "device_present", lambda: False)
    assert _host.route(None, True) is False


def test_attempt_raises_under_true_and_falls_back_under_none():
    def refuses():
        raise NotImplementedError("refused")

    def breaks():
        raise ValueError("not a refusal")
    assert _host.attempt(False, _touched, lambda: "host") == "host"
    assert _host.attempt(True, lambda: "device", _touched) == "device"
    assert _host.attempt(None, lambda: "device", _touched) == "device"
    assert _host.attempt(None, refuses, lambda: "host") == "host"
    with pytest.raises(NotImplementedError):
        _host.attempt(True, refuses, _touched)
    with pytest.raises(ValueError):                     # outside the stage's refusals: never swallowed
        _host.attempt(None, breaks, _touched)
    assert _host.attempt(None, breaks, lambda: "host", (ValueError,)) == "host"


# ---------------------------------------------------------------------------------------------- one patch, every stage
def _luby(device=None):
    p = splitting_io.problem("poisson_17x23")
    G = p["G"]
    n = G.shape[0]
    x = np.full(n, -1, dtype=np.intc)
    y = np.random.RandomState(3).rand(n)
    graph.luby(n, _host.i32(G.indptr), _host.i32(G.indices), -1, 1, 0, x, y, device=device)
    return x


def _cljp(device=None):
    return classical.CLJP(splitting_io.problem("poisson_17x23")["S"], device=device)


def _evolution(device=None):
    p = evolution_io.problem("iso_12x12")
    return evolution_strength_of_connection(p["A"], k=2, rho=p[2]["rho"], device=device)


def _energy(device=None):
    p = energy_io.problem("aniso_17x23")
    return energy_prolongation_smoother(p["A"], p["T"], p["Atilde"], p["Bc"], None, (False, {}), device=device)


def _same(a, b):
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) \
        and np.array_equal(a.data, b.data)


@pytest.mark.parametrize("stage", [_luby, _cljp, _evolution, _energy], ids=lambda f: f.__name__.strip("_"))
def test_one_patch_of_device_present_moves_every_stage(monkeypatch, stage):
    want = stage(device=False)
    monkeypatch.setattr(_lib, "lib", _touched)
    monkeypatch.setattr(_lib, "device_count", _touched)
    for module in (graph, classical, strength, smooth):
        monkeypatch.setattr(module, "DEVICE_AUTO", True)
    monkeypatch.setattr(util, "DEVICE_RHO_MIN_ROWS", 0)             # strength's own gate on the operator's size
    monkeypatch.setattr(_host, "device_present", lambda: False)
    assert _same(stage(), want)                                     # the host route: the library stays untouched
    monkeypatch.setattr(_host, "device_present", lambda: True)
    with pytest.raises(AssertionError, match="the library was touched"):
        stage()                                                     # the device route is live


# ---------------------------------------------------------------------------------------------- the signature table
def _defined():
    text = open(CSRC).read()
    return set(re.findall(r"^(?:int|void|int64_t)\s+(amgsetup_\w+)\s*\(", text, flags=re.M))


def test_every_entry_of_the_host_library_has_a_signature():
    defined = _defined()
    assert len(defined) > 40 and "amgsetup_mis_parallel" in defined and "amgsetup_extract_subblocks_c128" in defined
    table = _host._signatures()
    assert defined - set(table) == set()
    assert set(table) - defined == set()


def test_every_signature_resolves_and_is_applied():
    raw = ctypes.CDLL(os.path.join(os.path.dirname(CSRC), "..", "lib", "libamgsetup_host.so"))
    L = _host.host_lib()
    for name, (restype, argtypes) in _host._signatures().items():
        assert hasattr(raw, name), name
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name


def test_names_other_modules_import_stay_importable():
    from pyamg_amd import aggregation
    assert aggregation.host_lib is _host.host_lib and graph._host is _host.host_lib
    assert aggregation._ip is _host.ip and aggregation._dp is _host.dp
    for module, name in ((graph, "_luby_device"), (strength, "_device_measure"), (strength, "_canonical_csr"),
                         (smooth, "_cg_device"), (classical, "cljp_device")):
        assert callable(getattr(module, name)), name
