"""An exception raised by Python code that runs inside the engine's cycle -- a callable coarse solver, a Krylov
smoother -- comes out of the call that ran the cycle as itself, whichever entry of the mirror that was, and nothing
of it is left for the next call.  Two-level hierarchies of the 2-D Poisson operator on a 12 x 12 grid; the callback
fails on its first call only.  The engine answers a failed callback with an ordinary error code: no kernel faults."""
import numpy as np
import pytest
import scipy.sparse as sps

import pyamg_amd
from pyamg_amd.aggregation import poisson, smoothed_aggregation_solver

pytestmark = pytest.mark.gpu


class FailsOnce(object):
    """fn, except that the first call (and the first after arm()) raises KeyError('boom')"""

    def __init__(self, fn):
        self.fn, self.armed = fn, True

    def arm(self):
        self.armed = True

    def __call__(self, *args, **kwargs):
        if self.armed:
            self.armed = False
            raise KeyError("boom")
        return self.fn(*args, **kwargs)


def _dense_solve(A, b):
    return np.linalg.solve(A.toarray(), b)


def _two_level(coarse_solver="pinv"):
    np.random.seed(0)
    ml = smoothed_aggregation_solver(poisson((12, 12)), max_coarse=30, coarse_solver=coarse_solver)
    assert len(ml.levels) == 2
    return ml, np.random.RandomState(1).rand(144)


def _raises_once_then_runs(dev, call):
    """the three assertions every case makes"""
    with pytest.raises(KeyError):
        call()
    assert dev._callback_error is None
    call()


def test_plain_cycling():
    ml, b = _two_level(FailsOnce(_dense_solve))
    _raises_once_then_runs(ml.device_hierarchy(), lambda: ml.solve(b))


def test_device_pcg():
    # failed before the mirrors shared one _check: pcg() did not look for the callback's exception, so this call raised
    # AmgError("coarse solver callback failed") and the KeyError came out of the next one.  So did the device-tensor
    # case with accel="cg" and relax() in the Krylov smoother case below.
    ml, b = _two_level(FailsOnce(_dense_solve))
    _raises_once_then_runs(ml.device_hierarchy(), lambda: ml.solve(b, accel="cg"))


@pytest.mark.parametrize("accel", [None, "cg"])
def test_device_tensors(accel):
    torch = pytest.importorskip("torch")
    ml, b = _two_level(FailsOnce(_dense_solve))
    tb = torch.from_numpy(b).cuda()
    _raises_once_then_runs(ml.device_hierarchy(), lambda: ml.solve(tb, accel=accel))


def test_krylov_smoother(monkeypatch):
    from pyamg_amd import krylov
    ml, b = _two_level()
    pyamg_amd.change_smoothers(ml, ("cg", {"maxiter": 2}), ("cg", {"maxiter": 2}))
    run = FailsOnce(krylov.run)
    monkeypatch.setattr(krylov, "run", run)
    dev = ml.device_hierarchy()
    _raises_once_then_runs(dev, lambda: dev.relax(0, 0, b, np.zeros(144)))
    run.arm()
    _raises_once_then_runs(dev, lambda: ml.solve(b))


def test_complex128():
    mlr, b = _two_level()
    l0, l1 = pyamg_amd.multilevel_solver.level(), pyamg_amd.multilevel_solver.level()
    l0.A = sps.csr_matrix(mlr.levels[0].A.astype(np.complex128) + 0.5j * sps.identity(144))
    l0.P = sps.csr_matrix(mlr.levels[0].P)
    l0.R = l0.P.T.tocsr()
    l1.A = sps.csr_matrix(l0.R @ l0.A @ l0.P)
    ml = pyamg_amd.multilevel_solver([l0, l1], coarse_solver=FailsOnce(_dense_solve))
    pyamg_amd.change_smoothers(ml, "gauss_seidel", "gauss_seidel")
    _raises_once_then_runs(ml.device_hierarchy(), lambda: ml.solve(b + 1j * b[::-1]))
