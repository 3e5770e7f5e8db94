"""TEST INFRASTRUCTURE: the Krylov-accelerated complex128 fixtures (tests/golden/accel_c128/<case>__<method>.npz,
written by tools/gen_golden_accel_c128.py) and the rule a history is held to."""
import glob
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "accel_c128")


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))


def path(name):
    return os.path.join(GOLDEN, name + ".npz")


def load(name):
    """-> dict(case, meta, b, x0, x, residuals)"""
    z = np.load(path(name), allow_pickle=False)
    out = {k: z[k] for k in ("b", "x0", "x", "residuals")}
    out["case"] = str(z["case"])
    out["meta"] = json.loads(str(z["meta_json"]))
    return out


def x0_of(f):
    return f["x0"] if np.any(f["x0"]) else None


def assert_matches(res, x, ref, x_ref, what=""):
    """the project's rule for a device Krylov history against the reference's (tests/test_gpu_parity.py, the float64
    device PCG): the same number of iterations, every entry within rtol 1e-9 (atol 1e-13 of the first entry), the
    solution within 1e-10 relative.  The figures are printed before they are asserted."""
    res, ref = np.asarray(res, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    x, x_ref = np.ravel(x), np.ravel(x_ref)
    dx = float(np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref))
    if len(res) == len(ref):
        dev = np.abs(res - ref)
        print("%s iterations %d  max |res - ref| / ref %.3e  max |res - ref| / ref[0] %.3e  |x - x_ref| / |x_ref| %.3e"
              % (what, len(ref) - 1, float(np.max(dev / ref)), float(np.max(dev) / ref[0]), dx))
    assert len(res) == len(ref), "%s iterations %d, reference %d" % (what, len(res) - 1, len(ref) - 1)
    assert np.allclose(res, ref, rtol=1e-9, atol=1e-13 * ref[0]), what
    assert dx <= 1e-10, what
