"""Sub-range, strided, single-row and empty sweeps of the flat amg_core table on the GPU, in float32, float64,
complex64 and complex128, with a caller's temp and z that are never zero.

 * recorded: every case of tests/golden/ranges_<dtype>.npz (the reference's own answers at n = 300, written by
   tools/gen_golden_dtypes.py:gen_ranges) replayed through pyamg_amd.amg_core;
 * live: the same calls at n = 5000 (CSR) and 2000 block rows (BSR 3x3), where a strided Jacobi passes one
   256-thread block and every level launch spans many workgroups: float64 against the CPU oracle (pinned on
   the recorded cases by tests/test_oracle_ranges.py), the other dtypes against the reference's native module;
 * the argument contract: ranges that never end or leave the matrix raise ValueError and touch nothing.

Every array argument is compared after every call: one the reference changes (x, temp, z) bit for bit with the
reference's, every other one (Ax, b, Tx, ... and everything in an empty sweep) with its input bits."""
import os
import sys

import numpy as np
import pytest

import flat_ranges
import oracle_lib
from pyamg_amd import amg_core

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = list(flat_ranges.DTYPES)
RECORDED = {tag: flat_ranges.load(tag) for tag in TAGS}


@pytest.mark.parametrize("case", [c for tag in TAGS for c in flat_ranges.case_names(tag)])
def test_range_sweep_bit_exact_vs_reference(case):
    flat_ranges.replay(RECORDED[case.rsplit("@", 1)[1]], case, amg_core)


# ------------------------------------------------------------------ live, many workgroups
def _reference_table(tag):
    if tag == "f64":
        return flat_ranges.OracleTable(oracle_lib.load())
    path = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(path, "_amg_core.so")):
        pytest.skip("the reference's native module (oracle/_ref) has not been built here")
    if path not in sys.path:
        sys.path.insert(0, path)
    import _amg_core
    return _amg_core


@pytest.mark.parametrize("tag", TAGS)
def test_range_sweeps_live_many_workgroups(tag):
    ref = _reference_table(tag)
    bad, count = [], 0
    for case, fn, args in flat_ranges.sweep_calls(flat_ranges.DTYPES[tag], 5000, ((3, 2000),), 1000,
                                                  flat_ranges.NONTRIVIAL, seed=5000):
        want = flat_ranges.call_table(ref, fn, args)
        got = flat_ranges.call_table(amg_core, fn, args)
        changed = [k for k, v in args if isinstance(v, np.ndarray) and flat_ranges.bit_mismatches(want[k], v)]
        assert changed and set(changed) <= {"x", "temp", "z"}, (case, changed)    # the sweep did something
        for name in want:
            k = flat_ranges.bit_mismatches(got[name], want[name])
            if k:
                bad.append("%s@%s: %s differs in %d of %d entries" % (case, tag, name, k, len(want[name])))
        count += 1
    assert count == 38, count
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ the smallest systems
def _small_calls(n):
    """gauss_seidel_ne, jacobi_ne and overlapping_schwarz_csr (float64) over every row of an n-row system: row i holds
    its diagonal, its neighbours i - 1 and i + 1 and column (7 i + 3) mod n where these exist; one subdomain per row"""
    rng = np.random.RandomState(100 + n)
    Ap, Aj, Ax = [0], [], []
    for i in range(n):
        cols = sorted({c for c in (i - 1, i, i + 1, (7 * i + 3) % n) if 0 <= c < n})
        vals = rng.uniform(-1.0, 1.0, len(cols))
        vals[cols.index(i)] = 4.0 + rng.rand()
        Aj.extend(cols); Ax.extend(vals)
        Ap.append(len(Aj))
    Ap, Aj, Ax = np.array(Ap, dtype=np.intc), np.array(Aj, dtype=np.intc), np.array(Ax)
    x0, b, temp, delta = (rng.randn(n) for _ in range(4))
    A = [("Ap", Ap), ("Aj", Aj), ("Ax", Ax), ("x", x0), ("b", b)]
    full = [("rs", 0), ("re", n), ("rt", 1)]
    yield "gauss_seidel_ne", A + full + [("Tx", flat_ranges.inverse_norms(Ap, Ax, n, np.float64)), ("omega", 0.9)]
    yield "jacobi_ne", A + [("Tx", delta), ("temp", temp)] + full + [("omega", np.array([0.7]))]
    dense = np.zeros((n, n))
    dense[np.repeat(np.arange(n), np.diff(Ap)), Aj] = Ax
    Tx, Tp = [], [0]
    for d in range(n):
        idx = Aj[Ap[d]:Ap[d + 1]]
        Tx.extend(np.linalg.pinv(dense[np.ix_(idx, idx)]).ravel())
        Tp.append(len(Tx))
    yield "overlapping_schwarz_csr", A + [("Tx", np.array(Tx)), ("Tp", np.array(Tp, dtype=np.intc)), ("Sj", Aj.copy()),
                                          ("Sp", Ap.copy()), ("nsd", n), ("nrows", n)] + full


@pytest.mark.parametrize("n", [1, 65])
def test_one_row_and_one_past_a_wave_bit_exact_vs_oracle(n):
    # the shapes at which an upload of a handful of bytes, or the padding behind one, can go wrong; the empty sweep
    # (nothing is uploaded) is among the recorded cases above
    ref = flat_ranges.OracleTable(oracle_lib.load())
    count = 0
    for fn, args in _small_calls(n):
        want = flat_ranges.call_table(ref, fn, args)
        got = flat_ranges.call_table(amg_core, fn, args)
        assert flat_ranges.bit_mismatches(want["x"], dict(args)["x"]) > 0, fn         # the sweep did something
        flat_ranges.compare_all("%s@n=%d" % (fn, n), got, want)
        count += 1
    assert count == 3


# ------------------------------------------------------------------ the argument contract
def _contract_calls(dt):
    """(case, fn, args) whose range must be refused: every entry with the ranges that are wrong for it"""
    n, nb, bs, nsd = 300, 100, 3, 60
    limit = {"gauss_seidel_indexed": n // 2, "overlapping_schwarz_csr": nsd}
    base = {}
    for case, fn, args in flat_ranges.sweep_calls(dt, n, ((bs, nb),), nsd, ("sub_fwd",)):
        base.setdefault(fn, args)
    for fn, args in base.items():
        m = limit.get(fn, nb if any(k == "bs" for k, _ in args) else n)
        wrong = {"step0": (5, m - 7, 0), "leaves_low": (-1, 4, 1), "leaves_high": (0, m + 1, 1)}
        if fn == "jacobi_ne":                       # its loop is `i < stop`: only a positive step is defined
            wrong.update({"step_negative": (m - 8, 4, -1)})
        else:
            wrong.update({"never_ends_stride": (0, 7, 2), "never_ends_backward": (0, 5, -1),
                          "leaves_low_backward": (4, -2, -1)})
        if fn == "bsr_jacobi":
            wrong["step_negative"] = (m - 8, 4, -1)
        for nm, (rs, re, rt) in wrong.items():
            swapped = [(k, {"rs": rs, "re": re, "rt": rt}.get(k, v)) for k, v in args]
            yield "%s_%s" % (fn, nm), fn, swapped
    args = list(base["gauss_seidel_indexed"])
    for nm, value in (("Id_high", n), ("Id_negative", -1)):
        Id = dict(args)["Id"].copy()
        Id[40] = value                              # inside the walk (2, m-3, 1)
        yield "gauss_seidel_indexed_" + nm, "gauss_seidel_indexed", [(k, Id if k == "Id" else v) for k, v in args]


@pytest.mark.parametrize("tag", ["f64", "c64"])
def test_bad_ranges_raise_and_touch_nothing(tag):
    count = 0
    for case, fn, args in _contract_calls(flat_ranges.DTYPES[tag]):
        live = {k: v.copy() for k, v in args if isinstance(v, np.ndarray)}
        with pytest.raises(ValueError):
            getattr(amg_core, fn)(*[live[k] if isinstance(v, np.ndarray) else v for k, v in args])
            pytest.fail("%s@%s was accepted" % (case, tag))
        flat_ranges.compare_all("%s@%s" % (case, tag), live, {k: v for k, v in args if isinstance(v, np.ndarray)})
        count += 1
    assert count == 67, count      # 9 entries x 6, jacobi_ne 4, bsr_jacobi 7, Id 2
