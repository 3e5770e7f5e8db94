#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (development container only): the fixtures of the row-parallel classical setup stages.

Runs the REFERENCE's native module (oracle/_ref/_amg_core.so, staged by oracle/ref_env.py as in
tools/gen_golden_splitting.py) on small crafted operators that tests/golden/setup_kernels.npz does not reach, and
records under tests/golden/classical/ one <case>.npz each with the arguments and results of every native call:

  classical_strength_of_connection   per theta of the case
  maximum_row_value                  once
  rs_direct_interpolation_pass1/2    per (theta, splitting), on the S the strength call of that theta returned

Layout: the operator ``Ap, Aj, Ax`` once, ``calls`` (the entry names in call order) and per call k
``c<k>__<argument>_out`` for what came back (Sj, Sx cut to Sp[n]; Bj, Bx to Bp[n]) plus what went in beside the
operator: ``c<k>__theta``; ``c<k>__S`` (the strength call whose result is the S of an interpolation pass),
``c<k>__splitting`` and, for pass 2, ``c<k>__pass1`` (the call whose Bp it continues).  Data only.

Cases (see tests/golden/classical/README.md): wide_257 (a row of 300 entries, so with repeated columns: flat entries
only), wide_257c (the same operator with that row as a full row of 257 distinct columns: canonical), branches (empty
row, row without diagonal, all-zero off-diagonals, zero diagonal in an F row, strong sets all positive / all negative /
empty, positive weak entries without positive strong ones, all-C and all-F splittings) and unsorted (shuffled rows, a
repeated column, a repeated diagonal, a NaN entry: flat entries only).  The generator asserts that each of these
branches is taken.
Usage:  make -C oracle ref && python tools/gen_golden_classical.py
"""
import os
import sys

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_env  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "classical")
DBL_MIN = np.finfo(np.float64).tiny


def csr_arrays(rows, n):
    """rows: one list of (column, value) per row, kept in the order given"""
    Ap = np.zeros(n + 1, dtype=np.intc)
    Aj, Ax = [], []
    for i, row in enumerate(rows):
        for j, v in row:
            Aj.append(j)
            Ax.append(v)
        Ap[i + 1] = len(Aj)
    return Ap, np.array(Aj, dtype=np.intc), np.array(Ax, dtype=np.float64)


def wide(canonical, n=257, wide_row=128, seed=5):
    """a banded operator of mixed signs, one past a workgroup of rows, with one row longer than a workgroup"""
    rng = np.random.RandomState(seed)
    rows = []
    for i in range(n):
        row = []
        for j in range(max(0, i - 3), min(n, i + 4)):
            if j == i:
                row.append((j, 4.0 + rng.randint(0, 16) / 16.0))
            elif rng.rand() < 0.8:
                row.append((j, rng.choice([-1.0, 1.0]) * rng.randint(1, 25) / 16.0))
        rows.append(row)
    full = [(j, (6.0 if j == wide_row else rng.choice([-1.0, 1.0]) * rng.randint(1, 33) / 16.0)) for j in range(n)]
    if not canonical:
        extra = rng.choice(n, 300 - n, replace=False)
        full += [(int(j), rng.choice([-1.0, 1.0]) * rng.randint(1, 33) / 16.0) for j in extra]
    rows[wide_row] = full
    assert len(rows[wide_row]) == (n if canonical else 300)
    return csr_arrays(rows, n)


def branches():
    rows = [
        [],                                                     # 0  empty row
        [(0, -1.0), (2, 2.0)],                                  # 1  no diagonal
        [(1, 0.0), (2, 3.0), (3, 0.0)],                         # 2  off-diagonals all zero
        [(2, -1.0), (3, 0.0), (4, -1.0)],                       # 3  zero diagonal (F: non-finite weights)
        [(3, 1.0), (4, 4.0), (5, 1.0)],                         # 4  F, strong set all positive
        [(4, -1.0), (5, 4.0), (6, -1.5)],                       # 5  C
        [(5, -1.0), (6, 4.0), (7, -1.0)],                       # 6  C
        [(6, -2.0), (7, 4.0), (8, 0.1), (9, 0.2)],              # 7  F, positive weak entries, no positive strong one
        [(7, -1.0), (8, 4.0), (9, -1.0), (11, 1.0)],            # 8  F, every strong neighbour F: empty strong set
        [(8, -1.0), (9, 4.0), (10, -1.0)],                      # 9  F, strong set all negative
        [(9, -1.0), (10, 4.0), (11, 1.0)],                      # 10 C
        [(8, 1.0), (10, 1.0), (11, 4.0)],                       # 11 F
    ]
    return csr_arrays(rows, len(rows))


def unsorted():
    rows = [
        [(2, -1.0), (0, 4.0), (1, -2.0), (2, -0.5)],            # column 2 twice
        [(1, 2.0), (0, -1.0), (1, 2.0), (3, np.nan)],           # diagonal twice, a NaN entry
        [(3, -1.0), (1, 1.0), (2, 4.0), (0, -0.25)],
        [(3, 4.0), (2, -1.0), (0, 0.75), (1, -1.0)],
        [(4, 1.0)],
    ]
    return csr_arrays(rows, len(rows))


class Log(object):
    """the native calls of one case on its operator A"""

    def __init__(self, core, Ap, Aj, Ax):
        self.core = core
        self.n = len(Ap) - 1
        self.A = (Ap, Aj, Ax)
        self.out = {"Ap": Ap, "Aj": Aj, "Ax": Ax}
        self.names = []
        self.S = {}

    def _put(self, name, inputs, outputs):
        k = len(self.names)
        for arg, v in inputs.items():
            self.out["c%d__%s" % (k, arg)] = np.asarray(v)
        for arg, v in outputs.items():
            self.out["c%d__%s_out" % (k, arg)] = np.asarray(v)
        self.names.append(name)
        return k

    def strength(self, theta):
        Ap, Aj, Ax = self.A
        Sp = np.zeros(self.n + 1, dtype=np.intc); Sj = np.zeros_like(Aj); Sx = np.zeros_like(Ax)
        self.core.classical_strength_of_connection(self.n, theta, Ap, Aj, Ax, Sp, Sj, Sx)
        nnz = int(Sp[self.n])
        k = self._put("classical_strength_of_connection", dict(theta=theta), dict(Sp=Sp, Sj=Sj[:nnz], Sx=Sx[:nnz]))
        self.S[k] = (Sp, Sj[:nnz].copy(), Sx[:nnz].copy())
        return k

    def maximum(self):
        Ap, Aj, Ax = self.A
        x = np.zeros(self.n, dtype=np.float64)
        self.core.maximum_row_value(self.n, x, Ap, Aj, Ax)
        self._put("maximum_row_value", {}, dict(x=x))
        return x

    def interpolation(self, k, splitting):
        """both passes on the S of strength call k"""
        Ap, Aj, Ax = self.A
        Sp, Sj, Sx = self.S[k]
        Bp = np.zeros(self.n + 1, dtype=np.intc)
        self.core.rs_direct_interpolation_pass1(self.n, Sp, Sj, splitting, Bp)
        first = self._put("rs_direct_interpolation_pass1", dict(S=k, splitting=splitting), dict(Bp=Bp))
        Bj = np.zeros(Bp[self.n], dtype=np.intc); Bx = np.zeros(Bp[self.n], dtype=np.float64)
        self.core.rs_direct_interpolation_pass2(self.n, Ap, Aj, Ax, Sp, Sj, Sx, splitting, Bp, Bj, Bx)
        self._put("rs_direct_interpolation_pass2", dict(S=k, pass1=first), dict(Bj=Bj, Bx=Bx))
        return Bp, Bj, Bx

    def save(self, name):
        self.out["calls"] = np.array(self.names, dtype="U40")
        path = os.path.join(OUT, "%s.npz" % name)
        np.savez_compressed(path, **self.out)
        size = os.path.getsize(path)
        assert size < 20000, "%s: %d bytes" % (path, size)
        print("%-10s %2d calls %5.1f KB" % (name, len(self.names), size / 1024.0))


def row_sums(i, Ap, Aj, Ax, Sp, Sj, Sx, splitting):
    """(sum_strong_pos, sum_strong_neg, sum_all_pos, number of strong C neighbours) of F row i, for the branch checks"""
    strong = [Sx[jj] for jj in range(Sp[i], Sp[i + 1]) if splitting[Sj[jj]] == 1 and Sj[jj] != i]
    off = [Ax[jj] for jj in range(Ap[i], Ap[i + 1]) if Aj[jj] != i]
    return (sum(v for v in strong if not v < 0), sum(v for v in strong if v < 0), sum(v for v in off if not v < 0), len(strong))


def gen_wide(core):
    rng = np.random.RandomState(3)
    for name, canonical in (("wide_257", False), ("wide_257c", True)):
        Ap, Aj, Ax = wide(canonical)
        n = len(Ap) - 1
        assert n == 257 and np.diff(Ap).max() == (257 if canonical else 300)
        if canonical:
            A = sps.csr_matrix((Ax, Aj, Ap), shape=(n, n))
            assert A.has_canonical_format and np.all(A.data != 0)
        log = Log(core, Ap, Aj, Ax)
        log.maximum()
        log.strength(1.0)
        k = log.strength(0.25)
        Sp = log.S[k][0]
        assert 1 < Sp[129] - Sp[128] < Ap[129] - Ap[128]                  # the long row is really filtered
        log.interpolation(k, (rng.rand(n) < 0.4).astype(np.intc))
        log.save(name)


def gen_branches(core):
    Ap, Aj, Ax = branches()
    n = len(Ap) - 1
    log = Log(core, Ap, Aj, Ax)
    x = log.maximum()
    assert x[0] == DBL_MIN and Ap[1] == Ap[0]                             # the empty row
    assert 1 not in Aj[Ap[1]:Ap[2]]                                       # the row without a diagonal
    at = {theta: log.strength(theta) for theta in (0.0, 0.25, 1.0)}
    Sp0, Sp1 = log.S[at[0.0]][0], log.S[at[1.0]][0]
    assert Sp0[3] - Sp0[2] == 3 and Sp1[3] - Sp1[2] == 1                  # zero off-diagonals: kept at theta 0, dropped at 1
    Sp, Sj, Sx = log.S[at[0.25]]
    assert list(Sj[Sp[7]:Sp[8]]) == [6, 7]                                # row 7 loses its weak positive entries
    mixed = np.array([0, 1, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0], dtype=np.intc)
    seen = set()
    for splitting in (mixed, np.ones(n, dtype=np.intc), np.zeros(n, dtype=np.intc)):
        Bp, Bj, Bx = log.interpolation(at[0.25], splitting)
        if splitting.all():
            assert np.array_equal(Bj, np.arange(n)) and np.all(Bx == 1.0)
            seen.add("all C")
        elif not splitting.any():
            assert Bp[n] == 0
            seen.add("all F")
        for i in np.flatnonzero(splitting == 0):
            sp, sn, ap, k = row_sums(i, Ap, Aj, Ax, Sp, Sj, Sx, splitting)
            if k == 0:
                seen.add("empty strong set")
            elif sn == 0:
                seen.add("strong set all positive")
            elif sp == 0:
                seen.add("strong set all negative")
            if k > 0 and sp == 0 and ap > 0:
                seen.add("diag += sum_all_pos")
        if splitting is mixed:
            assert not np.all(np.isfinite(Bx[Bp[3]:Bp[4]])) and Bp[4] > Bp[3]     # the zero diagonal of F row 3
            seen.add("non-finite weights")
    want = {"all C", "all F", "empty strong set", "strong set all positive", "strong set all negative", "diag += sum_all_pos",
            "non-finite weights"}
    assert seen == want, want - seen
    log.save("branches")


def gen_unsorted(core):
    Ap, Aj, Ax = unsorted()
    n = len(Ap) - 1
    assert any(np.any(np.diff(Aj[Ap[i]:Ap[i + 1]]) < 0) for i in range(n))                        # an unsorted row
    assert any(len(set(Aj[Ap[i]:Ap[i + 1]])) < Ap[i + 1] - Ap[i] for i in range(n))               # a repeated column
    assert list(Aj[Ap[1]:Ap[2]]).count(1) == 2 and np.isnan(Ax).sum() == 1
    log = Log(core, Ap, Aj, Ax)
    x = log.maximum()
    assert np.all(np.isfinite(x))                                         # the NaN never replaces the maximum
    for theta in (0.0, 0.5):
        k = log.strength(theta)
        Sp, Sj, Sx = log.S[k]
        assert list(Sj[Sp[1]:Sp[2]]).count(1) == 2                        # the diagonal is kept once per stored entry
        for splitting in ([1, 0, 1, 0, 0], [0, 1, 0, 1, 1]):
            log.interpolation(k, np.array(splitting, dtype=np.intc))
    log.save("unsorted")


def main():
    os.makedirs(OUT, exist_ok=True)
    pyamg = ref_env.stage()
    core = pyamg.amg_core
    gen_wide(core)
    gen_branches(core)
    gen_unsorted(core)


if __name__ == "__main__":
    main()
