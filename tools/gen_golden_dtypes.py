#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (development container only): the float32 / complex64 / complex128 fixtures.

Runs the REFERENCE -- its Python staged by oracle/ref_env.py on top of its own native module
oracle/_ref/_amg_core.so, exactly as oracle/gen_golden.py does -- and records inputs and outputs:

  tests/golden/kernels_dtypes.npz     every amg_core case of oracle/gen_golden.py:gen_kernels in each of the
                                      three dtypes, and extra complex diagonals (zero, zero real part, both
                                      Smith branches)
  tests/golden/division_dtypes.npz    the division sweep: a diagonal matrix, one gauss_seidel call, so that
                                      x_i = b_i / d_i goes through the reference's compiled complex division
                                      (its own file: with it kernels_dtypes.npz would pass 1 MB)
  tests/golden/relaxation_dtypes.npz  the reference's pyamg.relaxation functions on small CSR and BSR 2x2
                                      systems in each dtype

  tests/golden/ranges_<dtype>.npz     sub-range, strided, single-row and empty sweeps of every sweeping entry with
                                      random (never zero) temp and z, one file per dtype, float64 included; the
                                      systems and the list of calls are tests/flat_ranges.py:sweep_calls

kernels_dtypes.npz, division_dtypes.npz and ranges_*.npz keep every distinct array once (``pool_<k>``); ``<case>__call`` describes the call
and names the pool entries of its inputs and of the arrays it changed (class Recorder).  Usage:  make -C oracle ref && python tools/gen_golden_dtypes.py
"""
import json
import os
import sys
import warnings

import numpy as np
import scipy.sparse as sps
from scipy.sparse import _sparsetools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_env  # noqa: E402
import flat_ranges  # noqa: E402
from gen_golden import random_system  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
DTYPES = {"f32": np.float32, "c64": np.complex64, "c128": np.complex128}
CAP = 1000 * 1000          # bytes: no fixture file may reach 1 MB


class Recorder:
    """Cases share their arrays through a pool (a matrix serves many calls): ``pool_<k>`` holds each distinct
    array once and ``<case>__call`` is JSON: the entry, its arguments in call order (["a", name, pool key] or
    ["s", value]) and ``out``, the pool key of every argument array the call changed."""
    def __init__(self):
        self.out, self.cases, self.keys = {}, [], {}

    def pool(self, v):
        h = (v.dtype.str, v.shape, v.tobytes())
        if h not in self.keys:
            self.keys[h] = "pool_%d" % len(self.keys)
            self.out[self.keys[h]] = v
        return self.keys[h]

    def call(self, core, name, fn, args, **meta):
        """args: (label, value) pairs in call order; arrays are copied, so their post-call values are outputs"""
        call_args, live = [], {}
        for label, v in args:
            if isinstance(v, np.ndarray):
                call_args.append(["a", label, self.pool(np.ascontiguousarray(v))])
                live[label] = v.copy()
            else:
                call_args.append(["s", v])
        getattr(core, fn)(*[live[a[1]] if a[0] == "a" else a[1] for a in call_args])
        outs = {}
        for a in call_args:
            if a[0] == "a" and live[a[1]].tobytes() != self.out[a[2]].tobytes():
                outs[a[1]] = self.pool(live[a[1]])
        self.cases.append(name)
        self.out["%s__call" % name] = np.array(json.dumps(dict(fn=fn, args=call_args, out=outs, **meta)))

    def save(self, path):
        self.out["cases"] = np.array(self.cases)
        np.savez_compressed(path, **self.out)
        print("%s: %d cases, %.0f KB" % (os.path.basename(path), len(self.cases), os.path.getsize(path) / 1024))


def cast(v, dt, rng):
    """real input -> dtype; complex: plus 1j times an independent randn draw of the same shape"""
    v = np.asarray(v, dtype=np.float64)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.randn(*v.shape)
    return np.ascontiguousarray(v.astype(dt))


def cast_matrix(A, dt, rng):
    A = A.copy()
    A.data = cast(A.data, dt, rng).reshape(A.data.shape)
    return A


def gen_kernels(core, rec, tag, dt):
    st = _sparsetools
    rng = np.random.RandomState(1234)
    c = lambda v: cast(v, dt, rng)
    for sys_tag, n, dens in (("a", 37, 0.15), ("b", 200, 0.03)):
        A = random_system(n, dens, seed=n)
        if sys_tag == "a":
            A = A.tolil(); A[5, 5] = 0.0; A = sps.csr_matrix(A); A.eliminate_zeros()
            A.sort_indices(); A.indices = A.indices.astype(np.intc); A.indptr = A.indptr.astype(np.intc)
        A = cast_matrix(A, dt, rng)
        Ap, Aj, Ax = A.indptr, A.indices, A.data
        x0, b = c(rng.randn(n)), c(rng.randn(n))
        for nm, (rs, re, rt) in (("fwd", (0, n, 1)), ("bwd", (n - 1, -1, -1)),
                                 ("part", (3, 3 + 2 * ((n - 7) // 2), 2))):
            rec.call(core, "gauss_seidel_%s_%s@%s" % (sys_tag, nm, tag), "gauss_seidel",
                     [("Ap", Ap), ("Aj", Aj), ("Ax", Ax), ("x", x0), ("b", b), ("rs", rs), ("re", re), ("rt", rt)])
        omegas = [1.0, 0.7] + ([0.7 + 0.2j] if np.dtype(dt).kind == "c" else [])
        for om in omegas:
            rec.call(core, "jacobi_%s_om%s@%s" % (sys_tag, str(om).replace("+", "p"), tag), "jacobi",
                     [("Ap", Ap), ("Aj", Aj), ("Ax", Ax), ("x", x0), ("b", b), ("temp", np.zeros(n, dt)),
                      ("rs", 0), ("re", n), ("rt", 1), ("omega", np.array([om], dtype=dt))])
        Id = rng.permutation(n)[: n // 2].astype(np.intc)
        for nm, (rs, re, rt) in (("fwd", (0, len(Id), 1)), ("bwd", (len(Id) - 1, -1, -1))):
            rec.call(core, "gauss_seidel_indexed_%s_%s@%s" % (sys_tag, nm, tag), "gauss_seidel_indexed",
                     [("Ap", Ap), ("Aj", Aj), ("Ax", Ax), ("x", x0), ("b", b), ("Id", Id), ("rs", rs), ("re", re),
                      ("rt", rt)])
        Dne = (1.0 / np.asarray(A.multiply(A.conjugate()).sum(axis=1)).ravel()).astype(dt)
        for nm, (rs, re, rt) in (("fwd", (0, n, 1)), ("bwd", (n - 1, -1, -1))):
            rec.call(core, "gauss_seidel_ne_%s_%s@%s" % (sys_tag, nm, tag), "gauss_seidel_ne",
                     [("Ap", Ap), ("Aj", Aj), ("Ax", Ax), ("x", x0), ("b", b), ("rs", rs), ("re", re), ("rt", rt),
                      ("Tx", Dne), ("omega", 0.9)])
        Ac = sps.csc_matrix(A); Ac.sort_indices()
        Ac.indices = Ac.indices.astype(np.intc); Ac.indptr = Ac.indptr.astype(np.intc)
        Dnr = (1.0 / np.asarray(Ac.multiply(Ac.conjugate()).sum(axis=0)).ravel()).astype(dt)
        z0 = (b - A * x0).astype(dt)
        for nm, (rs, re, rt) in (("fwd", (0, n, 1)), ("bwd", (n - 1, -1, -1))):
            rec.call(core, "gauss_seidel_nr_%s_%s@%s" % (sys_tag, nm, tag), "gauss_seidel_nr",
                     [("Ap", Ac.indptr), ("Aj", Ac.indices), ("Ax", Ac.data), ("x", x0), ("z", z0), ("rs", rs),
                      ("re", re), ("rt", rt), ("Tx", Dnr), ("omega", 1.1)])
        delta = ((b - A * x0) * Dne).astype(dt)
        rec.call(core, "jacobi_ne_%s@%s" % (sys_tag, tag), "jacobi_ne",
                 [("Ap", Ap), ("Aj", Aj), ("Ax", Ax), ("x", x0), ("b", b), ("Tx", delta), ("temp", np.zeros(n, dt)),
                  ("rs", 0), ("re", n), ("rt", 1), ("omega", np.array([0.8], dtype=dt))])

    for bs in (1, 2, 3, 4):
        n = 24 * bs
        A = random_system(n, 0.2, seed=100 + bs, bs=bs) if bs > 1 else \
            sps.bsr_matrix(random_system(n, 0.2, seed=100), blocksize=(1, 1))
        A.sort_indices()
        A = cast_matrix(A, dt, rng)
        Ap = A.indptr.astype(np.intc); Aj = A.indices.astype(np.intc); Ax = np.ravel(A.data).copy()
        nb = n // bs
        x0, b = c(rng.randn(n)), c(rng.randn(n))
        base = [("Ap", Ap), ("Aj", Aj), ("Ax", Ax), ("x", x0), ("b", b)]
        for nm, (rs, re, rt) in (("fwd", (0, nb, 1)), ("bwd", (nb - 1, -1, -1))):
            rec.call(core, "bsr_gauss_seidel_bs%d_%s@%s" % (bs, nm, tag), "bsr_gauss_seidel",
                     base + [("rs", rs), ("re", re), ("rt", rt), ("bs", bs)])
        rec.call(core, "bsr_jacobi_bs%d@%s" % (bs, tag), "bsr_jacobi",
                 base + [("temp", np.zeros(n, dt)), ("rs", 0), ("re", nb), ("rt", 1), ("bs", bs),
                         ("omega", np.array([0.6], dtype=dt))])
        Ad = sps.csr_matrix(A).toarray()
        Dinv = np.zeros((nb, bs, bs), dtype=dt)
        for i in range(nb):
            Dinv[i] = np.linalg.inv(Ad[i * bs:(i + 1) * bs, i * bs:(i + 1) * bs])
        Dinv = np.ravel(Dinv)
        rec.call(core, "block_jacobi_bs%d@%s" % (bs, tag), "block_jacobi",
                 base + [("Dinv", Dinv), ("temp", np.zeros(n, dt)), ("rs", 0), ("re", nb), ("rt", 1),
                         ("omega", np.array([0.8], dtype=dt)), ("bs", bs)])
        for nm, (rs, re, rt) in (("fwd", (0, nb, 1)), ("bwd", (nb - 1, -1, -1))):
            rec.call(core, "block_gauss_seidel_bs%d_%s@%s" % (bs, nm, tag), "block_gauss_seidel",
                     base + [("Dinv", Dinv), ("rs", rs), ("re", re), ("rt", rt), ("bs", bs)])

    # scipy SpMV (third-party arithmetic at the reference's call sites), y accumulated into
    A = cast_matrix(random_system(150, 0.05, seed=7), dt, rng)
    rec.call(st, "csr_matvec@%s" % tag, "csr_matvec",
             [("n_row", 150), ("n_col", 150), ("Ap", A.indptr), ("Aj", A.indices), ("Ax", A.data),
              ("x", c(rng.randn(150))), ("y", c(rng.randn(150)))])
    for (R, C) in ((2, 3), (3, 3), (1, 1)):
        nbr, nbc = 20, 17
        S = sps.random(nbr, nbc, density=0.3, random_state=np.random.RandomState(R * 10 + C), format="csr")
        S.sort_indices()
        data = c(rng.randn(S.nnz * R * C))
        rec.call(st, "bsr_matvec_%dx%d@%s" % (R, C, tag), "bsr_matvec",
                 [("n_brow", nbr), ("n_bcol", nbc), ("R", R), ("C", C), ("Ap", S.indptr.astype(np.intc)),
                  ("Aj", S.indices.astype(np.intc)), ("Ax", data), ("x", c(rng.randn(nbc * C))),
                  ("y", np.zeros(nbr * R, dt))])

    # Schwarz over the rows' own patterns with exact inverse blocks
    A = cast_matrix(random_system(20, 0.15, seed=20), dt, rng)
    n = A.shape[0]
    Sp, Sj = A.indptr.copy(), A.indices.copy()
    sizes = np.diff(Sp).astype(np.int64)
    Tp = np.zeros(n + 1, dtype=np.intc); Tp[1:] = np.cumsum(sizes * sizes)
    Ad = A.toarray()
    Tx = np.concatenate([np.ravel(np.linalg.inv(Ad[np.ix_(Sj[Sp[d]:Sp[d + 1]], Sj[Sp[d]:Sp[d + 1]])]))
                         for d in range(n)]).astype(dt)
    x0, b = c(rng.randn(n)), c(rng.randn(n))
    for nm, (rs, re, rt) in (("fwd", (0, n, 1)), ("bwd", (n - 1, -1, -1))):
        rec.call(core, "overlapping_schwarz_csr_%s@%s" % (nm, tag), "overlapping_schwarz_csr",
                 [("Ap", A.indptr), ("Aj", A.indices), ("Ax", A.data), ("x", x0), ("b", b), ("Tx", Tx), ("Tp", Tp),
                  ("Sj", Sj), ("Sp", Sp), ("nsd", n), ("nrows", n), ("rs", rs), ("re", re), ("rt", rt)])


def gen_complex_diagonals(core, rec, tag, dt):
    """rows whose diagonal is zero (stored 0, -0), has a zero real part, or |Im d| > |Re d| and the reverse"""
    rng = np.random.RandomState(77)
    n = 24
    A = random_system(n, 0.2, seed=24)
    A = cast_matrix(A, dt, rng)
    A = A.tolil()
    special = [0, -0.0, 1.7j, -2.5j, 0.3 + 4.0j, 4.0 + 0.3j, -3.0 - 0.2j, 0.1 - 5.0j, 2.0 + 2.0j]
    for i, d in enumerate(special):
        A[3 * i % n, 3 * i % n] = d
    A = sps.csr_matrix(A)
    A.sort_indices()
    Ap, Aj, Ax = A.indptr.astype(np.intc), A.indices.astype(np.intc), A.data.astype(dt)
    # rows 0 and 3: a stored zero and a stored negative zero diagonal (the sparse formats drop them)
    dense = {0: 0.0, 3: complex(-0.0, 0.0)}
    rows = []
    for i in range(n):
        cols = list(Aj[Ap[i]:Ap[i + 1]]); vals = list(Ax[Ap[i]:Ap[i + 1]])
        if i in dense and i not in cols:
            cols.append(i); vals.append(dense[i])
        o = np.argsort(cols, kind="stable")
        rows.append((np.array(cols)[o], np.array(vals, dtype=dt)[o]))
    Ap = np.zeros(n + 1, dtype=np.intc); Ap[1:] = np.cumsum([len(r[0]) for r in rows])
    Aj = np.concatenate([r[0] for r in rows]).astype(np.intc)
    Ax = np.concatenate([r[1] for r in rows]).astype(dt)
    x0, b = cast(rng.randn(n), dt, rng), cast(rng.randn(n), dt, rng)
    for nm, (rs, re, rt) in (("fwd", (0, n, 1)), ("bwd", (n - 1, -1, -1))):
        rec.call(core, "diag_gauss_seidel_%s@%s" % (nm, tag), "gauss_seidel",
                 [("Ap", Ap), ("Aj", Aj), ("Ax", Ax), ("x", x0), ("b", b), ("rs", rs), ("re", re), ("rt", rt)])
    rec.call(core, "diag_jacobi@%s" % tag, "jacobi",
             [("Ap", Ap), ("Aj", Aj), ("Ax", Ax), ("x", x0), ("b", b), ("temp", np.zeros(n, dt)), ("rs", 0),
              ("re", n), ("rt", 1), ("omega", np.array([0.7], dtype=dt))])
    rec.call(core, "diag_bsr_gauss_seidel@%s" % tag, "bsr_gauss_seidel",
             [("Ap", Ap), ("Aj", Aj), ("Ax", Ax), ("x", x0), ("b", b), ("rs", 0), ("re", n), ("rt", 1), ("bs", 1)])


def division_pairs(dt, count, seed):
    """numerators and divisors over moderate exponents, near overflow, near underflow, with subnormal parts"""
    rng = np.random.RandomState(seed)
    real = np.float32 if dt == np.complex64 else np.float64
    fi = np.finfo(real)
    emax, emin, mant = fi.maxexp, fi.minexp, fi.nmant
    bands = [(-40, 40), (emax - 24, emax), (emin - mant, emin + 24), (emin - mant, emax)]

    def draw(k, band):
        lo, hi = band
        m = rng.uniform(-1, 1, size=k)
        e = rng.randint(lo, hi + 1, size=k)
        return np.ldexp(m, e).astype(real)

    per = count // len(bands)
    parts = []
    for band in bands:
        q = [draw(per, band) for _ in range(4)]
        if band[0] == emin - mant:                         # keep some parts moderate next to tiny ones
            q[1][::3] = draw(len(q[1][::3]), (-10, 10))
        parts.append(q)
    a, b, c, d = [np.concatenate([p[i] for p in parts]) for i in range(4)]
    a[::17] = 0.0; d[5::19] = 0.0; c[7::23] = -0.0            # zero parts (never both parts of a divisor)
    num = np.empty(count, dtype=dt)
    num.real, num.imag = a, b
    den = np.empty(count, dtype=dt)
    den.real, den.imag = c, d
    zero = (den.real == 0) & (den.imag == 0)
    den.real[zero] = 1.0
    return num, den


def gen_division(core, rec, tag, dt):
    n = 4096
    num, den = division_pairs(dt, n, seed=4096 + len(tag))
    Ap = np.arange(n + 1, dtype=np.intc)
    Aj = np.arange(n, dtype=np.intc)
    rec.call(core, "divsweep@%s" % tag, "gauss_seidel",
             [("Ap", Ap), ("Aj", Aj), ("Ax", den), ("x", np.zeros(n, dt)), ("b", num), ("rs", 0), ("re", n), ("rt", 1)],
             division=True)


def gen_ranges(core):
    """tests/golden/ranges_<dtype>.npz: CSR n = 300 (two 256-row workgroups, three 128-thread level blocks, two
    1024-entry LDS chunks), BSR 2x2 (150 block rows) and 3x3 (100), 60 Schwarz subdomains; every recorded output
    is finite, so the tests compare bits with no NaN exemption"""
    for tag, dt in flat_ranges.DTYPES.items():
        calls = list(flat_ranges.sweep_calls(dt, 300, ((2, 150), (3, 100)), 60, list(flat_ranges.ranges(300))))
        path = os.path.join(OUT, "ranges_%s.npz" % tag)
        while True:
            rec = Recorder()
            for name, fn, args in calls:
                case = "%s@%s" % (name, tag)
                rec.call(core, case, fn, [(k, v.item() if isinstance(v, np.generic) else v) for k, v in args])
                out = json.loads(str(rec.out[case + "__call"]))["out"]
                assert all(np.all(np.isfinite(rec.out[key])) for key in out.values()), case
                assert bool(out) == ("_empty" not in name), case
            rec.save(path)
            if os.path.getsize(path) < CAP:
                break
            dropped = calls.pop()                              # the largest file sheds its last cases first
            print("%s is over the cap: dropping %s" % (os.path.basename(path), dropped[0]))


# --------------------------------------------------------------------------- pyamg.relaxation
def poisson1(n):
    return sps.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")


def relaxation_systems(dt, rng):
    """TestCommonRelaxation: 1-D Poisson; TestComplexRelaxation: a complex-shifted 2-D Poisson, random complex x, b"""
    out = [("p1d", poisson1(10).astype(dt))]
    P2 = sps.kronsum(poisson1(5), poisson1(5)).tocsr()
    if np.dtype(dt).kind == "c":
        A = (P2 + (0.4 + 0.3j) * sps.identity(25)).tocsr().astype(dt)
        A.data += (1j * 0.1 * rng.randn(A.nnz)).astype(dt)
    else:
        A = (P2 + 0.2 * sps.identity(25)).tocsr().astype(dt)
        A.data += (0.05 * rng.randn(A.nnz)).astype(dt)
    out.append(("p2d", A))
    return out


def gen_relaxation(pyamg, tag, dt, store):
    import pyamg.relaxation.relaxation as R
    from pyamg.util.utils import get_diagonal
    rng = np.random.RandomState(99)
    for sname, A0 in relaxation_systems(dt, rng):
        n = A0.shape[0]
        x0 = cast(rng.randn(n), dt, rng)
        b = cast(rng.randn(n), dt, rng)
        Dne = np.ravel(get_diagonal(A0.copy(), norm_eq=2, inv=True)).astype(dt)
        Dnr = np.ravel(get_diagonal(A0.copy(), norm_eq=1, inv=True)).astype(dt)
        Ad = A0.toarray()
        Dinv2 = np.array([np.linalg.inv(Ad[i:i + 2, i:i + 2]) for i in range(0, n - n % 2, 2)], dtype=dt)
        Sp, Sj = A0.indptr.astype(np.intc), A0.indices.astype(np.intc)
        sizes = np.diff(Sp).astype(np.int64)
        Tp = np.zeros(n + 1, dtype=np.intc); Tp[1:] = np.cumsum(sizes * sizes)
        Tx = np.concatenate([np.ravel(np.linalg.inv(Ad[np.ix_(Sj[Sp[d]:Sp[d + 1]], Sj[Sp[d]:Sp[d + 1]])]))
                             for d in range(n)]).astype(dt)
        calls = [("sor", "sor", (0.7,), {"iterations": 2})]
        for sw in ("forward", "backward", "symmetric"):
            calls.append(("gauss_seidel_%s" % sw, "gauss_seidel", (), {"sweep": sw, "iterations": 2}))
        calls += [("jacobi", "jacobi", (), {"omega": 0.6, "iterations": 2}),
                  ("polynomial", "polynomial", ([0.6, 0.1, -0.05],), {"iterations": 2}),
                  ("gauss_seidel_indexed", "gauss_seidel_indexed", (np.arange(n)[::-2].copy(),), {"sweep": "symmetric"}),
                  ("jacobi_ne", "jacobi_ne", (), {"omega": 0.7, "iterations": 2}),
                  ("gauss_seidel_ne", "gauss_seidel_ne", (), {"sweep": "symmetric", "omega": 0.9, "Dinv": Dne}),
                  ("gauss_seidel_nr", "gauss_seidel_nr", (), {"sweep": "symmetric", "omega": 1.1, "Dinv": Dnr}),
                  ("schwarz", "schwarz", (), {"sweep": "symmetric", "subdomain": Sj, "subdomain_ptr": Sp,
                                              "inv_subblock": Tx, "inv_subblock_ptr": Tp})]
        if n % 2 == 0:
            calls += [("block_jacobi", "block_jacobi", (), {"blocksize": 2, "Dinv": Dinv2, "omega": 0.8}),
                      ("block_gauss_seidel", "block_gauss_seidel", (), {"blocksize": 2, "Dinv": Dinv2,
                                                                         "sweep": "symmetric"})]
        fmts = [("csr", lambda A: A.tocsr())]
        if n % 2 == 0:
            fmts.append(("bsr2", lambda A: A.tobsr(blocksize=(2, 2))))
        for fname, conv in fmts:
            for cname, fn, args, kw in calls:
                if fname == "bsr2" and fn not in ("gauss_seidel", "jacobi", "sor", "polynomial", "block_jacobi",
                                                  "block_gauss_seidel"):
                    continue
                if fn == "gauss_seidel_nr":
                    A = A0.tocsc()
                else:
                    A = conv(A0.copy())
                x = x0.copy()
                getattr(R, fn)(A, x, b, *args, **kw)
                name = "%s_%s_%s@%s" % (cname, sname, fname, tag)
                store["cases"].append(name)
                store["arrays"]["%s__x0" % name] = x0
                store["arrays"]["%s__b" % name] = b
                store["arrays"]["%s__x" % name] = x
                meta = dict(fn=fn, system=sname, fmt=fname, dtype=tag,
                            args=[a.tolist() if isinstance(a, np.ndarray) else a for a in args])
                kwa = {}
                for k, v in kw.items():
                    if isinstance(v, np.ndarray):
                        store["arrays"]["%s__kw_%s" % (name, k)] = v
                    else:
                        kwa[k] = v
                meta["kwargs"] = kwa
                store["arrays"]["%s__call" % name] = np.array(json.dumps(meta))
                sysk = "system_%s@%s" % (sname, tag)
                if sysk + "__data" not in store["arrays"]:
                    store["arrays"][sysk + "__data"] = A0.data
                    store["arrays"][sysk + "__indices"] = A0.indices.astype(np.intc)
                    store["arrays"][sysk + "__indptr"] = A0.indptr.astype(np.intc)


def main():
    warnings.simplefilter("ignore")
    os.makedirs(OUT, exist_ok=True)
    pyamg = ref_env.stage()
    sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))
    import _amg_core as core
    rec, div = Recorder(), Recorder()
    for tag, dt in DTYPES.items():
        gen_kernels(core, rec, tag, dt)
        if np.dtype(dt).kind == "c":
            gen_complex_diagonals(core, rec, tag, dt)
            gen_division(core, div, tag, dt)
    rec.save(os.path.join(OUT, "kernels_dtypes.npz"))
    div.save(os.path.join(OUT, "division_dtypes.npz"))
    gen_ranges(core)
    store = {"cases": [], "arrays": {}}
    for tag, dt in DTYPES.items():
        gen_relaxation(pyamg, tag, dt, store)
    store["arrays"]["cases"] = np.array(store["cases"])
    path = os.path.join(OUT, "relaxation_dtypes.npz")
    np.savez_compressed(path, **store["arrays"])
    print("relaxation_dtypes.npz: %d cases, %.0f KB" % (len(store["cases"]), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
