"""TEST INFRASTRUCTURE: designed complex128 operators for the row kernels of the complex128 engine (csrc/hier_c128.hip:
csr_rows<T, Epi>, bsr_rows<T, Epi>, dense_apply<T>), on the patterns of tests/multi_cases.py, and the NumPy model
tests/test_gpu_c128_rows.py holds the device to.  tests/test_c128_cases_host.py checks the shapes and the model.
Nothing here needs a GPU."""
import numpy as np

import c128_cycle
import multi_cases as mc

# RESTATEMENTS of csrc/typed_kernels.hpp, which csr_rows uses: the rows of one workgroup (one thread per row) and the
# products staged in LDS at a time.  bsr_rows runs one thread per point row in workgroups of VEC_WG = 256.
ROWS_PER_WG = 256
CHUNK = 1024
N1 = mc.N1
GUARD = complex(mc.GUARD, -mc.GUARD)

CSR_FAMILIES = ("short_1", "short_255", "short_256", "short_257", "short_769", "short_staged_1100", "medium",
                "long_staged", "empty_300")
BSR_PATTERNS = ("short_257", "medium", "short_staged_1100")         # block rows 257, 300, 1100
BSR_TRANSFER_FAMILIES = ("short_256", "medium", "short_staged_1100", "long_staged")     # even n0: R in 1 x 2, P in 2 x 1 blocks


def complex_values(seed, real):
    """complex values on the pattern of `real` (any shape): the real parts as given, the imaginary parts from a second
    seeded draw in (-1, 1); an explicit zero stays 0 + 0i; about 6 % of the entries are purely real and 6 % purely imaginary"""
    rng = np.random.RandomState(seed)
    real = np.asarray(real, dtype=np.float64)
    imag = rng.uniform(-1.0, 1.0, size=real.shape)
    pick = rng.rand(*real.shape)
    re = np.where((pick >= 0.06) & (pick < 0.12), 0.0, real)
    im = np.where(pick < 0.06, 0.0, imag)
    zero = real == 0.0
    re[zero], im[zero] = 0.0, 0.0
    out = np.empty(real.shape, dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def complex_vector(seed, n):
    """n + 1 values in the unit square with some -0.0 parts and a few values six orders of magnitude larger; the last
    one is the guard"""
    rng = np.random.RandomState(seed)
    v = np.empty(n + 1, dtype=np.complex128)
    re, im = rng.uniform(-1.0, 1.0, n + 1), rng.uniform(-1.0, 1.0, n + 1)
    re[rng.rand(n + 1) < 0.03] = -0.0
    im[rng.rand(n + 1) < 0.03] = -0.0
    big = rng.rand(n + 1) < 0.02
    re[big] *= 1e6
    v.real, v.imag = re, im
    v[n] = GUARD
    return v


class Bsr(object):
    """an operator in the engine's terms: nrows x ncols point rows and columns, R x C blocks (1 x 1 with bsr False: CSR),
    Ap / Aj over block rows, Ax (nnzb, R, C) complex128"""

    def __init__(self, nrows, ncols, R, C, Ap, Aj, Ax, bsr):
        self.nrows, self.ncols, self.R, self.C, self.bsr = nrows, ncols, R, C, bsr
        self.Ap = np.ascontiguousarray(Ap, dtype=np.intc)
        self.Aj = np.ascontiguousarray(Aj, dtype=np.intc)
        self.Ax = np.ascontiguousarray(Ax, dtype=np.complex128).reshape(-1, R, C)
        self.nb = nrows // R
        assert nrows % R == 0 and ncols % C == 0 and len(self.Ap) == self.nb + 1 and len(self.Ax) == len(self.Aj) == self.Ap[-1]


def complex_csr(csr, seed):
    n, nc, Ap, Aj, Ax = csr
    return Bsr(n, nc, 1, 1, Ap, Aj, complex_values(seed, Ax), False)


def complex_bsr(csr, R, C, seed):
    """R x C blocks on the block pattern `csr`: the pattern's value in the block's first entry (so a block on the
    pattern's explicit zeros is a zero block), fresh draws in the others"""
    nb, ncb, Ap, Aj, Ax = csr
    rng = np.random.RandomState(seed)
    real = rng.uniform(-1.0, 1.0, size=(len(Ax), R, C))
    real[rng.rand(len(Ax), R, C) < 0.02] = 0.0
    real[:, 0, 0] = Ax
    real[Ax == 0.0] = 0.0
    return Bsr(nb * R, ncb * C, R, C, Ap, Aj, complex_values(seed + 1, real), True)


# ---------------------------------------------------------------------------------------------- the model
def _products(a, x):
    """each complex product in four real products, one difference and one sum, every one a rounding of its own
    (scalar.hpp mul: (a.re x.re - a.im x.im, a.re x.im + a.im x.re); c128_cycle.dense_apply forms them the same way)"""
    pr = np.subtract(np.multiply(a.real, x.real), np.multiply(a.imag, x.imag))
    pi = np.add(np.multiply(a.real, x.imag), np.multiply(a.imag, x.real))
    return pr, pi


def rows_through(A, v):
    """y = A v as csr_rows / bsr_rows sum it: point row p = i R + r from 0 + 0i over the blocks of block row i in stored
    order, the columns of a block left to right, real and imaginary sums apart"""
    v = np.asarray(v, dtype=np.complex128)
    y = np.zeros(A.nrows, dtype=np.complex128)
    cols = np.arange(A.C)
    for i in range(A.nb):
        s, e = int(A.Ap[i]), int(A.Ap[i + 1])
        if e == s:
            continue
        xv = v[(A.Aj[s:e, None].astype(np.int64) * A.C + cols[None, :]).ravel()]
        for r in range(A.R):
            pr, pi = _products(A.Ax[s:e, r, :].ravel(), xv)
            y[i * A.R + r] = complex(np.add.accumulate(np.concatenate(([0.0], pr)))[-1],
                                     np.add.accumulate(np.concatenate(([0.0], pi)))[-1])
    return y


def csub(a, b):
    out = np.empty(len(a), dtype=np.complex128)
    out.real, out.imag = np.subtract(a.real, b.real), np.subtract(a.imag, b.imag)
    return out


def cadd(a, b):
    out = np.empty(len(a), dtype=np.complex128)
    out.real, out.imag = np.add(a.real, b.real), np.add(a.imag, b.imag)
    return out


def transfer_cycle(A, R, P, M, b, x):
    """x + P (M (R (b - A x))): EpiResid, EpiStore, dense_apply, EpiAdd"""
    r = csub(b, rows_through(A, x))
    bc = rows_through(R, r)
    xc = c128_cycle.dense_apply(M, bc)
    return cadd(x, rows_through(P, xc))


# ---------------------------------------------------------------------------------------------- cases
class ApplyCase(object):
    """A (square) with an operand x and the model's y = A x; x and y carry a guard entry behind the last"""

    def __init__(self, name, A, seed):
        self.name, self.A = name, A
        self.x = complex_vector(seed, A.ncols)
        self._y = None

    def __repr__(self):
        return self.name

    def want(self):
        if self._y is None:
            self._y = rows_through(self.A, self.x[:-1])
            self._y.setflags(write=False)
        return self._y


class TransferCase(object):
    """A, R, P, a dense coarse M, b and x0, and the model's cycle"""

    def __init__(self, name, A, R, P, seed):
        self.name, self.A, self.R, self.P = name, A, R, P
        n1 = R.nrows
        rng = np.random.RandomState(seed)
        self.M = (rng.uniform(-1.0, 1.0, size=(n1, n1)) + 1j * rng.uniform(-1.0, 1.0, size=(n1, n1))).astype(np.complex128)
        self.A1 = Bsr(n1, n1, 1, 1, np.arange(n1 + 1), np.arange(n1), np.ones(n1, dtype=np.complex128), False)
        self.b = complex_vector(seed + 1, A.nrows)
        self.x0 = complex_vector(seed + 2, A.nrows)
        self._x = None

    def __repr__(self):
        return self.name

    def want(self):
        if self._x is None:
            self._x = transfer_cycle(self.A, self.R, self.P, self.M, self.b[:-1], self.x0[:-1])
            self._x.setflags(write=False)
        return self._x


_CACHE = {}


def _seed(name):
    return 9000 + sum(map(ord, name))


def apply_cases():
    if "apply" not in _CACHE:
        C = mc.by_name()
        out = [ApplyCase("csr_" + f, complex_csr(C[f].A, _seed(f)), _seed(f) + 1) for f in CSR_FAMILIES]
        for bs in (2, 3):
            for f in BSR_PATTERNS:
                name = "bsr%d_%s" % (bs, f)
                out.append(ApplyCase(name, complex_bsr(C[f].A, bs, bs, _seed(name)), _seed(name) + 2))
        _CACHE["apply"] = out
    return _CACHE["apply"]


def transfer_cases():
    if "transfer" not in _CACHE:
        C = mc.by_name()
        out = []
        for f in CSR_FAMILIES:
            c, s = C[f], _seed("t" + f)
            out.append(TransferCase("csr_" + f, complex_csr(c.A, s), complex_csr(c.R, s + 1), complex_csr(c.P, s + 2), s + 3))
        for f in BSR_TRANSFER_FAMILIES:
            c, s = C[f], _seed("b" + f)
            nh = c.n // 2
            R = complex_bsr(mc.restriction(nh, s, with_long=(f in mc.LONG_FAMILIES)), 1, 2, s + 1)
            P = complex_bsr(mc.prolongation(nh, s + 2, sparse_rows=False), 2, 1, s + 3)
            out.append(TransferCase("bsr_" + f, complex_csr(c.A, s + 4), R, P, s + 5))
        _CACHE["transfer"] = out
    return _CACHE["transfer"]


# ---------------------------------------------------------------------------------------------- shape properties
def straddling_rows(A, chunk=CHUNK, rows=ROWS_PER_WG):
    """CSR: rows with entries in two chunks or more of their workgroup's slice"""
    return mc.straddling_rows((A.nrows, A.ncols, A.Ap, A.Aj, None), rows, chunk)


def empty_workgroups(A, rows=ROWS_PER_WG):
    return mc.empty_workgroups((A.nrows, A.ncols, A.Ap, A.Aj, None), rows)


def bit_mismatches(a, b):
    return c128_cycle.bit_mismatches(np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128))
