"""pyamg_amd.krylov_c128 on the MI355X: the device-resident cg, bicgstab, gmres and fgmres around the complex128 cycle
reproduce the reference's histories (tests/golden/accel_c128/); the device-vector cycle and operator, the fixed-order
inner product, the BLAS-1 kernels and the Householder sequences are checked on their own through the C ABI."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sps

import accel_c128
import c128_cycle
import krylov_host_c128

pytestmark = pytest.mark.gpu
NAMES = accel_c128.names()
# run through the direct call (the first has restrt, which ml.solve does not pass on); the others through ml.solve
DIRECT = ("gs_sym_V_shifted2d__gmres", "cheb2_magnetic3d__bicgstab")
U = 1.2e-16           # a little above the unit roundoff 2^-53, as the bounds below are first-order
PARTIALS, SLOTS, WG = 512, 8, 256

_ML = {}


def ml_of(case):
    """the device hierarchy of a hier_c128 fixture, built once"""
    if case not in _ML:
        g = c128_cycle.load(case)
        _ML[case] = (c128_cycle.build_ml(g), g)
    return _ML[case]


def same(a, b):
    return c128_cycle.bit_mismatches(np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)) == 0


def run(name, direct):
    from pyamg_amd import krylov_c128
    f = accel_c128.load(name)
    m = f["meta"]
    ml, g = ml_of(f["case"])
    fn = krylov_c128.METHODS[m["method"]]
    res = []
    if direct:
        x, info = fn(ml.levels[0].A, f["b"], x0=accel_c128.x0_of(f), tol=m["tol"], restrt=m["restrt"],
                     maxiter=m["maxiter"], M=ml.aspreconditioner(cycle=m["cycle"]), residuals=res)
        assert info == 0
    else:
        x = ml.solve(f["b"], x0=accel_c128.x0_of(f), tol=m["tol"], maxiter=m["maxiter"], cycle=m["cycle"], accel=fn,
                     residuals=res)
    return f, x, res


# --------------------------------------------------------------------------- 1. the reference's histories
@pytest.mark.parametrize("name", NAMES)
def test_history_matches_reference(name):
    """iteration count equal, history within rtol 1e-9 / atol 1e-13 res[0], x within 1e-10: the rule of the float64
    device PCG.  On the host the numpy restatements (other summation orders in norms and inner products) deviate from
    these reference histories by at most 3e-16 res[0] (test_krylov_c128_host.py prints the figures)."""
    f, x, res = run(name, name in DIRECT)
    assert x.dtype == np.complex128 and x.shape == f["b"].shape
    assert all(type(r) is float for r in res)
    accel_c128.assert_matches(res, x, f["residuals"], f["x"], name)


def test_callbacks():
    from pyamg_amd import krylov_c128
    f = accel_c128.load("cheb2_magnetic3d__cg")
    m = f["meta"]
    ml, g = ml_of(f["case"])
    A = ml.levels[0].A
    xs, res = [], []
    x = ml.solve(f["b"], tol=m["tol"], maxiter=m["maxiter"], accel=krylov_c128.cg, residuals=res,
                 callback=lambda xk: xs.append(np.array(xk)))
    assert len(xs) == len(res) - 1 and same(xs[-1], x)
    assert all(v.dtype == np.complex128 and v.shape == f["b"].shape for v in xs)
    f = accel_c128.load("cheb2_magnetic3d__gmres")
    m = f["meta"]
    seen, res = [], []
    krylov_c128.gmres(A, f["b"], tol=m["tol"], maxiter=m["maxiter"], M=ml.aspreconditioner(), residuals=res,
                      callback=seen.append)
    assert seen == res[1:] and all(type(v) is float for v in seen)


# --------------------------------------------------------------------------- 2. M and A on device vectors
@pytest.mark.parametrize("case", sorted(set(n.split("__")[0] for n in NAMES)))
def test_cycle_and_operator_on_device_vectors(case):
    from pyamg_amd import krylov_c128
    ml, g = ml_of(case)
    A = g["levels"][0]["A"]
    with krylov_c128.DeviceSpaceC128(ml.device_hierarchy(), g["meta"]["cycle"]) as V:
        b = V.upload(g["b"])
        out = V.new()
        before = ml.device_hierarchy().device_bytes()
        V.M(b, out)
        assert same(V.download(out), g["Mb"])
        assert same(V.download(b), g["b"])
        x = g["x"]
        xd = V.upload(x)
        V.A(xd, out)
        y = V.download(out)
        assert ml.device_hierarchy().device_bytes() == before + 16 * len(x)
    assert ml.device_hierarchy().device_bytes() == before - 2 * 16 * len(x)
    Ac = sps.csr_matrix(A)
    absAx = abs(Ac) @ np.abs(x)
    nnz_row = np.diff(Ac.indptr)
    assert np.all(np.abs(y - A @ x) <= (nnz_row + 4) * 2.3e-16 * absAx)


# --------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("name", ["cheb2_magnetic3d__gmres", "jacobi_F_x0_magnetic2d__bicgstab", "sa_default_magnetic2d__cg",
                                  "sor_W_shifted2d__fgmres"])
def test_two_runs_are_bit_identical(name):
    _, x1, r1 = run(name, False)
    _, x2, r2 = run(name, False)
    assert same(x1, x2) and r1 == r2


# --------------------------------------------------------------------------- the C ABI on vectors of any length
class Vectors(object):
    """device vectors of any length on the stream and scratch of one small hierarchy"""

    def __init__(self):
        from pyamg_amd import _lib
        self.check = _lib.check
        self.L = _lib.lib()
        ml, _ = ml_of("one_level")
        self.h = ml.device_hierarchy().h
        self.stream = self.L.amg_hierx_stream(self.h)
        self.scratch = self.L.amg_hierx_scratch(self.h)
        assert self.stream and self.scratch
        self.owned = []

    def up(self, a):
        a = np.ascontiguousarray(a, dtype=np.complex128)
        p = self.L.amg_hierx_vec_alloc(self.h, len(a))
        assert p
        self.owned.append((p, len(a)))
        self.check(self.L.amg_devx_copy(p, a.ctypes.data, len(a), 0, self.stream))
        return p

    def down(self, p, n):
        out = np.empty(n, dtype=np.complex128)
        self.check(self.L.amg_devx_copy(out.ctypes.data, p, n, 1, self.stream))
        return out

    def slot(self, k):
        return self.down(self.scratch + 16 * (PARTIALS + k), 1)[0]

    def pointers(self, W):
        return (C.c_void_p * max(1, len(W)))(*W), len(W)

    def free(self):
        for p, n in self.owned:
            self.L.amg_hierx_vec_free(self.h, p, n)
        self.owned = []


@pytest.fixture
def vec():
    v = Vectors()
    yield v
    v.free()


def operands(n, seed, single=False):
    """random complex vectors with -0.0 entries; single: every part a float32 value, so that the four products of
    conj(x_i) y_i are exact in float64"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(2):
        v = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
        if single:
            v = v.astype(np.complex64).astype(np.complex128)
        v.real[::7] = -0.0
        v.imag[3::11] = -0.0
        out.append(v)
    return out


def chain(n):
    """the longest chain of additions in zdotc as written (csrc/krylov_c128.hip): one inside a product's part, a
    thread's strided sum over ceil(n / (512 * 256)) entries (from zero), the workgroup's tree of 8 levels, the final
    workgroup's strided sum over 512 / 256 = 2 partial sums (from zero) and its tree of 8 levels"""
    return 1 + -(-n // (PARTIALS * WG)) + 8 + PARTIALS // WG + 8


LENGTHS = [1, 63, 64, 65, 255, 256, 257, PARTIALS * WG + 1]       # the last: one past a full grid of the first stage


# --------------------------------------------------------------------------- 4. reduction and BLAS-1
@pytest.mark.parametrize("n", LENGTHS)
def test_zdotc(vec, n):
    x, y = operands(n, n, single=True)
    xd, yd = vec.up(x), vec.up(y)
    r = (C.c_double * 2)()
    vec.check(vec.L.amg_devx_zdotc(xd, yd, n, vec.scratch, 2, r, vec.stream))
    got = complex(r[0], r[1])
    assert same([got], [vec.slot(2)])
    re = math.fsum(np.concatenate([x.real * y.real, x.imag * y.imag]).tolist())         # exact products, exact sum
    im = math.fsum(np.concatenate([x.real * y.imag, -(x.imag * y.real)]).tolist())
    bound = (chain(n) + 3) * U * float(np.sum(np.abs(x) * np.abs(y)))
    print("n %d  error %.3e %.3e  bound %.3e" % (n, abs(got.real - re), abs(got.imag - im), bound))
    assert abs(got.real - re) <= bound and abs(got.imag - im) <= bound
    again = (C.c_double * 2)()
    vec.check(vec.L.amg_devx_zdotc(xd, yd, n, vec.scratch, 3, again, vec.stream))
    assert (again[0], again[1]) == (r[0], r[1])
    assert same([vec.slot(2)], [got])                                                     # slot 2 untouched by slot 3


def cmul(a, x):
    """a x with the complex product spelled as separate real operations (each correctly rounded, no contraction)"""
    a = np.broadcast_to(np.asarray(a, dtype=np.complex128), np.shape(x))
    out = np.empty(np.shape(x), dtype=np.complex128)
    out.real = np.subtract(np.multiply(a.real, x.real), np.multiply(a.imag, x.imag))
    out.imag = np.add(np.multiply(a.real, x.imag), np.multiply(a.imag, x.real))
    return out


def cadd(a, b):
    out = np.empty(np.shape(a), dtype=np.complex128)
    out.real, out.imag = np.add(a.real, b.real), np.add(a.imag, b.imag)
    return out


@pytest.mark.parametrize("n", LENGTHS)
def test_blas1_bits(vec, n):
    L, st = vec.L, vec.stream
    x, y = operands(n, 100 + n)
    a = complex(0.37, -1.21)
    xd, yd, od = vec.up(x), vec.up(y), vec.up(np.zeros(n))
    # y += a x
    vec.check(L.amg_devx_axpy(yd, xd, a.real, a.imag, n, st))
    want = cadd(y, cmul(a, x))
    assert same(vec.down(yd, n), want)
    # y += (f slot) x, the scalar read on the device
    vec.check(L.amg_devx_zdotc(xd, yd, n, vec.scratch, 4, None, st))
    s = vec.slot(4)
    f = -2.0
    vec.check(L.amg_devx_axpy_slot(yd, xd, vec.scratch, 4, f, n, st))
    want = cadd(want, cmul(complex(np.multiply(s.real, f), np.multiply(s.imag, f)), x))
    assert same(vec.down(yd, n), want)
    # p = beta p + z
    vec.check(L.amg_devx_xpby(yd, a.imag, a.real, xd, n, st))
    want = cadd(cmul(complex(a.imag, a.real), want), x)
    assert same(vec.down(yd, n), want)
    # out = c x; out = a - b
    vec.check(L.amg_devx_scale(od, xd, a.real, a.imag, n, st))
    assert same(vec.down(od, n), cmul(a, x))
    vec.check(L.amg_devx_sub(od, xd, yd, n, st))
    diff = np.empty(n, dtype=np.complex128)
    diff.real, diff.imag = np.subtract(x.real, want.real), np.subtract(x.imag, want.imag)
    assert same(vec.down(od, n), diff)
    # fill and copy from an element offset; one entry poked and peeked
    off = n // 3
    vec.check(L.amg_devx_fill(od + 16 * off, -0.0, 2.5, n - off, st))
    vec.check(L.amg_devx_copy(yd + 16 * off, xd + 16 * off, n - off, 2, st))
    one = np.array([complex(-0.0, 7.0)])
    vec.check(L.amg_devx_copy(od + 16 * (n - 1), one.ctypes.data, 1, 0, st))
    filled = np.concatenate([diff[:off], np.full(n - off, complex(-0.0, 2.5))])
    filled[n - 1] = one[0]
    assert same(vec.down(od, n), filled)
    assert same(vec.down(yd, n), np.concatenate([want[:off], x[off:]]))
    assert same(vec.down(od + 16 * (n - 1), 1), one)


# --------------------------------------------------------------------------- 5. Householder sequences
def reflector_bound(n, normv, alpha_abs):
    """the device's error, in the 2-norm, of one reflection v - 2 <w, v> w with ||w|| = 1.  The inner product is off by
    at most (chain + 3) U sum |w_i| |v_i| <= (chain + 3) U ||v|| per component (test_zdotc), sqrt(2) of that in modulus,
    and enters as 2 |d alpha| ||w||; the update rounds each component's two products, their sum and the final sum:
    below 6 U (||v|| + 2 |alpha|) in norm.  Reflections are unitary, so later ones carry the error on unchanged."""
    return 2 * math.sqrt(2) * (chain(n) + 3) * U * normv + 6 * U * (normv + 2 * alpha_abs)


@pytest.mark.parametrize("order", ["ascending", "descending", "horner"])
@pytest.mark.parametrize("k", [0, 1, 5])
@pytest.mark.parametrize("n", [2, 65, 1000])
def test_householder_sequences(vec, n, k, order):
    horner, descending = order == "horner", order != "ascending"       # the Horner scheme runs from the last one down
    k = min(k, n)
    rng = np.random.RandomState(7 * n + k)
    W = []
    for _ in range(k + 1):                     # one more than is applied: the range must leave it alone
        w = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
        W.append(w / np.linalg.norm(w))
    v = operands(n, 3 * n + k)[0]
    y = operands(n, 5 * n + k)[1]
    order = list(range(k - 1, -1, -1)) if descending else list(range(k))
    start, stop, step = (k - 1, -1, -1) if descending else (0, k, 1)
    # the sequential loop (amg_core/krylov.h:34-53, 97-120) in extended precision
    ref = v.astype(np.clongdouble)
    bound = 0.0
    for j in order:
        if horner:
            ref[j] += y[j]
        alpha = np.vdot(W[j].astype(np.clongdouble), ref)
        bound += reflector_bound(n, float(np.linalg.norm(ref)), float(abs(alpha)))
        ref = ref - 2 * alpha * W[j].astype(np.clongdouble)
    vd = vec.up(v)
    arr, nW = vec.pointers([vec.up(w) for w in W])
    if horner:
        vec.check(vec.L.amg_devx_horner(vd, arr, nW, vec.up(y), n, start, stop, step, vec.scratch, vec.stream))
    else:
        vec.check(vec.L.amg_devx_householders(vd, arr, nW, n, start, stop, step, vec.scratch, vec.stream))
    got = vec.down(vd, n)
    err = float(np.linalg.norm(got.astype(np.clongdouble) - ref))
    print("n %d k %d  error %.3e  bound %.3e" % (n, k, err, bound))
    if k == 0:
        assert same(got, v)
    assert err <= bound
    for p, w in zip(arr, W):
        assert same(vec.down(p, n), w)


def test_householder_range_is_checked(vec):
    v = vec.up(np.ones(4))
    arr, nW = vec.pointers([vec.up(np.ones(4))])
    for start, stop, step in ((0, 2, 1), (1, -1, -1), (0, 1, 0), (0, -2, -1)):
        with pytest.raises(ValueError):
            vec.check(vec.L.amg_devx_householders(v, arr, nW, 4, start, stop, step, vec.scratch, vec.stream))


def test_inner_iterations_cost_a_fixed_number_of_host_reads(monkeypatch):
    """the float64 module reads one inner product per reflector: O(inner) synchronisations in inner iteration `inner`;
    here the count does not depend on it"""
    from pyamg_amd import krylov_c128
    spaces = []
    base = krylov_c128.DeviceSpaceC128

    class Recording(base):
        def __init__(self, *a, **k):
            base.__init__(self, *a, **k)
            spaces.append(self)
    monkeypatch.setattr(krylov_c128, "DeviceSpaceC128", Recording)
    f = accel_c128.load("cheb2_magnetic3d__gmres")
    ml, g = ml_of(f["case"])
    reads = []
    krylov_c128.gmres(ml.levels[0].A, f["b"], tol=1e-30, maxiter=12, M=ml.aspreconditioner(),
                      callback=lambda r: reads.append(spaces[0].host_reads))
    assert len(reads) == 12              # inner iterations 0 .. 10, then the true residual after the cycle
    per_inner = np.diff([0] + reads[:11])
    print("host reads per inner iteration:", per_inner.tolist())
    assert per_inner[3] == per_inner[10] and per_inner[3] > 0


# --------------------------------------------------------------------------- 6. small-system edges
def small_ml():
    """two levels, 6 unknowns: a complex shifted 1-D Laplacian, pairwise aggregates, Jacobi as smoother and -- two
    sweeps -- as coarse solver (with an exact coarse solve M A has the eigenvalue 1 three times over, the Krylov space
    is exhausted after four steps and the sixth inner iteration is never reached)"""
    import pyamg_amd
    n = 6
    A = sps.diags([-np.ones(n - 1), (2 + 0.5j) * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr",
                  dtype=np.complex128)
    P = sps.csr_matrix(np.kron(np.eye(n // 2), np.ones((2, 1))))
    l0, l1 = pyamg_amd.multilevel_solver.level(), pyamg_amd.multilevel_solver.level()
    l0.A, l0.P, l0.R = A, P, P.T.tocsr()
    l1.A = sps.csr_matrix(P.T @ A @ P)
    ml = pyamg_amd.multilevel_solver([l0, l1], coarse_solver=("jacobi", {"iterations": 2}))
    pyamg_amd.change_smoothers(ml, ("jacobi", {"omega": 2.0 / 3.0}), ("jacobi", {"omega": 2.0 / 3.0}))
    return ml


@pytest.mark.parametrize("method", ["gmres", "fgmres"])
def test_as_many_inner_iterations_as_unknowns(method):
    """maxiter = n = 6: the last inner iteration has inner == n - 1 (no reflector, no rotation)"""
    from pyamg_amd import krylov_c128
    ml = small_ml()
    A = ml.levels[0].A
    M = ml.aspreconditioner()
    rng = np.random.RandomState(2)
    b = rng.rand(6) + 1j * rng.rand(6)
    x0 = rng.rand(6) - 1j * rng.rand(6)
    xr, ref, _ = krylov_host_c128.METHODS[method](lambda v: A @ v, lambda v: M * v, b, x0, 1e-30, maxiter=6)
    res = []
    x, info = krylov_c128.METHODS[method](A, b, x0=x0, tol=1e-30, maxiter=6, M=M, residuals=res)
    assert len(ref) == 7                 # no early exit: inner iterations 0 .. 5 all ran
    accel_c128.assert_matches(res, x, ref, xr, method)
