"""The float64 device vector kernels (the amg_dev_* entries of include/amgcore_hip.h, csrc/kernels.hip "vector kernels"
and "2-norm") and krylov.DeviceSpace on the MI355X, against tests/vector_models.py: the reductions and every
elementwise, gather and dense kernel bit for bit, at the lengths where a grid wraps, a workgroup ends or the grid is
capped; the Householder sequences within a derived bound; the nine Krylov methods against the same bodies on host
arrays.  tests/test_vector_models_host.py checks the models themselves."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sps

import accel_c128
import krylov_numpy
import vector_models as vm

pytestmark = pytest.mark.gpu
U, S = vm.U, vm.S
H2D, D2H, D2D = 0, 1, 2


def header_constant(name):
    """a #define of include/amgcore_hip.h (an integer, or AMG_DEV_PARTIALS + integer)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "amgcore_hip.h")
    with open(path) as f:
        m = re.search(r"^#define\s+%s\s+\(?(AMG_DEV_PARTIALS\s*\+\s*)?(\d+)\)?\s*$" % name, f.read(), re.M)
    assert m, name
    return int(m.group(2)) + (header_constant("AMG_DEV_PARTIALS") if m.group(1) else 0)


class Vectors(object):
    """device vectors of any length on the stream and scratch of a one-level device operator"""

    def __init__(self):
        from pyamg_amd import _lib
        from pyamg_amd.util import _DeviceOperator
        self.check = _lib.check
        self.L = _lib.lib()
        self.op = _DeviceOperator(sps.identity(4, format="csr"))
        self.bytes_before = self.op.device_bytes()
        self.stream = self.L.amg_hier_stream(self.op.h)
        self.scratch = self.L.amg_hier_scratch(self.op.h)
        assert self.scratch
        self.owned = []

    def alloc(self, n):
        p = self.L.amg_dev_alloc(n)
        assert p
        self.owned.append(p)
        return p

    def up(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = self.alloc(len(a))
        self.check(self.L.amg_dev_copy(p, a.ctypes.data, len(a), H2D, self.stream))
        return p

    def down(self, p, n):
        out = np.empty(n, dtype=np.float64)
        self.check(self.L.amg_dev_copy(out.ctypes.data, p, n, D2H, self.stream))
        return out

    def dot_host(self, x, y, n):
        r = C.c_double(-1.0)
        self.check(self.L.amg_dev_dot_host(x, y, n, self.scratch, C.byref(r), self.stream))
        return r.value

    def norm_host(self, x, n):
        r = C.c_double(-1.0)
        self.check(self.L.amg_dev_norm_host(x, n, self.scratch, C.byref(r), self.stream))
        return r.value

    def free(self):
        for p in self.owned:
            self.L.amg_dev_free(p)
        self.owned = []
        self.op.close()


@pytest.fixture
def vec():
    v = Vectors()
    yield v
    v.free()


def same(a, b):
    return vm.bit_mismatches(a, b) == 0


# --------------------------------------------------------------------------- 1. reductions
@pytest.mark.parametrize("single", [False, True], ids=["general", "single"])
@pytest.mark.parametrize("n", vm.RED)
def test_reductions_bits(vec, n, single):
    """amg_dev_dot_host / amg_dev_norm_host, amg_dev_dot / amg_dev_norm2 into device slots and amgcore_norm2_f64 give
    the bits of the restated order.  single: products and squares are exact, so the results also lie within
    (chain + 3) U sum |x_i y_i| of the exact sums (vector_models.dot_bound, norm_bound).  The device vectors hold a NaN
    one past the n entries: a kernel that read past its range would return it."""
    from pyamg_amd import _lib
    L, st = vec.L, vec.stream
    x, y = vm.operands(n, n, single=single)
    xd, yd, slots = vec.up(np.append(x, np.nan)), vec.up(np.append(y, np.nan)), vec.up(np.full(4, -7.0))
    want_dot, want_norm = vm.device_order_dot(x, y), vm.device_order_norm(x)
    dot, norm = vec.dot_host(xd, yd, n), vec.norm_host(xd, n)
    assert same(dot, want_dot) and same(norm, want_norm)
    # a device result slot; a second call into another slot repeats the bits and leaves the first alone
    vec.check(L.amg_dev_dot(xd, yd, n, vec.scratch, slots, st))
    vec.check(L.amg_dev_dot(xd, yd, n, vec.scratch, slots + 8, st))
    vec.check(L.amg_dev_norm2(xd, n, vec.scratch, slots + 16, st))
    vec.check(L.amg_dev_norm2(xd, n, vec.scratch, slots + 24, st))
    assert same(vec.down(slots, 4), [want_dot, want_dot, want_norm, want_norm])
    out = C.c_double(-1.0)
    vec.check(L.amgcore_norm2_f64(_lib.dp(x), n, C.byref(out)))
    assert same(out.value, want_norm)
    assert same(vec.down(xd, n), x) and same(vec.down(yd, n), y)
    if single:
        p = x * y
        e_dot, b_dot = abs(dot - math.fsum(p.tolist())), vm.dot_bound(n, float(np.sum(np.abs(p))))
        sumsq = math.fsum((x * x).tolist())
        e_norm, b_norm = abs(norm - math.sqrt(sumsq)), vm.norm_bound(n, sumsq)
        print("n %d  dot error %.3e bound %.3e  norm error %.3e bound %.3e" % (n, e_dot, b_dot, e_norm, b_norm))
        assert e_dot <= b_dot and e_norm <= b_norm


@pytest.mark.parametrize("n", vm.RED)
def test_reductions_see_every_single_entry(vec, n):
    """one non-zero pair at p in zero vectors gives exactly x_p y_p and |x_p| (every other term is +0.0, every sum
    exact), a NaN at p gives NaN: no entry at a wave, workgroup or grid-wrap boundary is skipped or taken twice"""
    xd, yd = vec.up(np.append(np.zeros(n), np.nan)), vec.up(np.append(np.zeros(n), np.nan))    # NaN past the range
    xp, yp = np.array([-1.7]), np.array([0.3])
    zero, nan = np.zeros(1), np.array([np.nan])
    for p in vm.positions(n):
        vec.check(vec.L.amg_dev_copy(xd + 8 * p, xp.ctypes.data, 1, H2D, vec.stream))
        vec.check(vec.L.amg_dev_copy(yd + 8 * p, yp.ctypes.data, 1, H2D, vec.stream))
        assert vec.dot_host(xd, yd, n) == xp[0] * yp[0], p
        assert vec.norm_host(xd, n) == abs(xp[0]), p
        vec.check(vec.L.amg_dev_copy(xd + 8 * p, nan.ctypes.data, 1, H2D, vec.stream))
        assert math.isnan(vec.dot_host(xd, yd, n)) and math.isnan(vec.norm_host(xd, n)), p
        vec.check(vec.L.amg_dev_copy(xd + 8 * p, zero.ctypes.data, 1, H2D, vec.stream))
        vec.check(vec.L.amg_dev_copy(yd + 8 * p, zero.ctypes.data, 1, H2D, vec.stream))
    assert vec.dot_host(xd, yd, n) == 0.0 and vec.norm_host(xd, n) == 0.0


def test_reductions_of_nothing(vec):
    xd, slots = vec.up(np.ones(4)), vec.up(np.full(2, -7.0))
    assert vec.dot_host(xd, xd, 0) == 0.0 and vec.norm_host(xd, 0) == 0.0
    assert vec.L.amg_dev_dot(xd, xd, 0, vec.scratch, slots, vec.stream) == 0
    assert vec.L.amg_dev_norm2(xd, 0, vec.scratch, slots + 8, vec.stream) == 0
    assert same(vec.down(slots, 2), [0.0, 0.0])


def test_norm_is_the_unscaled_root_of_the_inner_product(vec):
    """the reference's norm is sqrt(inner(x, x)) (pyamg/util/linalg.py norm), not a scaled dnrm2: squares that overflow
    give inf, squares that underflow give 0"""
    assert vec.norm_host(vec.up([1e200, 1e200]), 2) == math.inf
    assert vec.norm_host(vec.up([1e-200]), 1) == 0.0


def test_scratch_holds_what_the_host_reductions_write(vec):
    """amg_hier_scratch allocates AMG_DEV_SCRATCH doubles (read off the hierarchy's byte count); of these a reduction
    at a full grid rewrites the AMG_DEV_PARTIALS partial sums and the host entries' one result slot,
    AMG_DEV_HOST_SLOT, and nothing else"""
    partials, size, slot = (header_constant(k) for k in ("AMG_DEV_PARTIALS", "AMG_DEV_SCRATCH", "AMG_DEV_HOST_SLOT"))
    allocated = (vec.op.device_bytes() - vec.bytes_before) // 8
    print("scratch: %d doubles allocated, %d promised, host result at %d" % (allocated, size, slot))
    assert partials == vm.MAX_BLOCKS and allocated >= size > slot >= partials
    n = 3 * S + 1
    x = vm.operands(n, 1)[0]
    xd = vec.up(x)
    for call in (lambda: vec.dot_host(xd, xd, n), lambda: vec.norm_host(xd, n)):
        vec.check(vec.L.amg_dev_fill(vec.scratch, -7.0, size, vec.stream))
        call()
        after = vec.down(vec.scratch, size)
        written = np.flatnonzero(after != -7.0)
        assert written.tolist() == list(range(partials)) + [slot]


# --------------------------------------------------------------------------- 2. elementwise kernels
def elementwise(vec, name, x, y, off, alias):
    """run one amg_dev_* entry on the entries [off, n) of fresh copies of x and y -> (result vector of n entries, its
    expected value).  alias: the operand the output is written over ("x" | "y") where the entry has an output
    argument of its own"""
    L, st = vec.L, vec.stream
    n = len(x) - off
    guard = np.full(len(x), -7.0)
    xd, yd, od = (vec.up(np.append(v, -7.0)) for v in (x, y, guard))         # one more entry, which must stay
    px, py, po = xd + 8 * off, yd + 8 * off, od + 8 * off
    xs, ys = x[off:], y[off:]
    before, res = x, xd                           # the in-place entries write over x
    if name == "scale":
        po, res, before = (px, xd, x) if alias == "x" else (po, od, guard)
        vec.check(L.amg_dev_scale(po, px, vm.CC, n, st))
        want = vm.scale(vm.CC, xs)
    elif name == "sub":
        po, res, before = {"x": (px, xd, x), "y": (py, yd, y), None: (po, od, guard)}[alias]
        vec.check(L.amg_dev_sub(po, px, py, n, st))
        want = vm.sub(xs, ys)
    elif name == "axpy":
        vec.check(L.amg_dev_axpy(px, py, n, st))
        want = vm.axpy(xs, ys)
    elif name == "axpy_scaled":
        vec.check(L.amg_dev_axpy_scaled(px, py, vm.CC, n, st))
        want = vm.axpy_scaled(xs, ys, vm.CC)
    elif name == "axmy":
        vec.check(L.amg_dev_axmy(px, py, vm.A, n, st))
        want = vm.axmy(xs, ys, vm.A)
    elif name == "scale_add":
        vec.check(L.amg_dev_scale_add(px, vm.BETA, py, n, st))
        want = vm.scale_add(xs, vm.BETA, ys)
    elif name == "divide":
        vec.check(L.amg_dev_divide(px, vm.DIV, n, st))
        want = vm.divide(xs, vm.DIV)
    elif name == "fill":
        vec.check(L.amg_dev_fill(px, -0.0, n, st))
        want = np.full(n, -0.0)
    else:
        raise KeyError(name)
    got = vec.down(res, len(x) + 1)
    inputs_kept = all(same(vec.down(d, len(x) + 1), np.append(h, -7.0)) for d, h in ((xd, x), (yd, y)) if d != res)
    for p in (xd, yd, od):
        L.amg_dev_free(p)
        vec.owned.remove(p)
    return got, np.concatenate([before[:off], want, [-7.0]]), inputs_kept


ENTRIES = [("scale", None), ("scale", "x"), ("sub", None), ("sub", "x"), ("sub", "y"), ("axpy", None),
           ("axpy_scaled", None), ("axmy", None), ("scale_add", None), ("divide", None), ("fill", None)]


@pytest.mark.parametrize("shifted", [False, True], ids=["whole", "offset"])
@pytest.mark.parametrize("n", vm.ELT)
def test_elementwise_bits(vec, n, shifted):
    """the seven elementwise entries and amg_dev_fill against their models, bit for bit (-0.0 counts), also with the
    output over an input, and -- offset -- on [off, n) with off = n // 3 | 1 odd (the pointer is 8-byte aligned
    only), where [0, off) must stay as it was"""
    off = (n // 3 | 1) if shifted else 0
    x, y = vm.elt_operands(n)
    bad = []
    for name, alias in ENTRIES:
        got, want, inputs_kept = elementwise(vec, name, x, y, off, alias)
        if not (same(got, want) and inputs_kept):
            bad.append((name, alias, vm.bit_mismatches(got, want), inputs_kept))
    assert not bad, bad


@pytest.mark.parametrize("n", vm.ELT)
def test_fill_copy_norm_from_an_odd_offset(vec, n):
    """what the GMRES variants do on every inner iteration: fill, device-to-device copy and norm of [off, n)"""
    off = n // 3 | 1
    x, y = vm.elt_operands(n)
    xd, yd = vec.up(np.append(x, np.nan)), vec.up(np.append(y, np.nan))         # NaN past the range
    assert same(vec.norm_host(xd + 8 * off, n - off), vm.device_order_norm(x[off:]))
    vec.check(vec.L.amg_dev_copy(yd + 8 * off, xd + 8 * off, n - off, D2D, vec.stream))
    assert same(vec.down(yd, n + 1), np.concatenate([y[:off], x[off:], [np.nan]]))
    vec.check(vec.L.amg_dev_fill(xd + 8 * off, 2.5, n - off, vec.stream))
    assert same(vec.down(xd, n + 1), np.concatenate([x[:off], np.full(n - off, 2.5), [np.nan]]))


@pytest.mark.parametrize("n", vm.ELT)
def test_alloc_and_copies(vec, n):
    """amg_dev_alloc returns zeros; the three kinds of amg_dev_copy round-trip, also one entry poked and peeked"""
    L, st = vec.L, vec.stream
    x = vm.elt_operands(n)[0]
    a, b = vec.alloc(n), vec.alloc(n)
    assert same(vec.down(a, n), np.zeros(n))
    vec.check(L.amg_dev_copy(a, x.ctypes.data, n, H2D, st))
    vec.check(L.amg_dev_copy(b, a, n, D2D, st))
    assert same(vec.down(b, n), x)
    one = np.array([-0.0])
    vec.check(L.amg_dev_copy(b + 8 * (n - 1), one.ctypes.data, 1, H2D, st))
    assert same(vec.down(b + 8 * (n - 1), 1), one)
    assert same(vec.down(b, n), np.concatenate([x[:n - 1], one])) and same(vec.down(a, n), x)
    assert L.amg_dev_copy(b, a, 0, D2D, st) == 0


def up_ints(vec, idx):
    """int32 indices in device memory (amg_dev_copy moves 8-byte units)"""
    idx = np.ascontiguousarray(idx, dtype=np.intc)
    padded = np.concatenate([idx, np.zeros(len(idx) % 2, dtype=np.intc)])
    return vec.up(padded.view(np.float64))


@pytest.mark.parametrize("n", [255, 256, 257, vm.ELT_GRID + 1])
def test_gather_bits(vec, n):
    src = vm.operands(1000, 7)[0]
    rng = np.random.RandomState(n)
    idx = np.concatenate([np.arange(999, -1, -1), np.repeat(rng.randint(0, 1000, 40), 3), rng.randint(0, 1000, n)])[:n]
    sd, out = vec.up(src), vec.up(np.full(n + 1, -7.0))
    vec.check(vec.L.amg_dev_gather(out, sd, up_ints(vec, idx), n, vec.stream))
    assert same(vec.down(out, n + 1), np.concatenate([src[idx], [-7.0]]))
    assert same(vec.down(sd, 1000), src)
    vec.check(vec.L.amg_dev_gather(out, sd, up_ints(vec, idx), 0, vec.stream))        # n = 0: nothing happens
    assert same(vec.down(out, n + 1), np.concatenate([src[idx], [-7.0]]))


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 129, 300])
def test_dense_apply_bits(vec, n):
    """8 and 9: the edge of the unrolled loop; 63, 64, 65, 129: the edge of the 64-lane workgroups"""
    M = np.array([vm.operands(n, 11 * n + r)[0] for r in range(n)])
    b = vm.operands(n, 13 * n)[1]
    Mt, bd, out = vec.up(np.ravel(M.T)), vec.up(b), vec.up(np.full(n + 1, -7.0))
    vec.check(vec.L.amg_dev_dense_apply(Mt, bd, out, n, vec.stream))
    assert same(vec.down(out, n + 1), np.concatenate([vm.dense_apply_model(M, b), [-7.0]]))


# --------------------------------------------------------------------------- 3. DeviceSpace
class Counting(object):
    """the library, with the names of the entries called through it"""

    def __init__(self, L):
        self._L, self.calls = L, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._L, name)


class Space(object):
    """krylov.DeviceSpace(op, 0) over the n x n identity"""

    def __init__(self, n):
        from pyamg_amd import krylov
        from pyamg_amd.util import _DeviceOperator
        self.op = _DeviceOperator(sps.identity(n, format="csr"))
        self.op.level_size = lambda lvl: n
        self.V = krylov.DeviceSpace(self.op, 0)

    def __enter__(self):
        return self.V

    def __exit__(self, *exc):
        self.V.release()
        self.op.close()


def reflector_bound(n, normv, normw, alpha_abs):
    """the device's error, in the 2-norm, of one reflection v - 2 <w, v> w.  Every term of the inner product passes its
    product's rounding and at most chain_dot(n) additions, so the computed alpha is off by at most
    (chain_dot(n) + 1 + 3) U sum |w_i v_i| <= (chain_dot(n) + 4) U ||w|| ||v||  (vector_models.dot_bound with one more
    rounding; Cauchy-Schwarz), which enters the update as 2 |d alpha| ||w||.  The update w_i' = v_i - a w_i with
    a = 2 alpha (exact) rounds the product and the difference: U |a w_i| + U |v_i - a w_i| <= U (|v_i| + 2 |a| |w_i|)
    per entry, U (||v|| + 4 |alpha| ||w||) in norm to first order; it is doubled for the terms of second order and for
    alpha's own error in it.  ||w|| = 1 to rounding, so later reflections carry an error on unchanged."""
    return 2 * (vm.chain_dot(n) + 4) * U * normw * normv * normw + 2 * U * (normv + 4 * alpha_abs * normw)


@pytest.mark.parametrize("order", ["ascending", "descending", "horner"])
@pytest.mark.parametrize("k", [0, 1, 5])
@pytest.mark.parametrize("n", [2, 65, 1000, S + 1])
def test_householder_sequences(n, k, order):
    """reflect_range both ways and horner for k unit reflectors against the sequential loop in extended precision;
    k = 0 leaves v as it is, the reflectors keep their bits and the one past the range is not applied"""
    horner, descending = order == "horner", order != "ascending"
    k = min(k, n)
    rng = np.random.RandomState(7 * n + k)
    W = []
    for _ in range(k + 1):
        w = rng.uniform(-1, 1, n)
        W.append(w / np.linalg.norm(w))
    v = rng.uniform(-1, 1, n)
    v[::7] = -0.0
    y = rng.uniform(-1, 1, k + 1)
    ref = v.astype(np.longdouble)
    bound = 0.0
    for j in (range(k - 1, -1, -1) if descending else range(k)):
        wj = W[j].astype(np.longdouble)
        if horner:
            ref[j] += y[j]
            bound += U * float(abs(ref[j]))                    # the host's v[j] + y[j], rounded once
        alpha = np.dot(wj, ref)
        bound += reflector_bound(n, float(np.linalg.norm(ref)), float(np.linalg.norm(wj)), float(abs(alpha)))
        ref = ref - 2 * alpha * wj
    with Space(n) as V:
        vd = V.upload(v)
        Wd = [V.upload(w) for w in W]
        if horner:
            V.horner(vd, Wd, y, k - 1)
        elif descending:
            V.reflect_range(vd, Wd, k - 1, -1, -1)
        else:
            V.reflect_range(vd, Wd, 0, k, 1)
        got = V.download(vd)
        kept = [same(V.download(p), w) for p, w in zip(Wd, W)]
    err = float(np.linalg.norm(got.astype(np.longdouble) - ref))
    print("n %d k %d %s  error %.3e  bound %.3e" % (n, k, order, err, bound))
    if k == 0:
        assert same(got, v)
    assert err <= bound
    assert all(kept)


@pytest.mark.parametrize("n", [2, 65, 1000, S + 1])
def test_devicespace_offsets(n):
    """norm, fill and copy of [off, n) for off = 0, 1, n - 1 and n; at off = n the range is empty: norm is 0.0, nothing
    is launched and nothing raised"""
    x, y = vm.operands(n, 3 * n)
    with Space(n) as V:
        for off in (0, 1, n - 1, n):
            xd, yd = V.upload(x), V.upload(y)
            real = V.L
            V.L = Counting(real)
            norm = V.norm(xd, off)
            V.copy(yd, xd, off)
            V.fill(xd, -0.0, off)
            calls, V.L = V.L.calls, real
            assert same(norm, vm.device_order_norm(x[off:])), off
            assert same(V.download(yd), np.concatenate([y[:off], x[off:]])), off
            assert same(V.download(xd), np.concatenate([x[:off], np.full(n - off, -0.0)])), off
            assert calls == ([] if off == n else ["amg_dev_norm_host", "amg_dev_copy", "amg_dev_fill"]), off
            if off == n:
                assert norm == 0.0 and not np.signbit(norm)


# --------------------------------------------------------------------------- 4. whole methods, device against host
GRID = 20


def systems():
    """two small, well-conditioned systems, so that the recurrences do not amplify the difference between two orders
    of summation: the 5-point Laplacian on 20 x 20 plus 2 I (eigenvalues in (2, 10): condition number below 5), and a
    nonsymmetric, strictly diagonally dominant one of the same pattern (diagonal 6, off-diagonal sum 4)"""
    T = sps.diags([-np.ones(GRID - 1), np.zeros(GRID), -np.ones(GRID - 1)], [-1, 0, 1])
    I = sps.identity(GRID)
    spd = (sps.kron(I, T) + sps.kron(T, I) + 6.0 * sps.identity(GRID * GRID)).tocsr()
    Tx = sps.diags([-1.4 * np.ones(GRID - 1), np.zeros(GRID), -0.6 * np.ones(GRID - 1)], [-1, 0, 1])
    Ty = sps.diags([-0.7 * np.ones(GRID - 1), np.zeros(GRID), -1.3 * np.ones(GRID - 1)], [-1, 0, 1])
    nonsym = (sps.kron(I, Tx) + sps.kron(Ty, I) + 6.0 * sps.identity(GRID * GRID)).tocsr()
    for M in (spd, nonsym):
        M.sort_indices()
    return {"spd": spd, "nonsym": nonsym}


SYSTEM_OF = {"cg": "spd", "cr": "spd", "steepest_descent": "spd", "minimal_residual": "spd", "bicgstab": "nonsym",
             "gmres": "nonsym", "fgmres": "nonsym", "cgne": "nonsym", "cgnr": "nonsym"}
TOL, ITERATIONS = 1e-6, 15


def test_every_method_is_covered():
    from pyamg_amd import krylov
    assert sorted(SYSTEM_OF) == sorted(krylov.METHODS)


@pytest.mark.parametrize("method", sorted(SYSTEM_OF))
def test_method_on_device_matches_the_same_body_on_host(method, monkeypatch):
    """krylov.solve_host (DeviceSpace: the kernels above, and amg_hier_apply / amg_hier_apply_aux) against the same
    method body over tests/krylov_numpy.NumpyVectors, unpreconditioned, at most 15 iterations: the same return code,
    the same number of residuals, and history and x by the project's rule for the same method under another order of
    summation (accel_c128.assert_matches: rtol 1e-9, atol 1e-13 res[0], x to 1e-10).

    Measured on the MI355X (the figures are printed): the worst of the nine is gmres with max |res - ref| / ref
    1.2e-12 and |x - x_ref| / |x_ref| 1.2e-15; cg 1.3e-13 / 1.7e-16, fgmres 1.4e-13 / 1.5e-16, cr 1.0e-13 / 1.9e-16,
    bicgstab 8.2e-14 / 1.6e-16, the other four below 1.1e-14 / 2.3e-16.  Return codes agree (0 for cg, cr and
    bicgstab, the iteration count for the rest)."""
    from pyamg_amd import krylov
    A = systems()[SYSTEM_OF[method]]
    n = A.shape[0]
    rng = np.random.RandomState(5)
    b, x0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    restrt, maxiter = (5, ITERATIONS // 5) if method == "fgmres" else (None, ITERATIONS)
    # host
    V = krylov_numpy.NumpyVectors(A)
    bh, xh = V.upload(b), V.upload(x0)
    ref = []
    info_ref = krylov.run(method, V, bh, xh, TOL, maxiter, restrt=restrt, residuals=ref)
    x_ref = V.download(xh)
    assert 2 <= len(ref) <= ITERATIONS + 2, len(ref)
    # device: solve_host returns x alone, so the return code is taken where solve_host calls the method
    codes = []
    run = krylov.run
    monkeypatch.setattr(krylov, "run", lambda *a, **k: codes.append(run(*a, **k)) or codes[-1])
    res = []
    x = krylov.solve_host(A, b, x0, method, tol=TOL, maxiter=maxiter, restrt=restrt, residuals=res)
    print("%s: return code %s (host %s)" % (method, codes, info_ref))
    assert codes == [info_ref]
    accel_c128.assert_matches(res, x, ref, x_ref, method)
