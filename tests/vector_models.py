"""TEST INFRASTRUCTURE: NumPy restatements of the float64 device vector kernels (csrc/kernels.hip, "vector kernels" and
"2-norm"; csrc/devapi.hip), in the exact order of their floating-point operations, and the operands and lengths the
tests of them share.  tests/test_vector_models_host.py checks the models against exact sums before
tests/test_gpu_vector_kernels.py holds the kernels to them bit for bit.

The order of launch_dot and launch_norm2, as written: nb = min(max(ceil(n / 256), 1), 1024) workgroups of 256 threads;
thread t of workgroup g owns the entries g * 256 + t + j * nb * 256.  dot_stage1 sums their products one after the other
from 0.0; sumsq_stage1 sums their squares into two accumulators, s0 (j even) and s1 (j odd), and forms s0 + s1.  A
workgroup then reduces its 256 sums (block_reduce_sum): the wave64 butterfly with offsets 32, 16, 8, 4, 2, 1, of which
lane 0 keeps ((..(v_l + v_{l+32}) + (v_{l+16} + v_{l+48})..)), and thread 0 adds the four waves' sums from 0.0.  The
second stage is one workgroup: thread t sums the partial sums t, t + 256, ... from 0.0, and the same block reduction
follows; the norm takes the square root of the result.  The library is built with -ffp-contract=off, so every product
and every sum below is a rounding of its own -- NumPy's separate ufunc calls round the same way."""
import math

import numpy as np

U = 2.0 ** -53                      # unit roundoff of float64
WG, MAX_BLOCKS = 256, 1024          # threads of a workgroup; NORM_BLOCKS of kernels.hip
S = WG * MAX_BLOCKS                 # 262144: one full grid of the first stage
ELT_GRID = 4096 * WG                # 1048576: the capped grid of the elementwise kernels (vec_grid)

# S + 1: thread 0 alone enters the two-accumulator loop, every other thread takes the tail; 2 S: every thread runs the
# loop exactly once and there is no tail; 2 S + 1: once, and thread 0 has a tail; 3 S + 1: thread 0 runs it twice, every
# other thread once and then the tail
RED = [1, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S + 1]
ELT = [1, 255, 256, 257, ELT_GRID, ELT_GRID + 1]


def positions(n):
    """where a single entry is placed in a vector of n: wave, workgroup and grid-wrap boundaries"""
    return sorted(set(p for p in (0, 63, 64, 255, 256, n - 1, S - 1, S, S + 255, 2 * S, 2 * S + 1) if 0 <= p < n))


def blocks(n):
    return min(max(-(-n // WG), 1), MAX_BLOCKS)


# --------------------------------------------------------------------------- the reductions
def _block_reduce(v):
    """block_reduce_sum of every workgroup: v[g, t] -> r[g]"""
    a = v.reshape(len(v), WG // 64, 64)
    for half in (32, 16, 8, 4, 2, 1):             # lane l < half: v_l + v_{l + half}
        a = a[:, :, :half] + a[:, :, half:2 * half]
    r = np.zeros(len(v))
    for w in range(WG // 64):
        r = r + a[:, w, 0]
    return r


def _stage2(partial):
    s = np.zeros(WG)
    for lo in range(0, len(partial), WG):
        seg = partial[lo:lo + WG]
        s[:len(seg)] = s[:len(seg)] + seg
    return float(_block_reduce(s.reshape(1, WG))[0])


def device_order_dot(x, y):
    """sum x_i y_i in the order of launch_dot"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, nb = len(x), blocks(len(x))
    stride = nb * WG
    p = x * y
    s = np.zeros(stride)
    for lo in range(0, n, stride):
        seg = p[lo:lo + stride]
        s[:len(seg)] = s[:len(seg)] + seg
    return _stage2(_block_reduce(s.reshape(nb, WG)))


def device_order_sumsq(x):
    """sum x_i^2 in the order of launch_norm2, before its square root"""
    x = np.asarray(x, dtype=np.float64)
    n, nb = len(x), blocks(len(x))
    stride = nb * WG
    q = x * x
    s0, s1 = np.zeros(stride), np.zeros(stride)
    i = np.arange(stride)                         # every thread's index
    while True:
        m = i + stride < n                        # a thread that fails this once has left the loop for good
        if not m.any():
            break
        s0[m] = s0[m] + q[i[m]]
        s1[m] = s1[m] + q[i[m] + stride]
        i[m] += 2 * stride
    m = i < n                                     # the single tail entry
    s0[m] = s0[m] + q[i[m]]
    return _stage2(_block_reduce((s0 + s1).reshape(nb, WG)))


def device_order_norm(x):
    return math.sqrt(device_order_sumsq(x))


def _rounds(n):
    return -(-n // (blocks(n) * WG))


def chain_dot(n):
    """the longest chain of additions in launch_dot: a thread's strided sum over ceil(n / (nb * 256)) products (from
    zero), the butterfly's 6 levels, the 4 wave sums (from zero); then the second stage's strided sum over
    ceil(nb / 256) partial sums (from zero), its 6 levels and its 4 wave sums"""
    return _rounds(n) + 6 + 4 + -(-blocks(n) // WG) + 6 + 4


def chain_norm(n):
    """the same for launch_norm2: a thread's R = ceil(n / (nb * 256)) squares go alternately to two accumulators, so
    the longer one, s0, takes ceil(R / 2) additions (from zero), and s0 + s1 is one more; the rest as in chain_dot"""
    return -(-_rounds(n) // 2) + 1 + 6 + 4 + -(-blocks(n) // WG) + 6 + 4


def dot_bound(n, magnitude):
    """|device_order_dot - fsum of the exact products| when every product x_i y_i is exact: a chain of k additions
    leaves each term with a factor (1 + d)^k, |d| <= U, i.e. an error of at most k U / (1 - k U) sum |x_i y_i|, and
    fsum rounds the exact sum once more: together below (k + 3) U sum |x_i y_i| while k (k + 3) U <= 3.
    magnitude: sum |x_i y_i|"""
    return (chain_dot(n) + 3) * U * magnitude


def norm_bound(n, sumsq):
    """|sqrt(device_order_sumsq) - sqrt(fsum of the exact squares)|: with e = (chain_norm(n) + 3) U the computed sum s
    and the exact sum S satisfy |s - S| <= e S as in dot_bound (all terms are positive), so
    |sqrt(s) - sqrt(S)| = |s - S| / (sqrt(s) + sqrt(S)) <= e sqrt(S) / (1 + sqrt(1 - e)); each of the two square roots
    is rounded once: 2 U sqrt(S) more.  sumsq: S"""
    e = (chain_norm(n) + 3) * U
    return (e / (1.0 + math.sqrt(1.0 - e)) + 2 * U) * math.sqrt(sumsq)


# --------------------------------------------------------------------------- the multi-RHS engine's norm
# csrc/hier_multi.hip, norm_partial_multi / norm_final_multi, restated from the comment above them: "per-column ||v||^2
# in two stages over a FIXED grid: lane t of workgroup w adds rows w 256 + t, + 2048 256, ... in order, a binary tree
# joins the lanes, then one workgroup joins the 2048 partial sums the same way and takes the roots.  Columns never
# meet: the tree of a column depends on n only."
MULTI_NORM_BLOCKS, MULTI_NORM_WG = 2048, 256
MULTI_NORM_GRID = MULTI_NORM_BLOCKS * MULTI_NORM_WG          # 524288 rows: above it a lane adds more than one row


def _multi_tree(a):
    """the binary tree over the last axis (256 lanes): for w = 128, 64, .. 1, lane t < w takes s[t] + s[t + w]"""
    w = a.shape[-1] // 2
    while w > 0:
        a = a[..., :w] + a[..., w:2 * w]
        w //= 2
    return a[..., 0]


def multi_norm_model(v):
    """||v||_2 of one column as the multi-RHS engine forms it"""
    v = np.asarray(v, dtype=np.float64)
    q = v * v
    acc = np.zeros(MULTI_NORM_GRID)                    # lane w 256 + t, from 0.0
    for lo in range(0, len(q), MULTI_NORM_GRID):
        seg = q[lo:lo + MULTI_NORM_GRID]
        acc[:len(seg)] = acc[:len(seg)] + seg
    part = _multi_tree(acc.reshape(MULTI_NORM_BLOCKS, MULTI_NORM_WG))
    lane = np.zeros(MULTI_NORM_WG)                     # lane t adds partial sums t, t + 256, ... from 0.0
    for lo in range(0, MULTI_NORM_BLOCKS, MULTI_NORM_WG):
        lane = lane + part[lo:lo + MULTI_NORM_WG]
    return math.sqrt(float(_multi_tree(lane)))


# --------------------------------------------------------------------------- elementwise, in the kernels' order
def scale(c, x):                    # scale_kernel
    return np.multiply(c, x)


def axpy(x, h):                     # axpy_inplace_kernel (amg_dev_axpy)
    return np.add(x, h)


def axpy_scaled(x, r, c):           # axpy_scaled_kernel: h = c * r; x + h
    h = np.multiply(c, r)
    return np.add(x, h)


def axmy(w, v, a):                  # axpy_kernel (amg_dev_axmy): w - a * v
    t = np.multiply(a, v)
    return np.subtract(w, t)


def scale_add(p, beta, z):          # scale_add_kernel: t = p * beta; t + z
    t = np.multiply(p, beta)
    return np.add(t, z)


def sub(a, b):                      # sub_kernel
    return np.subtract(a, b)


def divide(w, a):                   # divide_kernel: a division, not a product with 1 / a
    return np.divide(w, a)


def dense_apply_model(M, b):
    """x = M b as dense_apply_kernel sums it: s = s + M[i, k] * b[k] for k = 0 .. n-1, from 0.0 (the device reads
    Mt[k * n + i] = M[i, k])"""
    M, b = np.asarray(M, dtype=np.float64), np.asarray(b, dtype=np.float64)
    s = np.zeros(M.shape[0])
    for k in range(M.shape[1]):
        s = s + M[:, k] * b[k]
    return s


# --------------------------------------------------------------------------- operands
def operands(n, seed, single=False):
    """two vectors of signed values with magnitudes from 2^-20 to 2^20 and -0.0 entries.  single: every value is a
    float32 value (24 significant bits), so every product and every square is exact in float64 (48 bits; the
    exponents stay within +-41)"""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(2):
        v = rng.uniform(1.0, 2.0, n) * np.exp2(rng.randint(-20, 20, n)) * rng.choice([-1.0, 1.0], n)
        if single:
            v = v.astype(np.float32).astype(np.float64)
        v[(0, 3)[k]::(7, 11)[k]] = -0.0
        out.append(v)
    return out


A, BETA, CC, DIV = 0.37, 0.83, -1.21, 3.0          # the scalars of the elementwise tests: no powers of two


def elt_operands(n):
    """the operands of the elementwise GPU tests at length n"""
    return operands(n, 100 + n)


def bit_mismatches(a, b):
    """entries whose bits differ, so that -0.0 is not +0.0; a NaN matches any NaN (test_gpu_dtypes.bit_mismatches)"""
    a = np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64)
    b = np.ascontiguousarray(np.atleast_1d(b), dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int(np.count_nonzero((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))))
