"""tests/vector_models.py is the oracle of tests/test_gpu_vector_kernels.py, so it is checked first, without a GPU: its
reductions against exact sums, its operands for their power to tell a contracted multiply-add and a reciprocal
multiplication from what the kernels write."""
import math
from fractions import Fraction

import numpy as np
import pytest

import vector_models as vm

A, BETA, CC, DIV = vm.A, vm.BETA, vm.CC, vm.DIV


@pytest.mark.parametrize("n", vm.RED)
def test_dot_model_within_bound_of_exact_sum(n):
    """single=True: every product is exact, math.fsum of them is the correctly rounded exact sum, and the model lies
    within dot_bound = (chain_dot(n) + 3) U sum |x_i y_i| of it (derivation: vector_models.dot_bound)"""
    x, y = vm.operands(n, n, single=True)
    p = x * y
    assert all(Fraction(a) * Fraction(b) == Fraction(c) for a, b, c in zip(x[:64], y[:64], p[:64]))
    exact = math.fsum(p.tolist())
    got = vm.device_order_dot(x, y)
    bound = vm.dot_bound(n, float(np.sum(np.abs(p))))
    print("n %d  chain %d  error %.3e  bound %.3e" % (n, vm.chain_dot(n), abs(got - exact), bound))
    assert abs(got - exact) <= bound


@pytest.mark.parametrize("n", vm.RED)
def test_norm_model_within_bound_of_exact_sum(n):
    """the same bound carried through the square root: with e = (chain_norm(n) + 3) U and S the exact sum of squares,
    |sqrt(device_order_sumsq) - sqrt(S)| <= (e / (1 + sqrt(1 - e)) + 2 U) sqrt(S)  (vector_models.norm_bound)"""
    x = vm.operands(n, n, single=True)[0]
    S_exact = math.fsum((x * x).tolist())
    got = math.sqrt(vm.device_order_sumsq(x))
    bound = vm.norm_bound(n, S_exact)
    print("n %d  chain %d  error %.3e  bound %.3e" % (n, vm.chain_norm(n), abs(got - math.sqrt(S_exact)), bound))
    assert abs(got - math.sqrt(S_exact)) <= bound


def test_chains():
    """the derivations of chain_dot / chain_norm at the lengths where a term changes"""
    assert vm.chain_dot(1) == 1 + 10 + 1 + 10 and vm.chain_dot(257) == 1 + 10 + 1 + 10
    assert vm.chain_dot(vm.S) == 1 + 10 + 4 + 10 and vm.chain_dot(vm.S + 1) == 2 + 10 + 4 + 10
    assert vm.chain_dot(3 * vm.S + 1) == 4 + 10 + 4 + 10
    assert vm.chain_norm(vm.S) == 1 + 1 + 10 + 4 + 10 and vm.chain_norm(2 * vm.S) == 1 + 1 + 10 + 4 + 10
    assert vm.chain_norm(2 * vm.S + 1) == 2 + 1 + 10 + 4 + 10 and vm.chain_norm(3 * vm.S + 1) == 2 + 1 + 10 + 4 + 10


def fused(a, b, c):
    """a * b + c rounded once: exact rational arithmetic, and float() of a Fraction rounds correctly"""
    return np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in np.broadcast(a, b, c)])


@pytest.mark.parametrize("n", [n for n in vm.ELT if n >= 64])
def test_operands_tell_a_fused_multiply_add_from_two_roundings(n):
    """a library built with contraction would compute axmy, axpy_scaled and scale_add with one rounding: on the very
    operands of the GPU tests (vector_models.elt_operands) that differs from the model within the first 64 entries"""
    x, y = (v[:64] for v in vm.elt_operands(n))
    pairs = {"axmy": (vm.axmy(x, y, A), fused(-A, y, x)),
             "axpy_scaled": (vm.axpy_scaled(x, y, CC), fused(CC, y, x)),
             "scale_add": (vm.scale_add(x, BETA, y), fused(x, BETA, y))}
    for name, (two, one) in pairs.items():
        differ = vm.bit_mismatches(two, one)
        print("n %d %s: %d of 64 entries differ" % (n, name, differ))
        assert differ >= 1, name


@pytest.mark.parametrize("n", [n for n in vm.ELT if n >= 64])
def test_operands_tell_a_division_from_a_reciprocal_product(n):
    w = vm.elt_operands(n)[0][:64]
    assert vm.bit_mismatches(vm.divide(w, DIV), w * (1.0 / DIV)) >= 1


def test_operands_have_what_they_promise():
    for single in (False, True):
        x, y = vm.operands(1000, 5, single)
        for v in (x, y):
            nz = v[v != 0]
            assert np.signbit(v[v == 0]).all() and (v == 0).sum() >= 90
            assert (nz > 0).any() and (nz < 0).any()
            assert 2.0 ** -20 <= np.abs(nz).min() < 2.0 ** -15 and 2.0 ** 15 < np.abs(nz).max() < 2.0 ** 20
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v) == single


@pytest.mark.parametrize("n", vm.RED)
def test_models_see_every_single_entry(n):
    """one non-zero pair at p in zero vectors: every other term is +0.0 and every sum is exact, so the dot is the
    rounded product x_p y_p itself and the sum of squares x_p^2 -- a model that skipped p would give 0, one that took
    it twice 2 x_p y_p"""
    for p in vm.positions(n):
        x, y = np.zeros(n), np.zeros(n)
        x[p], y[p] = -1.7, 0.3
        assert vm.device_order_dot(x, y) == x[p] * y[p]
        assert vm.device_order_sumsq(x) == x[p] * x[p]
        x[p] = np.nan
        assert math.isnan(vm.device_order_dot(x, y)) and math.isnan(vm.device_order_sumsq(x))


def test_empty_reductions_are_zero():
    assert vm.device_order_dot(np.zeros(0), np.zeros(0)) == 0.0 and vm.device_order_sumsq(np.zeros(0)) == 0.0


def test_sumsq_model_against_the_scalar_loop():
    """the vectorised two-accumulator loop against sumsq_stage1 transcribed thread by thread, at a grid of 2 x 256
    brought about by a small MAX_BLOCKS: every case of the loop and its tail"""
    def thread_by_thread(x, nb):
        n, stride = len(x), nb * vm.WG
        out = np.zeros(stride)
        for t in range(stride):
            s0 = s1 = 0.0
            i = t
            while i + stride < n:
                s0 += x[i] * x[i]
                s1 += x[i + stride] * x[i + stride]
                i += 2 * stride
            if i < n:
                s0 += x[i] * x[i]
            out[t] = s0 + s1
        return out
    saved = vm.MAX_BLOCKS
    vm.MAX_BLOCKS = 2
    try:
        for n in (1, 300, 512, 513, 1024, 1025, 1536, 1537, 2049):
            x = vm.operands(n, n)[0]
            want = vm._stage2(vm._block_reduce(thread_by_thread(x, vm.blocks(n)).reshape(vm.blocks(n), vm.WG)))
            assert vm.device_order_sumsq(x) == want
    finally:
        vm.MAX_BLOCKS = saved


def test_dense_apply_model_is_left_to_right():
    rng = np.random.RandomState(3)
    M, b = rng.randn(9, 9), rng.randn(9)
    want = []
    for i in range(9):
        s = 0.0
        for k in range(9):
            s = s + M[i, k] * b[k]
        want.append(s)
    assert vm.bit_mismatches(vm.dense_apply_model(M, b), np.array(want)) == 0
