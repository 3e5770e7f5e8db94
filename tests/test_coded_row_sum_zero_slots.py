"""The two forms of the coded row sum (kernels.hip coded_row_sum), restated in numpy float64.

select form      acc = +0.0; for each slot u in order: if the slot is present, acc = acc + v[u] * (gscale * xv[u])
zero-slot form   acc = +0.0; for each slot u in order: acc = acc + d[u] * (gscale * xv[u]), d[u] = v[u] if present else +0.0

The level-0 chains run the second: code 255 ("slot not stored") reads a dictionary entry that holds +0.0.  The forms
agree bit for bit for finite operands because acc is never -0.0 (it starts at +0.0, and a round-to-nearest sum is -0.0
only when both addends are), so adding the +-0.0 of an absent slot leaves it as it is.  Checked over all 128
present/absent patterns of the 7 slots; numpy's float64 scalar arithmetic rounds every product and sum separately, as
the kernels do (-ffp-contract=off).  With a start value of -0.0 (the modes that start from b) the forms differ, which
is why coded_row_sum rejects the zero-slot form for them at compile time.
"""
import itertools

import numpy as np
import pytest

TINY = np.float64(5e-324)                          # the smallest denormal
DEN = np.float64(2.2250738585072014e-308) / 4      # a denormal
CHEB = np.float64(-0.22668004012036107)            # a Chebyshev(2) coefficient of the size the smoother uses
GSCALES = (np.float64(1.0), CHEB, np.float64(-3.0))

# 7 (value, operand) pairs per set.  Between them: +0.0 and -0.0 operands, denormal operands and values, products that
# cancel exactly, products that underflow to +-0.0, a stored 0.0 and a stored -0.0 among the dictionary values.
SETS = {
    "poisson": ([-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0], [0.25, -0.5, 0.125, 1.0, 3.0, -7.0, 0.0625]),
    "signed zero operands": ([-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0], [0.0, -0.0, 0.0, -0.0, -0.0, 0.0, -0.0]),
    "zeros then data": ([-1.0, 2.0, -1.0, 6.0, -1.0, 2.0, -1.0], [-0.0, -0.0, 0.0, 0.5, -0.0, 0.0, 1.5]),
    "exact cancellation": ([1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 4.0], [3.0, 3.0, 1.5, 1.5, -6.0, -6.0, -0.0]),
    "cancel to zero, then a negative zero": ([2.0, -4.0, 1.0, 1.0, -1.0, 6.0, -1.0], [1.0, 0.5, -0.0, 0.0, 0.0, -0.0, 0.0]),
    "denormals": ([DEN, -1.0, TINY, 6.0, -DEN, 1.0, -TINY], [1.0, TINY, 1.0, DEN, -0.5, -TINY, 3.0]),
    "underflowing products": ([TINY, -TINY, DEN, -DEN, TINY, 0.25, -0.25], [0.25, 0.25, TINY, TINY, -0.25, TINY, TINY]),
    "stored zeros": ([0.0, -0.0, -1.0, 6.0, -0.0, 0.0, -1.0], [0.75, -0.75, 2.0, -0.0, 5.0, -5.0, 0.0]),
    "stored zeros only": ([0.0, -0.0, 0.0, -0.0, -0.0, 0.0, -0.0], [1.0, 2.0, -3.0, -0.0, 0.0, -5.0, 7.0]),
    "stored negative zero meets negative operands": ([-0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0], [-1.0, -1.0, 1.0, 1.0, -0.0, -0.0, 0.0]),
}
MASKS = list(itertools.product((False, True), repeat=7))


def select_form(v, xv, gscale, present, start=np.float64(0.0)):
    acc = np.float64(start)
    for u in range(7):
        pr = v[u] * (gscale * xv[u])
        nx = acc + pr
        acc = nx if present[u] else acc
    return acc


def zero_slot_form(v, xv, gscale, present, start=np.float64(0.0)):
    acc = np.float64(start)
    for u in range(7):
        d = v[u] if present[u] else np.float64(0.0)          # what sdict[255] holds
        acc = acc + d * (gscale * xv[u])
    return acc


def bits(x):
    return int(np.array([x], dtype=np.float64).view(np.int64)[0])


def _arrays(name):
    v, xv = SETS[name]
    return np.array(v, dtype=np.float64), np.array(xv, dtype=np.float64)


def test_the_sets_hold_what_they_are_for():
    assert len(MASKS) == 128
    allv = np.concatenate([_arrays(n)[0] for n in SETS])
    allx = np.concatenate([_arrays(n)[1] for n in SETS])
    for a in (allv, allx):
        assert np.isfinite(a).all()
        assert ((a == 0) & ~np.signbit(a)).any() and ((a == 0) & np.signbit(a)).any()      # +0.0 and -0.0
        assert ((a != 0) & (np.abs(a) < np.finfo(np.float64).tiny)).any()                  # denormals
    v, xv = _arrays("exact cancellation")
    assert (v * xv)[:6].sum() == 0.0 and (v * xv)[0] != 0.0


@pytest.mark.parametrize("gscale", GSCALES, ids=["one", "chebyshev", "negative"])
@pytest.mark.parametrize("name", list(SETS))
def test_forms_agree_bit_for_bit_on_every_mask(name, gscale):
    v, xv = _arrays(name)
    with np.errstate(under="ignore"):
        for present in MASKS:
            s, z = select_form(v, xv, gscale, present), zero_slot_form(v, xv, gscale, present)
            assert bits(s) == bits(z), (name, float(gscale), present, s, z)
            assert not (s == 0 and np.signbit(s)), (name, present)                         # acc is never -0.0


@pytest.mark.parametrize("gscale", GSCALES, ids=["one", "chebyshev", "negative"])
def test_forms_agree_on_seeded_operands_with_zeros_mixed_in(gscale):
    rng = np.random.RandomState(18)
    special = np.array([0.0, -0.0, TINY, -TINY, DEN, -DEN, 1.0, -1.0])
    with np.errstate(under="ignore"):
        for _ in range(40):
            v = np.where(rng.rand(7) < 0.3, rng.choice(special, 7), rng.randn(7))
            xv = np.where(rng.rand(7) < 0.4, rng.choice(special, 7), rng.randn(7))
            for present in MASKS:
                assert bits(select_form(v, xv, gscale, present)) == bits(zero_slot_form(v, xv, gscale, present))


def test_a_negative_zero_start_tells_the_forms_apart():
    """The counter-case: a sum that starts from -0.0 (the modes that start from b) keeps -0.0 through skipped slots but
    turns to +0.0 on the first stored zero times a positive operand."""
    v, xv = _arrays("poisson")
    absent = (False,) * 7
    start = np.float64(-0.0)
    s, z = select_form(v, xv, np.float64(1.0), absent, start), zero_slot_form(v, xv, np.float64(1.0), absent, start)
    assert bits(s) == bits(np.float64(-0.0))
    assert bits(z) == bits(np.float64(0.0))
    assert bits(s) != bits(z)
    # and from +0.0 the same inputs agree
    assert bits(select_form(v, xv, np.float64(1.0), absent)) == bits(zero_slot_form(v, xv, np.float64(1.0), absent)) == 0
