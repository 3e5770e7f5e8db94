"""The designed Gauss-Seidel cases of tests/gs_cases.py, pinned on the host: the restated build_levels returns the
designed level widths, every property a case states holds, the C oracle equals the plain-Python model bit for bit, and
the comparison the device tests make is sensitive -- a row sum in reversed order, a stale operand from the level before,
the first instead of the last stored diagonal, or the other flavour's rounding each change at least one bit."""
import copy

import numpy as np
import pytest

import gs_cases as gc

CASES = gc.all_cases()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_designed_levels_and_stated_properties(case):
    level_ptr, order = case.levels()
    widths = [level_ptr[l + 1] - level_ptr[l] for l in range(len(level_ptr) - 1)]
    if case.widths is not None:
        assert case.order is None and widths == case.widths
    else:
        assert case.order is not None and sum(widths) == len(case.order)
    assert case.n <= 5000 and case.nnz <= 70000
    if case.longest is not None:
        assert case.longest_offdiag() == case.longest
    tasks = case.tasks()
    if case.short is not None:
        assert (sum(len(case.rows[i]) for i in tasks) <= 10 * len(tasks)) == case.short
    # what the case says it is meant for agrees with the restated selection rules, and names real fields
    info = case.info(2)
    assert set(case.expect) <= set(gc.INFO_FIELDS) and case.expect
    assert {k: info[k] for k in case.expect} == case.expect
    # every stored diagonal dominates unless the case planted a zero or left it out
    for i in tasks[:50]:
        d = [v for c, v in case.rows[i] if c == i]
        if d and d[-1] != 0.0:
            assert abs(d[-1]) > sum(abs(v) for c, v in case.rows[i] if c != i)


def test_families_and_thresholds_are_all_present():
    fam = {}
    for c in CASES:
        fam.setdefault(c.family, []).append(c)
    assert set(fam) == {"flow_lpr", "flow_grid", "flow_gate", "chain_short", "chain_long", "level_launch", "oddities"}
    lpr = [(c.longest, c.info()["flow"], c.info()["lpr"]) for c in fam["flow_lpr"]]
    assert lpr == [(0, 1, 1), (1, 1, 1), (8, 1, 1), (9, 1, 2), (16, 1, 2), (17, 1, 4), (32, 1, 4), (33, 1, 8), (64, 1, 8), (65, 1, 16),
                   (128, 1, 16), (129, 1, 32), (256, 1, 32), (257, 1, 64), (512, 1, 64), (513, 0, 1)]
    for c in fam["flow_lpr"][1:-1]:
        R = 64 // c.info()["lpr"]
        assert {R - 1, R, R + 1} - {0} <= set(c.widths)
        last = sum(c.widths[:-1])
        assert [cc for cc, v in c.rows[last] if cc != last] == []          # a diagonal-only row in the last level
    assert sorted(c.info()["nchunks"] for c in fam["flow_grid"]) == [1, 1, 1, 2, 3, 15, 16, 17, 23, 31, 32, 33]
    assert {c.info()["c2_pf"] for c in fam["chain_short"] if c.info()["chain2"]} == {4, 8, 12}
    assert {w for c in fam["chain_short"] for w in c.info()["chain_widths"]} == {64, 128, 256, 512}
    assert {w for c in fam["chain_long"] for w in c.info()["chain_widths"]} == {64, 128, 256, 512}
    assert any(c.info()["levels"] > 4096 for c in fam["chain_short"]) and any(c.info()["levels"] > 1024 for c in fam["chain_long"])


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_level_order_reproduces_the_sequential_sweep(case):
    """the restated build_levels is a valid schedule: sweeping its level order gives the sequential sweep's bits"""
    level_ptr, order = case.levels()
    tasks = case.tasks()
    by_level = copy.copy(case)
    by_level.order = np.array([tasks[t] for t in order], dtype=np.intc)
    for seq in ([0], [1]):
        assert gc.bit_mismatches(gc.model(case, seq, False, case.x, case.b), gc.model(by_level, seq, False, case.x, case.b)) == 0


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_oracle_equals_the_plain_python_model(case):
    for bsr1 in (False, True):
        for seq in ([0], [1], [0, 1]):
            want = gc.model(case, seq, bsr1, case.x, case.b)
            got = gc.oracle(case, seq, bsr1, case.x, case.b)
            assert np.all(np.isfinite(want))
            assert gc.bit_mismatches(got, want) == 0, (case.name, bsr1, seq)


def test_nine_sweeps_stay_finite():
    for case in CASES:
        assert np.all(np.isfinite(gc.oracle(case, gc.SEQUENCES[-1], False, case.x, case.b))), case.name


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_the_comparison_is_sensitive(case):
    seq = [0, 1]
    base = [gc.model(case, seq, bsr1, case.x, case.b) for bsr1 in (False, True)]
    for check in gc.SENSITIVITY:
        if check in case.exempt:
            continue
        if check == "flavour":
            assert gc.bit_mismatches(base[0], base[1]) > 0, check
            continue
        wrong = [gc.model(case, seq, bsr1, case.x, case.b, mutate=check) for bsr1 in (False, True)]
        assert gc.bit_mismatches(base[0], wrong[0]) + gc.bit_mismatches(base[1], wrong[1]) > 0, check


def test_at_most_one_case_in_ten_exempts_a_check():
    for check in gc.SENSITIVITY:
        exempt = [c.name for c in CASES if check in c.exempt]
        assert 10 * len(exempt) <= len(CASES), (check, exempt)
    assert all(c.exempt <= set(gc.SENSITIVITY) for c in CASES)


def test_sentinel_case():
    c = gc.sentinel_case()
    owned, halo = c.sentinel_positions
    assert owned < c.n <= halo < c.ncols
    assert int(c.x.view(np.uint64)[owned]) == gc.FLOW_SENTINEL == int(c.x.view(np.uint64)[halo])
    for bsr1 in (False, True):
        want = gc.model(c, [0], bsr1, c.x, c.b)
        got = gc.oracle(c, [0], bsr1, c.x, c.b)
        nan = np.isnan(want[:c.n])
        assert 0 < np.count_nonzero(nan) < c.n                  # some rows read the sentinel, not all
        assert np.array_equal(np.isnan(got[:c.n]), nan)
        assert gc.bit_mismatches(got[:c.n][~nan], want[:c.n][~nan]) == 0
