"""CPU: the float64 oracle against the reference's sub-range, strided, single-row and empty sweeps recorded in
tests/golden/ranges_f64.npz (tools/gen_golden_dtypes.py:gen_ranges).  Every array argument is compared after the
call: what the reference changed (x, temp, z) bit for bit with the recording, everything else with its input.
This is what lets tests/test_gpu_flat_ranges.py take the oracle as the float64 reference at larger sizes."""
import pytest

import flat_ranges
import oracle_lib

RANGES = flat_ranges.load("f64")


def test_fixture_covers_every_entry_and_range():
    names = [str(c) for c in RANGES["cases"]]
    assert len(names) == len(set(names))
    for entry in ("gauss_seidel", "jacobi", "gauss_seidel_ne", "gauss_seidel_nr", "overlapping_schwarz_csr",
                  "bsr_gauss_seidel_bs2", "bsr_gauss_seidel_bs3", "block_gauss_seidel_bs2", "block_gauss_seidel_bs3",
                  "block_jacobi_bs2", "block_jacobi_bs3"):
        for rng in flat_ranges.ranges(300):
            assert "%s_%s@f64" % (entry, rng) in names
    for entry in ("jacobi_ne", "bsr_jacobi_bs2", "bsr_jacobi_bs3"):
        for rng in ("sub_fwd", "stride2_fwd", "single", "empty"):
            assert "%s_%s@f64" % (entry, rng) in names
    for walk in flat_ranges.indexed_walks(150):
        assert "gauss_seidel_indexed_%s@f64" % walk in names


@pytest.mark.parametrize("case", flat_ranges.case_names("f64"))
def test_oracle_range_sweep_bit_exact_vs_reference(oracle, case):
    flat_ranges.replay(RANGES, case, flat_ranges.OracleTable(oracle))
