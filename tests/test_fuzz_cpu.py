"""Randomised differential test of the host logic (CPU ranks + the oracle's C test double) against the numpy oracle:
random schedule, grid (powers of two and grids with remainders, up to 18 ranks), sizes (incl. M < p, non-square, 1-nonzero
matrices), chunk counts and heights, adaptive window grouping, ring modes, accumulator halves, borrowed value arrays, shift payload
and both set-up pipelines.  A fixed seed keeps the suite deterministic; `python tests/fuzz_common.py SEED COUNT` (the generator) explores further (round 4:
4 x 1500 draws, 4 153 valid configurations, no deviation; round 5, with the window-grouping switches: 3 x 300 draws, 645 valid, no deviation)."""
import pytest

import hnh_testlib as T
from distributed_sddmm_amd import api as H
from fuzz_common import sweep


@pytest.mark.parametrize("seed", [11, 12])
def test_random_configurations_match_the_oracle(seed):
    H.load_backend(T.ORACLE_BACKEND)
    assert len(sweep(seed, 16)) >= 6
