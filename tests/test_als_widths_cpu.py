"""ALS-CG through the operator on CPU ranks against the numpy definition (tests/als_ref.py): widths that take other kernel paths,
a rectangular graph with hub rows on both sides and empty rows, three alternating steps, every schedule — served by the oracle's C
test double, so what is under test is the host logic (holds, landing buffers, R splits, epilogue placement).  Same body as
test_als_widths_gpu.py (tests/als_common.py)."""
import pytest

import als_common as C
import hnh_testlib as T
from distributed_sddmm_amd import api as H


@pytest.fixture(autouse=True, scope="module")
def cpu_test_double():
    H.load_backend(T.ORACLE_BACKEND)
    yield


@pytest.mark.parametrize("case", C.cpu_solver_cases(), ids=C.case_id)
def test_als_meets_the_model(case):
    C.run_case(*case)


@pytest.mark.parametrize("case", C.artificial_cases(), ids=C.case_id)
def test_artificial_ground_truth_and_hashed_embeddings(case):
    C.run_artificial(*case)


def test_the_cases_are_the_ones_listed():
    """2 grids x 2 modes x 5 widths of 15d_fusion2, the four other schedules at R = 8 in both modes, the built-in set-up on five
    schedules at two widths."""
    assert len(C.cpu_solver_cases()) == 20 + 8 and len(set(C.cpu_solver_cases())) == 28
    assert len(C.artificial_cases()) == 10
