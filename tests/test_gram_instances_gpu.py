"""hnh_gram_rows_f64 (include/hnh_als_implicit.h) on the device at every kernel instance and load width, exactly, and api.ImplicitALS
at the widths and rows where tests/test_als_implicit_gpu.py was blind.

tests/gram_cases.py holds the design: the table of (rows, R, alignment) cases over all five gram_rows_kernel<NJ, MI, WAVES> instances
with 16-byte and with 8-byte loads of X, round the wave tile, the workgroup and a second workgroup with a remainder; integer operands
for the product and rowdot; for cg mode operands on which x, r and rs are exact in every order of addition, beta is one division and p
one fused multiply-add, so that every comparison is an equality against a host model in integer and rational arithmetic; NaN guards
round every device array, checked after every call; planted rows that are not live.  tests/test_gram_instances_cpu.py checks the table
and the model themselves.  The operator in both modes at R in {16, 32, 48, 64} and with rows that are not live on every rank, against
tests/als_implicit_ref.py at T.TOL.  Weights of exactly zero run on the CPU test double only (tests/test_gram_instances_cpu.py): the
GPU case passed alone and then ended a kernel-traced run of this file with a segmentation fault of the host process inside half_step
on four loopback ranks, whose cause was not found; it is left out until it is.

The log of this file on an MI355X is profiles/gram_instances_gputests.log, the kernels it launched profiles/gram_instances_kernels.txt."""
import pytest

import als_common
import gram_cases as G
import hnh_testlib as T
from gat_gpu_harness import ctx, hip_backend  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_product_and_rowdot_are_exact(ctx, case):
    G.run_plain(ctx, case)


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_guarded_update_is_the_model_bit_for_bit(ctx, case):
    G.run_cg(ctx, case)


def test_refusals_write_nothing(ctx):
    assert G.refusals(ctx) == 9


@pytest.mark.parametrize("case", G.OPERATOR_WIDTHS, ids=als_common.case_id)
def test_both_modes_at_the_widths_no_older_test_ran(case):
    worst, diff = G.run_widths(case, "gpu")
    print("gram widths %s: worst against the definition %.2e" % (case, worst))
    assert worst <= T.TOL and diff <= T.TOL


@pytest.mark.parametrize("folded", [True, False], ids=["folded", "composed"])
def test_rows_that_are_not_live_stay_exactly_zero(folded):
    worst = G.run_dead_rows(folded)
    print("gram dead rows %s: %.2e" % ("folded" if folded else "composed", worst))
    assert worst <= T.TOL
