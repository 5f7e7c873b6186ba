"""The case list of tests/gat_double_cases.py on the HIP library: the same operands, guards, references and bounds that
tests/test_gat_double_cpu.py holds the second CPU test double to, so that a drift between the double's restatement of
include/hnh_grad.h, hnh_attention.h, hnh_attn_grad.h, hnh_train.h and the kernels is seen.  Observed on an MI355X:
profiles/gat_double_gputests.log."""
import pytest

import gat_double_cases as D
from gat_gpu_harness import ctx, hip_backend  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,case", D.CASES, ids=D.IDS)
def test_case_on_the_hip_library(ctx, name, case):
    case(ctx.lib, ctx)
