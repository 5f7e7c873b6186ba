"""Both MFMA GEMMs, the ALS row helpers and the streaming element-wise kernels of include/hnh_kernels.h and include/hnh_grad.h on the
device, exactly, and past their grid caps.

tests/dense_cases.py holds the design: integer matrices and power-of-two scalars, so that every order of addition gives the same bits and
every comparison is an equality of bit patterns against a numpy model; every operand, output and workspace between two NaN guards,
checked after every call together with the inputs; a case table per kernel family with the (LPR, W) instance each width and alignment
selects; and one case per grid-stride kernel whose size takes the loop round a second, ragged trip (ew_grid() caps a launch at 8192
blocks of 256 threads; the benchmark's matrices are beyond that, the older tests all below).  tests/test_dense_instances_cpu.py runs the
same cases through the CPU test doubles and checks the tables themselves.

hnh_gemm_f64 runs on a context with HNH_GEMM_WAVES unset (128 x 128 tiles of 4 waves) and on one with 8 (256 x 128 tiles of 8 waves):
each the model's bits twice, and the two tile shapes bit-equal to each other.  The log of this file on an MI355X is
profiles/dense_instances_gputests.log."""
import pytest

import dense_cases as D
from distributed_sddmm_amd import _kernels as K
from gat_gpu_harness import ctx, hip_backend  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gemm_ctxs():
    """hnh_ctx_create reads the switch: one context without it, one with HNH_GEMM_WAVES=8"""
    mp = pytest.MonkeyPatch()
    mp.delenv("HNH_GEMM_WAVES", raising=False)
    four = K.Ctx(0)
    mp.setenv("HNH_GEMM_WAVES", "8")
    eight = K.Ctx(0)
    mp.undo()
    yield {4: four, 8: eight}
    four.close()
    eight.close()


@pytest.mark.parametrize("case", D.GEMM_CASES, ids=[D.gemm_id(c) for c in D.GEMM_CASES])
def test_gemm_on_both_tile_shapes(gemm_ctxs, case):
    c4, c8 = D.gemm(gemm_ctxs[4], *case), D.gemm(gemm_ctxs[8], *case)
    assert D.same_bits(c4, c8), "the 4-wave and the 8-wave tile must give the same bits"


def test_gemm_refusals(gemm_ctxs):
    D.gemm_refusals(gemm_ctxs[4])
    D.gemm_refusals(gemm_ctxs[8])


@pytest.mark.parametrize("case", D.TN_CASES, ids=[D.tn_id(c) for c in D.TN_CASES])
def test_gemm_tn(ctx, case):
    D.gemm_tn(ctx, *case)


def test_gemm_tn_refusals(ctx):
    D.gemm_tn_refusals(ctx)


@pytest.mark.parametrize("case", D.ROWDOT_CASES, ids=[D.row_id(c) for c in D.ROWDOT_CASES])
def test_rowdot(ctx, case):
    D.rowdot(ctx, *case)


@pytest.mark.parametrize("case", D.CG_CASES, ids=[D.row_id(c) for c in D.CG_CASES])
def test_cg_step(ctx, case):
    D.cg_step(ctx, *case)


@pytest.mark.parametrize("case", D.EPILOGUE_CASES, ids=[D.row_id(c) for c in D.EPILOGUE_CASES])
def test_row_epilogue(ctx, case):
    D.row_epilogue(ctx, *case)


@pytest.mark.parametrize("case", D.SCALE_ADD_CASES, ids=[D.row_id(c) for c in D.SCALE_ADD_CASES])
def test_row_scale_add(ctx, case):
    D.row_scale_add(ctx, *case)


def test_row_scale_add_past_the_cap(ctx):
    D.row_scale_add(ctx, D.SCALE_ADD_PAST[1], rows=D.SCALE_ADD_PAST[0])


@pytest.mark.parametrize("case", D.CHUNK_CASES + [D.CHUNK_PAST], ids=[D.chunk_id(c) for c in D.CHUNK_CASES] + ["past_the_cap"])
def test_sum_chunked_blocks(ctx, case):
    D.sum_chunked(ctx, *case)


@pytest.mark.parametrize("case", D.EW_CASES, ids=[D.ew_id(c) for c in D.EW_CASES])
def test_elementwise_at_every_size(ctx, case):
    D.run_ew_sizes(ctx, *case)


@pytest.mark.parametrize("name", D.EW_PAST)
def test_elementwise_past_the_cap(ctx, name):
    D.run_ew(ctx, name, D.EW[name].past_cap())
