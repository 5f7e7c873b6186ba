"""tests/dense_cases.py without a GPU: every case of tests/test_dense_instances_gpu.py through the oracle's C test doubles (the plain one
for include/hnh_kernels.h, the second one for include/hnh_grad.h), with the same guarded buffers, moved pointers and bit-pattern
comparisons.  That proves the numpy model, the guard logic and the pointer arithmetic before a kernel sees them and pins device and
double to one statement of every result and every refusal text.  The conditions on the inputs live here too: the sizes of the case
tables, the split-K plan of each shape, the (LPR, W) instance each width and alignment selects, which cases pass a grid cap and by how
much, and that a result cannot be mistaken for an untouched buffer."""
import numpy as np
import pytest

import dense_cases as D
import hnh_testlib as T
import row_pass_cases as RC
from distributed_sddmm_amd import _kernels as K


@pytest.fixture(scope="module")
def ctx():
    c = RC.DoubleCtx(T.ORACLE_BACKEND)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gctx():
    c = D.GradDoubleCtx(T.ORACLE_GAT_BACKEND)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ conditions on the inputs
def test_case_tables_have_the_sizes_stated():
    assert len(D.GEMM_SHAPES) == 12 and len(D.GEMM_CASES) == 15 and D.GEMM_CASES[0] == (4, 3, 0, None)
    assert len(D.TN_SLICES) == 11 and len(D.TN_EMPTY) == 3 and len(D.TN_CASES) == 16
    assert len(D.ROWDOT_CASES) == 11 + 9 + 2 * 4 and len(D.CG_CASES) == 9 + 6 + 4 * 3
    assert len(D.EPILOGUE_CASES) == (9 + 6 + 2 * 3) * 2 * 2
    assert len(D.SCALE_ADD_CASES) == 6 * 4 + 6 * 2 and len(D.CHUNK_CASES) == 3 * 3 + 2 * 2
    assert D.EW_SIZES == [1, 2, 3, 7, 8, 9, 2047, 2048, 2049, 100003] and all(r * c == n for n, (r, c) in D.COLS_SHAPE.items())
    assert sorted(D.COLS_SHAPE) == D.EW_SIZES
    assert len(D.EW) == 15 and len(D.EW_CASES) == sum(1 + len(e.operands) for e in D.EW.values()) == 45 and len(D.EW_PAST) == 12
    assert D.ROWS == 523 and all(D.ROWS % k for k in range(2, 257)) and D.ROWS > 2 * 256


def test_past_cap_cases_take_a_second_ragged_trip():
    """8192 blocks of 256 threads: the plain loops take ceil(n / 2 097 152) trips, the unrolled ones ceil(pairs / 8 388 608)"""
    assert D.PLAIN_CAP == 2097152 and D.UNROLLED_CAP == 16777216
    assert max(D.EW_SIZES) < D.PLAIN_CAP, "the small sizes all run a single trip"
    assert D.ew_trips(D.PAST_PLAIN, D.PLAIN_CAP) == 3 and D.PAST_PLAIN % D.PLAIN_CAP == 259
    assert D.PAST_COLS[0] * D.PAST_COLS[1] == D.PAST_PLAIN and D.PAST_COLS[1] == 17
    pairs = D.PAST_UNROLLED // 2
    assert D.PAST_UNROLLED % 2 == 1 and D.ew_trips(pairs, D.PLAIN_CAP * 4) == 2 and pairs - D.PLAIN_CAP * 4 == D.PLAIN_CAP + 100
    assert D.PAST_UNROLLED * 8 * 3 < 0.6e9
    rows, R = D.SCALE_ADD_PAST
    assert rows * R == 20971776 and D.ew_trips(rows * R // 2, D.PLAIN_CAP * 4) == 2
    R, cuts, nb, _ = D.CHUNK_PAST
    assert (R, cuts, nb) == (256, (0, 16500), 2) and D.PLAIN_CAP < cuts[1] * R // 2 < 2 * D.PLAIN_CAP
    assert 1449 * 1449 == 2099601 > D.PLAIN_CAP, "the slab reduce of the largest A^T B case wraps"


def test_tn_plan_gives_the_slices_stated():
    for (M, N, Kk, pad), slices in D.TN_SLICES.items():
        assert D.tn_plan(M, N, Kk)[0] == slices, (M, N, Kk)
    assert D.tn_plan(1, 1, 1009) == (2, 512) and 1009 - 512 == 497 and 497 % 16 == 1
    assert D.tn_plan(129, 130, 1040) == (2, 33 * 16) and -(-1040 // 16) - 33 == 32
    assert D.tn_plan(128, 128, 4099) == (8, 33 * 16) and 4099 % 16 == 3
    assert D.tn_plan(16, 16, 32768) == (64, 512) and D.tn_plan(16, 16, 32753) == (64, 512) and 32753 - 63 * 512 == 497
    assert D.tn_plan(16, 16, 32769) == (63, 33 * 16) and 32769 - 62 * 33 * 16 == 33
    assert D.tn_plan(257, 257, 2049)[0] == 4 and (-(-257 // 128)) ** 2 == 9
    assert max(c[2] for c in D.TN_CASES) == 32769, "the longest sum of the exactness argument"


def test_workspace_sizes_agree_with_the_plan(gctx):
    """hnh_gemm_tn_f64_workspace of the double and of the device library (dlopen needs no GPU) against the Python copy"""
    hip = K.load()
    for M, N, Kk, pad, _ in D.TN_CASES:
        want = D.tn_workspace(M, N, Kk)
        assert want == (D.TN_SLICES.get((M, N, Kk, pad), 1) * M * N if D.TN_SLICES.get((M, N, Kk, pad), 1) > 1 else 0)
        assert gctx.lib.hnh_gemm_tn_f64_workspace(M, N, Kk) == want and hip.hnh_gemm_tn_f64_workspace(M, N, Kk) == want, (M, N, Kk)


def test_every_row_instance_is_named():
    """rowdot_kernel has 14 instances, cg_step_kernel and row_epilogue_kernel 8 each: the tables name all of them"""
    assert set(D.ROWDOT_EXPECTED.values()) == {(l, w) for l in (1, 2, 4, 8, 16, 32, 64) for w in (1, 2)}
    want8 = {(l, w) for l in (1, 4, 16, 64) for w in (1, 2)}
    assert set(D.CG_EXPECTED.values()) == want8
    assert {v for c, v in D.EPILOGUE_EXPECTED.items() if c[2] != 0.0 or c[3]} == want8
    # what the existing test missed: W = 2 at LPR 1, 2, 16 and W = 1 from LPR 4 up
    assert D.ROWDOT_EXPECTED[(2, None)] == (1, 2) and D.ROWDOT_EXPECTED[(4, None)] == (2, 2) and D.ROWDOT_EXPECTED[(32, None)] == (16, 2)
    assert [D.ROWDOT_EXPECTED[(R, None)] for R in (5, 9, 17, 33, 65)] == [(4, 1), (8, 1), (16, 1), (32, 1), (64, 1)]
    for moved in ("A", "B"):
        assert [D.ROWDOT_EXPECTED[(R, moved)] for R in (2, 8, 32, 128)] == [(2, 1), (8, 1), (32, 1), (64, 1)]
    for moved in ("X", "Rm", "P", "MP"):
        assert [D.CG_EXPECTED[(R, moved)] for R in (4, 16, 128)] == [(4, 1), (16, 1), (64, 1)]


def test_results_cannot_pass_for_untouched_buffers(ctx, gctx):
    """most entries of every output differ from what the buffer held before the call"""
    for R in (1, 2, 9, 128):
        assert np.count_nonzero(D.rowdot(ctx, R)) >= (0.5 if R == 1 else 0.8) * D.ROWS
        x1, r1, rs, (x, rm) = D.cg_step(ctx, R)
        assert np.count_nonzero(x1 != x) >= 0.8 * x.size and np.count_nonzero(r1 != rm) >= 0.8 * x.size and np.count_nonzero(rs) >= 0.8 * D.ROWS
        out, out1, dot = D.row_epilogue(ctx, R, None, -0.5, True)
        assert np.count_nonzero(out1 != out) >= 0.9 * out.size
        y, y1 = D.row_scale_add(ctx, R)
        assert np.count_nonzero(y1 != y) >= 0.8 * y.size
    for name, e in D.EW.items():
        c = gctx if e.grad else ctx
        operands, outputs = D.run_ew(c, name, e.shape(2049))
        for k, want in outputs.items():
            changed = np.count_nonzero(RC.bits(np.ascontiguousarray(want).reshape(-1)) != RC.bits(operands[k].reshape(-1)))
            block = want.size if not e.cols else 2049
            assert changed >= 0.4 * block, (name, k, changed)
    assert np.count_nonzero(D.gemm_data(127, 127, 15)[2]) >= 0.9 * 127 * 127


def test_exactness_bound_is_checked():
    D.bounded(np.array([D.SUM_BOUND, 0.0625]))
    with pytest.raises(AssertionError):
        D.bounded(np.array([D.SUM_BOUND + 1.0]))
    with pytest.raises(AssertionError):
        D.bounded(np.array([1.0 / 3.0]))
    big = D.ints(1, 3 * D.TILE_PERIOD)
    assert np.array_equal(big[:D.TILE_PERIOD], big[D.TILE_PERIOD:2 * D.TILE_PERIOD]) and set(np.unique(big)) == set(range(-4, 5))
    assert not np.any(np.signbit(big) & (big == 0))


def test_buffers_report_guards_inputs_and_outputs(ctx):
    with D.Buffers(ctx) as bufs:
        p = bufs.add("v", np.arange(8.0), moved=True)
        bufs.add("w", np.arange(4.0), scratch=True)
        bufs.verify("fresh")
        for off in (-8, 64):
            ctx.check(ctx.lib.hnh_memset(ctx.h, p + off, 0, 8, 0), "memset")
            with pytest.raises(AssertionError, match="guard of v"):
                bufs.verify("stray write")
            bufs.a["v"].set(np.arange(8.0))
        ctx.check(ctx.lib.hnh_memset(ctx.h, p + 8, 0, 8, 0), "memset")
        with pytest.raises(AssertionError, match="input v"):
            bufs.verify("changed input")
        with pytest.raises(AssertionError, match="output v"):
            bufs.verify("wrong output", v=np.arange(8.0))
        ctx.check(ctx.lib.hnh_memset(ctx.h, bufs.a["w"].ptr, 0, 8, 0), "memset")
        bufs.a["v"].set(np.arange(8.0))
        bufs.verify("scratch contents are free")


# ------------------------------------------------------------------------------------------------ the cases, through the doubles
@pytest.mark.parametrize("case", D.GEMM_CASES, ids=[D.gemm_id(c) for c in D.GEMM_CASES])
def test_gemm(ctx, case):
    D.gemm(ctx, *case)


def test_gemm_refusals(ctx):
    D.gemm_refusals(ctx)


@pytest.mark.parametrize("case", D.TN_CASES, ids=[D.tn_id(c) for c in D.TN_CASES])
def test_gemm_tn(gctx, case):
    D.gemm_tn(gctx, *case)


def test_gemm_tn_refusals(gctx):
    D.gemm_tn_refusals(gctx)


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
def test_elementwise_at_every_size(ctx, gctx, case):
    D.run_ew_sizes(gctx if D.EW[case[0]].grad else ctx, *case)


@pytest.mark.parametrize("name", D.EW_PAST)
def test_elementwise_past_the_cap(ctx, gctx, name):
    D.run_ew(gctx if D.EW[name].grad else ctx, name, D.EW[name].past_cap())
