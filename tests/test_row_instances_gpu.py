"""SDDMM, SpMM and the fused pass of include/hnh_kernels.h at every kernel instance launch_shape / dispatch_row can pick, exactly.

tests/row_pass_cases.py holds the design: integer inputs, so that every order of addition gives the same bits and every comparison here
is an equality of bit patterns against a numpy model (no distance, no bound); every device array between two NaN guards, checked after
every call together with the inputs; a graph whose row lengths sit round the unroll batches (0 1 2 3 4 5 7 8 9 15 16 17 63 64 65) and
whose 523 rows no workgroup size divides.  tests/test_row_instances_cpu.py runs the same cases through the CPU test double.

Widths: every exact instance (LPR 1 .. 64, VEC 1 .. 7; the NARROW ones at 8 / 16 / 32 and, with the CSR streams moved by one element, the
plain ones), NX(V, 2) and NX(V, 1), the 64 W column tiles (the fused entry composes them itself), the 128-column slabs, and W = 1 at even
widths (dense operands moved by 8 bytes).  Per width: SDDMM (hinted, unhinted, COO, scaled), SpMM, the fused pass with every combination
of the overwrite flags, svalues and LeakyReLU, and the row epilogue.  Then each context switch in a context of its own (NARROW off, slabs
off, 5 forced column panels, hub rows under HNH_LONG_ROW=64 as ordered partial rows / atomics / without scratch, a structure plan used
twice), caller windows, and degenerate blocks.  The CG epilogue, the ReLU delivery and the softmax pass stay with their own files.

Every test passed on an MI355X on first contact but one finding about the test's own data (the sign of a zero result depends on how a
sum is split: row_pass_cases.Data): 139 tests, 27.5 s under a kernel trace.  profiles/row_instances_kernels.txt lists the kernels that
run launched beside the expected-instance table (tools/row_instances_profile.py): all 22 instances per operation, every long_row_kernel
instance of the switch widths, reduce_long_kernel<1> and <2>; profiles/row_instances_gputests.log is its log."""
import contextlib

import pytest

import row_pass_cases as RC
from distributed_sddmm_amd import _kernels as K
from gat_gpu_harness import ctx, hip_backend  # noqa: F401

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def switched(monkeypatch, **env):
    """a context created under the given environment (the switches are read by hnh_ctx_create)"""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    c = K.Ctx(0)
    for k in env:
        monkeypatch.delenv(k)
    try:
        yield c
    finally:
        c.close()


@pytest.mark.parametrize("R,align", RC.WIDTH_CASES, ids=[RC.case_id(p) for p in RC.WIDTH_CASES])
def test_every_operation_at_every_width(ctx, R, align):
    RC.run(ctx, RC.edge_graph(tail_empty=R % 3 == 0), R, align, RC.Block.every_operation)


@pytest.mark.parametrize("R", RC.W_SWITCHES)
def test_narrow_rows_switched_off(monkeypatch, R):
    with switched(monkeypatch, HNH_NARROW_ROWS=0) as c:
        RC.run(c, RC.edge_graph(), R, "a16", RC.Block.switch_operations)


@pytest.mark.parametrize("R", RC.W_SWITCHES + [320, 384, 512])
def test_wide_slabs_switched_off(monkeypatch, R):
    """SDDMM and SpMM at 320 .. 512 then run the wide exact instances (32, 5) (64, 3) (32, 7) (64, 4) instead of 128-column slabs"""
    with switched(monkeypatch, HNH_WIDE_SLABS=0) as c:
        RC.run(c, RC.edge_graph(), R, "a16", RC.Block.switch_operations)


@pytest.mark.parametrize("R", RC.W_SWITCHES)
def test_forced_column_panels(monkeypatch, R):
    """5 launches over column panels of the block instead of one (slab widths: 5 per 128-column slab): the single launch's bits, also
    through a structure plan that keeps the panel boundaries"""
    g = RC.edge_graph()
    per_row = min(R, 128) if (R >= RC.SLAB_MIN_R and R % 64 == 0) else R
    with switched(monkeypatch, HNH_PANEL_BYTES=g.cols * per_row * 8 / 5, HNH_MAX_PANELS=8) as c:
        if RC.pick_shape(R, True)[3] or R <= 64 * RC.pick_shape(R, True)[2] * 4:  # a single-pass width
            assert c.lib.hnh_panel_count(c.h, g.rows, g.nnz, g.cols, per_row, g.max_row) == 5
        RC.run(c, g, R, "a16", RC.Block.switch_operations)
        RC.run(c, g, R, "a16", RC.Block.planned_operations)


HUB_FORMS = {"ordered": {}, "atomics": {"HNH_HUB_ATOMICS": 1}, "no_scratch": {"HNH_HUB_SCRATCH_MB": 0}}


@pytest.mark.parametrize("R", RC.W_SWITCHES)
@pytest.mark.parametrize("form", list(HUB_FORMS))
def test_hub_rows_in_segments(monkeypatch, form, R):
    """HNH_LONG_ROW=64: the rows of 65 .. 700 nonzeros go to long_row_kernel in 1, 2 or 3 segments of 256 (the row of exactly 64 stays in
    the row kernel): partial rows added up in order by reduce_long_kernel<2> (<1> at odd widths), or fp64 atomics, or no scratch at all —
    with exact data all three give the model's bits"""
    with switched(monkeypatch, HNH_LONG_ROW=64, **HUB_FORMS[form]) as c:
        RC.run(c, RC.hub_graph(), R, "a16", RC.Block.switch_operations)


@pytest.mark.parametrize("R", RC.W_SWITCHES)
def test_structure_plan_used_twice(monkeypatch, R):
    """the _p entry points with a plan: the second round reuses the plan's hub-row list"""
    with switched(monkeypatch, HNH_LONG_ROW=64) as c:
        RC.run(c, RC.hub_graph(), R, "a16", RC.Block.planned_operations)


@pytest.mark.parametrize("R", RC.W_WINDOWS)
def test_windows_equal_the_whole_block(ctx, R):
    """hnh_csr_window_bounds and the _w entry points: three bounds, four windows, one of them empty"""
    RC.run(ctx, RC.edge_graph(), R, "a16", lambda b: b.windows([80, 80, 200]))


@pytest.mark.parametrize("kind", ["all_empty", "one_row", "one_row_one_nonzero"])
@pytest.mark.parametrize("R", [16, 100, 301])
def test_degenerate_blocks(ctx, kind, R):
    RC.run(ctx, RC.degenerate_graph(kind), R, "a16", RC.Block.every_operation)
