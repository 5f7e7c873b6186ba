"""tests/row_pass_cases.py without a GPU: every case of tests/test_row_instances_gpu.py through the oracle's C test double
(oracle/hnh_oracle_backend.c, the same entry points), with the same guarded buffers, interior and moved pointers and bit-pattern
comparisons.  That proves the numpy model, the guard logic and the pointer arithmetic before a kernel sees them, and pins the GPU
tests and the double to one statement of the result.  The conditions on the INPUTS live here too: exactness (the model asserts it in
every call), and that a result cannot be mistaken for an untouched buffer."""
import numpy as np
import pytest

import hnh_testlib as T
import row_pass_cases as RC
from oracle import oracle as O


@pytest.fixture(scope="module")
def ctx():
    c = RC.DoubleCtx(T.ORACLE_BACKEND)
    yield c
    c.close()


ALL_WIDTHS = sorted({w for w, _ in RC.WIDTH_CASES} | set(RC.W_SWITCHES) | set(RC.W_WINDOWS))


# ------------------------------------------------------------------------------------------------ conditions on the inputs
def test_graphs_are_what_the_cases_need():
    g = RC.edge_graph()
    assert g.rows == 523 and g.cols == 300 and all(g.rows % k for k in range(2, 257)) and g.rows > 2 * 256
    assert sorted(set(g.lens)) == sorted(RC.EDGE) and g.lens[0] == 0 and g.lens[-1] > 0
    t = RC.edge_graph(tail_empty=True)
    assert np.all(t.lens[-3:] == 0) and t.lens[-4] > 0
    for gr in (g, t):
        assert gr.colidx.min() == 0 and gr.colidx.max() == gr.cols - 1
    h = RC.hub_graph()
    assert h.rows == 70 and h.cols == 1024 and set(RC.HUB_LENS.values()) <= set(h.lens)
    assert sorted(set(h.lens) - set(RC.HUB_LENS.values())) == list(range(41))
    assert sorted(-(-n // 256) for n in h.lens if n > 64) == [1, 1, 2, 2, 3, 3]  # segments of 256 under HNH_LONG_ROW=64


@pytest.mark.parametrize("R", ALL_WIDTHS)
def test_results_cannot_pass_for_untouched_buffers(R):
    """At least 90 % of the nonzeros have a non-zero dot product and at least 90 % of the entries of non-empty output rows change, in every
    operation's result, at every width: an instance that leaves its buffer alone (or drops a tail) cannot go unnoticed."""
    for g in (RC.edge_graph(), RC.edge_graph(tail_empty=True), RC.hub_graph()):
        d = RC.data_for(g, R)
        live = g.lens > 0
        assert np.count_nonzero(RC.dots(g, d.X, d.Y)) >= 0.9 * g.nnz
        assert np.count_nonzero(RC.sddmm(g, d.v0, d.X, d.Y, d.sv, True) != d.v0) >= 0.9 * g.nnz
        assert np.count_nonzero(RC.spmm(g, d.v0, d.Y, d.out0) != d.out0) >= 0.9 * d.out0[live].size
        for flags in (0, RC.VOW | RC.OOW, RC.VOW | RC.OOW | RC.LEAKY, RC.LEAKY):
            for sv in (None, d.sv):
                vals, out, dot = RC.fused(g, d.v0, sv, d.X, d.Y, d.out0, flags, RC.ALPHA, RC.X_SCALE, True)
                assert np.count_nonzero(vals != d.v0) >= 0.9 * g.nnz
                assert np.count_nonzero(out[live] != d.out0[live]) >= 0.9 * d.out0[live].size
        if R >= 2:  # (one product per row at R = 1: a zero in X or Out makes it vanish)
            assert np.count_nonzero(dot) >= 0.9 * g.rows


@pytest.mark.parametrize("R", [1, 16, 100, 301])
def test_model_follows_the_oracle(R):
    """the model against oracle.sddmm_local / spmm_local (sparse_kernels.cpp:44-55, 95-107) and the formulas of test_kernels_gpu.py"""
    g = RC.edge_graph()
    d = RC.data_for(g, R)
    assert np.array_equal(RC.sddmm(g, d.v0, d.X, d.Y), O.sddmm_local(g.ridx, g.colidx, d.v0, d.X, d.Y))
    assert np.array_equal(RC.spmm(g, d.v0, d.Y, d.out0), O.spmm_local(g.rowptr, g.colidx, d.v0, d.Y, d.out0))
    for flags, sv in ((0, None), (RC.VOW | RC.OOW, d.sv), (RC.LEAKY | RC.VOW, d.sv), (RC.LEAKY | RC.OOW, None)):
        vb = np.zeros(g.nnz) if flags & RC.VOW else d.v0
        ob = np.zeros_like(d.out0) if flags & RC.OOW else d.out0
        vals = O.sddmm_local(g.ridx, g.colidx, vb, d.X, d.Y)
        if flags & RC.LEAKY:
            vals = vals * (sv if sv is not None else 1.0)
            vals = np.where(vals > 0, vals, RC.ALPHA * vals)
            w = vals
        else:
            w = vals * (sv if sv is not None else 1.0)
        out = O.spmm_local(g.rowptr, g.colidx, w, d.Y, ob) + RC.X_SCALE * d.X
        got = RC.fused(g, d.v0, sv, d.X, d.Y, d.out0, flags, RC.ALPHA, RC.X_SCALE, True)
        assert np.array_equal(got[0], vals) and np.array_equal(got[1], out) and np.array_equal(got[2], np.einsum("ij,ij->i", d.X, out))


def test_exactness_precondition_is_checked():
    with pytest.raises(AssertionError):
        RC.exact(np.array([1.0, 0.03125]))
    with pytest.raises(AssertionError):
        RC.exact(np.array([2.0 ** 40]))
    with pytest.raises(AssertionError):
        RC.exact(np.array([1.0, -0.0]))
    g = RC.edge_graph()
    d = RC.data_for(g, 16)
    with pytest.raises(AssertionError):
        RC.dots(g, d.X * (1.0 / 3.0), d.Y)


def test_guards_catch_stray_writes_and_reads(ctx):
    """the guard logic itself: a write one element before / behind the interior, a changed input and a wrong output are each reported"""
    g = RC.edge_graph()
    b = RC.Block(ctx, g, RC.data_for(g, 8), "csr1")
    try:
        b.verify("fresh")
        v = b.a["values"]
        for off in (-8, g.nnz * 8):  # one element before, one behind
            ctx.check(ctx.lib.hnh_memset(ctx.h, v.ptr + off, 0, 8, 0), "memset")
            with pytest.raises(AssertionError, match="guard of values"):
                b.verify("stray write")
            v.set(v.host)
        ctx.check(ctx.lib.hnh_memset(ctx.h, b.p("colidx") + 4, 0, 4, 0), "memset")
        with pytest.raises(AssertionError, match="input colidx"):
            b.verify("changed input")
        b.a["colidx"].set(g.colidx)
        with pytest.raises(AssertionError, match="output Out"):
            b.verify("wrong output", out=b.d.out0 + 0.0625)
        assert not RC.same_bits(np.array([0.0]), np.array([-0.0])) and RC.same_bits(np.array([np.nan]), np.array([np.nan]))
    finally:
        b.free()


# ------------------------------------------------------------------------------------------------ the cases, through the double
@pytest.mark.parametrize("R,align", RC.WIDTH_CASES, ids=[RC.case_id(p) for p in RC.WIDTH_CASES])
def test_every_operation_at_every_width(ctx, R, align):
    RC.run(ctx, RC.edge_graph(tail_empty=R % 3 == 0), R, align, RC.Block.every_operation)


@pytest.mark.parametrize("R", RC.W_SWITCHES)
def test_switch_and_plan_operations(ctx, R):
    RC.run(ctx, RC.edge_graph(), R, "a16", RC.Block.switch_operations)
    RC.run(ctx, RC.hub_graph(), R, "a16", RC.Block.switch_operations)
    RC.run(ctx, RC.hub_graph(), R, "a16", RC.Block.planned_operations)


@pytest.mark.parametrize("R", RC.W_WINDOWS)
def test_windows(ctx, R):
    RC.run(ctx, RC.edge_graph(), R, "a16", lambda b: b.windows([80, 80, 200]))


@pytest.mark.parametrize("kind", ["all_empty", "one_row", "one_row_one_nonzero"])
@pytest.mark.parametrize("R", [16, 100, 301])
def test_degenerate_blocks(ctx, kind, R):
    RC.run(ctx, RC.degenerate_graph(kind), R, "a16", RC.Block.every_operation)


def test_expected_instance_table_covers_the_families():
    """the table of step 4 names about 25 instances per operation: every exact, NARROW, NX(V, 1 | 2) and tile instance of launch_shape"""
    table = RC.expected_table()
    for op in (RC.SDDMM, RC.SPMM, RC.FUSED):
        got = {i[1:] for i in table if i[0] == op}
        exact = {(l, 1, 2, True, False) for l in (1, 2, 4, 8, 16, 32, 64)} | {(64, v, 2, True, False) for v in (2, 3, 4)} | \
                {(32, v, 2, True, False) for v in (3, 5, 7)}
        narrow = {(l, 1, 2, True, True) for l in (4, 8, 16)}
        nx = {(64, v, w, False, False) for v in (1, 2, 4) for w in (1, 2)}
        assert got == exact | narrow | nx, (op, sorted(got ^ (exact | narrow | nx)))
