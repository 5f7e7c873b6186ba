"""The GAT at odd and wide head widths on the GPU, forward and backward, in both attention modes.

Every other GAT test uses heads of 4 .. 256 features, powers of two.  Here two layer stacks (input, features per head, heads):
    odd   [(16, 7, 3), (21, 101, 2), (202, 201, 2)]   the softmax instances NX(1,1), NX(2,1), NX(4,1); heads at odd column offsets
    wide  [(24, 200, 2), (400, 300, 1), (300, 512, 1)] NX(2,2), NX(4,2) and the 512 limit
on er8_r16 and an R-MAT graph with hub rows (2^12 vertices).  Softmax attention (15d_fusion2, c = 1, p = 1 and 4) and attention "none" (also a head of 301 features, whose odd width above 256 takes the composed fallback of the
fused pass and the column-block epilogue kernels) on 15d_fusion2 and 15d_fusion1 grids, both against tests/gat_ref.py.  A softmax
head wider than the one-pass limit is refused with an error that names it.

Observed on an MI355X (max |x - ref| / max |ref| per matrix, worst of the output, dW of every (layer, head) and dX): softmax <= 2.4e-15,
none <= 3.7e-15.  The bound asserted is 1e-10 (TOL of the other GAT tests)."""
import numpy as np
import pytest

import gat_gpu_harness as G
import hnh_testlib as T
from distributed_sddmm_amd import api as H
from gat_gpu_harness import hip_backend  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu

STACKS = {"odd": [(16, 7, 3), (21, 101, 2), (202, 201, 2)], "wide": [(24, 200, 2), (400, 300, 1), (300, 512, 1)], "odd301": [(16, 301, 2)]}


def problem(graph, layers):
    """(rows, cols, m, x, g): the graph, an input of the stack's width and dL/d(output)."""
    if graph == "er8":
        case = T.case_inputs("er8_r16")
        rows, cols, m = case["rows"], case["cols"], case["M"]
    else:
        m = 1 << 12
        rows, cols = H.generate_rmat(12, m * 16)
        assert np.bincount(rows, minlength=m).max() >= 256
    x = O.dense_fill(m, layers[0][0], 41) * 16.0
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 3) * 32.0
    return rows, cols, m, x, g


@pytest.mark.parametrize("p", [1, 4])
@pytest.mark.parametrize("graph", ["er8", "rmat"])
@pytest.mark.parametrize("stack", ["odd", "wide"])
def test_softmax_gat_widths(stack, graph, p):
    layers = STACKS[stack]
    rows, cols, m, x, g = problem(graph, layers)
    w = G.hashed_weights(layers)
    per_rank = H.run_spmd(p, lambda wd: G.run_rounds(wd, rows, cols, m, x, layers, w, None, g, out_after=True, attention="softmax"))
    got = G.assembled(per_rank, 0, m, layers)
    assert np.count_nonzero(got["out"]) > got["out"].size // 10 and np.count_nonzero(got["out"] == 0.0) > got["out"].size // 10  # both sides of the ReLU
    G.compare(got, G.reference(rows, cols, m, x, layers, w, None, g, attention="softmax"), "gat_softmax", "widths %s %s p%d" % (stack, graph, p), p)


NONE_GRIDS = [("15d_fusion2", 1, 1), ("15d_fusion1", 1, 1), ("15d_fusion1", 4, 1)]
NONE_CASES = [(s, gr, grid) for s in STACKS for gr in ("er8", "rmat") for grid in NONE_GRIDS] + \
             [("wide", gr, ("15d_fusion1", 4, 2)) for gr in ("er8", "rmat")]  # (c = 2: the stack whose widths are all even)


@pytest.mark.parametrize("stack,graph,grid", NONE_CASES, ids=["%s-%s-%s_p%d_c%d" % (s, gr, *grid) for s, gr, grid in NONE_CASES])
def test_none_gat_widths(stack, graph, grid):
    alg, p, c = grid
    layers = STACKS[stack]
    rows, cols, m, x, g = problem(graph, layers)
    w = G.hashed_weights(layers)
    per_rank = H.run_spmd(p, lambda wd: G.run_rounds(wd, rows, cols, m, x, layers, w, None, g, out_after=True, alg=alg, c=c))
    got, want = G.assembled(per_rank, 0, m, layers), G.reference(rows, cols, m, x, layers, w, None, g)
    assert T.rel(got["out"], want["out"]) <= G.TOL, T.rel(got["out"], want["out"])
    G.compare(got, want, "gat_backward", "widths %s %s %s p%d c%d" % (stack, graph, alg, p, c), p, check=("dw", "dx"))


@pytest.mark.parametrize("layers", [[(16, 301, 2)], [(16, 8, 2), (16, 514, 1)]], ids=["f301", "f514"])
def test_softmax_refuses_wider_heads(layers):
    case = T.case_inputs("er8_r16")
    rows, cols, m = case["rows"], case["cols"], case["M"]

    def rank(world):
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, "15d_fusion2", sp, 16, 1)
        gnn = H.GAT(d, layers, T.GAT_ALPHA, attention="softmax")
        with pytest.raises(H.HnhError, match="at most 512 features") as e:
            gnn.forwardPass()
        assert str(max(f for _, f, _ in layers)) in str(e.value)
        world.sync()  # nothing was left in flight
        for h in (gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(1, rank))
