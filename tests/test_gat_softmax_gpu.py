"""GAT softmax attention on the GPU (include/hnh_attention.h, GAT attention mode "softmax"): the fused softmax pass against numpy over
widths and row lengths (empty rows up to hub rows), with forced column panels and scores far beyond exp's range; its independence of
how a row's nonzeros are grouped into launches; a closed form that does not need numpy; the backward kernels; and the operator's
forward output, dW of every (layer, head) and dX against tests/gat_ref.py over loopback ranks, determinism, side effects,
SGD training and the schedules that must refuse.

Observed on an MI355X (max |x - ref| / max |ref| per matrix, worst of the output, dW of every (layer, head) and dX): er8_r16 at
p = 1, 2, 4, 8 <= 1.2e-15; benchmark widths (256, 128, 64 features per head) <= 1.4e-15; R-MAT with hub rows <= 1.2e-15.  The bound
asserted is 1e-10."""
import ctypes as C

import numpy as np
import pytest

import gat_gpu_harness as G
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import ALPHA, check_against_numpy, ctx, hashed_weights, hip_backend, mixed_degrees, softmax_pass, square_graph  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("width", [1, 2, 7, 16, 64, 100, 128, 256])
def test_softmax_pass_vs_numpy(ctx, width):
    m = 2048
    deg = mixed_degrees(m, width, empty=())
    rowptr, colidx, rows = square_graph(m, deg, width + 1)
    rng = np.random.default_rng(width)
    x, y = rng.uniform(-1, 1, (m, width)), rng.uniform(-1, 1, (m, width))
    got = softmax_pass(ctx, rowptr, colidx, x, y, ALPHA)
    check_against_numpy(got, rows, colidx, m, x, y)
    again = softmax_pass(ctx, rowptr, colidx, x, y, ALPHA)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls must be bit-identical"


@pytest.mark.parametrize("width", [16, 128, 256])
def test_scores_beyond_the_range_of_exp(ctx, width):
    """Scores up to +-1e3: exp of a raw score would overflow (or underflow to a 0 / 0 row); the online softmax stays exact."""
    m = 1024
    rowptr, colidx, rows = square_graph(m, mixed_degrees(m, 3, empty=()), 4)
    rng = np.random.default_rng(9)
    scale = np.sqrt(3e3 / np.sqrt(width))
    x, y = rng.uniform(-1, 1, (m, width)) * scale, rng.uniform(-1, 1, (m, width)) * scale
    got = softmax_pass(ctx, rowptr, colidx, x, y, ALPHA)
    assert np.abs(got[4]).max() > 700.0
    check_against_numpy(got, rows, colidx, m, x, y)


# one width per instance of the softmax pass (launch_shape<Op::kFusedSoftmax>), the earlier three included: exact (32,1,2) 64,
# (64,1,2) 128, (64,2,2) 256; bounds-checked NX(1,2) 16 / 100, NX(2,2) 200, NX(4,2) 300, NX(1,1) 7, NX(2,1) 101, NX(4,1) 201
INSTANCE_WIDTHS = [7, 16, 64, 100, 101, 128, 200, 201, 256, 300]


@pytest.mark.parametrize("width", INSTANCE_WIDTHS)
def test_forced_panels_are_bit_identical(monkeypatch, width):
    """Column panels (several launches over every row) continue the row state nonzero by nonzero: the same bits as one launch."""
    m = 4096
    rowptr, colidx, rows = square_graph(m, mixed_degrees(m, 5, empty=()), 6)
    rng = np.random.default_rng(2)
    x, y = rng.uniform(-1, 1, (m, width)), rng.uniform(-1, 1, (m, width))
    c1 = K.Ctx(0)
    one = softmax_pass(c1, rowptr, colidx, x, y, ALPHA)
    c1.close()
    monkeypatch.setenv("HNH_PANEL_BYTES", str(m * width * 8 / 5))
    monkeypatch.setenv("HNH_MAX_PANELS", "8")
    monkeypatch.setenv("HNH_PANELS_WITH_HUBS", "1")  # (hnh_panel_count's rule for the other passes; the softmax pass never splits hub rows)
    c5 = K.Ctx(0)
    assert c5.lib.hnh_panel_count(c5.h, m, int(rowptr[-1]), m, width, int(np.diff(rowptr).max())) == 5
    five = softmax_pass(c5, rowptr, colidx, x, y, ALPHA)
    c5.close()
    assert all(np.array_equal(a, b) for a, b in zip(one, five))
    check_against_numpy(five, rows, colidx, m, x, y)


@pytest.mark.parametrize("width", INSTANCE_WIDTHS)
def test_grouping_independence(ctx, width):
    """The same block walked with its 6 windows grouped as 1, 2 or 5 launches (and window by window): bit-identical outputs, lse,
    row state and scores — what a launch-local state merged at the end would not give."""
    m = 2048
    rowptr, colidx, rows = square_graph(m, mixed_degrees(m, 8, empty=()), 9)
    rng = np.random.default_rng(width)
    x, y = rng.uniform(-1, 1, (m, width)) * 3.0, rng.uniform(-1, 1, (m, width)) * 3.0
    results = [softmax_pass(ctx, rowptr, colidx, x, y, ALPHA, groups=g)
               for g in ([(0, 6)], [(0, 3), (3, 6)], [(0, 1), (1, 2), (2, 4), (4, 5), (5, 6)], [(q, q + 1) for q in range(6)])]
    whole = softmax_pass(ctx, rowptr, colidx, x, y, ALPHA)
    for r in results:
        assert all(np.array_equal(a, b) for a, b in zip(r, whole))
    check_against_numpy(whole, rows, colidx, m, x, y)


@pytest.mark.parametrize("width", [7, 64, 256])
def test_constant_column_closed_form(ctx, width):
    """A with a constant column kappa: the softmax weights of a row sum to 1, so every non-empty row gets kappa there; empty rows 0."""
    m, kappa = 2048, 0.75
    rowptr, colidx, rows = square_graph(m, mixed_degrees(m, 11, empty=()), 12)
    a = np.random.default_rng(13).uniform(-1, 1, (m, width)) * 2.0
    a[:, 0] = kappa
    got = softmax_pass(ctx, rowptr, colidx, a, a, ALPHA)[0]
    live = np.diff(rowptr) > 0
    assert np.max(np.abs(got[live, 0] - kappa)) <= 1e-13 and np.all(got[~live] == 0.0)


def test_wide_rows_and_bad_calls_are_refused(ctx):
    lib = ctx.lib
    m, width = 64, 600
    rowptr, colidx, _ = square_graph(m, np.full(m, 3), 1)
    drp, dci = ctx.upload(rowptr), ctx.upload(colidx)
    x = ctx.upload(np.ones((m, width)))
    out, dst = K.DevArray(ctx, m * width, np.float64), ctx.upload(np.zeros((m, width)))
    vals, rmax, rsum, lse = (K.DevArray(ctx, max(int(rowptr[-1]), m), np.float64) for _ in range(4))
    blk = K.CsrBlock(m, int(rowptr[-1]), m, 3, 0, drp.ptr, dci.ptr, None)
    st = K.AttnState(rmax.ptr, rsum.ptr, lse.ptr, ALPHA, dst.ptr, width)
    flags = K.FUSED_VALUES_OVERWRITE | K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH
    assert lib.hnh_attn_softmax_csr_p(ctx.h, C.byref(blk), vals.ptr, x.ptr, x.ptr, out.ptr, width, flags, C.byref(st), None, K.STREAM_COMPUTE) == 4
    assert b"one-pass" in lib.hnh_last_error(ctx.h)
    not_last = K.CsrWindow(None, None, 0)
    assert lib.hnh_attn_softmax_csr_p(ctx.h, C.byref(blk), vals.ptr, x.ptr, x.ptr, out.ptr, 64, flags, C.byref(st), C.byref(not_last),
                                      K.STREAM_COMPUTE) == 1
    assert lib.hnh_attn_softmax_csr_p(ctx.h, C.byref(blk), vals.ptr, x.ptr, x.ptr, out.ptr, 64, flags | 4, C.byref(st), None, K.STREAM_COMPUTE) == 1
    ctx.sync()
    for a in (drp, dci, x, out, dst, vals, rmax, rsum, lse):
        a.free()


def test_backward_kernels_exact(ctx):
    lib = ctx.lib
    rng = np.random.default_rng(5)
    n = 10007
    e, da = rng.uniform(-2, 2, n), rng.uniform(-1, 1, n)
    e[::97] = 0.0
    lse, delta = rng.uniform(0, 3, n), rng.uniform(-1, 1, n)
    de_, dd, dl, dde = ctx.upload(e), ctx.upload(da), ctx.upload(lse), ctx.upload(delta)
    ctx.check(lib.hnh_softmax_gate_f64(ctx.h, de_.ptr, dd.ptr, dl.ptr, dde.ptr, ALPHA, n, K.STREAM_COMPUTE), "softmax gate")
    a = np.exp(np.where(e > 0, e, ALPHA * e) - lse)
    assert T.rel(de_.get(), a) <= 1e-15
    assert T.rel(dd.get(), a * (da - delta) * np.where(e > 0, 1.0, ALPHA)) <= 1e-15
    rows, f, ld, col0 = 1001, 100, 260, 128
    dz, o = rng.uniform(-1, 1, (rows, f)), rng.uniform(-1, 1, (rows, ld))
    ddz, do_, dout = ctx.upload(dz), ctx.upload(o), ctx.upload(np.full(rows + 1, 9.0))
    ctx.check(lib.hnh_rowdot_cols_f64(ctx.h, dout.ptr, ddz.ptr, f, do_.ptr, ld, col0, rows, f, K.STREAM_COMPUTE), "rowdot cols")
    got = dout.get()
    assert T.rel(got[:rows], np.sum(dz * o[:, col0:col0 + f], axis=1)) <= 1e-14 and got[rows] == 9.0
    for d in (de_, dd, dl, dde, ddz, do_, dout):
        d.free()


# ------------------------------------------------------------------------------------------------ the operator
def run_softmax_gat(world, alg, c, rows, cols, m, x, layers, weights, g_glob, rounds=1):
    """Forward + backward with softmax attention on one rank; returns this rank's blocks and the results of every round."""
    return G.run_rounds(world, rows, cols, m, x, layers, weights, None, g_glob, rounds, out_after=True, alg=alg, c=c, attention="softmax")


def check_against_reference(per_rank, rows, cols, m, x, layers, weights, g_glob, label):
    got = G.assembled(per_rank, 0, m, layers)
    assert np.count_nonzero(got["out"]) > got["out"].size // 10 and np.count_nonzero(got["out"] == 0.0) > got["out"].size // 10  # both sides of the ReLU
    G.compare(got, G.reference(rows, cols, m, x, layers, weights, None, g_glob, attention="softmax"), "gat_softmax", label, len(per_rank))


@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_softmax_gat_er8(p):
    case = T.case_inputs("er8_r16")
    rows, cols, m = case["rows"], case["cols"], case["M"]
    x = case["A"] * T.GAT_INPUT_SCALE
    layers = T.GAT_LAYERS
    w = hashed_weights(layers)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 9) * 16.0
    per_rank = H.run_spmd(p, lambda wd: run_softmax_gat(wd, "15d_fusion2", 1, rows, cols, m, x, layers, w, g))
    check_against_reference(per_rank, rows, cols, m, x, layers, w, g, "er8_r16 p%d" % p)


@pytest.mark.parametrize("p", [1, 4])
def test_softmax_gat_at_benchmark_widths(p):
    """256 features per head (the benchmark's GAT), then 128 and 64: the exact-width instances of the softmax pass."""
    m, layers = 1 << 12, [(64, 256, 1), (256, 128, 2), (256, 64, 3)]
    rows, cols = H.generate_er(m, m, m * 16, 77)
    x = O.dense_fill(m, 64, 41) * 16.0
    w = hashed_weights(layers)
    g = O.dense_fill(m, 192, 3) * 64.0
    per_rank = H.run_spmd(p, lambda wd: run_softmax_gat(wd, "15d_fusion2", 1, rows, cols, m, x, layers, w, g))
    check_against_reference(per_rank, rows, cols, m, x, layers, w, g, "benchmark widths p%d" % p)


@pytest.mark.parametrize("p", [1, 4])
def test_softmax_gat_rmat_hub_rows(p):
    m, layers = 1 << 13, [(64, 64, 2), (128, 32, 2)]
    rows, cols = H.generate_rmat(13, m * 16)
    assert np.bincount(rows, minlength=m).max() >= 512 and np.bincount(cols, minlength=m).max() >= 512
    x = O.dense_fill(m, 64, 8) * 8.0
    w = hashed_weights(layers)
    g = O.dense_fill(m, 64, 4) * 32.0
    per_rank = H.run_spmd(p, lambda wd: run_softmax_gat(wd, "15d_fusion2", 1, rows, cols, m, x, layers, w, g))
    check_against_reference(per_rank, rows, cols, m, x, layers, w, g, "rmat hubs p%d" % p)


@pytest.mark.parametrize("graph_kind", ["er", "rmat"])
def test_two_rounds_are_bit_identical_and_backward_leaves_the_output(graph_kind):
    if graph_kind == "er":
        case = T.case_inputs("er8_r16")
        rows, cols, m = case["rows"], case["cols"], case["M"]
        x, layers = case["A"] * T.GAT_INPUT_SCALE, T.GAT_LAYERS
    else:
        m, layers = 1 << 12, [(16, 16, 2), (32, 8, 2)]
        rows, cols = H.generate_rmat(12, m * 16)
        x = O.dense_fill(m, 16, 8) * 8.0
    w = hashed_weights(layers)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 9) * 16.0
    per_rank = H.run_spmd(4, lambda wd: run_softmax_gat(wd, "15d_fusion2", 1, rows, cols, m, x, layers, w, g, rounds=2))
    for pr in per_rank:
        a, b = pr["rounds"]
        assert np.array_equal(a["out"], a["out_after"]) and np.array_equal(b["out"], b["out_after"]), "backward changed the output"
        assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["dx"], b["dx"])
        for k in w:
            assert np.array_equal(a["dw"][k], b["dw"][k])


@pytest.mark.parametrize("p", [1, 2])
def test_sgd_lowers_the_loss(p):
    case = T.case_inputs("er8_r16")
    rows, cols, m = case["rows"], case["cols"], case["M"]
    x = case["A"] * T.GAT_INPUT_SCALE
    target = O.dense_fill(m, 12, 21) * 0.05
    w = hashed_weights(T.GAT_LAYERS)
    per_rank = H.run_spmd(p, lambda wd: G.sgd(wd, rows, cols, m, x, T.GAT_LAYERS, target, 5, 0.02, w, attention="softmax"))
    loss = np.sum(np.array([pr[0] for pr in per_rank]), axis=0)
    assert all(loss[i + 1] < loss[i] for i in range(5)), loss


@pytest.mark.parametrize("alg,p,c", [("15d_fusion1", 2, 1), ("15d_fusion1", 4, 2), ("15d_sparse", 2, 1), ("25d_dense_replicate", 4, 1),
                                     ("25d_sparse_replicate", 4, 1), ("15d_fusion2", 4, 2)])
def test_unsupported_schedules_refuse(alg, p, c):
    case = T.case_inputs("er8_r16")
    rows, cols, m = case["rows"], case["cols"], case["M"]

    def rank(world):
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, alg, sp, 16, c)
        gnn = H.GAT(d, [(16, 8, 2)], ALPHA, attention="softmax")
        with pytest.raises(H.HnhError, match="softmax"):
            gnn.forwardPass()
        world.sync()  # nothing was left in flight
        gnn.set_attention("none")
        gnn.forwardPass()  # the operator lives on
        world.sync()
        for h in (gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(p, rank))
