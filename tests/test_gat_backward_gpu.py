"""GAT backward pass on the GPU (GAT::backwardPass, include/hnh_grad.h): the split-K weight-gradient GEMM and the gate kernels
against numpy, then dW of every (layer, head) and the input gradient against the numpy definition (tests/gat_ref.py, attention none)
over loopback ranks, determinism, side effects, a few SGD steps, and the schedules that must refuse.

Observed on an MI355X (max |x - ref| / max |ref| per matrix, worst of dW of every (layer, head) and dX): er8_r16 over every
grid below <= 9.8e-16; benchmark widths (input 256, 128 / 64 features per head) <= 1.6e-15; R-MAT with hub rows <= 1.6e-15.
The bound asserted is 1e-10."""
import numpy as np
import pytest

import gat_gpu_harness as G
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import ctx, hashed_weights, hip_backend  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("M,N,Kd,pad", [(16, 8, 1, 0), (17, 9, 4099, 3), (128, 128, 4096, 0), (130, 250, 777, 2),
                                        (256, 1024, (1 << 16) + 3, 0), (200, 72, 5000, 6)])
def test_gemm_tn_vs_numpy(ctx, M, N, Kd, pad):
    """C = A^T B with A stored K x M and B stored K x N, leading dimensions wider than the widths when pad > 0; ragged in M, N, K."""
    lib = ctx.lib
    rng = np.random.default_rng(M * 7 + N + Kd)
    lda, ldb, ldc = M + pad, N + pad, N + 2 * pad
    a = rng.uniform(-1, 1, (Kd, lda))
    b = rng.uniform(-1, 1, (Kd, ldb))
    want = a[:, :M].T @ b[:, :N]
    need = lib.hnh_gemm_tn_f64_workspace(M, N, Kd)
    da, db = ctx.upload(a), ctx.upload(b)
    c0 = np.full((M, ldc), 7.0)
    dc = ctx.upload(c0)
    work = K.DevArray(ctx, max(need, 1), np.float64)
    outs = []
    for _ in range(2):
        ctx.check(lib.hnh_gemm_tn_f64(ctx.h, M, N, Kd, da.ptr, lda, db.ptr, ldb, dc.ptr, ldc, work.ptr, need, K.STREAM_COMPUTE), "gemm_tn")
        outs.append(dc.get())
    assert np.array_equal(outs[0], outs[1]), "two calls must be bit-identical"
    got = outs[0]
    assert np.all(got[:, N:] == 7.0), "columns beyond N are not written"
    assert T.rel(got[:, :N], want) <= 1e-12, T.rel(got[:, :N], want)
    for d in (da, db, dc, work):
        d.free()


def test_gemm_tn_rejects_a_short_workspace(ctx):
    lib = ctx.lib
    M, N, Kd = 64, 64, 1 << 14
    need = lib.hnh_gemm_tn_f64_workspace(M, N, Kd)
    assert need > 0
    a = ctx.upload(np.ones((Kd, M)))
    c = ctx.upload(np.zeros((M, N)))
    work = K.DevArray(ctx, need, np.float64)
    assert lib.hnh_gemm_tn_f64(ctx.h, M, N, Kd, a.ptr, M, a.ptr, N, c.ptr, N, work.ptr, need - 1, K.STREAM_COMPUTE) == 1
    ctx.check(lib.hnh_gemm_tn_f64(ctx.h, M, N, Kd, a.ptr, M, a.ptr, N, c.ptr, N, work.ptr, need, K.STREAM_COMPUTE), "gemm_tn")
    assert np.all(c.get() == float(Kd))
    for d in (a, c, work):
        d.free()


def test_gate_kernels_exact(ctx):
    lib = ctx.lib
    rng = np.random.default_rng(5)
    n, alpha = 10007, 0.2
    e = rng.uniform(-1, 1, n)
    e[::97] = 0.0
    da = rng.uniform(-1, 1, n)
    de_, dd = ctx.upload(e), ctx.upload(da)
    ctx.check(lib.hnh_leaky_relu_grad_f64(ctx.h, de_.ptr, dd.ptr, alpha, n, K.STREAM_COMPUTE), "leaky_relu_grad")
    assert np.array_equal(de_.get(), np.maximum(e, 0.0) + np.minimum(e, 0.0) * alpha)
    assert np.array_equal(dd.get(), np.where(e > 0, da, da * alpha))
    rows, ld, col0, f = 333, 40, 12, 16
    g, out = rng.uniform(-1, 1, (rows, ld)), rng.uniform(-1, 1, (rows, ld))
    out[::7, :] = 0.0
    dg, do, dz = ctx.upload(g), ctx.upload(out), ctx.upload(np.full((rows, f + 3), 5.0))
    ctx.check(lib.hnh_relu_grad_cols_f64(ctx.h, dz.ptr, f + 3, dg.ptr, ld, do.ptr, ld, col0, rows, f, K.STREAM_COMPUTE), "relu_grad_cols")
    got = dz.get()
    assert np.array_equal(got[:, :f], np.where(out[:, col0:col0 + f] > 0, g[:, col0:col0 + f], 0.0)) and np.all(got[:, f:] == 5.0)
    x, y, z = (rng.uniform(-1, 1, (rows, f)) for _ in range(3))
    dx_, dy_, dz_ = ctx.upload(x), ctx.upload(y), ctx.upload(z)
    dst = ctx.upload(np.full((rows, ld), 3.0))
    ctx.check(lib.hnh_sum3_cols_f64(ctx.h, dst.ptr, ld, col0, dx_.ptr, dy_.ptr, dz_.ptr, rows, f, K.STREAM_COMPUTE), "sum3")
    got = dst.get()
    assert np.array_equal(got[:, col0:col0 + f], (x + y) + z) and np.all(got[:, :col0] == 3.0) and np.all(got[:, col0 + f:] == 3.0)
    w = rng.uniform(-1, 1, (24, f))
    dw, wt = ctx.upload(w), ctx.upload(np.zeros((3 * f, 24)))
    ctx.check(lib.hnh_transpose_into_f64(ctx.h, wt.ptr, 24, f, dw.ptr, 24, f, K.STREAM_COMPUTE), "transpose_into")
    got = wt.get()
    assert np.array_equal(got[f:2 * f], w.T) and not got[:f].any() and not got[2 * f:].any()
    for d in (de_, dd, dg, do, dz, dx_, dy_, dz_, dst, dw, wt):
        d.free()


# ------------------------------------------------------------------------------------------------ the operator
def run_backward(world, alg, c, rows, cols, m, x, layers, weights, g_glob, rounds=1):
    """Forward + backward on one rank; returns this rank's blocks and the results of every round."""
    return G.run_rounds(world, rows, cols, m, x, layers, weights, None, g_glob, rounds, out_after=True, alg=alg, c=c)


def check_against_reference(per_rank, rows, cols, m, x, layers, weights, g_glob, label):
    G.compare(G.assembled(per_rank, 0, m, layers), G.reference(rows, cols, m, x, layers, weights, None, g_glob), "gat_backward", label, len(per_rank),
              check=("dw", "dx"))


GRIDS = [("15d_fusion1", 1, 1), ("15d_fusion1", 4, 1), ("15d_fusion1", 4, 2), ("15d_fusion1", 8, 2), ("15d_fusion1", 6, 2),
         ("15d_fusion1", 9, 3), ("15d_fusion2", 1, 1), ("15d_fusion2", 4, 1)]


@pytest.mark.parametrize("alg,p,c", GRIDS)
def test_backward_er8(alg, p, c):
    case = T.case_inputs("er8_r16")
    rows, cols, m = case["rows"], case["cols"], case["M"]
    x = case["A"] * T.GAT_INPUT_SCALE
    layers = T.GAT_LAYERS
    w = hashed_weights(layers, 40.0)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 9) * 16.0
    per_rank = H.run_spmd(p, lambda wd: run_backward(wd, alg, c, rows, cols, m, x, layers, w, g))
    check_against_reference(per_rank, rows, cols, m, x, layers, w, g, "er8_r16 %s p%d c%d" % (alg, p, c))


@pytest.mark.parametrize("alg,p,c", [("15d_fusion2", 1, 1), ("15d_fusion1", 4, 2)])
def test_backward_at_benchmark_widths(alg, p, c):
    """Layer input 256, 128 and 64 features per head: the exact-width kernel instances and full MFMA tiles of both GEMMs."""
    m, layers = 1 << 13, [(256, 128, 2), (256, 64, 3)]
    rows, cols = H.generate_er(m, m, m * 16, 77)
    x = O.dense_fill(m, 256, 41) * 16.0
    w = hashed_weights(layers, 8.0)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 3) * 64.0
    per_rank = H.run_spmd(p, lambda wd: run_backward(wd, alg, c, rows, cols, m, x, layers, w, g))
    out = T.assemble_dense([dict(o=pr["rounds"][0]["out"], subA=pr["subA"]) for pr in per_rank], "o", "subA", m, 192)
    assert np.count_nonzero(out) > out.size // 10 and np.count_nonzero(out == 0.0) > out.size // 10  # both sides of the ReLU
    check_against_reference(per_rank, rows, cols, m, x, layers, w, g, "benchmark widths %s p%d c%d" % (alg, p, c))


@pytest.mark.parametrize("alg,p,c", [("15d_fusion1", 1, 1), ("15d_fusion1", 4, 2), ("15d_fusion2", 1, 1)])
def test_backward_rmat_hub_rows(alg, p, c):
    """R-MAT degrees: hub rows and hub columns take the long-row paths of the SDDMM / SpMM passes on both S and S^T."""
    m, layers = 1 << 13, [(64, 64, 2), (128, 32, 2)]
    rows, cols = H.generate_rmat(13, m * 16)
    deg = np.bincount(rows, minlength=m)
    assert deg.max() >= 512 and np.bincount(cols, minlength=m).max() >= 512
    x = O.dense_fill(m, 64, 8) * 8.0
    w = hashed_weights(layers, 4.0)
    g = O.dense_fill(m, 64, 4) * 32.0
    per_rank = H.run_spmd(p, lambda wd: run_backward(wd, alg, c, rows, cols, m, x, layers, w, g))
    check_against_reference(per_rank, rows, cols, m, x, layers, w, g, "rmat hubs %s p%d c%d" % (alg, p, c))


def test_backward_is_deterministic_and_leaves_the_forward_alone():
    case = T.case_inputs("er8_r16")
    rows, cols, m = case["rows"], case["cols"], case["M"]
    x = case["A"] * T.GAT_INPUT_SCALE
    w = hashed_weights(T.GAT_LAYERS, 40.0)
    g = O.dense_fill(m, 12, 9) * 16.0
    per_rank = H.run_spmd(4, lambda wd: run_backward(wd, "15d_fusion1", 2, rows, cols, m, x, T.GAT_LAYERS, w, g, rounds=2))
    for pr in per_rank:
        a, b = pr["rounds"]
        assert np.array_equal(a["out"], a["out_after"]) and np.array_equal(b["out"], b["out_after"]), "backward changed the output"
        assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["dx"], b["dx"])
        for k in w:
            assert np.array_equal(a["dw"][k], b["dw"][k])


@pytest.mark.parametrize("alg,p,c", [("15d_fusion2", 1, 1), ("15d_fusion1", 4, 2)])
def test_sgd_lowers_the_loss(alg, p, c):
    case = T.case_inputs("er8_r16")
    rows, cols, m = case["rows"], case["cols"], case["M"]
    x = case["A"] * T.GAT_INPUT_SCALE
    target = O.dense_fill(m, 12, 21) * 4.0
    w = hashed_weights(T.GAT_LAYERS, 40.0)
    per_rank = H.run_spmd(p, lambda wd: G.sgd(wd, rows, cols, m, x, T.GAT_LAYERS, target, 5, 0.02, w, alg=alg, c=c))
    loss = np.sum(np.array([pr[0] for pr in per_rank]), axis=0)
    assert all(loss[i + 1] < loss[i] for i in range(5)), loss


@pytest.mark.parametrize("alg,p,c", [("15d_sparse", 2, 1), ("25d_dense_replicate", 4, 1), ("25d_sparse_replicate", 4, 1),
                                     ("15d_fusion2", 4, 2)])
def test_unsupported_schedules_refuse(alg, p, c):
    case = T.case_inputs("er8_r16")
    rows, cols, m = case["rows"], case["cols"], case["M"]
    layers = [(16, 8, 2)]

    def rank(world):
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, alg, sp, 16, c)
        gnn = H.GAT(d, layers, T.GAT_ALPHA)
        g = H.Dense.create(world, *gnn.buffer_shape(1))
        with pytest.raises(H.HnhError, match="backwardPass"):
            gnn.backwardPass(g)
        world.sync()  # nothing was left in flight
        for h in (g, gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(p, rank))


def test_backward_needs_a_current_forward():
    case = T.case_inputs("er8_r16")
    rows, cols, m = case["rows"], case["cols"], case["M"]
    layers = T.GAT_LAYERS
    w = hashed_weights(layers)

    def rank(world):
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, "15d_fusion1", sp, 16, 1)
        gnn = H.GAT(d, layers, T.GAT_ALPHA)
        for k, wk in w.items():
            gnn.set_weight(*k, wk)
        g = H.Dense.create(world, *gnn.buffer_shape(len(layers)), fill=1.0)
        with pytest.raises(H.HnhError, match="forwardPass"):
            gnn.backwardPass(g)
        gnn.forwardPass()
        gnn.set_weight(0, 0, w[(0, 0)])
        with pytest.raises(H.HnhError, match="forwardPass"):
            gnn.backwardPass(g)
        x = H.Dense.create(world, *gnn.buffer_shape(0))
        gnn.forwardPass()
        gnn.set_input(x)
        with pytest.raises(H.HnhError, match="forwardPass"):
            gnn.backwardPass(g)
        gnn.forwardPass()
        gnn.backwardPass(g)  # and with a current forward pass it runs
        world.sync()
        for h in (g, x, gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(2, rank))
