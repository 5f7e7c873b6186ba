"""One case list for two implementations of four optional kernel groups (include/hnh_grad.h, hnh_attention.h, hnh_attn_grad.h,
hnh_train.h): the HIP library (tests/test_gat_double_gpu.py) and the second CPU test double, oracle/liboracle_backend_gat.so, under
the stream-order checker (tests/test_gat_double_cpu.py).  A case takes (lib, ctx) of either backend through the ctypes signatures of
distributed_sddmm_amd/_kernels.py, builds operands whose pitches are wider than their widths and whose outputs sit inside guard
columns and one guard row, launches, checks the guards and compares with the numpy definitions the GAT tests already have:
gat_ref.xent_rows / stored_grad_ld / adam_step / sgd_step, gat_pass_ref.attention_ld / fused_row_pass / fused_col_pass / fused_pack,
and numpy in np.longdouble for the dense kernels.  The two backends need not agree with each other; each meets the bound.

Bounds (max |x - ref| / max |ref|): gat_gpu_harness.FTOL = 1e-12 for the forward pass (inside check_against_numpy), gat_gpu_harness.TOL
= 1e-10 for the backward kernels, hnh_testlib.TOL = 1e-11 for the loss and the optimizer (what tests/test_gat_train_gpu.py asserts for
them); the gate kernels and the pack kernel are exact.  Every case prints its observed error before it asserts.

Shapes are the smallest that still reach each path: see the case builders.  CASES is the list (refusals_case: every refused call)."""
import ctypes as C

import numpy as np

import gat_gpu_harness as G
import gat_pass_ref as P
import gat_ref as R
import hnh_testlib as T
import softmax_schedules as S
from distributed_sddmm_amd import _kernels as K
from test_gat_fused_backward_gpu import Problem as GradProblem  # the operands of one backward pass (backend-neutral)
from test_gat_train_gpu import OptimProblem, run_xent, xent_inputs  # ... of the loss and the optimizer kernels

ALPHA, FTOL, TOL, NWIN = G.ALPHA, G.FTOL, G.TOL, G.NWIN
GUARD = 7.0
INVALID, UNSUPPORTED = 1, K.ERR_UNSUPPORTED
GROUP_SIGNATURES = dict(list(K.GRAD_SIGNATURES.items()) + list(K.ATTN_SIGNATURES.items()) + list(K.ATTN_GRAD_SIGNATURES.items()) +
                        list(K.TRAIN_SIGNATURES.items()))
LD = np.longdouble


def bind(path):
    """The library at `path` with the mandatory table and the four groups bound (AttributeError if one is missing)."""
    lib = C.CDLL(path)
    for name, (res, args) in list(K.SIGNATURES.items()) + list(GROUP_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class Api(K.Ctx):
    """K.Ctx over a library of the caller's choice: what K.DevArray and the harness functions take as `ctx`."""

    def __init__(self, lib, device=0):
        self.lib = lib
        h = C.c_void_p()
        assert lib.hnh_ctx_create(device, C.byref(h)) == 0
        self.h = h


def observed(case, worst):
    T.record_observed("gat_double", case=case, worst=float(worst))
    print("observed gat_double %s worst %.2e" % (case, float(worst)))
    return float(worst)


def free(*arrays):
    for a in arrays:
        a.free()


# ------------------------------------------------------------------------------------------------ hnh_gemm_tn_f64
# (M, N, K, pad) -> the K slices of tn_plan: one 128 x 128 tile and 257 K tiles of 16 give eight slices of 33
GEMM_SHAPES = {(16, 8, 1, 0): 1, (17, 9, 4099, 3): 8, (128, 128, 4096, 0): 8, (130, 250, 777, 2): 1, (17, 9, 0, 3): 1}


def gemm_tn_case(M, N, Kk, pad):
    """C = A^T B with A, B at pitches M + pad, N + pad (pad 0 and even: the 16-byte loads; odd: scalar loads), C inside two guard columns
    and a guard row, the workspace between two guard words.  K = 0 zeroes C.  Twice: the same bits."""
    def run(lib, ctx):
        rng = np.random.default_rng(M * 1000 + N + Kk)
        lda, ldb, ldc = M + pad, N + pad, N + pad + 2
        a, b = np.full((max(Kk, 1), lda), 1e300), np.full((max(Kk, 1), ldb), 1e300)  # beyond the widths: never read
        a[:, :M], b[:, :N] = rng.uniform(-1, 1, (max(Kk, 1), M)), rng.uniform(-1, 1, (max(Kk, 1), N))
        c0 = rng.uniform(-1, 1, (M + 1, ldc))
        need = int(lib.hnh_gemm_tn_f64_workspace(M, N, Kk))
        slices = GEMM_SHAPES[(M, N, Kk, pad)]
        assert need == (slices * M * N if slices > 1 else 0), (need, slices)
        da, db, dc, dw = ctx.upload(a), ctx.upload(b), ctx.upload(c0), ctx.upload(np.full(need + 2, GUARD))

        def once():
            dc.set(c0)
            ctx.check(lib.hnh_gemm_tn_f64(ctx.h, M, N, Kk, da.ptr, lda, db.ptr, ldb, dc.ptr, ldc, dw.ptr + 8, need, K.STREAM_COMPUTE), "gemm_tn")
            ctx.sync()
            got, work = dc.get(), dw.get()
            assert np.array_equal(got[:, N:], c0[:, N:]) and np.array_equal(got[M], c0[M]), "pad columns and the row past the last are kept"
            assert work[0] == GUARD and work[-1] == GUARD, "guards round the workspace"
            return got[:M, :N]
        got = once()
        assert np.array_equal(once(), got), "a repeat must be bit-identical"
        if Kk == 0:
            assert np.all(got == 0.0)
            err = 0.0
        else:
            want = np.dot(np.asarray(a[:Kk, :M], dtype=LD).T, np.asarray(b[:Kk, :N], dtype=LD))
            err = T.rel(np.asarray(got, dtype=LD), want)
        free(da, db, dc, dw)
        assert observed("gemm_tn %s" % ((M, N, Kk, pad),), err) <= TOL
    return run


# ------------------------------------------------------------------------------------------------ the gate kernels: exact
def gate_kernels_case(lib, ctx):
    """hnh_leaky_relu_grad_f64, hnh_relu_grad_cols_f64, hnh_sum3_cols_f64, hnh_transpose_into_f64: the bits of the numpy expressions
    (the statements of test_gate_kernels_exact), inside guards."""
    rng = np.random.default_rng(5)
    n, alpha = 10007, 0.2
    e, da = rng.uniform(-1, 1, n + 1), rng.uniform(-1, 1, n + 1)
    e[:n:97] = 0.0
    de, dd = ctx.upload(e), ctx.upload(da)
    ctx.check(lib.hnh_leaky_relu_grad_f64(ctx.h, de.ptr, dd.ptr, alpha, n, K.STREAM_COMPUTE), "leaky_relu_grad")
    got_e, got_d = de.get(), dd.get()
    assert np.array_equal(got_e[:n], np.maximum(e[:n], 0.0) + np.minimum(e[:n], 0.0) * alpha) and got_e[n] == e[n]
    assert np.array_equal(got_d[:n], np.where(e[:n] > 0, da[:n], da[:n] * alpha)) and got_d[n] == da[n]
    free(de, dd)
    for rows, ld, col0, f in ((333, 40, 12, 16), (333, 41, 3, 33), (1, 5, 0, 1)):
        g, out = rng.uniform(-1, 1, (rows, ld)), rng.uniform(-1, 1, (rows, ld))
        out[::7, :] = 0.0
        dz0 = np.full((rows + 1, f + 3), 5.0)
        dg, do, dz = ctx.upload(g), ctx.upload(out), ctx.upload(dz0)
        ctx.check(lib.hnh_relu_grad_cols_f64(ctx.h, dz.ptr, f + 3, dg.ptr, ld, do.ptr, ld, col0, rows, f, K.STREAM_COMPUTE), "relu_grad_cols")
        got = dz.get()
        assert np.array_equal(got[:rows, :f], np.where(out[:, col0:col0 + f] > 0, g[:, col0:col0 + f], 0.0))
        assert np.all(got[:, f:] == 5.0) and np.all(got[rows] == 5.0)
        x, y, z = (rng.uniform(-1, 1, (rows, f)) for _ in range(3))
        dx, dy, dzz, dst = ctx.upload(x), ctx.upload(y), ctx.upload(z), ctx.upload(np.full((rows + 1, ld), 3.0))
        ctx.check(lib.hnh_sum3_cols_f64(ctx.h, dst.ptr, ld, col0, dx.ptr, dy.ptr, dzz.ptr, rows, f, K.STREAM_COMPUTE), "sum3")
        got = dst.get()
        assert np.array_equal(got[:rows, col0:col0 + f], (x + y) + z)
        assert np.all(got[:, :col0] == 3.0) and np.all(got[:, col0 + f:] == 3.0) and np.all(got[rows] == 3.0)
        free(dg, do, dz, dx, dy, dzz, dst)
    for wr, f, ld in ((24, 16, 24), (7, 33, 10), (1, 1, 3)):  # W (wr x f) into rows [f, 2 f) of a 3 f x ld matrix
        w = rng.uniform(-1, 1, (wr, f))
        dw, wt = ctx.upload(w), ctx.upload(np.full((3 * f, ld), 2.0))
        ctx.check(lib.hnh_transpose_into_f64(ctx.h, wt.ptr, ld, f, dw.ptr, wr, f, K.STREAM_COMPUTE), "transpose_into")
        got = wt.get()
        assert np.array_equal(got[f:2 * f, :wr], w.T) and np.all(got[:f] == 2.0) and np.all(got[2 * f:] == 2.0) and np.all(got[:, wr:] == 2.0)
        free(dw, wt)


# ------------------------------------------------------------------------------------------------ hnh_act_grad_cols_f64
def act_grad_case(rows, cols, even):
    """The middle one of three heads of `cols` columns in G and out, dZ at its own pitch with guard columns and a guard row, delta between
    guards; relu, elu and identity; outputs with +0, -0, exactly -1, and tiny negatives.  even: every pitch and col0 even (16-byte lanes
    when cols is even), else odd.  dZ exact for relu and identity (G or 0), TOL for elu's dZ and for delta, against gat_ref.stored_grad_ld."""
    def run(lib, ctx):
        worst = 0.0
        for act in R.ACTIVATIONS:
            rng = np.random.default_rng(1000 * rows + 10 * cols + even)
            col0 = cols + (cols & 1) if even else cols + 1 - (cols & 1)
            ld_g, ld_o, ld_dz = (v + (v % 2 if even else 1 - v % 2) for v in (3 * cols + 4, 3 * cols + 6, cols + 2))
            assert all(v % 2 == (0 if even else 1) for v in (ld_g, ld_o, ld_dz, col0))
            g = rng.uniform(-3, 3, (rows, ld_g))
            o = rng.uniform(-8, 4, (rows, ld_o))
            out = R.act(o, act)
            special = np.array([-1.0, 0.0, -0.0, -1.0 + 2.0 ** -53, -1e-300, 1e-300, -5e-324, -1e-17, 1e-17, -0.999999999999])
            flat = out[:, col0:col0 + cols].reshape(-1)
            idx = rng.permutation(flat.size)[:min(flat.size, len(special))]
            flat[idx] = special[:len(idx)] if act != "relu" else np.abs(special[:len(idx)])
            out[:, col0:col0 + cols] = flat.reshape(rows, cols)
            dz0, dl0 = np.full((rows + 1, ld_dz), GUARD), np.full(rows + 2, 9.0)
            d = dict(g=ctx.upload(g), out=ctx.upload(out), dz=ctx.upload(dz0), dl=ctx.upload(dl0))
            ctx.check(lib.hnh_act_grad_cols_f64(ctx.h, d["dz"].ptr, ld_dz, d["dl"].ptr + 8, d["g"].ptr, ld_g, d["out"].ptr, ld_o, col0, rows, cols,
                                                R.ACT_CODE[act], K.STREAM_COMPUTE), "act_grad_cols")
            ctx.sync()
            dz, dl = d["dz"].get(), d["dl"].get()
            free(*d.values())
            assert np.all(dz[:rows, cols:] == GUARD) and np.all(dz[rows] == GUARD) and dl[0] == 9.0 and dl[rows + 1] == 9.0, "guards"
            gg, oo = g[:, col0:col0 + cols], out[:, col0:col0 + cols]
            want_dz, want_dl = R.stored_grad_ld(gg, oo, act)
            if act == "relu":
                assert np.array_equal(dz[:rows, :cols], np.where(oo > 0, gg, 0.0))
            elif act == "identity":
                assert np.array_equal(dz[:rows, :cols], gg)
            else:
                assert np.all(dz[:rows, :cols][oo == -1.0] == 0.0), "a unit saturated at -1 has dZ = 0"
            assert not np.any(np.isnan(dl[1:rows + 1]))
            worst = max(worst, T.rel(np.asarray(dz[:rows, :cols], dtype=LD), want_dz), T.rel(np.asarray(dl[1:rows + 1], dtype=LD), want_dl))
        assert observed("act_grad rows=%d cols=%d %s" % (rows, cols, "even" if even else "odd"), worst) <= TOL
    return run


# ------------------------------------------------------------------------------------------------ hnh_attn_softmax_csr_p
def softmax_run(ctx, rowptr, colidx, x, y, groups=None, off=2):
    """gat_gpu_harness.softmax_pass with a guard row under relu_dst and a guard word behind lse, row_max and row_sum: returns (relu
    output, lse, row_max, row_sum, values)."""
    lib = ctx.lib
    m, R_ = x.shape
    nnz = int(rowptr[-1])
    ld = R_ + 4
    d = dict(rp=ctx.upload(rowptr), ci=ctx.upload(np.concatenate([colidx, [0]]).astype(np.int32)), x=ctx.upload(x), y=ctx.upload(y),
             out=ctx.upload(np.full(m * R_ + 1, 9.0)), vals=ctx.upload(np.full(nnz + 1, 3.0)), rmax=ctx.upload(np.full(m + 1, 5.0)),
             rsum=ctx.upload(np.full(m + 1, 5.0)), lse=ctx.upload(np.full(m + 1, 5.0)), dst=ctx.upload(np.full((m + 1, ld), GUARD)))
    blk = K.CsrBlock(m, nnz, m, int(np.diff(rowptr).max()), 0, d["rp"].ptr, d["ci"].ptr, None)
    st = K.AttnState(d["rmax"].ptr, d["rsum"].ptr, d["lse"].ptr, ALPHA, d["dst"].ptr + off * 8, ld)
    base = K.FUSED_VALUES_OVERWRITE

    def call(flags, win):
        ctx.check(lib.hnh_attn_softmax_csr_p(ctx.h, C.byref(blk), d["vals"].ptr, d["x"].ptr, d["y"].ptr, d["out"].ptr, R_, flags, C.byref(st), win,
                                             K.STREAM_COMPUTE), "softmax pass")
    if groups is None:
        call(base | K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH, None)
    else:
        bounds = (C.c_int32 * (NWIN - 1))(*[int(m * (b + 1) / NWIN) for b in range(NWIN - 1)])
        d["split"] = K.DevArray(ctx, (NWIN - 1) * m, np.int32)
        sp = d["split"].ptr
        ctx.check(lib.hnh_csr_window_bounds(ctx.h, m, d["rp"].ptr, d["ci"].ptr, NWIN - 1, bounds, sp, K.STREAM_COMPUTE), "window bounds")
        for k, (a, b) in enumerate(groups):
            win = K.CsrWindow(None if a == 0 else sp + (a - 1) * m * 4, None if b == NWIN else sp + (b - 1) * m * 4, int(b == NWIN))
            call(base | (K.FUSED_OUT_OVERWRITE if k == 0 else 0) | (K.ATTN_FINISH if b == NWIN else 0), C.byref(win))
    ctx.sync()
    dst, lse, rmax, rsum, vals = (d[k].get() for k in ("dst", "lse", "rmax", "rsum", "vals"))
    free(*d.values())
    assert np.all(dst[:, :off] == GUARD) and np.all(dst[:, off + R_:] == GUARD) and np.all(dst[m] == GUARD), "guards round the head's block"
    assert lse[m] == 5.0 and rmax[m] == 5.0 and rsum[m] == 5.0 and vals[nnz] == 3.0, "guards behind the row state and the scores"
    return dst[:m, off:off + R_], lse[:m], rmax[:m], rsum[:m], vals[:nnz]


def softmax_degrees(m, seed):
    """mixed_degrees' rows (empty rows, a few of 200 .. 300) with ONE hub row, of 600"""
    d = G.mixed_degrees(m, seed)
    d[m // 2] = 30
    assert d.max() == 600 and np.count_nonzero(d == 0) > m // 10
    return d


def softmax_case(width, off):
    """m = 512: one launch against gat_pass_ref.attention_ld (FTOL inside check_against_numpy), and the six windows in the groupings of
    gat_gpu_harness.GROUPINGS bit-identical to it."""
    def run(lib, ctx):
        m = 512
        rowptr, colidx, rows = G.square_graph(m, softmax_degrees(m, width + off), width)
        rng = np.random.default_rng(width * 10 + off)
        x, y = rng.uniform(-1, 1, (m, width)) * 2.0, rng.uniform(-1, 1, (m, width)) * 2.0
        whole = softmax_run(ctx, rowptr, colidx, x, y, off=off)
        G.check_against_numpy(whole, rows, colidx, m, x, y)
        o, lse, _ = P.attention_ld(rows, colidx.astype(np.int64), m, x, y, ALPHA)
        observed("softmax R=%d off=%d" % (width, off), max(T.rel(np.asarray(whole[0], dtype=LD), np.maximum(o, 0)), float(np.max(np.abs(whole[1] - lse)))))
        for name, groups in G.GROUPINGS.items():
            if groups is not None:
                again = softmax_run(ctx, rowptr, colidx, x, y, groups=groups, off=off)
                assert all(np.array_equal(a, b) for a, b in zip(again, whole)), "grouping %r differs from the single launch" % name
    return run


def softmax_schedule_case(lib, ctx):
    """The designed schedules of tests/softmax_schedules.py (m = 1024, width 16): the running max rises exactly where designed, so the
    rescale branch runs (also past exp's range: the jump rows); per schedule against the extended reference; windows bit-identical."""
    m, width = 1024, 16
    rowptr, colidx, x, y, rises, group = S.build(m, width, 3, nwin=NWIN)
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    one = softmax_run(ctx, rowptr, colidx, x, y)
    assert all(np.array_equal(a, b) for a, b in zip(P.max_rises(rowptr, one[4]), rises)), "the scores do not rise where designed"
    assert sum(len(r) > 1 for r in rises) > m // 4
    g = np.array(group)
    G.check_against_numpy(one, rows, colidx, m, x, y, sels=[g == name for name in S.SCHEDULES])
    again = softmax_run(ctx, rowptr, colidx, x, y, groups=G.GROUPINGS["uneven a"])
    assert all(np.array_equal(a, b) for a, b in zip(again, one))


def softmax_empty_block_case(width):
    """b->rowptr == NULL with each flag combination (the statements of test_empty_block in tests/test_attention_instances_gpu.py), with a
    guard row: a reset starts every row empty, a finish of it writes 0; without the reset the state passes (and is finished) as given."""
    def run(lib, ctx):
        m = 300
        rng = np.random.default_rng(width)
        mx0, l0, out0 = rng.uniform(-3, 3, m + 1), rng.uniform(0.5, 4.0, m + 1), rng.uniform(-2, 2, (m + 1, width))
        l0[:m:9], mx0[:m:9], out0[:m:9] = 0.0, -np.inf, 0.0
        ld, off = width + 4, 2
        blk = K.CsrBlock(m, 0, -1, 0, 0, None, None, None)

        def call(flags):
            d = dict(out=ctx.upload(out0), dst=ctx.upload(np.full((m + 1, ld), GUARD)), lse=ctx.upload(np.full(m + 1, 5.0)), rmax=ctx.upload(mx0),
                     rsum=ctx.upload(l0))
            st = K.AttnState(d["rmax"].ptr, d["rsum"].ptr, d["lse"].ptr, ALPHA, d["dst"].ptr + off * 8, ld)
            ctx.check(lib.hnh_attn_softmax_csr_p(ctx.h, C.byref(blk), None, None, None, d["out"].ptr, width, flags, C.byref(st), None, K.STREAM_COMPUTE),
                      "empty block")
            ctx.sync()
            res = {k: v.get() for k, v in d.items()}
            free(*d.values())
            assert np.all(res["dst"][:, :off] == GUARD) and np.all(res["dst"][:, off + width:] == GUARD) and np.all(res["dst"][m] == GUARD)
            assert res["lse"][m] == 5.0 and res["rmax"][m] == mx0[m] and res["rsum"][m] == l0[m] and np.array_equal(res["out"][m], out0[m])
            res["dst"] = res["dst"][:m, off:off + width]
            return {k: v[:m] for k, v in res.items()}
        r = call(K.FUSED_OUT_OVERWRITE)
        assert np.all(r["rmax"] == -np.inf) and np.all(r["rsum"] == 0.0) and np.all(r["out"] == 0.0) and np.all(r["dst"] == GUARD) and np.all(r["lse"] == 5.0)
        r = call(K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH)
        assert np.all(r["rmax"] == -np.inf) and np.all(r["rsum"] == 0.0) and np.all(r["dst"] == 0.0) and np.all(r["lse"] == 0.0)
        r = call(0)
        assert np.array_equal(r["rmax"], mx0[:m]) and np.array_equal(r["rsum"], l0[:m]) and np.array_equal(r["out"], out0[:m])
        assert np.all(r["dst"] == GUARD) and np.all(r["lse"] == 5.0)
        live = l0[:m] > 0
        o = np.zeros((m, width), dtype=LD)
        o[live] = np.asarray(out0[:m][live], dtype=LD) / np.asarray(l0[:m][live, None], dtype=LD)
        lse = np.zeros(m, dtype=LD)
        lse[live] = np.asarray(mx0[:m][live], dtype=LD) + np.log(np.asarray(l0[:m][live], dtype=LD))
        worst = 0.0
        for flag, name in ((0, "relu"), (K.ATTN_ACT_ELU, "elu"), (K.ATTN_ACT_IDENTITY, "identity")):
            r = call(K.ATTN_FINISH | flag)
            assert np.array_equal(r["rmax"], mx0[:m]) and np.array_equal(r["rsum"], l0[:m])
            assert np.all(r["dst"][~live] == 0.0) and np.all(r["lse"][~live] == 0.0) and np.count_nonzero(r["dst"]) > r["dst"].size // 3
            worst = max(worst, T.rel(np.asarray(r["dst"], dtype=LD), R.act_ld(o, name)), float(np.max(np.abs(r["lse"] - lse) / np.maximum(1.0, np.abs(lse)))))
        assert observed("softmax empty block R=%d" % width, worst) <= FTOL
    return run


# ------------------------------------------------------------------------------------------------ hnh_attn_grad_{row,col}_csr_p, _pack_f64
def grad_degrees(m, seed):
    """mixed_degrees with the 600-nonzero hub row (past the long-row threshold) and without the one of 1500"""
    d = G.mixed_degrees(m, seed)
    d[m // 2] = 30
    return d


def attn_grad_case(column_side, softmax, f):
    """m = 512 rows over 384 columns, a planted repeated pair, empty rows, a hub row of 600: overwrite and accumulate against
    gat_pass_ref.fused_row_pass / fused_col_pass, and the six windows in two groupings bit-identical to the single launch."""
    def run(lib, ctx):
        m = 512
        p = GradProblem(ctx, column_side, softmax, f, m=m, ncols=384, seed=2, degrees=grad_degrees(m, f))
        empty = np.diff(p.rowptr) == 0
        assert np.diff(p.rowptr).max() == 600 and np.count_nonzero(empty) > 50
        errs = []
        for overwrite in (True, False):
            got = p.run(overwrite)  # (asserts the guard columns and the guard row)
            want = p.want(overwrite)
            errs.append(T.rel(got, want))
            assert np.array_equal(got[empty], np.zeros((int(empty.sum()), f)) if overwrite else p.out0[:m, :f][empty])
            for name in ("uneven a", "one call per window"):
                assert np.array_equal(p.run(overwrite, G.GROUPINGS[name]), got), "grouping %r differs from the single launch" % name
        p.free()
        assert observed("attn_grad %s %s f=%d" % ("col" if column_side else "row", "softmax" if softmax else "none", f), max(errs)) <= TOL
    return run


def attn_grad_empty_block_case(lib, ctx):
    """rowptr == NULL: overwrite leaves zeros in the f columns of every row, accumulate leaves everything alone"""
    for column_side in (False, True):
        p = GradProblem(ctx, column_side, False, 33, m=256, ncols=96, degrees=np.full(256, 2))
        a, none = p.args(), K.CsrBlock(p.m, 0, -1, 0, 0, None, None, None)
        ctx.check(p.fn()(ctx.h, C.byref(none), C.byref(a), 0, None, K.STREAM_COMPUTE), "empty block, accumulate")
        ctx.sync()
        assert np.array_equal(p.d["out"].get(), p.out0)
        ctx.check(p.fn()(ctx.h, C.byref(none), C.byref(a), K.FUSED_OUT_OVERWRITE, None, K.STREAM_COMPUTE), "empty block, overwrite")
        ctx.sync()
        got = p.d["out"].get()
        assert np.all(got[:p.m, :33] == 0.0) and np.array_equal(got[:, 33:], p.out0[:, 33:]) and np.array_equal(got[p.m], p.out0[p.m])
        p.free()


def pack_case(lib, ctx):
    """The packed layout of include/hnh_attn_grad.h, exactly, for every f and both attentions, inside guard columns and a guard row."""
    rng = np.random.default_rng(4)
    for f in (1, 7, 33, 64, 128, 200, 256):
        for softmax in (False, True):
            rows, ld_a, ld_dz = 301, f + 3, f + 5
            pw = P.fused_packed_width(f, softmax)
            ld_p = pw + 2
            a, dz = rng.uniform(-1, 1, (rows, ld_a)), rng.uniform(-1, 1, (rows, ld_dz))
            lse, delta = rng.uniform(0, 3, rows), rng.uniform(-1, 1, rows)
            da, ddz, dl, dd, dp = ctx.upload(a), ctx.upload(dz), ctx.upload(lse), ctx.upload(delta), ctx.upload(np.full((rows + 1, ld_p), GUARD))
            ctx.check(lib.hnh_attn_grad_pack_f64(ctx.h, dp.ptr, ld_p, da.ptr, ld_a, ddz.ptr, ld_dz, dl.ptr if softmax else None, dd.ptr if softmax else None,
                                                 rows, f, K.STREAM_COMPUTE), "pack")
            got = dp.get()
            want = P.fused_pack(a[:, :f], dz[:, :f], lse if softmax else None, delta if softmax else None)
            assert np.array_equal(got[:rows, :pw], want) and np.all(got[:rows, pw:] == GUARD) and np.all(got[rows] == GUARD), (f, softmax)
            free(da, ddz, dl, dd, dp)


# ------------------------------------------------------------------------------------------------ hnh_softmax_gate_f64, hnh_rowdot_cols_f64
def gate_rowdot_case(lib, ctx):
    rng = np.random.default_rng(5)
    n = 10007
    e, da = rng.uniform(-2, 2, n + 1), rng.uniform(-1, 1, n + 1)
    e[:n:97] = 0.0
    lse, delta = rng.uniform(0, 3, n), rng.uniform(-1, 1, n)
    de, dd, dl, dde = ctx.upload(e), ctx.upload(da), ctx.upload(lse), ctx.upload(delta)
    ctx.check(lib.hnh_softmax_gate_f64(ctx.h, de.ptr, dd.ptr, dl.ptr, dde.ptr, ALPHA, n, K.STREAM_COMPUTE), "softmax gate")
    got_a, got_de = de.get(), dd.get()
    assert got_a[n] == e[n] and got_de[n] == da[n], "the entry past the last is kept"
    el, dal = np.asarray(e[:n], dtype=LD), np.asarray(da[:n], dtype=LD)
    a = np.exp(np.where(el > 0, el, LD(ALPHA) * el) - np.asarray(lse, dtype=LD))
    worst = max(T.rel(np.asarray(got_a[:n], dtype=LD), a),
                T.rel(np.asarray(got_de[:n], dtype=LD), a * (dal - np.asarray(delta, dtype=LD)) * np.where(el > 0, LD(1), LD(ALPHA))))
    free(de, dd, dl, dde)
    rows = 333
    for cols in (1, 16, 33):
        for col0 in (0, 3):
            ld_dz, ld_o = cols + 3, col0 + cols + 5
            dz, o = rng.uniform(-1, 1, (rows, ld_dz)), rng.uniform(-1, 1, (rows, ld_o))
            ddz, do_, dout = ctx.upload(dz), ctx.upload(o), ctx.upload(np.full(rows + 1, 9.0))
            ctx.check(lib.hnh_rowdot_cols_f64(ctx.h, dout.ptr, ddz.ptr, ld_dz, do_.ptr, ld_o, col0, rows, cols, K.STREAM_COMPUTE), "rowdot cols")
            got = dout.get()
            want = np.sum(np.asarray(dz[:, :cols], dtype=LD) * np.asarray(o[:, col0:col0 + cols], dtype=LD), axis=1)
            assert got[rows] == 9.0
            worst = max(worst, T.rel(np.asarray(got[:rows], dtype=LD), want))
            free(ddz, do_, dout)
    assert observed("softmax_gate / rowdot_cols", worst) <= TOL


# ------------------------------------------------------------------------------------------------ hnh_xent_rows_f64
def xent_case(heads, classes, rows):
    """xent_inputs of tests/test_gat_train_gpu.py (unlabelled rows, exact ties, logits up to +-700) through its run_xent (pitches wider than
    the row, guards round G, the result words and the workspace): loss_sum and G within hnh_testlib.TOL of gat_ref.xent_rows in
    np.longdouble, `correct` exactly; G null, and G aliasing out, give the same bits."""
    def run(lib, ctx):
        out, labels, _ = xent_inputs(rows, heads, classes, seed=heads * 1000 + classes + rows)
        inv_n = 1.0 / 137.0
        want_loss, want_correct, want_g = R.xent_rows(out, labels, heads, inv_n, LD)
        loss, correct, g = run_xent(ctx, out, labels, heads, classes, inv_n)
        assert np.all(g[labels < 0] == 0.0), "unlabelled rows get G = 0"
        want_loss = float(np.asarray(want_loss, dtype=np.float64).reshape(-1)[0])
        scale = abs(want_loss) if (classes > 1 and abs(want_loss) > 0) else 1.0
        errs = dict(loss=abs(loss - want_loss) / scale, g=T.rel(g, np.asarray(want_g, dtype=np.float64)))
        observed("xent heads=%d classes=%d rows=%d" % (heads, classes, rows), max(errs.values()))
        assert correct == want_correct, "argmax with ties to the lowest index, exactly"
        assert max(errs.values()) <= T.TOL, errs
        no_g = run_xent(ctx, out, labels, heads, classes, inv_n, with_g=False)
        assert no_g[0] == loss and no_g[1] == correct
        in_place = run_xent(ctx, out, labels, heads, classes, inv_n, in_place=True)
        assert in_place[0] == loss and np.array_equal(in_place[2], g), "G may alias out"
    return run


def xent_bad_label_case(lib, ctx):
    """A label >= classes: result[0] NaN, result[1] minus their number, the rows unlabelled; no rows: both sums zero."""
    out, labels, _ = xent_inputs(50, 2, 5, seed=1)
    labels[[3, 17]] = [5, 99]
    loss, correct, g = run_xent(ctx, out, labels, 2, 5, 0.1)
    assert np.isnan(loss) and correct == -2.0 and np.all(g[[3, 17]] == 0.0)
    res, work = ctx.upload(np.full(2, GUARD)), ctx.upload(np.zeros(8))
    ctx.check(lib.hnh_xent_rows_f64(ctx.h, None, 4, None, 0, 1, 4, 1.0, None, 0, res.ptr, work.ptr, 8, K.STREAM_COMPUTE), "no rows")
    assert np.all(res.get() == 0.0)
    free(res, work)


# ------------------------------------------------------------------------------------------------ hnh_optim_step_f64
def optim_case(kind, hyper):
    """OptimProblem of tests/test_gat_train_gpu.py: 60 tensors (two launches of HNH_OPTIM_MAX_TENSORS), gradients that are column blocks
    of a wider matrix or interleave at pitch 2, padded parameter pitches with guards; two steps against gat_ref (hnh_testlib.TOL per
    tensor, asserted inside step)."""
    def run(lib, ctx):
        p = OptimProblem(ctx, kind, seed=3)
        assert len(p.tensors) > K.OPTIM_MAX_TENSORS and any(t["ld_p"] > t["cols"] for t in p.tensors) and any(t["ld_g"] > t["cols"] for t in p.tensors)
        worst = 0.0
        for step in (1, 2):
            worst = max(worst, p.step(step, hyper))
            p.new_gradients()
        p.free()
        observed("optim %s" % kind, worst)
    return run


def optim_three_tensors_case(lib, ctx):
    """Three tensors of different sizes, the middle one without elements (and without pointers): the others move, nothing else does."""
    rng = np.random.default_rng(8)
    hyper = dict(lr=0.05, momentum=0.9, weight_decay=5e-4)
    shapes = [(5, 3, 4, 7), (0, 6, 6, 6), (1, 9, 11, 9)]  # rows, cols, ld_p, ld_g
    host, dev, tab = [], [], (K.OptimTensor * 3)()
    for k, (rows, cols, ld_p, ld_g) in enumerate(shapes):
        if rows == 0:
            tab[k] = K.OptimTensor(None, ld_p, None, ld_g, None, None, rows, cols)
            host.append(None)
            dev.append(None)
            continue
        p, g, v = rng.standard_normal((rows + 1, ld_p)), rng.standard_normal((rows, ld_g)), rng.standard_normal((rows, cols))
        dp, dg, dv = ctx.upload(p), ctx.upload(g), ctx.upload(np.concatenate([v.reshape(-1), [GUARD]]))
        tab[k] = K.OptimTensor(dp.ptr, ld_p, dg.ptr, ld_g, None, dv.ptr, rows, cols)
        host.append((p, g, v))
        dev.append((dp, dg, dv))
    hy = K.Optim(K.OPTIM_SGD, 0, hyper["lr"], 0.9, 0.999, 1e-8, hyper["momentum"], hyper["weight_decay"], 0.1, 0.001)
    ctx.check(lib.hnh_optim_step_f64(ctx.h, tab, 3, C.byref(hy), K.STREAM_COMPUTE), "optim step")
    ctx.sync()
    worst = 0.0
    for (rows, cols, ld_p, ld_g), h, d in zip(shapes, host, dev):
        if h is None:
            continue
        p, g, v = h
        want_p, want_v = R.sgd_step(p[:rows, :cols], g[:, :cols], v, hyper["lr"], momentum=hyper["momentum"], weight_decay=hyper["weight_decay"])
        got_p, got_v = d[0].get(), d[2].get()
        assert np.array_equal(got_p[:, cols:], p[:, cols:]) and np.array_equal(got_p[rows], p[rows]) and got_v[-1] == GUARD, "guards"
        assert np.array_equal(d[1].get(), g), "the gradient is only read"
        worst = max(worst, T.rel(got_p[:rows, :cols], want_p), T.rel(got_v[:-1].reshape(rows, cols), want_v))
        free(*d)
    assert observed("optim three tensors", worst) <= T.TOL


# ------------------------------------------------------------------------------------------------ refused calls
def refusals_case(lib, ctx):
    """Every refusal the headers and the HIP sources name: the status class, hnh_last_error naming the entry point, and nothing written
    (one sentinel buffer holds every operand)."""
    S_ = K.STREAM_COMPUTE
    n_reg, reg_doubles = 16, 1024
    sent = np.full(n_reg * reg_doubles, GUARD)
    buf = ctx.upload(sent)
    m, deg = 8, 2
    rp, ci = ctx.upload((np.arange(m + 1) * deg).astype(np.int32)), ctx.upload(np.concatenate([np.tile([0, 1], m), [0]]).astype(np.int32))

    def r(k, off=0):  # region k of the sentinel buffer (16-byte aligned; off doubles into it)
        return buf.ptr + 8 * (reg_doubles * k + off)
    blk = K.CsrBlock(m, m * deg, m, deg, 0, rp.ptr, ci.ptr, None)
    no_rowptr = K.CsrBlock(m, m * deg, m, deg, 0, None, ci.ptr, None)
    last, not_last = K.CsrWindow(None, None, 1), K.CsrWindow(None, None, 0)
    vo, ov, fin = K.FUSED_VALUES_OVERWRITE, K.FUSED_OUT_OVERWRITE, K.ATTN_FINISH
    calls = []

    # hnh_attn_softmax_csr_p(block, values, X, Y, Out, R, flags, state, window)
    def softmax(b=blk, vals=r(0), x=r(1), y=r(2), out=r(3), R_=4, flags=vo | ov | fin, st="ok", win=None, relu=r(4), relu_ld=8, lse=r(5)):
        state = None if st is None else C.byref(K.AttnState(r(6), r(7), lse, ALPHA, relu, relu_ld))
        return lib.hnh_attn_softmax_csr_p(ctx.h, None if b is None else C.byref(b), vals, x, y, out, R_, flags, state, None if win is None else C.byref(win), S_)
    sm = "hnh_attn_softmax_csr_p"
    calls += [(sm, lambda: softmax(b=None), INVALID), (sm, lambda: softmax(st=None), INVALID), (sm, lambda: softmax(R_=0), INVALID),
              (sm, lambda: softmax(flags=vo | ov | fin | K.FUSED_LEAKY_RELU), INVALID), (sm, lambda: softmax(flags=vo | ov | fin | 0x80), INVALID),
              (sm, lambda: softmax(flags=vo | ov | fin | K.ATTN_ACT_ELU | K.ATTN_ACT_IDENTITY), INVALID),
              (sm, lambda: softmax(flags=vo | ov | K.ATTN_ACT_ELU), INVALID), (sm, lambda: softmax(flags=vo | ov | K.ATTN_ACT_IDENTITY), INVALID),
              (sm, lambda: softmax(win=not_last), INVALID), (sm, lambda: softmax(relu_ld=3), INVALID), (sm, lambda: softmax(lse=None), INVALID),
              (sm, lambda: softmax(relu=None), INVALID), (sm, lambda: softmax(out=None), INVALID), (sm, lambda: softmax(vals=None), INVALID),
              (sm, lambda: softmax(x=None), INVALID), (sm, lambda: softmax(out=r(1)), INVALID), (sm, lambda: softmax(b=no_rowptr), INVALID),
              (sm, lambda: softmax(R_=514, relu_ld=516), UNSUPPORTED), (sm, lambda: softmax(R_=257, relu_ld=258), UNSUPPORTED),
              (sm, lambda: softmax(R_=300, relu_ld=304, relu=r(4, 1)), UNSUPPORTED), (sm, lambda: softmax(R_=300, relu_ld=303), UNSUPPORTED)]

    # hnh_attn_grad_{row,col}_csr_p(block, args, flags, window)
    def grad(col, b=blk, args="ok", flags=ov, win=None, x=r(1), ld_x=4, dz=r(2), ld_dz=4, lse=None, delta=None, y=r(3), ld_y=None, out=r(4), ld_out=6,
             f=4, softmax=0):
        ld_y = (K.attn_grad_packed_width(f, bool(softmax)) if col else f) if ld_y is None else ld_y
        a = None if args is None else C.byref(K.AttnGrad(x, ld_x, dz, ld_dz, lse, delta, y, ld_y, out, ld_out, f, softmax, ALPHA))
        fn = lib.hnh_attn_grad_col_csr_p if col else lib.hnh_attn_grad_row_csr_p
        return fn(ctx.h, None if b is None else C.byref(b), a, flags, None if win is None else C.byref(win), S_)
    for col in (0, 1):
        who = "hnh_attn_grad_col_csr_p" if col else "hnh_attn_grad_row_csr_p"
        for kw, code in ((dict(b=None), INVALID), (dict(args=None), INVALID), (dict(f=0), INVALID), (dict(flags=K.FUSED_LEAKY_RELU), INVALID),
                         (dict(flags=ov | fin), INVALID), (dict(f=257, ld_x=258, ld_dz=258, ld_out=258), UNSUPPORTED), (dict(out=None), INVALID),
                         (dict(ld_out=3), INVALID), (dict(ld_x=3), INVALID), (dict(x=None), INVALID), (dict(y=None), INVALID), (dict(out=r(1)), INVALID),
                         (dict(b=no_rowptr), INVALID)):
            calls.append((who, lambda col=col, kw=kw: grad(col, **kw), code))
    row, colp = "hnh_attn_grad_row_csr_p", "hnh_attn_grad_col_csr_p"
    calls += [(row, lambda: grad(0, dz=None), INVALID), (row, lambda: grad(0, ld_dz=3), INVALID), (row, lambda: grad(0, ld_y=3), INVALID),
              (row, lambda: grad(0, lse=r(5)), INVALID), (row, lambda: grad(0, delta=r(5)), INVALID), (row, lambda: grad(0, dz=r(4)), INVALID),
              (colp, lambda: grad(1, ld_y=6), INVALID), (colp, lambda: grad(1, softmax=1, ld_y=8), INVALID), (colp, lambda: grad(1, ld_y=9), INVALID),
              (colp, lambda: grad(1, y=r(3, 1)), INVALID)]

    # hnh_attn_grad_pack_f64(P, ld_p, A, ld_a, dZ, ld_dz, lse, delta, rows, f)
    def pack(p=r(0), ld_p=10, a=r(1), ld_a=4, dz=r(2), ld_dz=4, lse=r(3), delta=r(4), rows=8, f=4):
        return lib.hnh_attn_grad_pack_f64(ctx.h, p, ld_p, a, ld_a, dz, ld_dz, lse, delta, rows, f, S_)
    calls += [("hnh_attn_grad_pack_f64", lambda kw=kw: pack(**kw), INVALID) for kw in
              (dict(delta=None), dict(lse=None), dict(ld_p=8), dict(ld_p=11), dict(ld_a=3), dict(ld_dz=3), dict(p=None), dict(a=None), dict(dz=None),
               dict(f=0), dict(rows=-1))]

    # hnh_gemm_tn_f64(M, N, K, A, lda, B, ldb, C, ldc, work, work_doubles): (17, 9, 4099) needs eight slabs
    def gemm(M=4, N=4, Kk=4, a=r(0), lda=4, b=r(1), ldb=4, c=r(2), ldc=4, work=None, wd=0):
        return lib.hnh_gemm_tn_f64(ctx.h, M, N, Kk, a, lda, b, ldb, c, ldc, work, wd, S_)
    need = 8 * 17 * 9
    calls += [("hnh_gemm_tn_f64", lambda kw=kw: gemm(**kw), INVALID) for kw in
              (dict(M=-1), dict(Kk=-1), dict(lda=3), dict(ldb=3), dict(ldc=3), dict(c=None), dict(a=None), dict(b=None),
               dict(M=17, N=9, Kk=4099, lda=17, ldb=9, ldc=9, work=r(3), wd=need - 1), dict(M=17, N=9, Kk=4099, lda=17, ldb=9, ldc=9, work=None, wd=need))]

    # the dense helpers of hnh_grad.h and hnh_attention.h
    calls += [("hnh_leaky_relu_grad_f64", lambda: lib.hnh_leaky_relu_grad_f64(ctx.h, r(0), r(1), 0.2, -1, S_), INVALID),
              ("hnh_leaky_relu_grad_f64", lambda: lib.hnh_leaky_relu_grad_f64(ctx.h, None, r(1), 0.2, 4, S_), INVALID),
              ("hnh_leaky_relu_grad_f64", lambda: lib.hnh_leaky_relu_grad_f64(ctx.h, r(0), None, 0.2, 4, S_), INVALID)]

    def relu_grad(dz=r(0), ld_dz=4, g=r(1), ld_g=8, out=r(2), ld_o=8, col0=2, rows=2, cols=4):
        return lib.hnh_relu_grad_cols_f64(ctx.h, dz, ld_dz, g, ld_g, out, ld_o, col0, rows, cols, S_)

    def act_grad(dz=r(0), ld_dz=4, dl=r(3), g=r(1), ld_g=8, out=r(2), ld_o=8, col0=2, rows=2, cols=4, act=1):
        return lib.hnh_act_grad_cols_f64(ctx.h, dz, ld_dz, dl, g, ld_g, out, ld_o, col0, rows, cols, act, S_)
    shape_kws = (dict(dz=None), dict(g=None), dict(out=None), dict(rows=-1), dict(cols=-1), dict(col0=-1), dict(col0=5), dict(ld_dz=3), dict(ld_g=5), dict(ld_o=5))
    calls += [("hnh_relu_grad_cols_f64", lambda kw=kw: relu_grad(**kw), INVALID) for kw in shape_kws]
    calls += [("hnh_act_grad_cols_f64", lambda kw=kw: act_grad(**kw), INVALID) for kw in shape_kws + (dict(dl=None), dict(act=3), dict(act=-1))]

    def sum3(dst=r(0), ld=8, col0=2, x=r(1), y=r(2), z=r(3), rows=2, cols=4):
        return lib.hnh_sum3_cols_f64(ctx.h, dst, ld, col0, x, y, z, rows, cols, S_)
    calls += [("hnh_sum3_cols_f64", lambda kw=kw: sum3(**kw), INVALID) for kw in (dict(col0=5), dict(col0=-1), dict(rows=-1), dict(dst=None), dict(x=None), dict(y=None), dict(z=None))]

    def transpose(dst=r(0), ld=4, row0=1, w=r(1), rows=4, cols=3):
        return lib.hnh_transpose_into_f64(ctx.h, dst, ld, row0, w, rows, cols, S_)
    calls += [("hnh_transpose_into_f64", lambda kw=kw: transpose(**kw), INVALID) for kw in (dict(ld=3), dict(row0=-1), dict(rows=-1), dict(dst=None), dict(w=None))]

    def gate(e=r(0), da=r(1), lse=r(2), delta=r(3), n=4):
        return lib.hnh_softmax_gate_f64(ctx.h, e, da, lse, delta, ALPHA, n, S_)
    calls += [("hnh_softmax_gate_f64", lambda kw=kw: gate(**kw), INVALID) for kw in (dict(n=-1), dict(e=None), dict(da=None), dict(lse=None), dict(delta=None))]

    def rowdot(out=r(0), dz=r(1), ld_dz=4, o=r(2), ld_o=8, col0=2, rows=2, cols=4):
        return lib.hnh_rowdot_cols_f64(ctx.h, out, dz, ld_dz, o, ld_o, col0, rows, cols, S_)
    calls += [("hnh_rowdot_cols_f64", lambda kw=kw: rowdot(**kw), INVALID) for kw in
              (dict(ld_dz=3), dict(ld_o=5), dict(col0=-1), dict(rows=-1), dict(out=None), dict(dz=None), dict(o=None))]

    # hnh_xent_rows_f64(out, ld_out, labels, rows, heads, classes, inv_n, G, ld_g, result, work, work_doubles): include/hnh_train.h and the
    # HIP entry point answer heads * classes > HNH_XENT_MAX_WIDTH with HNH_ERR_INVALID
    def xent(out=r(0), ld_out=4, labels=r(1), rows=2, heads=1, classes=4, g=None, ld_g=0, res=r(2), work=r(3), wd=8):
        return lib.hnh_xent_rows_f64(ctx.h, out, ld_out, labels, rows, heads, classes, 1.0, g, ld_g, res, work, wd, S_)
    calls += [("hnh_xent_rows_f64", lambda kw=kw: xent(**kw), INVALID) for kw in
              (dict(heads=0), dict(classes=0), dict(rows=-1), dict(heads=1, classes=K.XENT_MAX_WIDTH + 1, ld_out=K.XENT_MAX_WIDTH + 1),
               dict(heads=8, classes=513, ld_out=8 * 513), dict(ld_out=3), dict(g=r(4), ld_g=3), dict(res=None), dict(work=None), dict(wd=5), dict(out=None),
               dict(labels=None))]

    # hnh_optim_step_f64(tensors, n, hyper)
    def optim(kind=K.OPTIM_SGD, n=1, table="ok", hyper="ok", p=r(0), ld_p=2, g=r(1), ld_g=2, mm=None, v=r(2), bias1=0.1):
        tab = None if table is None else (K.OptimTensor * 1)(K.OptimTensor(p, ld_p, g, ld_g, mm, v, 2, 2))
        hy = None if hyper is None else C.byref(K.Optim(kind, 0, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.0, bias1, 0.001))
        return lib.hnh_optim_step_f64(ctx.h, tab, n, hy, S_)
    calls += [("hnh_optim_step_f64", lambda kw=kw: optim(**kw), INVALID) for kw in
              (dict(hyper=None), dict(table=None), dict(n=-1), dict(kind=5), dict(kind=K.OPTIM_ADAM), dict(kind=K.OPTIM_ADAM, mm=r(3), bias1=0.0),
               dict(ld_p=1), dict(ld_g=1), dict(p=None), dict(g=None), dict(v=None))]

    for k, (who, call, code) in enumerate(calls):
        rc = call()
        msg = lib.hnh_last_error(ctx.h)
        assert rc == code, (k, who, rc, code, msg)
        assert who.encode() in msg, (k, who, msg)
    ctx.sync()
    assert np.array_equal(buf.get(), sent), "a refused call writes nothing"
    # ... and the calls next to the refused ones are accepted: the finish on the last window, widths at the limits, an empty table
    ctx.check(softmax(win=last), "the finish on the last window")
    ctx.check(optim(n=0, table=None), "an empty table")
    ctx.check(gemm(M=0), "no rows")
    ctx.sync()
    assert len(calls) >= 140
    print("observed gat_double refusals: %d refused calls, each with its status, its entry point named, nothing written" % len(calls))
    free(buf, rp, ci)


CASES = [("gemm_tn-%d-%d-%d-%d" % s, gemm_tn_case(*s)) for s in GEMM_SHAPES]
CASES += [("gate_kernels", gate_kernels_case)]
CASES += [("act_grad-rows%d-cols%d-%s" % (rows, cols, "even" if even else "odd"), act_grad_case(rows, cols, even))
          for rows in (1, 257) for cols in (1, 2, 7, 64, 100, 129) for even in (1, 0)]
CASES += [("softmax-R%d-off%d" % (w, off), softmax_case(w, off)) for w in (7, 64, 100, 128, 200, 256, 300) for off in (2, 3) if not (w > 256 and off % 2)]
CASES += [("softmax-schedule", softmax_schedule_case)] + [("softmax-empty-block-R%d" % w, softmax_empty_block_case(w)) for w in (7, 200)]
CASES += [("attn_grad-%s-%s-f%d" % ("col" if cs else "row", "softmax" if sm else "none", f), attn_grad_case(cs, sm, f))
          for cs in (False, True) for sm in (False, True) for f in (7, 33, 64, 128, 200, 256)]
CASES += [("attn_grad-empty-block", attn_grad_empty_block_case), ("attn_grad-pack", pack_case), ("softmax_gate-rowdot_cols", gate_rowdot_case)]
CASES += [("xent-h%d-c%d-rows%d" % (h, c, rows), xent_case(h, c, rows)) for h, c in ((1, 1), (1, 7), (3, 5), (2, 40), (1, 121), (6, 121))
          for rows in (1, 5, 1000)]
CASES += [("xent-bad-label", xent_bad_label_case), ("optim-sgd", optim_case("sgd", dict(lr=0.05, momentum=0.9, weight_decay=5e-4))),
          ("optim-adam", optim_case("adam", dict(lr=0.01, weight_decay=5e-4))), ("optim-three-tensors", optim_three_tensors_case),
          ("refusals", refusals_case)]
IDS = [name for name, _ in CASES]
