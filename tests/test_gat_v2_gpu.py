"""The GAT's score "gatv2" on the GPU (include/hnh_attn_v2.h, GAT score "gatv2").

Kernel level, through ctypes: the forward pass against the extended-precision numpy reference (tests/gat_v2_ref.py, fwd_pass_ld), the backward
row and column passes and the dense finish against numpy, at widths 1, 7, 8, 33, 64, 100, 128, 200, 255, 256 on mixed_degrees(300, ..) blocks
(empty rows, a repeated pair, rows of 200 - 300, hub rows of 600 and 1500; a square block for the forward and the row pass, a rectangular one
standing for S^T for the column pass), with pitches wider than the widths, every operand at an odd column offset (the 8-byte lanes) or an even
one, guard values round every output, a vector of mixed signs, and A scaled until |z| reaches about 800; the passes' independence of how a
row's nonzeros are split into launches (whole rows, one call per window, two uneven groupings of six windows, forced Infinity-Cache panels),
bit for bit; run-to-run bit identity of every kernel, the da reduction included; the width limit; empty blocks.
Operator level: GAT(..., attention="softmax", score="gatv2") on 15d_fusion2, c = 1 over 1, 2, 4, 8 loopback ranks against the numpy definition
— output, every dW, da and dX — at the small shape, the benchmark widths and on an R-MAT graph with hub rows, with feature dropout and with the
published activations; p = 8 against p = 1; scores "dot" and "additive" bit-identical before and after a "gatv2" round on the same object; a
ten-step Adam trajectory of the published layers through train_step, parameters bit-equal across ranks.

Bounds: FTOL = 1e-12 for the forward kernel, TOL = 1e-10 for the backward kernels, the finish and the operator (the bounds of
test_gat_additive_gpu.py); the trajectory within 10 x the divergence of a reference run whose gradients are perturbed at 1e-10 (the rule of
test_gat_train_gpu.py).  The observed worst cases are recorded with T.record_observed.

Observed on an MI355X (max |x - ref| / max |ref| per matrix): forward kernel <= 1.0e-15 over every width and both alignments, <= 3.8e-14 at
|z| = 800; backward row pass <= 4.3e-15, column pass <= 7.9e-15, <= 1.3e-13 at |z| = 800; finish <= 1e-10 asserted; the operator (worst of the
output, dW, da of every (layer, head) and dX) <= 1.8e-15 on er8_r16 over p = 1 .. 8 in the three configurations, <= 7.9e-15 at the benchmark
widths, <= 7.2e-15 at odd heads, <= 7.1e-15 on the R-MAT graph; p = 8 against p = 1 <= 1.2e-15; the Adam trajectory 5.3e-16 in the parameters
(bound 1.6e-8), 3.1e-16 in the loss (bound 2.1e-11), loss 1.422 -> 0.954 in ten steps."""
import ctypes as C

import numpy as np
import pytest

import gat_gpu_harness as G
import gat_pass_ref as P
import gat_ref as R
import gat_v2_ref as V
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import (ALPHA, COL, FTOL, FWD, GROUPINGS, NWIN, PASS_NAMES, ROW, TOL, assembled, ctx, er8, errors, hashed_weights,  # noqa: F401
                             hip_backend, one_round, same, setup, teardown)
from oracle import oracle as O

pytestmark = pytest.mark.gpu
WIDTHS = [1, 7, 8, 33, 64, 100, 128, 200, 255, 256]
ACT_FLAG = {"relu": 0, "elu": K.ATTN_ACT_ELU, "identity": K.ATTN_ACT_IDENTITY}
GUARD = 1e300  # beyond an operand's width: never read (a read would show as inf or NaN)


def padded(mat, ld, off):
    """`mat` at column offset `off` of a GUARD-filled matrix of pitch ld"""
    out = np.full((mat.shape[0], ld), GUARD)
    out[:, off:off + mat.shape[1]] = mat
    return out


class V2Problem:
    """One pass's operands on the device.  odd=True puts every operand but the packed one (whose layout asks for 16 bytes) at an odd column
    offset of an odd pitch: the 8-byte instances; otherwise offsets and pitches are even and an even f takes the 16-byte lanes.  big > 0
    scales A (both sides: z is homogeneous in it) so that |z| reaches about `big`."""

    def __init__(self, ctx, pas, f, m=300, ncols=None, seed=0, odd=False, big=0.0):
        self.ctx, self.pas, self.f, self.m, self.odd = ctx, pas, f, m, odd
        ncols = self.ncols = ncols or (211 if pas == COL else m)
        fp = self.fp = f + (f & 1)
        rng = np.random.default_rng(1000 * f + seed + 17 * pas)
        self.rowptr, self.colidx, self.rows = G.graph(m, ncols, G.mixed_degrees(m, seed + f), seed + 1)
        rows, cols = self.rows, self.colidx.astype(np.int64)
        a = rng.standard_normal(f) / np.sqrt(f)
        if f > 1:
            a[0], a[1] = abs(a[0]), -abs(a[1])  # mixed signs for certain
        x, y = rng.uniform(-1, 1, (m, f)), rng.uniform(-1, 1, (ncols, f))
        if big:
            scale = big / np.abs(V.scores(x, y, rows, cols, a, ALPHA)[0]).max()
            x, y = x * scale, y * scale
        self.a, self.x, self.y = a, x, y
        self.z = V.scores(x, y, rows, cols, a, ALPHA)[0]
        owner, n_own = (cols, ncols) if pas == COL else (rows, m)  # the S rows: the gathered rows of the column pass
        _, self.lse_in = R.row_softmax(owner, n_own, self.z)
        self.delta = rng.uniform(-1, 1, n_own)
        self.dz = rng.uniform(-1, 1, (n_own, f))
        off = self.off = 1 if odd else 2
        ld = lambda w: w + off + (3 if (w + off) % 2 == (0 if odd else 1) else 2)  # odd: an odd pitch; else an even one  # noqa: E731
        self.ld_x, self.ld_dz = ld(f), ld(f)
        if pas == COL:
            self.pw = P.fused_packed_width(f, True)
            self.ld_y, self.yoff = self.pw + 4, 0
            self.packed = P.fused_pack(y, self.dz, self.lse_in, self.delta)
            ymat = padded(self.packed, self.ld_y, 0)
        else:
            self.ld_y, self.yoff = ld(f), off
            ymat = padded(y, self.ld_y, off)
        assert (self.ld_x % 2 == 1) == odd
        self.col0 = 3 if odd else 2
        self.ld_out = self.col0 + f + (4 if (self.col0 + f) % 2 == 0 else 3) + (1 if odd else 0)
        self.out0 = rng.uniform(-1, 1, (m + 1, self.ld_out))
        self.out20 = rng.uniform(-1, 1, (m + 1, self.ld_out))
        self.state0 = rng.uniform(1, 2, (4, m + 1))  # row_max, row_sum, lse, (unused)
        self.acc0 = rng.uniform(-1, 1, (m + 1, fp + 2))  # the forward pass's running accumulator (scratch of the pass)
        host = dict(rowptr=self.rowptr, colidx=np.concatenate([self.colidx, [0]]).astype(np.int32), x=padded(x, self.ld_x, off),
                    a=padded(a[None, :], f + 4, off), y=ymat, dz=padded(self.dz, self.ld_dz, off) if pas == ROW else np.zeros(1),
                    lse_in=self.lse_in if pas == ROW else np.zeros(1), delta=self.delta if pas == ROW else np.zeros(1), out=self.out0,
                    out2=self.out20, state=self.state0, acc=self.acc0)
        self.d = {k: ctx.upload(v) for k, v in host.items()}
        self.split = None

    def args(self):
        d, m, f, off = self.d, self.m, self.f, self.off
        a = K.AttnV2()
        a.X, a.ld_x, a.a, a.f, a.leaky_alpha = d["x"].ptr + 8 * off, self.ld_x, d["a"].ptr + 8 * off, f, ALPHA
        a.Y, a.ld_y = d["y"].ptr + 8 * self.yoff, self.ld_y
        if self.pas == FWD:
            a.Out, a.ld_out = d["acc"].ptr, self.fp + 2
            a.row_max, a.row_sum, a.lse = d["state"].ptr, d["state"].ptr + 8 * (m + 1), d["state"].ptr + 16 * (m + 1)
            a.relu_dst, a.relu_ld = d["out"].ptr + 8 * self.col0, self.ld_out
        else:
            a.Out, a.ld_out = d["out"].ptr + 8 * self.col0, self.ld_out
        if self.pas == ROW:
            a.dZ, a.ld_dz, a.lse, a.delta = d["dz"].ptr + 8 * off, self.ld_dz, d["lse_in"].ptr, d["delta"].ptr
        if self.pas == COL:
            a.Out2, a.ld_out2 = d["out2"].ptr + 8 * self.col0, self.ld_out
        return a

    def block(self):
        return K.CsrBlock(self.m, int(self.rowptr[-1]), self.ncols, int(np.diff(self.rowptr).max()), 0, self.d["rowptr"].ptr, self.d["colidx"].ptr, None)

    def fn(self):
        lib = self.ctx.lib
        return (lib.hnh_attn_v2_fwd_csr_p, lib.hnh_attn_v2_row_csr_p, lib.hnh_attn_v2_col_csr_p)[self.pas]

    def reset(self):
        for k, v in (("out", self.out0), ("out2", self.out20), ("state", self.state0), ("acc", self.acc0)):
            self.d[k].set(v)

    def collect(self):
        m, f, c0 = self.m, self.f, self.col0
        out, out2, state = self.d["out"].get(), self.d["out2"].get(), self.d["state"].get()
        for got, first in ((out, self.out0), (out2, self.out20)):
            assert np.array_equal(got[:, :c0], first[:, :c0]) and np.array_equal(got[:, c0 + f:], first[:, c0 + f:]), "guard columns are not written"
            assert np.array_equal(got[m], first[m]), "the row past the last one is not written"
        res = dict(out=out[:m, c0:c0 + f])
        if self.pas == COL:
            res["out2"] = out2[:m, c0:c0 + f]
        else:
            assert np.array_equal(out2, self.out20)
        if self.pas == FWD:
            assert np.array_equal(state[:, m], self.state0[:, m]) and np.array_equal(state[3], self.state0[3])
            res["lse"], res["state"] = state[2, :m], state[:2, :m]
        else:
            assert np.array_equal(state, self.state0)
        return res

    def run(self, overwrite=True, groups=None, act="relu"):
        """dict(out, [out2], [lse, state]) as far as the pass writes them; checks the guards."""
        ctx, lib, m = self.ctx, self.ctx.lib, self.m
        self.reset()
        a, blk = self.args(), self.block()
        first = K.FUSED_OUT_OVERWRITE if (overwrite or self.pas == FWD) else 0
        finish = (K.ATTN_FINISH | ACT_FLAG[act]) if self.pas == FWD else 0
        if groups is None:
            ctx.check(self.fn()(ctx.h, C.byref(blk), C.byref(a), first | finish, None, K.STREAM_COMPUTE), "gatv2 pass")
        else:
            if self.split is None:
                bounds = (C.c_int32 * (NWIN - 1))(*[int(self.ncols * (b + 1) / NWIN) for b in range(NWIN - 1)])
                self.split = K.DevArray(ctx, (NWIN - 1) * m, np.int32)
                ctx.check(lib.hnh_csr_window_bounds(ctx.h, m, self.d["rowptr"].ptr, self.d["colidx"].ptr, NWIN - 1, bounds, self.split.ptr,
                                                    K.STREAM_COMPUTE), "window bounds")
            sp = self.split.ptr
            for k, (w0, w1) in enumerate(groups):
                win = K.CsrWindow(None if w0 == 0 else sp + (w0 - 1) * m * 4, None if w1 == NWIN else sp + (w1 - 1) * m * 4, int(w1 == NWIN))
                fl = (first if k == 0 else 0) | (finish if w1 == NWIN else 0)
                ctx.check(self.fn()(ctx.h, C.byref(blk), C.byref(a), fl, C.byref(win), K.STREAM_COMPUTE), "gatv2 window")
        ctx.sync()
        return self.collect()

    def want(self, overwrite=True, act="relu"):
        f, m, cols, c0 = self.f, self.m, self.colidx.astype(np.int64), self.col0
        if self.pas == FWD:
            o, lse = V.fwd_pass_ld(self.rows, cols, m, self.x, self.y, self.a, f, ALPHA)
            return dict(out=R.act_ld(o, act), lse=lse)
        base = None if overwrite else self.out0[:m, c0:c0 + f]
        if self.pas == ROW:
            return dict(out=V.row_pass(self.rows, cols, m, self.x, self.dz, self.lse_in, self.delta, self.y, self.a, f, ALPHA, out=base))
        cm, dagg = V.col_pass(self.rows, cols, m, self.x, self.a, self.packed, f, ALPHA, out=base, out2=None if overwrite else self.out20[:m, c0:c0 + f])
        return dict(out=cm, out2=dagg)

    def free(self):
        for v in self.d.values():
            v.free()
        if self.split is not None:
            self.split.free()


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd-offset"])
@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_pass_vs_numpy(ctx, pas, f, odd):
    """Against numpy (extended precision for the forward pass), guards untouched, rows without nonzeros zero, a repeat bit-identical,
    accumulate on top of overwrite for the backward passes."""
    p = V2Problem(ctx, pas, f, odd=odd)
    deg = np.diff(p.rowptr)
    assert deg.max() >= 1500 and np.count_nonzero(deg == 0) > 20 and np.count_nonzero((deg >= 200) & (deg <= 300)) >= 3 and 600 in deg
    act = "relu" if pas != FWD else ("relu", "elu", "identity")[f % 3]
    got, want = p.run(True, act=act), p.want(True, act=act)
    empty = deg == 0
    for k in got:
        if k != "state":
            assert np.all(got[k][empty] == 0.0), "rows without nonzeros: o = 0, lse = 0, sums = 0"
    assert all(np.abs(np.float64(v)).max() > 0 for v in want.values())
    errs = errors(got, want)
    assert same(p.run(True, act=act), got), "a repeat must be bit-identical"
    if pas != FWD:
        acc = p.run(False)
        errs.update({"acc " + k: v for k, v in errors(acc, p.want(False)).items()})
        assert np.array_equal(acc["out"][empty], p.out0[:p.m, p.col0:p.col0 + f][empty]), "accumulating leaves rows without nonzeros alone"
    p.free()
    T.record_observed("gat_v2_kernel", case="%s f=%d%s" % (PASS_NAMES[pas], f, " odd" if odd else ""), worst=max(errs.values()))
    print("observed", PASS_NAMES[pas], f, odd, errs)
    assert max(errs.values()) <= (FTOL if pas == FWD else TOL), errs


@pytest.mark.parametrize("f", [7, 64, 256])
@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_scores_far_outside_exps_range(ctx, pas, f):
    p = V2Problem(ctx, pas, f, seed=2, big=800.0)
    assert np.abs(p.z).max() > 790.0 and p.a.min() < 0 < p.a.max()
    got, want = p.run(True), p.want(True)
    for k, v in got.items():  # (the running max of a row without nonzeros is -inf by definition: the empty state)
        assert np.all(np.isfinite(v)) or (k == "state" and np.all(np.isfinite(v[1])) and np.all(np.isneginf(v[0][~np.isfinite(v[0])]))), k
    errs = errors(got, want)
    p.free()
    T.record_observed("gat_v2_kernel", case="%s f=%d |z|=800" % (PASS_NAMES[pas], f), worst=max(errs.values()))
    print("observed big", PASS_NAMES[pas], f, errs)
    assert max(errs.values()) <= (FTOL if pas == FWD else TOL), errs


@pytest.mark.parametrize("pas,f", [(FWD, 7), (FWD, 128), (FWD, 256), (ROW, 33), (ROW, 64), (ROW, 128), (ROW, 256), (COL, 33), (COL, 64), (COL, 128),
                                   (COL, 256)], ids=lambda v: str(v))
def test_grouping_independence(ctx, pas, f):
    """Whole rows, one call per window and two uneven groupings of six windows: the same bits (forward output with elu, lse and the row
    state; R; C and dAgg), overwriting and accumulating, because every launch continues the row's state nonzero by nonzero."""
    p = V2Problem(ctx, pas, f, seed=3)
    for overwrite in ((True,) if pas == FWD else (True, False)):
        whole = p.run(overwrite, act="elu")
        for name, groups in GROUPINGS.items():
            assert same(p.run(overwrite, groups, act="elu"), whole), (name, overwrite)
    p.free()


@pytest.mark.parametrize("pas,f", [(FWD, 7), (FWD, 128), (FWD, 256), (ROW, 33), (ROW, 64), (ROW, 128), (ROW, 256), (COL, 33), (COL, 64), (COL, 128),
                                   (COL, 256)], ids=lambda v: str(v))
def test_forced_panels_are_bit_identical(monkeypatch, pas, f):
    """Column panels (several launches over every row, hub rows after the last): the same bits as one launch."""
    ncols = 1536
    c1 = K.Ctx(0)
    p1 = V2Problem(c1, pas, f, ncols=ncols, seed=5)
    one, want = p1.run(True, act="elu"), p1.want(True, act="elu")
    p1.free()
    c1.close()
    gather_w = P.fused_packed_width(f, True) if pas == COL else f
    monkeypatch.setenv("HNH_PANEL_BYTES", str(ncols * gather_w * 8 / 5))
    monkeypatch.setenv("HNH_MAX_PANELS", "8")
    monkeypatch.setenv("HNH_PANELS_WITH_HUBS", "1")
    c5 = K.Ctx(0)
    p5 = V2Problem(c5, pas, f, ncols=ncols, seed=5)
    # (the query answers for widths up to 512 only, and the packed operand of f = 256 is 514 wide: asked at 512, where the same bytes round to 5 too)
    assert c5.lib.hnh_panel_count(c5.h, p5.m, int(p5.rowptr[-1]), ncols, min(gather_w, 512), int(np.diff(p5.rowptr).max())) == 5
    five = p5.run(True, act="elu")
    p5.free()
    c5.close()
    assert same(one, five)
    assert max(errors(five, want).values()) <= (FTOL if pas == FWD else TOL)


@pytest.mark.parametrize("rows", [1, 301, 5000])
def test_finish_vs_numpy_and_run_to_run(ctx, rows):
    """dA = dAgg + (R + C) o a into a guarded column block, da = colsum(A o (R + C)) at a pitch of 2; twice the same bits."""
    lib = ctx.lib
    rng = np.random.default_rng(rows)
    for f in WIDTHS:
        ld_g, ld_r, ld_c, ld_a, ld_da, col0 = f + 1, f + 2, f + 3, f + 4, 2 * f + 7, 3
        dagg, rm, cm, am = (rng.uniform(-1, 1, (rows, ld)) for ld in (ld_g, ld_r, ld_c, ld_a))
        a = rng.standard_normal(f)
        dev = {k: ctx.upload(v) for k, v in dict(dagg=dagg, rm=rm, cm=cm, am=am, a=a, da=np.full((rows + 1, ld_da), 7.0), dav=np.full((f + 1, 2), 7.0),
                                                 work=np.full(K.attn_v2_finish_work(f) + 1, 7.0)).items()}

        def launch(work_doubles=K.attn_v2_finish_work(f)):
            return lib.hnh_attn_v2_finish_f64(ctx.h, dev["da"].ptr, ld_da, col0, dev["dagg"].ptr, ld_g, dev["rm"].ptr, ld_r, dev["cm"].ptr, ld_c, dev["am"].ptr,
                                              ld_a, dev["a"].ptr, dev["dav"].ptr, 2, rows, f, dev["work"].ptr, work_doubles, K.STREAM_COMPUTE)

        ctx.check(launch(), "finish")
        gda, gdav = dev["da"].get(), dev["dav"].get()
        ctx.check(launch(), "finish")
        assert np.array_equal(dev["da"].get(), gda) and np.array_equal(dev["dav"].get(), gdav), "a repeat must be bit-identical"
        wda, wdav = V.finish(dagg[:, :f], rm[:, :f], cm[:, :f], am[:, :f], a)
        errs = dict(dA=float(T.rel(gda[:rows, col0:col0 + f], wda)), da=float(T.rel(gdav[:f, 0], wdav)))
        assert np.all(gda[:rows, :col0] == 7.0) and np.all(gda[:rows, col0 + f:] == 7.0) and np.all(gda[rows] == 7.0)
        assert np.all(gdav[:, 1] == 7.0) and gdav[f, 0] == 7.0 and dev["work"].get()[-1] == 7.0
        assert launch(K.attn_v2_finish_work(f) - 1) == 1, "a short workspace is refused"
        for d in dev.values():
            d.free()
        T.record_observed("gat_v2_kernel", case="finish f=%d rows=%d" % (f, rows), worst=max(errs.values()))
        assert max(errs.values()) <= TOL, (f, errs)
    a = ctx.upload(np.zeros(4))
    assert lib.hnh_attn_v2_finish_f64(ctx.h, a.ptr, 600, 0, a.ptr, 300, a.ptr, 300, a.ptr, 300, a.ptr, 300, a.ptr, a.ptr, 2, 1, 257, a.ptr, 1 << 20,
                                      K.STREAM_COMPUTE) == K.ERR_UNSUPPORTED
    a.free()


@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_wide_heads_and_bad_arguments_are_refused_and_write_nothing(ctx, pas):
    p = V2Problem(ctx, pas, 33)
    a, blk = p.args(), p.block()
    a.f = 257
    assert p.fn()(ctx.h, C.byref(blk), C.byref(a), K.FUSED_OUT_OVERWRITE, None, K.STREAM_COMPUTE) == K.ERR_UNSUPPORTED
    assert b"256" in ctx.lib.hnh_last_error(ctx.h)
    a.f = 33
    assert p.fn()(ctx.h, C.byref(blk), C.byref(a), 4, None, K.STREAM_COMPUTE) == 1  # an unknown flag
    a.a = None
    assert p.fn()(ctx.h, C.byref(blk), C.byref(a), K.FUSED_OUT_OVERWRITE, None, K.STREAM_COMPUTE) == 1  # no vector
    a = p.args()
    a.ld_y = 32
    assert p.fn()(ctx.h, C.byref(blk), C.byref(a), K.FUSED_OUT_OVERWRITE, None, K.STREAM_COMPUTE) == 1  # a gathered operand narrower than it must be
    ctx.sync()
    for k, first in (("out", p.out0), ("out2", p.out20), ("state", p.state0)):
        assert np.array_equal(p.d[k].get(), first)
    p.free()


@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_empty_block(ctx, pas):
    """rowptr == NULL: overwrite (and the forward finish) leave zeros in the pass's outputs, accumulate leaves everything alone."""
    f = 33
    p = V2Problem(ctx, pas, f)
    a = p.args()
    none = K.CsrBlock(p.m, 0, -1, 0, 0, None, None, None)
    ctx.check(p.fn()(ctx.h, C.byref(none), C.byref(a), 0, None, K.STREAM_COMPUTE), "empty block, accumulate")
    ctx.sync()
    assert np.array_equal(p.d["out"].get(), p.out0) and np.array_equal(p.d["out2"].get(), p.out20) and np.array_equal(p.d["state"].get(), p.state0)
    fl = K.FUSED_OUT_OVERWRITE | (K.ATTN_FINISH if pas == FWD else 0)
    ctx.check(p.fn()(ctx.h, C.byref(none), C.byref(a), fl, None, K.STREAM_COMPUTE), "empty block, overwrite")
    ctx.sync()
    got = p.collect()
    assert np.all(got["out"] == 0.0) and (pas != COL or np.all(got["out2"] == 0.0))
    if pas == FWD:
        assert np.all(got["lse"] == 0.0) and np.all(got["state"][1] == 0.0) and np.all(np.isneginf(got["state"][0]))
    p.free()


# ------------------------------------------------------------------------------------------------ the operator
def vectors(layers, seed=78):
    """{(layer, head): (a, zeros)}: what set_attention_vectors takes; the reference reads the first of the pair"""
    return {k: (a, np.zeros_like(a)) for k, a in V.vectors_of(layers, seed=seed).items()}


def run_v2(world, rows, cols, m, x, layers, weights, av, g_glob, rounds=1, **kw):
    return G.run_rounds(world, rows, cols, m, x, layers, weights, av, g_glob, rounds, attention="softmax", score="gatv2", **kw)


def reference(rows, cols, m, x, layers, w, av, g, **mode):
    dw, da, dx = V.backward(rows, cols, m, x, layers, ALPHA, g, w, av, **mode)
    return dict(out=V.forward(rows, cols, m, x, layers, ALPHA, w, av, **mode), dw=dw, da=da, dx=dx)


def check_against(got, want, label, ranks):
    """output, every dW, every da and dX against the reference (da2 is zeros); the worst is recorded and asserted <= TOL"""
    errs = {name: T.rel(got[name], want[name]) for name in ("out", "dx")}
    for key in want["dw"]:
        assert np.abs(want["dw"][key]).max() > 0 and np.abs(V.vec(want["da"][key])).max() > 0
        errs[("dw",) + key] = T.rel(got["dw"][key], want["dw"][key])
        errs[("da",) + key] = T.rel(got["da"][key][0], V.vec(want["da"][key]))
        assert np.all(got["da"][key][1] == 0.0), "the second vector has no gradient"
    worst = max(errs.values())
    T.record_observed("gat_v2", case=label, ranks=ranks, worst=worst)
    print("observed gat_v2", label, ranks, "worst %.2e" % worst)
    assert worst <= TOL, errs


ER8_RESULTS = {}
CONFIGS = {"relu": dict(), "published": dict(activation=("elu", "identity")), "feature dropout": dict(dropout=(0.0, 0.3), seed=11)}


def ref_mode(kw):
    return dict(activations=kw.get("activation"), rates=kw.get("dropout", (0.0, 0.0)), seed=kw.get("seed", 0))


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_gatv2_er8(p, config):
    rows, cols, m, x = er8()
    layers, kw = T.GAT_LAYERS, CONFIGS[config]
    w, av = hashed_weights(layers), vectors(layers)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 9) * 16.0
    per_rank = H.run_spmd(p, lambda wd: run_v2(wd, rows, cols, m, x, layers, w, av, g, rounds=2, **kw))
    got = assembled(per_rank, 0, m, layers)
    check_against(got, reference(rows, cols, m, x, layers, w, av, g, **ref_mode(kw)), "er8_r16 %s p%d" % (config, p), p)
    again = assembled(per_rank, 1, m, layers)
    assert np.array_equal(got["out"], again["out"]) and np.array_equal(got["dx"], again["dx"]), "two rounds must be bit-identical"
    assert all(np.array_equal(got["dw"][k], again["dw"][k]) and np.array_equal(got["da"][k][0], again["da"][k][0]) for k in w)
    ER8_RESULTS[(p, config)] = got


def test_one_rank_and_eight_ranks_agree():
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w, av = hashed_weights(layers), vectors(layers)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 9) * 16.0
    res = {}
    for p in (1, 8):
        res[p] = ER8_RESULTS.get((p, "relu")) or assembled(H.run_spmd(p, lambda wd: run_v2(wd, rows, cols, m, x, layers, w, av, g)), 0, m, layers)
    want = dict(res[1], da={k: v[0] for k, v in res[1]["da"].items()})
    check_against(res[8], want, "er8_r16 p8 against p1", 8)


WIDE = {"benchmark widths": (1 << 12, [(256, 256, 1), (256, 128, 2), (256, 64, 3)]), "odd heads": (1 << 11, [(24, 33, 2), (66, 7, 3)])}


@pytest.mark.parametrize("p", [1, 4])
@pytest.mark.parametrize("shape", sorted(WIDE))
def test_gatv2_widths(shape, p):
    m, layers = WIDE[shape]
    rows, cols = H.generate_er(m, m, m * 16, 77)
    x = O.dense_fill(m, layers[0][0], 41) * 16.0
    w, av = hashed_weights(layers), vectors(layers, seed=5)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 3) * 64.0
    kw = dict(activation=("elu",) * (len(layers) - 1) + ("identity",))
    per_rank = H.run_spmd(p, lambda wd: run_v2(wd, rows, cols, m, x, layers, w, av, g, **kw))
    check_against(assembled(per_rank, 0, m, layers), reference(rows, cols, m, x, layers, w, av, g, **ref_mode(kw)), "%s p%d" % (shape, p), p)


@pytest.mark.parametrize("p", [1, 4])
def test_gatv2_rmat_hub_rows(p):
    m, layers = 1 << 13, [(64, 64, 2), (128, 32, 2)]
    rows, cols = H.generate_rmat(13, m * 16)
    assert np.bincount(rows, minlength=m).max() >= 512 and np.bincount(cols, minlength=m).max() >= 512
    x = O.dense_fill(m, 64, 8) * 8.0
    w, av = hashed_weights(layers), vectors(layers, seed=6)
    g = O.dense_fill(m, 64, 4) * 32.0
    per_rank = H.run_spmd(p, lambda wd: run_v2(wd, rows, cols, m, x, layers, w, av, g, rounds=2))
    got = assembled(per_rank, 0, m, layers)
    check_against(got, reference(rows, cols, m, x, layers, w, av, g), "rmat hubs p%d" % p, p)
    again = assembled(per_rank, 1, m, layers)
    assert np.array_equal(got["dx"], again["dx"]) and all(np.array_equal(got["da"][k][0], again["da"][k][0]) for k in w), "a repeat must be bit-identical"


@pytest.mark.parametrize("score", ["dot", "additive"])
@pytest.mark.parametrize("p", [1, 4])
def test_other_scores_are_untouched_by_a_gatv2_round(p, score):
    """score -> gatv2 -> score on one object: the results are bit-identical before and after, and equal those of a GAT that never selected
    gatv2."""
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w, av = hashed_weights(layers), R.vectors_of(layers)
    g = O.dense_fill(m, 12, 9) * 16.0
    additive = score == "additive"
    kw = dict(attention="softmax", backward="fused", score=score)

    def trip(world):
        s = setup(world, rows, cols, m, x, layers, w, av, g, **kw)
        before = one_round(s, w, additive)
        s["gnn"].set_score("gatv2")
        with pytest.raises(H.HnhError, match="forwardPass"):
            s["gnn"].backwardPass(s["g"])  # a change of score invalidates the stored forward pass
        mid = one_round(s, w, True)
        s["gnn"].set_score(score)
        after = one_round(s, w, additive)
        teardown(s)
        return before, mid, after

    def plain(world):
        s = setup(world, rows, cols, m, x, layers, w, av, g, **kw)
        r = one_round(s, w, additive)
        teardown(s)
        return r

    for (before, mid, after), old in zip(H.run_spmd(p, trip), H.run_spmd(p, plain)):
        for a in (after, old):
            assert np.array_equal(before["out"], a["out"]) and np.array_equal(before["dx"], a["dx"])
            assert all(np.array_equal(before["dw"][k], a["dw"][k]) for k in w)
            assert not additive or all(np.array_equal(before["da"][k][i], a["da"][k][i]) for k in w for i in (0, 1))
        assert not np.array_equal(mid["out"], before["out"]), "the gatv2 round computed something else"


def test_refusals_on_the_device():
    rows, cols, m, _ = er8()

    def rank(world):
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, "15d_fusion2", sp, 16, 1)
        for layers, kw, words in (([(16, 8, 2)], dict(attention="none"), "score gatv2.*attention mode softmax only"),
                                  ([(16, 257, 1)], dict(attention="softmax"), "score gatv2.*at most 256 features, not 257"),
                                  ([(16, 8, 2)], dict(attention="softmax", dropout=(0.5, 0.0)), "attention dropout.*gatv2")):
            gnn = H.GAT(d, layers, ALPHA, score="gatv2", **kw)
            g = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
            with pytest.raises(H.HnhError, match=words):
                gnn.forwardPass()
            with pytest.raises(H.HnhError, match=words):
                gnn.backwardPass(g)
            world.sync()  # nothing was left in flight
            g.free()
            gnn.free()
        for h in (d, sp):
            h.free()
        return True

    assert all(H.run_spmd(2, rank))


# ------------------------------------------------------------------------------------------------ training
PUBLISHED = ("elu", "identity")
ADAM = dict(kind="adam", lr=0.01, weight_decay=5e-4)


def device_train(world, pp, layers, av, steps):
    s = setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["w"], av, None, attention="softmax", score="gatv2", activation=PUBLISHED)
    gnn = s["gnn"]
    gnn.set_labels(pp["labels"], pp["mask"], heads="mean")
    opt = dict(ADAM)
    gnn.set_optimizer(opt.pop("kind"), opt.pop("lr"), **opt)
    res = dict(losses=[], accs=[])
    for _ in range(steps):
        loss, acc = gnn.train_step()
        res["losses"].append(loss)
        res["accs"].append(acc)
    res["w"] = {k: gnn.get_weight(*k) for k in pp["w"]}
    res["av"] = {k: gnn.get_attention_vectors(*k) for k in pp["w"]}
    teardown(s)
    return res


@pytest.mark.parametrize("p", [1, 4])
def test_adam_trajectory_of_the_published_layers(p):
    """Ten steps of train_step: within 10 x the divergence of a reference run whose gradients are perturbed at 1e-10, the loss falls, the
    parameters are bit-equal across ranks, a2 is never touched."""
    layers, steps = T.GAT_LAYERS, 10
    pp = R.planted_partition(layers)
    av = {k: (v[0], np.zeros_like(v[0])) for k, v in pp["av"].items()}
    args = (pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, pp["labels"], pp["mask"], "mean", pp["w"], av)
    ref = V.train(*args, ADAM, steps, activations=PUBLISHED)
    per = V.train(*args, ADAM, steps, activations=PUBLISHED, perturb=(1e-10, np.random.default_rng(7)))
    bound_p = 10.0 * V.parameter_divergence(per[2], per[3], ref[2], ref[3])
    bound_l = 10.0 * float(np.max(np.abs(np.array(per[0]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    assert bound_p > 0 and bound_l > 0
    per_rank = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, av, steps))
    r0 = per_rank[0]
    for pr in per_rank:
        assert pr["losses"] == r0["losses"] and pr["accs"] == r0["accs"]
        for k in r0["w"]:
            assert np.array_equal(pr["w"][k], r0["w"][k]) and np.array_equal(pr["av"][k][0], r0["av"][k][0]), "parameters are bit-equal across ranks"
            assert np.all(pr["av"][k][1] == 0.0), "a2 is kept and not trained"
    got_p = V.parameter_divergence(r0["w"], r0["av"], ref[2], ref[3])
    got_l = float(np.max(np.abs(np.array(r0["losses"]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    T.record_observed("gat_v2_trajectory", ranks=p, parameters=got_p, parameters_bound=bound_p, loss=got_l, loss_bound=bound_l, first=r0["losses"][0],
                      last=r0["losses"][-1])
    print("observed gat_v2 trajectory", p, "parameters %.2e (bound %.2e) loss %.2e (bound %.2e)" % (got_p, bound_p, got_l, bound_l), r0["losses"])
    assert got_p <= bound_p and got_l <= bound_l
    assert r0["accs"] == ref[1]
    assert r0["losses"][-1] < r0["losses"][0], "the planted-partition loss falls"
    assert all(np.abs(r0["av"][k][0] - av[k][0]).max() > 0 for k in av), "every a has moved"
