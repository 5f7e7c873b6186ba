"""The GAT's score "transformer" on the GPU (include/hnh_attn_qkv.h, GAT score "transformer").

Kernel level, through ctypes: the forward pass against the extended-precision numpy reference (tests/gat_qkv_ref.py, fwd_pass_ld), the
backward row and column passes against numpy, at widths 1, 7, 8, 33, 64, 100, 128, 200, 255, 256 on mixed_degrees(1024, ..) blocks (empty
rows, a repeated pair, rows of 200 - 300, hub rows of 600 and 1500; a square block for the forward and the row pass, a rectangular one
standing for S^T for the column pass), with pitches wider than the widths, every operand but the packed one at an odd column offset (the
8-byte lanes) or an even one, 1e300 beyond every operand's width, guard zones round every output (both outputs of the column pass, the
score vector of the forward pass); the forward finish with HNH_ATTN_ADDEND at every width and both alignments under relu, elu and the
identity; Q scaled until |s| passes 800; the forced rescales of tests/softmax_schedules.py with scale = 1 (the
rise positions are the designed ones, the jump rows rise by more than 745); the passes' independence of how a row's nonzeros are split into
launches (whole rows, one call per window, two uneven groupings of six windows, forced Infinity-Cache panels), bit for bit; run-to-run bit
identity; the width limit, misaligned packed operands, a finish without the last window, both activation bits; empty blocks.
Operator level: GAT(..., attention="softmax", score="transformer") on 15d_fusion2, c = 1 over 1, 2, 4, 8 loopback ranks against the numpy
definition — output, every dW_v, dW_q, dW_k, db, dW_res and dX — at the small shape in four configurations, at heads of 256, 128, 64, 33 and 7
on 2^12 vertices, and on an R-MAT graph with hub rows; p = 8 against p = 1; the tied-weights identity against the product's own dot-product
softmax with the fused backward at alpha = 1; scores dot, additive and gatv2 bit-identical before and after a transformer round on the same
object; a ten-step Adam trajectory of the published layers through train_step, parameters bit-equal across ranks; refusals on the device.

Bounds: FTOL = 1e-12 for the forward kernel against np.longdouble, TOL = 1e-10 for the backward kernels and the operator (the bounds of
tests/gat_gpu_harness.py); the trajectory within 10 x the divergence of a reference run whose gradients are perturbed at 1e-10 (the rule of
test_gat_train_gpu.py).  The observed worst cases are recorded with T.record_observed.

Observed on an MI355X (max |x - ref| / max |ref| per matrix): forward kernel <= 4.9e-16 over every width and both alignments (<= 4.5e-16 with the addend), <= 3.8e-14 at
|s| = 800, <= 8.1e-16 on the forced rescales; backward row pass <= 5.3e-15, column pass <= 7.4e-15, <= 2.1e-13 at |s| = 800; the operator (worst
of the output, every dW_v, dW_q, dW_k, db, dW_res and dX) <= 1.7e-15 on er8_r16 over p = 1 .. 8 in the four configurations, <= 2.1e-15 at the
exact widths and at odd heads, <= 1.7e-15 on the R-MAT graph; the tied-weights identity <= 1.8e-15; the Adam trajectory 5.9e-16 in the
parameters (bound 4.8e-9), 2.3e-16 in the loss (bound 4.5e-12), loss 1.438 -> 0.752 in ten steps."""
import ctypes as C

import numpy as np
import pytest

import gat_gpu_harness as G
import gat_pass_ref as P
import gat_qkv_ref as Q
import gat_ref as R
import hnh_testlib as T
import softmax_schedules as SS
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import (ALPHA, COL, FTOL, FWD, GROUPINGS, NWIN, PASS_NAMES, ROW, TOL, ctx, er8, errors, hashed_weights, hip_backend, same,  # noqa: F401
                             setup, teardown)
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


class QKVProblem:
    """One pass's operands on the device.  odd=True puts every operand but the packed one (whose layout asks for 16 bytes) at an odd column
    offset of an odd pitch: the 8-byte instances; otherwise offsets and pitches are even and an even f takes the 16-byte lanes.  big > 0
    scales the own rows so that |s| reaches about `big`.  given = (rowptr, colidx, rows, own rows, gathered first half, scale): a designed
    block (the forced rescales)."""

    def __init__(self, ctx, pas, f, m=1024, ncols=None, seed=0, odd=False, big=0.0, given=None):
        self.ctx, self.pas, self.f, self.odd = ctx, pas, f, odd
        rng = np.random.default_rng(1000 * f + seed + 17 * pas)
        if given is not None:
            self.rowptr, self.colidx, self.rows, x, y1, self.scale = given
            m = len(self.rowptr) - 1
            ncols = y1.shape[0]
        else:
            ncols = ncols or (768 if pas == COL else m)
            self.rowptr, self.colidx, self.rows = G.graph(m, ncols, G.mixed_degrees(m, seed + f), seed + 1)
            x, y1 = rng.uniform(-1, 1, (m, f)), rng.uniform(-1, 1, (ncols, f))
            self.scale = Q.scale_of(f)
        self.m, self.ncols = m, ncols
        fp = self.fp = f + (f & 1)
        rows, cols = self.rows, self.colidx.astype(np.int64)
        if big:
            x = x * (big / np.abs(self.scale * np.einsum("ij,ij->i", x[rows], y1[cols])).max())
        self.x, self.y1 = x, y1  # own rows: Q (fwd, row) or K (col); the gathered first half: K (fwd, row) or Q (col)
        self.s = self.scale * np.einsum("ij,ij->i", x[rows], y1[cols])
        owner, n_own = (cols, ncols) if pas == COL else (rows, m)  # the S rows: the gathered rows of the column pass
        _, self.lse_in = R.row_softmax(owner, n_own, self.s)
        self.delta = rng.uniform(-1, 1, n_own)
        self.dz = rng.uniform(-1, 1, (n_own, f))
        self.x2 = rng.uniform(-1, 1, (m, f))      # column pass: the own rows of V
        self.v = rng.uniform(-1, 1, (ncols, f))   # forward, row pass: the gathered V
        off = self.off = 1 if odd else 2
        ld = lambda w: w + off + (3 if (w + off) % 2 == (0 if odd else 1) else 2)  # odd: an odd pitch; else an even one  # noqa: E731
        self.ld_x, self.ld_x2, self.ld_dz = ld(f), ld(f) + 2, ld(f)
        assert (self.ld_x % 2 == 1) == odd
        self.pw = P.fused_packed_width(f, pas == COL)
        self.ld_y = self.pw + 4
        self.packed = P.fused_pack(y1, self.dz, self.lse_in, self.delta) if pas == COL else P.fused_pack(y1, self.v)
        assert fp == f or np.all(self.packed[:, f] == 0.0), "the pad column is zero"
        self.col0 = 3 if odd else 2
        self.ld_out = self.col0 + f + (4 if (self.col0 + f) % 2 == 0 else 3) + (1 if odd else 0)
        self.out0 = rng.uniform(-1, 1, (m + 1, self.ld_out))
        self.out20 = rng.uniform(-1, 1, (m + 1, self.ld_out))
        self.state0 = rng.uniform(1, 2, (4, m + 1))  # row_max, row_sum, lse, (unused)
        self.acc0 = rng.uniform(-1, 1, (m + 1, fp + 2))  # the forward pass's running accumulator (scratch of the pass)
        self.nnz = int(self.rowptr[-1])
        self.vals0 = rng.uniform(3, 4, self.nnz + 2)  # the forward pass's score vector with a sentinel at either end
        host = dict(rowptr=self.rowptr, colidx=np.concatenate([self.colidx, [0]]).astype(np.int32), x=padded(x, self.ld_x, off),
                    x2=padded(self.x2, self.ld_x2, off) if pas == COL else np.zeros(1), y=padded(self.packed[:, :self.pw], self.ld_y, 0),
                    dz=padded(self.dz, self.ld_dz, off) if pas == ROW else np.zeros(1), lse_in=self.lse_in if pas == ROW else np.zeros(1),
                    delta=self.delta if pas == ROW else np.zeros(1), out=self.out0, out2=self.out20, state=self.state0, acc=self.acc0,
                    vals=self.vals0)
        self.d = {k: ctx.upload(v) for k, v in host.items()}
        self.split = None

    def args(self):
        d, m, f, off = self.d, self.m, self.f, self.off
        a = K.AttnQKV()
        a.X, a.ld_x, a.f, a.scale = d["x"].ptr + 8 * off, self.ld_x, f, self.scale
        a.Y, a.ld_y = d["y"].ptr, self.ld_y
        if self.pas == FWD:
            a.Out, a.ld_out = d["acc"].ptr, self.fp + 2
            a.row_max, a.row_sum, a.lse = d["state"].ptr, d["state"].ptr + 8 * (m + 1), d["state"].ptr + 16 * (m + 1)
            a.relu_dst, a.relu_ld = d["out"].ptr + 8 * self.col0, self.ld_out
            a.values = d["vals"].ptr + 8
        else:
            a.Out, a.ld_out = d["out"].ptr + 8 * self.col0, self.ld_out
        if self.pas == ROW:
            a.dZ, a.ld_dz, a.lse, a.delta = d["dz"].ptr + 8 * off, self.ld_dz, d["lse_in"].ptr, d["delta"].ptr
        if self.pas == COL:
            a.X2, a.ld_x2 = d["x2"].ptr + 8 * off, self.ld_x2
            a.Out2, a.ld_out2 = d["out2"].ptr + 8 * self.col0, self.ld_out
        return a

    def block(self):
        return K.CsrBlock(self.m, self.nnz, self.ncols, int(np.diff(self.rowptr).max()), 0, self.d["rowptr"].ptr, self.d["colidx"].ptr, None)

    def fn(self):
        lib = self.ctx.lib
        return (lib.hnh_attn_qkv_fwd_csr_p, lib.hnh_attn_qkv_row_csr_p, lib.hnh_attn_qkv_col_csr_p)[self.pas]

    def reset(self):
        for k, v in (("out", self.out0), ("out2", self.out20), ("state", self.state0), ("acc", self.acc0), ("vals", self.vals0)):
            self.d[k].set(v)

    def untouched(self):
        return all(np.array_equal(self.d[k].get(), v) for k, v in (("out", self.out0), ("out2", self.out20), ("state", self.state0), ("vals", self.vals0)))

    def collect(self):
        m, f, c0 = self.m, self.f, self.col0
        out, out2, state, vals = self.d["out"].get(), self.d["out2"].get(), self.d["state"].get(), self.d["vals"].get()
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
            assert vals[0] == self.vals0[0] and vals[-1] == self.vals0[-1], "the sentinels round the score vector are not written"
            res["lse"], res["state"], res["values"] = state[2, :m], state[:2, :m], vals[1:-1]
        else:
            assert np.array_equal(state, self.state0) and np.array_equal(vals, self.vals0)
        return res

    def addend(self):
        """what waits in the forward pass's destination before a launch (reset() writes it back)"""
        return self.out0[:self.m, self.col0:self.col0 + self.f]

    def run(self, overwrite=True, groups=None, act="relu", addend=False):
        """dict(out, [out2], [lse, state, values]) as far as the pass writes them; checks the guards.  addend: the forward finish with
        HNH_ATTN_ADDEND, act(o + what waits in the destination)."""
        ctx, lib, m = self.ctx, self.ctx.lib, self.m
        self.reset()
        a, blk = self.args(), self.block()
        first = K.FUSED_OUT_OVERWRITE if (overwrite or self.pas == FWD) else 0
        finish = (K.ATTN_FINISH | ACT_FLAG[act] | (K.ATTN_ADDEND if addend else 0)) if self.pas == FWD else 0
        if groups is None:
            ctx.check(self.fn()(ctx.h, C.byref(blk), C.byref(a), first | finish, None, K.STREAM_COMPUTE), "qkv pass")
        else:
            sp = self.windows()
            for k, (w0, w1) in enumerate(groups):
                win = K.CsrWindow(None if w0 == 0 else sp + (w0 - 1) * m * 4, None if w1 == NWIN else sp + (w1 - 1) * m * 4, int(w1 == NWIN))
                fl = (first if k == 0 else 0) | (finish if w1 == NWIN else 0)
                ctx.check(self.fn()(ctx.h, C.byref(blk), C.byref(a), fl, C.byref(win), K.STREAM_COMPUTE), "qkv window")
        ctx.sync()
        return self.collect()

    def windows(self):
        ctx, m = self.ctx, self.m
        if self.split is None:
            bounds = (C.c_int32 * (NWIN - 1))(*[int(self.ncols * (b + 1) / NWIN) for b in range(NWIN - 1)])
            self.split = K.DevArray(ctx, (NWIN - 1) * m, np.int32)
            ctx.check(ctx.lib.hnh_csr_window_bounds(ctx.h, m, self.d["rowptr"].ptr, self.d["colidx"].ptr, NWIN - 1, bounds, self.split.ptr,
                                                    K.STREAM_COMPUTE), "window bounds")
        return self.split.ptr

    def want(self, overwrite=True, act="relu", addend=False):
        f, m, cols, c0 = self.f, self.m, self.colidx.astype(np.int64), self.col0
        packed = np.nan_to_num(self.packed)
        if self.pas == FWD:
            o, lse, s = Q.fwd_pass_ld(self.rows, cols, m, self.x, packed, f, self.scale)
            return dict(out=R.act_ld(o + self.addend().astype(np.longdouble) if addend else o, act), lse=lse, values=s)
        base = None if overwrite else self.out0[:m, c0:c0 + f]
        if self.pas == ROW:
            return dict(out=Q.row_pass(self.rows, cols, m, self.x, self.dz, self.lse_in, self.delta, packed, f, self.scale, out=base))
        dk, dv = Q.col_pass(self.rows, cols, m, self.x, self.x2, packed, f, self.scale, out=base, out2=None if overwrite else self.out20[:m, c0:c0 + f])
        return dict(out=dk, out2=dv)

    def free(self):
        for v in self.d.values():
            v.free()
        if self.split is not None:
            self.split.free()


def bound_of(pas, key):
    """FTOL for what the forward pass writes, but 1e-13 for its scores (one dot product: "same maths, other summation order"); TOL behind"""
    return (1e-13 if key == "values" else FTOL) if pas == FWD else TOL


def assert_within(pas, errs):
    assert all(v <= bound_of(pas, k.replace("acc ", "")) for k, v in errs.items()), errs


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd-offset"])
@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_pass_vs_numpy(ctx, pas, f, odd):
    """Against numpy (extended precision for the forward pass), guards untouched, rows without nonzeros zero, a repeat bit-identical,
    accumulate on top of overwrite for the backward passes."""
    p = QKVProblem(ctx, pas, f, odd=odd)
    deg = np.diff(p.rowptr)
    assert deg.max() >= 1500 and np.count_nonzero(deg == 0) > 20 and np.count_nonzero((deg >= 200) & (deg <= 300)) >= 3 and 600 in deg
    act = "relu" if pas != FWD else ("relu", "elu", "identity")[f % 3]
    got, want = p.run(True, act=act), p.want(True, act=act)
    empty = deg == 0
    for k in got:
        if k not in ("state", "values"):
            assert np.all(got[k][empty] == 0.0), "rows without nonzeros: o = 0, lse = 0, sums = 0"
    assert all(np.abs(np.float64(v)).max() > 0 for v in want.values())
    errs = errors(got, want)
    assert same(p.run(True, act=act), got), "a repeat must be bit-identical"
    if pas != FWD:
        acc = p.run(False)
        errs.update({"acc " + k: v for k, v in errors(acc, p.want(False)).items()})
        for k, first in (("out", p.out0), ("out2", p.out20)):
            assert k not in acc or np.array_equal(acc[k][empty], first[:p.m, p.col0:p.col0 + f][empty]), "accumulating leaves rows without nonzeros alone"
    p.free()
    T.record_observed("gat_qkv_kernel", case="%s f=%d%s" % (PASS_NAMES[pas], f, " odd" if odd else ""), worst=max(errs.values()))
    print("observed", PASS_NAMES[pas], f, odd, errs)
    assert_within(pas, errs)


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd-offset"])
@pytest.mark.parametrize("f", WIDTHS)
def test_forward_finish_with_addend(ctx, f, odd):
    """HNH_ATTN_ADDEND on the finishing call of the forward pass, in every instance (the exact widths and the 8-byte lanes of wide heads
    included): act(o + addend) with the addend in [-1, 1] waiting in the destination, under relu, elu and the identity, against the
    extended-precision reference; a row without nonzeros gives act(addend); lse, the row state and the scores do not see the flag; whole
    rows and one call per window give the same bits."""
    p = QKVProblem(ctx, FWD, f, seed=4, odd=odd)
    empty = np.diff(p.rowptr) == 0
    add = p.addend()
    assert np.count_nonzero(empty) > 20 and add.min() < -0.9 and add.max() > 0.9
    errs = {}
    for act in ("relu", "elu", "identity"):
        got, want = p.run(True, act=act, addend=True), p.want(True, act=act, addend=True)
        errs.update({act + " " + k: v for k, v in errors(got, want).items()})
        assert not np.any(np.isnan(got["out"]))
        if act != "elu":
            assert np.array_equal(got["out"][empty], R.act_ld(add[empty].astype(np.longdouble), act).astype(np.float64)), "a row without nonzeros: act(addend)"
        assert same(p.run(True, act=act, addend=True), got), "a repeat must be bit-identical"
        assert same(p.run(True, GROUPINGS["one call per window"], act=act, addend=True), got), "one call per window"
        plain = p.run(True, act=act)
        assert all(np.array_equal(plain[k], got[k]) for k in ("lse", "state", "values")), "lse, the row state and the scores do not see the flag"
        assert not np.array_equal(plain["out"], got["out"])
    p.free()
    T.record_observed("gat_qkv_kernel", case="fwd addend f=%d%s" % (f, " odd" if odd else ""), worst=max(errs.values()))
    print("observed addend", f, odd, errs)
    assert all(v <= bound_of(FWD, k.split(" ", 1)[1]) for k, v in errs.items()), errs


@pytest.mark.parametrize("f", [7, 64, 256])
@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_scores_far_outside_exps_range(ctx, pas, f):
    p = QKVProblem(ctx, pas, f, seed=2, big=820.0)
    assert p.s.max() > 800.0 or p.s.min() < -800.0
    got, want = p.run(True), p.want(True)
    for k, v in got.items():  # (the running max of a row without nonzeros is -inf by definition: the empty state)
        assert np.all(np.isfinite(v)) or (k == "state" and np.all(np.isfinite(v[1])) and np.all(np.isneginf(v[0][~np.isfinite(v[0])]))), k
    errs = errors(got, want)
    p.free()
    T.record_observed("gat_qkv_kernel", case="%s f=%d |s|=800" % (PASS_NAMES[pas], f), worst=max(errs.values()))
    print("observed big", PASS_NAMES[pas], f, errs)
    assert_within(pas, errs)


@pytest.mark.parametrize("f", [8, 64, 256])
def test_forced_rescales(ctx, f):
    """The blocks of softmax_schedules with scale = 1: Q = the schedule's row operand, K = its map of the column index, so the score of a
    nonzero is set by its column and (no LeakyReLU: the score is monotone in the designed map) the running max rises exactly where designed,
    by more than 745 in the jump rows.  Against the extended-precision reference per schedule, and the same bits for every grouping."""
    m = 1024
    rowptr, colidx, x, y, rises, group = SS.build(m, f, seed=f, nwin=NWIN)
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    p = QKVProblem(ctx, FWD, f, given=(rowptr, colidx, rows, x, y, 1.0))
    found = P.max_rises(rowptr, p.s)
    assert all(np.array_equal(a, b) for a, b in zip(found, rises)), "the rise positions are the designed ones"
    jumps = [i for i in range(m) if group[i] == "jump" and len(rises[i]) > 1]
    assert len(jumps) > 20
    for i in jumps:
        seg = p.s[rowptr[i]:rowptr[i + 1]]
        assert np.all(np.diff(seg[rises[i]]) > 745.0), "exp(m_old - m_new) underflows at every rise of a jump row"
    got, want = p.run(True, act="identity"), p.want(True, act="identity")
    group = np.array(group)
    errs = {}
    for g in SS.SCHEDULES:  # (the schedules' scales differ by orders of magnitude: each group of rows on its own)
        sel = group == g
        nz = sel[rows]
        errs[g] = max(float(T.rel(np.longdouble(got["out"][sel]), want["out"][sel])), float(T.rel(np.longdouble(got["lse"][sel]), want["lse"][sel])))
        assert T.rel(np.longdouble(got["values"][nz]), want["values"][nz]) <= 1e-13
    assert np.all(np.isfinite(got["out"])) and np.all(np.isfinite(got["lse"]))
    for name, groups in GROUPINGS.items():
        assert same(p.run(True, groups, act="identity"), got), name
    p.free()
    T.record_observed("gat_qkv_kernel", case="forced rescales f=%d" % f, worst=max(errs.values()))
    print("observed rescales", f, errs)
    assert max(errs.values()) <= FTOL, errs


SPLIT_CASES = [(pas, f) for pas in (FWD, ROW, COL) for f in (33, 100, 64, 128, 256)]  # one odd, one bounds-checked even, the three exact widths


@pytest.mark.parametrize("pas,f", SPLIT_CASES, ids=lambda v: str(v))
def test_grouping_independence(ctx, pas, f):
    """Whole rows, one call per window and two uneven groupings of six windows: the same bits (forward output with elu, lse, the scores and
    the row state; dQ; dK and dV), overwriting and accumulating, because every launch continues the row's state nonzero by nonzero."""
    p = QKVProblem(ctx, pas, f, seed=3)
    for overwrite in ((True,) if pas == FWD else (True, False)):
        whole = p.run(overwrite, act="elu")
        for name, groups in GROUPINGS.items():
            assert same(p.run(overwrite, groups, act="elu"), whole), (name, overwrite)
    p.free()


@pytest.mark.parametrize("pas,f", SPLIT_CASES, ids=lambda v: str(v))
def test_forced_panels_are_bit_identical(monkeypatch, pas, f):
    """Column panels (several launches over every row, hub rows after the last): the same bits as one launch."""
    ncols = 1536
    c1 = K.Ctx(0)
    p1 = QKVProblem(c1, pas, f, ncols=ncols, seed=5)
    one, want = p1.run(True, act="elu"), p1.want(True, act="elu")
    p1.free()
    c1.close()
    gather_w = P.fused_packed_width(f, pas == COL)
    monkeypatch.setenv("HNH_PANEL_BYTES", str(ncols * gather_w * 8 / 5))
    monkeypatch.setenv("HNH_MAX_PANELS", "8")
    monkeypatch.setenv("HNH_PANELS_WITH_HUBS", "1")
    c5 = K.Ctx(0)
    p5 = QKVProblem(c5, pas, f, ncols=ncols, seed=5)
    # (the query answers for widths up to 512 only, and the packed operand of f = 256 is wider: asked at 512, where the same bytes round to 5 too)
    assert c5.lib.hnh_panel_count(c5.h, p5.m, p5.nnz, ncols, min(gather_w, 512), int(np.diff(p5.rowptr).max())) == 5
    five = p5.run(True, act="elu")
    p5.free()
    c5.close()
    assert same(one, five)
    assert_within(pas, errors(five, want))


@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_wide_heads_and_bad_arguments_are_refused_and_write_nothing(ctx, pas):
    p = QKVProblem(ctx, pas, 34)
    a, blk = p.args(), p.block()
    call = lambda a, flags, win=None: p.fn()(ctx.h, C.byref(blk), C.byref(a), flags, win, K.STREAM_COMPUTE)  # noqa: E731
    a.f = 257
    assert call(a, K.FUSED_OUT_OVERWRITE) == K.ERR_UNSUPPORTED
    assert b"256" in ctx.lib.hnh_last_error(ctx.h) and b"HNH_ATTN_QKV_MAX_F" in ctx.lib.hnh_last_error(ctx.h)
    a.f = 34
    assert call(a, 4) == 1  # an unknown flag
    a.Y = p.d["y"].ptr + 8
    assert call(a, K.FUSED_OUT_OVERWRITE) == 1 and b"16-byte aligned" in ctx.lib.hnh_last_error(ctx.h)  # a misaligned packed operand
    a = p.args()
    a.ld_y = p.pw + 1
    assert call(a, K.FUSED_OUT_OVERWRITE) == 1  # ... and one of an odd pitch
    a.ld_y = p.pw - 2
    assert call(a, K.FUSED_OUT_OVERWRITE) == 1  # a gathered operand narrower than the pack
    a = p.args()
    if pas == FWD:
        assert call(a, K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH | K.ATTN_ACT_ELU | K.ATTN_ACT_IDENTITY) == 1  # both activation bits at once
        win = K.CsrWindow(None, p.windows(), 0)
        assert call(a, K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH, C.byref(win)) == 1 and b"last window" in ctx.lib.hnh_last_error(ctx.h)
    else:
        assert call(a, K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH) == 1  # a backward pass has no finish
    if pas == COL:
        a.X2 = None
        assert call(a, K.FUSED_OUT_OVERWRITE) == 1  # no own rows of V
    ctx.sync()
    assert p.untouched()
    p.free()


@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_empty_block(ctx, pas):
    """rowptr == NULL: overwrite (and the forward finish) leave zeros in the pass's outputs, accumulate leaves everything alone."""
    p = QKVProblem(ctx, pas, 33)
    a = p.args()
    none = K.CsrBlock(p.m, 0, -1, 0, 0, None, None, None)
    ctx.check(p.fn()(ctx.h, C.byref(none), C.byref(a), 0, None, K.STREAM_COMPUTE), "empty block, accumulate")
    ctx.sync()
    assert p.untouched()
    fl = K.FUSED_OUT_OVERWRITE | (K.ATTN_FINISH if pas == FWD else 0)
    ctx.check(p.fn()(ctx.h, C.byref(none), C.byref(a), fl, None, K.STREAM_COMPUTE), "empty block, overwrite")
    ctx.sync()
    got = p.collect()
    assert np.all(got["out"] == 0.0) and (pas != COL or np.all(got["out2"] == 0.0))
    if pas == FWD:
        assert np.all(got["lse"] == 0.0) and np.all(got["state"][1] == 0.0) and np.all(np.isneginf(got["state"][0]))
        assert np.array_equal(got["values"], p.vals0[1:-1]), "no nonzero, no score"
    p.free()


# ------------------------------------------------------------------------------------------------ the operator
def skip_parameters(layers, seed=12):
    rng = np.random.default_rng(seed)
    bias = {li: rng.standard_normal(fph * heads) * 0.5 for li, (fin, fph, heads) in enumerate(layers)}
    res_weights = {li: rng.standard_normal((fin, fph * heads)) / np.sqrt(fin) for li, (fin, fph, heads) in enumerate(layers)}
    return bias, res_weights


def qkv_setup(world, rows, cols, m, x, layers, w, wq, wk, g, bias=None, res_weights=None, **kw):
    s = setup(world, rows, cols, m, x, layers, w, None, g, attention="softmax", score="transformer", **kw)
    gnn = s["gnn"]
    for k in w:
        gnn.set_query_weight(*k, wq[k])
        gnn.set_key_weight(*k, wk[k])
    for li, b in (bias or {}).items():
        gnn.set_bias(li, b)
    for li, wr in (res_weights or {}).items():
        gnn.set_residual_weight(li, wr)
    return s


def qkv_round(s, w, bias=None, res_weights=None):
    gnn = s["gnn"]
    gnn.forwardPass()
    gnn.get_output(s["out"])
    r = dict(out=s["out"].download())
    gnn.backwardPass(s["g"])
    gnn.get_input_grad(s["dx"])
    r.update(dx=s["dx"].download(), dw={k: gnn.weight_grad(*k) for k in w}, dwq={k: gnn.query_weight_grad(*k) for k in w},
             dwk={k: gnn.key_weight_grad(*k) for k in w}, db={li: gnn.bias_grad(li) for li in (bias or {})},
             dwr={li: gnn.residual_weight_grad(li) for li in (res_weights or {})})
    return r


def run_qkv(world, rows, cols, m, x, layers, w, wq, wk, g, rounds=1, bias=None, res_weights=None, **kw):
    s = qkv_setup(world, rows, cols, m, x, layers, w, wq, wk, g, bias, res_weights, **kw)
    res = dict(subA=s["subA"], subB=s["subB"], rounds=[qkv_round(s, w, bias, res_weights) for _ in range(rounds)])
    teardown(s)
    return res


REPLICATED = ("dw", "dwq", "dwk", "db", "dwr")


def assembled(per_rank, k, m, layers):
    """The global output and dX of round k, and rank 0's replicated gradients (asserted equal on every rank)."""
    r0 = per_rank[0]["rounds"][k]
    for pr in per_rank:
        for name in REPLICATED:
            assert all(np.array_equal(pr["rounds"][k][name][key], r0[name][key]) for key in r0[name]), "%s must be equal on every rank" % name
    hf = layers[-1][1] * layers[-1][2]
    out = T.assemble_dense([dict(o=pr["rounds"][k]["out"], subA=pr["subA"]) for pr in per_rank], "o", "subA", m, hf)
    dx = T.assemble_dense([dict(dx=pr["rounds"][k]["dx"], subB=pr["subB"]) for pr in per_rank], "dx", "subB", m, layers[0][0])
    return dict({name: r0[name] for name in REPLICATED}, out=out, dx=dx)


def reference(rows, cols, m, x, layers, w, wq, wk, g, **mode):
    dw, dwq, dwk, db, dwr, dx = Q.backward(rows, cols, m, x, layers, g, w, wq, wk, **mode)
    return dict(out=Q.forward(rows, cols, m, x, layers, w, wq, wk, **mode), dw=dw, dwq=dwq, dwk=dwk, db=db, dwr=dwr, dx=dx)


def check_against(got, want, label, ranks):
    """output, every dW_v, dW_q, dW_k, db, dW_res and dX against the reference; none vacuous; the worst is recorded and asserted <= TOL"""
    errs = {name: T.rel(got[name], want[name]) for name in ("out", "dx")}
    for name in REPLICATED:
        assert got[name].keys() == want[name].keys(), name
        for key in want[name]:
            assert np.abs(want[name][key]).max() > 0, (name, key)
            errs[(name, key)] = T.rel(got[name][key], want[name][key])
    worst = max(errs.values())
    T.record_observed("gat_qkv", case=label, ranks=ranks, worst=worst)
    print("observed gat_qkv", label, ranks, "worst %.2e" % worst)
    assert worst <= TOL, errs


ER8_RESULTS = {}
_BIAS, _WRES = skip_parameters(T.GAT_LAYERS)
CONFIGS = {"relu": dict(), "published": dict(activation=("elu", "identity")), "feature dropout": dict(dropout=(0.0, 0.3), seed=11),
           "bias + projection": dict(activation=("elu", "relu"), residual="projection", bias=True)}


def ref_mode(kw):
    mode = dict(activations=kw.get("activation"), rates=kw.get("dropout", (0.0, 0.0)), seed=kw.get("seed", 0))
    if kw.get("bias"):
        mode.update(residual=kw["residual"], bias=_BIAS, res_weights=_WRES)
    return mode


def er8_problem():
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    wq, wk = Q.qk_weights_of(layers, scale=0.25)  # (the inputs are small after the hashed fill: scores of order one)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 9) * 16.0
    return rows, cols, m, x, layers, hashed_weights(layers), wq, wk, g


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_transformer_er8(p, config):
    rows, cols, m, x, layers, w, wq, wk, g = er8_problem()
    kw = CONFIGS[config]
    extra = dict(bias=_BIAS, res_weights=_WRES) if kw.get("bias") else {}
    per_rank = H.run_spmd(p, lambda wd: run_qkv(wd, rows, cols, m, x, layers, w, wq, wk, g, rounds=2, **dict(kw, **extra)))
    got = assembled(per_rank, 0, m, layers)
    want = reference(rows, cols, m, x, layers, w, wq, wk, g, **ref_mode(kw))
    s = Q.forward(rows, cols, m, x, layers, w, wq, wk, keep_trace=True, **ref_mode(kw))[1][0][3][0][1]
    assert np.ptp(s) > 0.5, "the attention is not uniform: the scores of a head spread"
    check_against(got, want, "er8_r16 %s p%d" % (config, p), p)
    again = assembled(per_rank, 1, m, layers)
    assert np.array_equal(got["out"], again["out"]) and np.array_equal(got["dx"], again["dx"]), "two rounds must be bit-identical"
    assert all(np.array_equal(got[name][k], again[name][k]) for name in REPLICATED for k in got[name])
    ER8_RESULTS[(p, config)] = got


def test_one_rank_and_eight_ranks_agree():
    rows, cols, m, x, layers, w, wq, wk, g = er8_problem()
    res = {}
    for p in (1, 8):
        res[p] = ER8_RESULTS.get((p, "relu")) or assembled(H.run_spmd(p, lambda wd: run_qkv(wd, rows, cols, m, x, layers, w, wq, wk, g)), 0, m, layers)
    check_against(res[8], res[1], "er8_r16 p8 against p1", 8)


WIDE = {"exact widths": [(256, 256, 1), (256, 128, 2), (256, 64, 3)], "odd heads": [(24, 33, 2), (66, 7, 3)]}


@pytest.mark.parametrize("p", [1, 4])
@pytest.mark.parametrize("shape", sorted(WIDE))
def test_transformer_widths(shape, p):
    m, layers = 1 << 12, WIDE[shape]
    rows, cols = H.generate_er(m, m, m * 16, 77)
    x = O.dense_fill(m, layers[0][0], 41) * 16.0
    w = hashed_weights(layers)
    wq, wk = Q.qk_weights_of(layers, seed=5, scale=0.2)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 3) * 64.0
    kw = dict(activation=("elu",) * (len(layers) - 1) + ("identity",))
    per_rank = H.run_spmd(p, lambda wd: run_qkv(wd, rows, cols, m, x, layers, w, wq, wk, g, **kw))
    check_against(assembled(per_rank, 0, m, layers), reference(rows, cols, m, x, layers, w, wq, wk, g, **ref_mode(kw)), "%s p%d" % (shape, p), p)


@pytest.mark.parametrize("p", [1, 4])
def test_transformer_rmat_hub_rows(p):
    m, layers = 1 << 13, [(64, 64, 2), (128, 32, 2)]
    rows, cols = H.generate_rmat(13, m * 16)
    assert np.bincount(rows, minlength=m).max() >= 512 and np.bincount(cols, minlength=m).max() >= 512
    x = O.dense_fill(m, 64, 8) * 8.0
    w = hashed_weights(layers)
    wq, wk = Q.qk_weights_of(layers, seed=6, scale=0.3)
    g = O.dense_fill(m, 64, 4) * 32.0
    per_rank = H.run_spmd(p, lambda wd: run_qkv(wd, rows, cols, m, x, layers, w, wq, wk, g, rounds=2))
    got = assembled(per_rank, 0, m, layers)
    check_against(got, reference(rows, cols, m, x, layers, w, wq, wk, g), "rmat hubs p%d" % p, p)
    again = assembled(per_rank, 1, m, layers)
    assert np.array_equal(got["dx"], again["dx"]) and all(np.array_equal(got[n][k], again[n][k]) for n in REPLICATED for k in got[n]), "a repeat must be bit-identical"


@pytest.mark.parametrize("p", [1, 4])
def test_tied_weights_equal_the_products_dot_path(p):
    """W_k = W_v = W and W_q = W / scale against GAT(leaky_relu_alpha=1.0, attention="softmax", score="dot", backward="fused") on the same
    graph: the same output, and dW_dot = dW_v + dW_k + dW_q / scale, dX the same.  The yardstick shares no code with the new passes.  f = 16
    and 64: scale is a power of two."""
    rows, cols, m, x = er8()
    layers = [(16, 16, 2), (32, 64, 1)]
    rng = np.random.default_rng(4)
    w = {(li, h): rng.standard_normal((fin, fph)) * 0.2 / np.sqrt(fin * np.sqrt(fph)) for li, (fin, fph, heads) in enumerate(layers) for h in range(heads)}
    wq = {k: v / Q.scale_of(v.shape[1]) for k, v in w.items()}
    g = O.dense_fill(m, 64, 9) * 16.0
    kw = dict(activation=("elu", "identity"))

    def dot_path(world):
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, "15d_fusion2", sp, layers[0][0], 1)
        gnn = H.GAT(d, layers, 1.0, attention="softmax", score="dot", backward="fused", **kw)
        for k, v in w.items():
            gnn.set_weight(*k, v)
        s = dict(sp=sp, d=d, gnn=gnn)
        d.setRValue(layers[0][0])
        s["subB"] = d.submatrices(H.BMAT)
        d.setRValue(64)
        s["subA"] = d.submatrices(H.AMAT)
        for name, idx in (("x", 0), ("dx", 0), ("g", len(layers)), ("out", len(layers))):
            s[name] = H.Dense.create(world, *gnn.buffer_shape(idx))
        s["x"].upload(T.fill_local(s["subB"], s["x"].shape, x))
        s["g"].upload(T.fill_local(s["subA"], s["g"].shape, g))
        gnn.set_input(s["x"])
        gnn.forwardPass()
        gnn.get_output(s["out"])
        r = dict(out=s["out"].download())
        gnn.backwardPass(s["g"])
        gnn.get_input_grad(s["dx"])
        r.update(dx=s["dx"].download(), dw={k: gnn.weight_grad(*k) for k in w})
        res = dict(subA=s["subA"], subB=s["subB"], rounds=[dict(r, dwq={}, dwk={}, db={}, dwr={})])
        teardown(s)
        return res

    tied = assembled(H.run_spmd(p, lambda wd: run_qkv(wd, rows, cols, m, x, layers, w, wq, w, g, **kw)), 0, m, layers)
    dot = assembled(H.run_spmd(p, dot_path), 0, m, layers)
    errs = dict(out=T.rel(tied["out"], dot["out"]), dx=T.rel(tied["dx"], dot["dx"]))
    assert np.abs(dot["out"]).max() > 0 and np.abs(dot["dx"]).max() > 0
    for k in w:
        assert np.abs(dot["dw"][k]).max() > 0
        errs[k] = T.rel(tied["dw"][k] + tied["dwk"][k] + tied["dwq"][k] / Q.scale_of(w[k].shape[1]), dot["dw"][k])
    s = Q.forward(rows, cols, m, x, layers, w, wq, w, activations=kw["activation"], keep_trace=True)[1][0][3][0][1]
    assert np.ptp(s) > 0.5, "the attention is not uniform"
    T.record_observed("gat_qkv_tied", ranks=p, worst=max(errs.values()))
    print("observed tied", p, errs)
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("score", ["dot", "additive", "gatv2"])
@pytest.mark.parametrize("p", [1, 4])
def test_other_scores_are_untouched_by_a_transformer_round(p, score):
    """score -> transformer -> score on one object: the results are bit-identical before and after, and equal those of a GAT that never
    selected the new score."""
    rows, cols, m, x, layers, w, wq, wk, g = er8_problem()
    av = R.vectors_of(layers)
    vectors = score != "dot"
    kw = dict(attention="softmax", backward="fused", score=score)

    def trip(world):
        s = setup(world, rows, cols, m, x, layers, w, av, g, **kw)
        before = G.one_round(s, w, vectors)
        s["gnn"].set_score("transformer")
        for k in w:
            s["gnn"].set_query_weight(*k, wq[k])
            s["gnn"].set_key_weight(*k, wk[k])
        with pytest.raises(H.HnhError, match="forwardPass"):
            s["gnn"].backwardPass(s["g"])  # a change of score invalidates the stored forward pass
        mid = qkv_round(s, w)
        s["gnn"].set_score(score)
        after = G.one_round(s, w, vectors)
        with pytest.raises(H.HnhError, match="no GAT query/key weight gradient yet"):
            s["gnn"].query_weight_grad(0, 0)  # (dW_q and dW_k of the transformer round left with its score: no stale gradient)
        teardown(s)
        return before, mid, after

    def plain(world):
        s = setup(world, rows, cols, m, x, layers, w, av, g, **kw)
        r = G.one_round(s, w, vectors)
        teardown(s)
        return r

    for (before, mid, after), old in zip(H.run_spmd(p, trip), H.run_spmd(p, plain)):
        for a in (after, old):
            assert np.array_equal(before["out"], a["out"]) and np.array_equal(before["dx"], a["dx"])
            assert all(np.array_equal(before["dw"][k], a["dw"][k]) for k in w)
            assert not vectors or all(np.array_equal(before["da"][k][i], a["da"][k][i]) for k in w for i in (0, 1))
        assert not np.array_equal(mid["out"], before["out"]), "the transformer round computed something else"


def test_refusals_on_the_device():
    rows, cols, m, _ = er8()

    def rank(world):
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, "15d_fusion2", sp, 16, 1)
        for layers, kw, words in (([(16, 8, 2)], dict(attention="none"), "score transformer.*attention mode softmax only"),
                                  ([(16, 257, 1)], dict(attention="softmax"), "score transformer.*at most 256 features, not 257"),
                                  ([(16, 8, 2)], dict(attention="softmax", dropout=(0.5, 0.0)), "attention dropout.*transformer")):
            gnn = H.GAT(d, layers, ALPHA, score="transformer", **kw)
            g = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
            with pytest.raises(H.HnhError, match=words):
                gnn.forwardPass()
            with pytest.raises(H.HnhError, match=words):
                gnn.backwardPass(g)
            world.sync()  # nothing was left in flight
            g.free()
            gnn.free()
        gnn = H.GAT(d, [(16, 8, 2)], ALPHA, attention="softmax", score="transformer")
        with pytest.raises(H.HnhError, match="attention_coefficients does not support score transformer"):
            gnn.attention_coefficients(0, 0)
        world.sync()
        gnn.free()
        for h in (d, sp):
            h.free()
        return True

    assert all(H.run_spmd(2, rank))


# ------------------------------------------------------------------------------------------------ training
PUBLISHED = ("elu", "identity")
ADAM = dict(kind="adam", lr=0.01, weight_decay=5e-4)


def device_train(world, pp, layers, wq, wk, steps):
    s = qkv_setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["w"], wq, wk, None, activation=PUBLISHED)
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
    res["wq"] = {k: gnn.get_query_weight(*k) for k in pp["w"]}
    res["wk"] = {k: gnn.get_key_weight(*k) for k in pp["w"]}
    teardown(s)
    return res


@pytest.mark.parametrize("p", [1, 4])
def test_adam_trajectory_of_the_published_layers(p):
    """Ten steps of train_step: within 10 x the divergence of a reference run whose gradients are perturbed at 1e-10, the loss falls, the
    parameters are bit-equal across ranks, every W_q and W_k moves."""
    layers, steps = T.GAT_LAYERS, 10
    pp = R.planted_partition(layers)
    wq, wk = Q.qk_weights_of(layers)
    args = (pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["labels"], pp["mask"], "mean", pp["w"], wq, wk)
    ref = Q.train(*args, ADAM, steps, activations=PUBLISHED)
    per = Q.train(*args, ADAM, steps, activations=PUBLISHED, perturb=(1e-10, np.random.default_rng(7)))
    bound_p = 10.0 * Q.parameter_divergence(per, ref)
    bound_l = 10.0 * float(np.max(np.abs(np.array(per[0]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    assert bound_p > 0 and bound_l > 0
    per_rank = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, wq, wk, steps))
    r0 = per_rank[0]
    for pr in per_rank:
        assert pr["losses"] == r0["losses"] and pr["accs"] == r0["accs"]
        assert all(np.array_equal(pr[n][k], r0[n][k]) for n in ("w", "wq", "wk") for k in r0["w"]), "parameters are bit-equal across ranks"
    got_p = Q.parameter_divergence((None, None, r0["w"], r0["wq"], r0["wk"]), ref[:5])
    got_l = float(np.max(np.abs(np.array(r0["losses"]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    T.record_observed("gat_qkv_trajectory", ranks=p, parameters=got_p, parameters_bound=bound_p, loss=got_l, loss_bound=bound_l, first=r0["losses"][0],
                      last=r0["losses"][-1])
    print("observed gat_qkv trajectory", p, "parameters %.2e (bound %.2e) loss %.2e (bound %.2e)" % (got_p, bound_p, got_l, bound_l), r0["losses"])
    assert got_p <= bound_p and got_l <= bound_l
    assert r0["accs"] == ref[1]
    assert r0["losses"][-1] < r0["losses"][0], "the planted-partition loss falls"
    assert all(np.abs(r0["wq"][k] - wq[k]).max() > 0 and np.abs(r0["wk"][k] - wk[k]).max() > 0 for k in wq), "every W_q and W_k has moved"
