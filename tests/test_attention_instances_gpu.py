"""The softmax pass of include/hnh_attention.h at every kernel instance it can pick, with inputs that force its rescale branch.

launch_shape<Op::kFusedSoftmax> picks one of nine row-kernel instances (LPR, VEC, W) by the width R and by whether every operand
allows 16-byte accesses (W = 2): exact (32,1,2) R = 64, (64,1,2) 128, (64,2,2) 256; bounds-checked NX(V, W) with LPR = 64 for the other
widths: NX(1,2) even <= 128, NX(2,2) even 130 .. 256, NX(4,2) even 258 .. 512, NX(1,1) <= 64, NX(2,1) 65 .. 128, NX(4,1) 129 .. 256 when
W = 1 (odd widths, or a relu_dst that is 8-byte aligned only).  Every width below is checked against the extended-precision reference
(gat_pass_ref.attention_ld), for untouched columns outside the head's block and for bit-identical repeats.

The rescale of the running state (process_row: `if (fu != 1.0)`) runs only where a row's running max rises, which uniform random
scores do mostly in a row's first nonzeros.  tests/softmax_schedules.py designs the score sequences instead (monotone rows, a spike at
every position 0 .. 18 and at a hub row's last nonzero, a spike at the first nonzero of every window and every forced panel, ties with
the max, rises beyond exp's range); the kernel's own scores are checked to rise exactly there, and the pass as one launch, as 5 forced
column panels and as 6 windows grouped into 1, 2, 5 and 6 launches must give the same bits.  Then the width limits, the refused calls
(nothing written) and the block without nonzeros (attn_empty_rows_kernel).

Every test passed on an MI355X (45 tests, 13 s wall under a kernel trace, all nine row-kernel instances launched); the bounds
asserted are those of gat_gpu_harness.check_against_numpy (1e-12 output and lse, 1e-13 scores)."""
import ctypes as C

import numpy as np
import pytest

import gat_pass_ref as R
import hnh_testlib as T
import softmax_schedules as S
from distributed_sddmm_amd import _kernels as K
from gat_gpu_harness import ALPHA, check_against_numpy, ctx, hip_backend, mixed_degrees, softmax_pass, square_graph  # noqa: F401

pytestmark = pytest.mark.gpu
ERR_UNSUPPORTED = 4

# (width, column offset of the head's block in relu_dst): an odd offset leaves relu_dst 8-byte aligned, which forces W = 1
WIDTHS = [(w, 2) for w in (64, 100, 128, 130, 192, 200, 256, 258, 300, 384, 512, 1, 63, 65, 101, 127, 129, 201, 255)] + \
         [(w, 3) for w in (64, 128, 200, 256)]
# one (width, offset) per instance: (32,1,2) (64,1,2) (64,2,2) NX(1,2) NX(2,2) NX(4,2) NX(1,1) NX(2,1) NX(4,1), and W = 1 at even widths
SCHEDULE_WIDTHS = [(64, 2), (128, 2), (256, 2), (100, 2), (200, 2), (300, 2), (7, 2), (101, 2), (201, 2), (64, 3), (200, 3)]
GROUPINGS = ([(0, 6)], [(0, 3), (3, 6)], [(0, 1), (1, 2), (2, 4), (4, 5), (5, 6)], [(q, q + 1) for q in range(6)])


def wid(p):
    return "R%d%s" % (p[0], "_w1" if p[1] % 2 else "")


@pytest.mark.parametrize("width,off", WIDTHS, ids=[wid(p) for p in WIDTHS])
def test_every_width_vs_extended_reference(ctx, width, off):
    m = 4096
    rowptr, colidx, rows = square_graph(m, mixed_degrees(m, width + off, empty=()), width)
    rng = np.random.default_rng(width * 10 + off)
    x, y = rng.uniform(-1, 1, (m, width)) * 2.0, rng.uniform(-1, 1, (m, width)) * 2.0
    got = softmax_pass(ctx, rowptr, colidx, x, y, ALPHA, off=off)  # (asserts the columns outside the head's block)
    check_against_numpy(got, rows, colidx, m, x, y)
    again = softmax_pass(ctx, rowptr, colidx, x, y, ALPHA, off=off)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls must be bit-identical"


def panel_ctx(monkeypatch, m, width):
    monkeypatch.setenv("HNH_PANEL_BYTES", str(m * width * 8 / 5))
    monkeypatch.setenv("HNH_MAX_PANELS", "8")
    monkeypatch.setenv("HNH_PANELS_WITH_HUBS", "1")
    c = K.Ctx(0)
    monkeypatch.delenv("HNH_PANEL_BYTES")
    return c


@pytest.mark.parametrize("width,off", SCHEDULE_WIDTHS, ids=[wid(p) for p in SCHEDULE_WIDTHS])
def test_forced_rescales(ctx, monkeypatch, width, off):
    """The designed schedules: the kernel's scores rise exactly where designed; output, lse and scores against the extended reference
    (per schedule: the jump rows' lse is 2000); one launch == 5 forced panels == windows grouped as 1, 2, 5, 6 launches, bit for bit."""
    m = 4096
    rowptr, colidx, x, y, rises, group = S.build(m, width, width + off)
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    one = softmax_pass(ctx, rowptr, colidx, x, y, ALPHA, off=off)
    got_rises = R.max_rises(rowptr, one[4])
    assert all(np.array_equal(a, b) for a, b in zip(got_rises, rises)), "the kernel's scores do not rise where designed"
    g = np.array(group)
    check_against_numpy(one, rows, colidx, m, x, y, sels=[g == name for name in S.SCHEDULES])
    cp = panel_ctx(monkeypatch, m, width)
    try:
        assert cp.lib.hnh_panel_count(cp.h, m, int(rowptr[-1]), m, width, int(np.diff(rowptr).max())) == 5
        runs = [softmax_pass(cp, rowptr, colidx, x, y, ALPHA, off=off)]
    finally:
        cp.close()
    runs += [softmax_pass(ctx, rowptr, colidx, x, y, ALPHA, groups=gr, off=off) for gr in GROUPINGS]
    for k, r in enumerate(runs):
        assert all(np.array_equal(a, b) for a, b in zip(r, one)), "run %d differs from the single launch" % k


# ------------------------------------------------------------------------------------------------ width limits and refused calls
class Call:
    """Device buffers of one direct call with sentinels everywhere: relu_dst 7, lse 5, row_max 6, row_sum 8, Out 9."""

    def __init__(self, ctx, m, width, off=2, ld=None, deg=3):
        self.ctx, self.m, self.width, self.off = ctx, m, width, off
        self.ld = ld or width + 4
        self.rowptr, self.colidx, self.rows = square_graph(m, np.full(m, deg), width)
        rng = np.random.default_rng(width)
        self.x = rng.uniform(-1, 1, (m, width))
        self.d = dict(rp=ctx.upload(self.rowptr), ci=ctx.upload(self.colidx), x=ctx.upload(self.x), vals=ctx.upload(np.full(m * deg, 3.0)),
                      out=ctx.upload(np.full(m * width, 9.0)), dst=ctx.upload(np.full((m, self.ld), 7.0)),
                      lse=ctx.upload(np.full(m, 5.0)), rmax=ctx.upload(np.full(m, 6.0)), rsum=ctx.upload(np.full(m, 8.0)))
        self.blk = K.CsrBlock(m, m * deg, m, deg, 0, self.d["rp"].ptr, self.d["ci"].ptr, None)
        self.st = K.AttnState(self.d["rmax"].ptr, self.d["rsum"].ptr, self.d["lse"].ptr, ALPHA, self.d["dst"].ptr + off * 8, self.ld)

    def run(self, flags=K.FUSED_VALUES_OVERWRITE | K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH):
        d = self.d
        return self.ctx.lib.hnh_attn_softmax_csr_p(self.ctx.h, C.byref(self.blk), d["vals"].ptr, d["x"].ptr, d["x"].ptr, d["out"].ptr, self.width, flags,
                                                   C.byref(self.st), None, K.STREAM_COMPUTE)

    def get(self, name):
        return self.d[name].get()

    def free(self):
        for a in self.d.values():
            a.free()


@pytest.mark.parametrize("width,off", [(514, 2), (257, 2), (300, 3), (512, 3)], ids=["R514", "R257", "R300_misaligned", "R512_misaligned"])
def test_refused_widths_write_nothing(ctx, width, off):
    """Beyond the one-pass instances (hnh_attention.h): even R > 512, odd R > 256, and R > 256 when relu_dst is not 16-byte aligned.
    The refusal names the limit and leaves relu_dst, lse, row_max, row_sum, Out and the scores as they were."""
    c = Call(ctx, 256, width, off=off)
    try:
        assert c.run() == ERR_UNSUPPORTED
        msg = ctx.lib.hnh_last_error(ctx.h)
        assert b"one-pass" in msg and b"512" in msg and b"256" in msg and str(width).encode() in msg
        ctx.sync()
        assert np.all(c.get("dst") == 7.0) and np.all(c.get("lse") == 5.0) and np.all(c.get("rmax") == 6.0) and np.all(c.get("rsum") == 8.0)
        assert np.all(c.get("out") == 9.0) and np.all(c.get("vals") == 3.0)
    finally:
        c.free()


@pytest.mark.parametrize("width,off", [(512, 2), (255, 2), (256, 3)], ids=["R512", "R255", "R256_misaligned"])
def test_widths_at_the_limit_are_accepted(ctx, width, off):
    c = Call(ctx, 256, width, off=off, deg=5)
    try:
        ctx.check(c.run(), "softmax pass at the limit")
        ctx.sync()
        got = (c.get("dst")[:, off:off + width], c.get("lse"), c.get("rmax"), c.get("rsum"), c.get("vals"))
        check_against_numpy(got, c.rows, c.colidx, 256, c.x, c.x)
    finally:
        c.free()


# ------------------------------------------------------------------------------------------------ the block without nonzeros
@pytest.mark.parametrize("width", [7, 64, 200, 512])
def test_empty_block(ctx, width):
    """b->rowptr == NULL (attn_empty_rows_kernel): OUT_OVERWRITE starts every row empty (-inf, 0, Out 0) and a finish of it writes 0; a
    call without it continues the given state: unchanged without the finish, relu_dst = max(Out / l, 0) and lse = M + log l with it,
    and a row with l = 0 ends at 0 and lse 0."""
    lib, m = ctx.lib, 1000
    rng = np.random.default_rng(width)
    mx0 = rng.uniform(-3, 3, m)
    l0 = rng.uniform(0.5, 4.0, m)
    l0[::9] = 0.0
    mx0[::9] = -np.inf
    out0 = rng.uniform(-2, 2, (m, width))
    out0[::9] = 0.0
    ld, off = width + 4, 2
    blk = K.CsrBlock(m, 0, -1, 0, 0, None, None, None)

    def call(flags):
        d = dict(out=ctx.upload(out0), dst=ctx.upload(np.full((m, ld), 7.0)), lse=ctx.upload(np.full(m, 5.0)), rmax=ctx.upload(mx0),
                 rsum=ctx.upload(l0))
        st = K.AttnState(d["rmax"].ptr, d["rsum"].ptr, d["lse"].ptr, ALPHA, d["dst"].ptr + off * 8, ld)
        ctx.check(lib.hnh_attn_softmax_csr_p(ctx.h, C.byref(blk), None, None, None, d["out"].ptr, width, flags, C.byref(st), None,
                                             K.STREAM_COMPUTE), "empty block")
        ctx.sync()
        res = {k: v.get() for k, v in d.items()}
        for v in d.values():
            v.free()
        assert np.all(res["dst"][:, :off] == 7.0) and np.all(res["dst"][:, off + width:] == 7.0)
        res["dst"] = res["dst"][:, off:off + width]
        res["out"] = res["out"].reshape(m, width)
        return res

    r = call(K.FUSED_OUT_OVERWRITE)  # reset, no finish
    assert np.all(r["rmax"] == -np.inf) and np.all(r["rsum"] == 0.0) and np.all(r["out"] == 0.0)
    assert np.all(r["dst"] == 7.0) and np.all(r["lse"] == 5.0)
    r = call(K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH)  # reset and finish: every row without nonzeros
    assert np.all(r["rmax"] == -np.inf) and np.all(r["rsum"] == 0.0) and np.all(r["dst"] == 0.0) and np.all(r["lse"] == 0.0)
    r = call(0)  # continue, no finish: the state passes unchanged
    assert np.array_equal(r["rmax"], mx0) and np.array_equal(r["rsum"], l0) and np.array_equal(r["out"], out0)
    assert np.all(r["dst"] == 7.0) and np.all(r["lse"] == 5.0)
    r = call(K.ATTN_FINISH)  # continue and finish
    live = l0 > 0
    want = np.zeros((m, width))
    want[live] = np.maximum(out0[live] / l0[live, None], 0.0)
    assert np.array_equal(r["rmax"], mx0) and np.array_equal(r["rsum"], l0)
    assert T.rel(r["dst"], want) <= 1e-15 and np.all(r["dst"][~live] == 0.0) and np.count_nonzero(r["dst"]) > r["dst"].size // 3
    lse = np.zeros(m)
    lse[live] = mx0[live] + np.log(l0[live])
    assert np.all(np.abs(r["lse"] - lse) <= 1e-15 * np.maximum(1.0, np.abs(lse))) and np.all(r["lse"][~live] == 0.0)
