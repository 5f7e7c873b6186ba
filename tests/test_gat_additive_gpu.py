"""The GAT's additive (a1, a2) attention score on the GPU (include/hnh_attn_additive.h, GAT score "additive").

Kernel level, through ctypes: the forward pass against the extended-precision numpy reference (tests/gat_additive_ref.py, fwd_pass_ld),
the backward row and column passes against numpy, at widths 1, 2, 7, 16, 64, 100, 128, 256 on blocks with empty rows, rows of 200 - 300,
hub rows of 600 and 1500 and repeated pairs, with pitches wider than the widths, an output block at an odd column offset of an odd
pitch, guard values around every output, and scores far outside exp's range (|z| about 800); their independence of how a row's
nonzeros are split into launches (whole rows, one call per window, two uneven groupings of six windows, forced Infinity-Cache panels),
bit for bit; the dense helpers; the width limit; empty blocks.
Operator level: GAT(..., attention="softmax", score="additive") on 15d_fusion2, c = 1 over 1, 2, 4, 8 loopback ranks against the numpy
definition — output, every dW, da1, da2 and dX — at the small shape, the benchmark widths and on an R-MAT graph with hub rows; p = 1
against p = 8; score "dot" bit-identical before and after a round trip through "additive" and with or without the new argument; SGD on
W, a1 and a2.

Bounds: 1e-12 for the forward kernel (the bound of test_gat_softmax_gpu.py), 1e-10 for the backward kernels and the operator (the bound
the fused backward asserts with softmax).  The observed worst cases are recorded with T.record_observed.

Observed on an MI355X (max |x - ref| / max |ref| per matrix): forward kernel <= 2.3e-14 over every width, both alignments and |z| = 800
(<= 3.9e-16 at ordinary scores); backward kernels <= 4.6e-15; the operator (worst of the output, dW, da1, da2 of every (layer, head) and dX)
<= 1.3e-14 on er8_r16 over p = 1 .. 8, <= 3.7e-14 at the benchmark widths, <= 4.9e-15 on the R-MAT graph; p = 8 against p = 1 <= 1.1e-14."""
import ctypes as C

import numpy as np
import pytest

import gat_additive_ref as R
import gat_softmax_ref as RS
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from oracle import oracle as O
from test_gat_fused_backward_gpu import graph, mixed_degrees

pytestmark = pytest.mark.gpu
FTOL = 1e-12  # forward kernel against the extended-precision reference
TOL = 1e-10   # backward kernels, operator
ALPHA = T.GAT_ALPHA
WIDTHS = [1, 2, 7, 16, 64, 100, 128, 256]
NWIN = 6
GROUPINGS = {"whole": None, "one call per window": [(q, q + 1) for q in range(NWIN)], "uneven a": [(0, 1), (1, 4), (4, 6)],
             "uneven b": [(0, 3), (3, 4), (4, 5), (5, 6)]}
FWD, ROW, COL = 0, 1, 2
PASS_NAMES = {FWD: "fwd", ROW: "row", COL: "col"}


@pytest.fixture(autouse=True, scope="module")
def hip_backend():
    assert H.load_backend(None) == "hip-gfx950"
    yield


@pytest.fixture(scope="module")
def ctx():
    c = K.Ctx(0)
    assert K.load().hnh_backend_name() == b"hip-gfx950"
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ kernels
class Problem:
    """One pass's operands on the device, with pitches wider than the widths and guards round every output: run() launches the pass
    (whole block, or one call per window group) and returns its outputs.  odd=True puts the output block (the ReLU destination of the
    forward pass, dAgg of the column pass) at an odd column offset of an odd pitch and dZ at an odd pitch: the 8-byte instances.
    big > 0 scales a1, a2 so that |z| reaches about `big`."""

    def __init__(self, ctx, pas, f, m=2048, ncols=1536, seed=0, odd=False, big=0.0, degrees=None):
        self.ctx, self.pas, self.f, self.m, self.ncols, self.odd = ctx, pas, f, m, ncols, odd
        fp = self.fp = f + (f & 1)
        rng = np.random.default_rng(1000 * f + seed + 17 * pas)
        deg = mixed_degrees(m, seed + f) if degrees is None else degrees
        self.rowptr, self.colidx, self.rows = graph(m, ncols, deg, seed + 1)
        rows, cols = self.rows, self.colidx.astype(np.int64)
        a1, a2 = rng.standard_normal(f) / np.sqrt(f), rng.standard_normal(f) / np.sqrt(f)
        a_rows, a_cols = rng.uniform(-1, 1, (m, f)), rng.uniform(-1, 1, (ncols, f))
        if big:
            z0 = ((a_cols @ a1)[cols] + (a_rows @ a2)[rows]) if pas == COL else ((a_rows @ a1)[rows] + (a_cols @ a2)[cols])
            scale = big / np.abs(z0).max()  # (z is linear in (a1, a2))
            a1, a2 = a1 * scale, a2 * scale
        self.a1, self.a2 = a1, a2
        self.ld_m, self.ld_y = fp + 4, (fp + 2 if pas != COL else fp + 4) + 4
        # S-row side and S-column side of the scores: for FWD / ROW the block's rows are S rows (s_i) and the gathered rows S columns
        # (t_j); for COL the block's rows are S columns (t_j) and the gathered rows S rows (s_i, lse_i, delta_i)
        self.m_rows = R.scored(a_rows, a1, a2, ld=self.ld_m)
        m_cols = R.scored(a_cols, a1, a2, ld=self.ld_y)
        s_nz = (m_cols[cols, fp] + self.m_rows[rows, fp + 1]) if pas == COL else (self.m_rows[rows, fp] + m_cols[cols, fp + 1])
        self.z = s_nz
        owner, n_own = (cols, ncols) if pas == COL else (rows, m)
        _, lse = RS.row_softmax(owner, n_own, RS.leaky(s_nz, ALPHA))
        self.lse_in = lse
        self.delta = rng.uniform(-1, 1, n_own)
        self.ld_dz = f + (3 if odd else 2 + (f & 1))
        self.dz = rng.uniform(-1, 1, (m, self.ld_dz))
        if pas == COL:
            self.dz_cols = rng.uniform(-1, 1, (ncols, f))
            self.y = R.pack(self.dz_cols, m_cols[:, fp], lse, self.delta, ld=self.ld_y)
        else:
            self.y = m_cols
        self.y = np.where(np.isnan(self.y), 1e300, self.y)       # beyond the gathered width: never read
        self.m_rows = np.where(np.isnan(self.m_rows), 1e300, self.m_rows)
        # outputs: a matrix of m + 1 rows whose block [col0, col0 + f) is the pass's, everything else a guard
        self.col0 = 3 if odd else 2
        self.ld_out = self.col0 + f + (4 if (self.col0 + f) % 2 == 0 else 3) + (1 if odd else 0)
        if not odd:
            assert self.ld_out % 2 == 0
        self.out0 = rng.uniform(-1, 1, (m + 1, self.ld_out))
        self.vec0 = rng.uniform(-1, 1, (m + 1, 2))
        self.state0 = rng.uniform(1, 2, (4, m + 1))  # row_max, row_sum, lse, (unused)
        self.acc0 = rng.uniform(-1, 1, (m + 1, fp + 2))  # the forward pass's running accumulator (scratch of the pass)
        host = dict(rowptr=self.rowptr, colidx=np.concatenate([self.colidx, [0]]).astype(np.int32), m_rows=self.m_rows, dz=self.dz, y=self.y,
                    out=self.out0, vec=self.vec0, state=self.state0, acc=self.acc0, lse_in=self.lse_in if pas == ROW else np.zeros(1),
                    delta=self.delta if pas == ROW else np.zeros(1))
        self.d = {k: ctx.upload(v) for k, v in host.items()}
        self.split = None

    def args(self):
        d, m, f = self.d, self.m, self.f
        a = K.AttnAdd()
        a.M, a.ld_m, a.Y, a.ld_y, a.f, a.leaky_alpha = d["m_rows"].ptr, self.ld_m, d["y"].ptr, self.ld_y, f, ALPHA
        if self.pas == FWD:
            a.Out, a.ld_out = d["acc"].ptr, self.fp + 2
            a.row_max, a.row_sum, a.lse = d["state"].ptr, d["state"].ptr + 8 * (m + 1), d["state"].ptr + 16 * (m + 1)
            a.relu_dst, a.relu_ld = d["out"].ptr + 8 * self.col0, self.ld_out
        elif self.pas == ROW:
            a.dZ, a.ld_dz, a.lse, a.delta = d["dz"].ptr, self.ld_dz, d["lse_in"].ptr, d["delta"].ptr
            a.vec, a.ld_vec = d["vec"].ptr, 2
        else:
            a.Out, a.ld_out = d["out"].ptr + 8 * self.col0, self.ld_out
            a.vec, a.ld_vec = d["vec"].ptr + 8, 2
        return a

    def block(self):
        return K.CsrBlock(self.m, int(self.rowptr[-1]), self.ncols, int(np.diff(self.rowptr).max()), 0, self.d["rowptr"].ptr, self.d["colidx"].ptr, None)

    def fn(self):
        lib = self.ctx.lib
        return (lib.hnh_attn_add_fwd_csr_p, lib.hnh_attn_add_row_csr_p, lib.hnh_attn_add_col_csr_p)[self.pas]

    def run(self, overwrite=True, groups=None):
        """Returns dict(out=block rows x f, vec=rows, lse=rows, state=(max, sum)) as far as the pass writes them; checks the guards."""
        ctx, lib, m, f = self.ctx, self.ctx.lib, self.m, self.f
        for k, v in (("out", self.out0), ("vec", self.vec0), ("state", self.state0), ("acc", self.acc0)):
            self.d[k].set(v)
        a, blk = self.args(), self.block()
        first = K.FUSED_OUT_OVERWRITE if (overwrite or self.pas == FWD) else 0
        finish = K.ATTN_FINISH if self.pas == FWD else 0
        if groups is None:
            ctx.check(self.fn()(ctx.h, C.byref(blk), C.byref(a), first | finish, None, K.STREAM_COMPUTE), "additive pass")
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
                ctx.check(self.fn()(ctx.h, C.byref(blk), C.byref(a), fl, C.byref(win), K.STREAM_COMPUTE), "additive window")
        ctx.sync()
        out, vec, state = self.d["out"].get(), self.d["vec"].get(), self.d["state"].get()
        c0 = self.col0
        res = {}
        if self.pas != ROW:
            assert np.array_equal(out[:, :c0], self.out0[:, :c0]) and np.array_equal(out[:, c0 + f:], self.out0[:, c0 + f:]), "guard columns are not written"
            assert np.array_equal(out[m], self.out0[m]), "the row past the last one is not written"
            res["out"] = out[:m, c0:c0 + f]
        else:
            assert np.array_equal(out, self.out0)
        if self.pas == FWD:
            assert np.array_equal(vec, self.vec0) and np.array_equal(state[:, m], self.state0[:, m]) and np.array_equal(state[3], self.state0[3])
            res["lse"], res["state"] = state[2, :m], state[:2, :m]
        else:
            col = 0 if self.pas == ROW else 1
            assert np.array_equal(vec[:, 1 - col], self.vec0[:, 1 - col]) and np.array_equal(vec[m], self.vec0[m]), "the other scalar column is not written"
            assert np.array_equal(state, self.state0)
            res["vec"] = vec[:m, col]
        return res

    def want(self, overwrite=True):
        f, m, cols = self.f, self.m, self.colidx.astype(np.int64)
        if self.pas == FWD:
            o, lse = R.fwd_pass_ld(self.rows, cols, m, self.m_rows, self.y, f, ALPHA)
            return dict(out=np.maximum(o, 0), lse=lse)
        if self.pas == ROW:
            ds = R.row_pass(self.rows, cols, m, self.dz[:, :f], self.m_rows, self.lse_in, self.delta, self.y, f, ALPHA)
            return dict(vec=ds + (0 if overwrite else self.vec0[:m, 0]))
        dagg, dt = R.col_pass(self.rows, cols, m, self.m_rows, self.y, f, ALPHA)
        if not overwrite:
            dagg, dt = dagg + self.out0[:m, self.col0:self.col0 + f], dt + self.vec0[:m, 1]
        return dict(out=dagg, vec=dt)

    def free(self):
        for v in self.d.values():
            v.free()
        if self.split is not None:
            self.split.free()


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def errors(got, want):
    return {k: float(T.rel(np.asarray(got[k], dtype=np.longdouble), want[k])) for k in want}


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd-offset"])
@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_pass_vs_numpy(ctx, pas, f, odd):
    """Against numpy (extended precision for the forward pass), guards untouched, rows without nonzeros zero, a repeat bit-identical,
    accumulate on top of overwrite for the backward passes."""
    p = Problem(ctx, pas, f, odd=odd)
    deg = np.diff(p.rowptr)
    assert deg.max() >= 1500 and np.count_nonzero(deg == 0) > 100 and np.count_nonzero((deg >= 200) & (deg <= 300)) > 5 and 600 in deg
    got, want = p.run(True), p.want(True)
    empty = deg == 0
    for k in got:
        if k != "state":
            assert np.all(got[k][empty] == 0.0), "rows without nonzeros: o = 0, lse = 0, sums = 0"
    assert all(np.abs(np.float64(v)).max() > 0 for v in want.values())
    errs = errors(got, want)
    assert same(p.run(True), got), "a repeat must be bit-identical"
    if pas != FWD:
        acc = p.run(False)
        errs.update({"acc " + k: v for k, v in errors(acc, p.want(False)).items()})
        assert np.array_equal(acc["vec"][empty], p.vec0[:p.m, 0 if pas == ROW else 1][empty]), "accumulating leaves rows without nonzeros alone"
    p.free()
    T.record_observed("gat_additive_kernel", case="%s f=%d%s" % (PASS_NAMES[pas], f, " odd" if odd else ""), worst=max(errs.values()))
    print("observed", PASS_NAMES[pas], f, odd, errs)
    assert max(errs.values()) <= (FTOL if pas == FWD else TOL), errs


@pytest.mark.parametrize("f", [7, 64, 256])
@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_scores_far_outside_exps_range(ctx, pas, f):
    p = Problem(ctx, pas, f, seed=2, big=800.0)
    assert np.abs(p.z).max() > 790.0
    got, want = p.run(True), p.want(True)
    for k, v in got.items():  # (the running max of a row without nonzeros is -inf by definition: the empty state)
        assert np.all(np.isfinite(v)) or (k == "state" and np.all(np.isfinite(v[1])) and np.all(np.isneginf(v[0][~np.isfinite(v[0])]))), k
    errs = errors(got, want)
    p.free()
    T.record_observed("gat_additive_kernel", case="%s f=%d |z|=800" % (PASS_NAMES[pas], f), worst=max(errs.values()))
    print("observed big", PASS_NAMES[pas], f, errs)
    assert max(errs.values()) <= (FTOL if pas == FWD else TOL), errs


@pytest.mark.parametrize("f", [7, 64, 100, 128, 256])
@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_grouping_independence(ctx, pas, f):
    """Whole rows, one call per window and two uneven groupings of six windows: the same bits (forward output, lse and the row state;
    ds; dt and dAgg), overwriting and accumulating, because every launch continues the row's state nonzero by nonzero."""
    p = Problem(ctx, pas, f, seed=3)
    for overwrite in ((True,) if pas == FWD else (True, False)):
        whole = p.run(overwrite)
        for name, groups in GROUPINGS.items():
            assert same(p.run(overwrite, groups), whole), (name, overwrite)
    p.free()


@pytest.mark.parametrize("f", [7, 64, 128, 256])
@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_forced_panels_are_bit_identical(monkeypatch, pas, f):
    """Column panels (several launches over every row, hub rows after the last): the same bits as one launch."""
    ncols = 1536
    c1 = K.Ctx(0)
    p1 = Problem(c1, pas, f, seed=5)
    one, want = p1.run(True), p1.want(True)
    p1.free()
    c1.close()
    gather_w = R.packed_width(f) if pas == COL else R.scored_width(f)
    monkeypatch.setenv("HNH_PANEL_BYTES", str(ncols * gather_w * 8 / 5))
    monkeypatch.setenv("HNH_MAX_PANELS", "8")
    monkeypatch.setenv("HNH_PANELS_WITH_HUBS", "1")
    c5 = K.Ctx(0)
    p5 = Problem(c5, pas, f, seed=5)
    assert c5.lib.hnh_panel_count(c5.h, p5.m, int(p5.rowptr[-1]), ncols, gather_w, int(np.diff(p5.rowptr).max())) == 5
    five = p5.run(True)
    p5.free()
    c5.close()
    assert same(one, five)
    assert max(errors(five, want).values()) <= (FTOL if pas == FWD else TOL)


def test_dense_helpers(ctx):
    lib = ctx.lib
    rng = np.random.default_rng(4)
    for f in WIDTHS + [33, 255]:
        rows, fp = 301, f + (f & 1)
        ld_a, ld_m, ld_q, ld_dz, ld_da, col0 = f + 3, fp + 4, fp + 6, f + 5, 2 * f + 7, 3
        a, dz, dagg = rng.uniform(-1, 1, (rows, ld_a)), rng.uniform(-1, 1, (rows, ld_dz)), rng.uniform(-1, 1, (rows, f))
        a1, a2 = rng.uniform(-1, 1, f), rng.uniform(-1, 1, f)
        lse, delta, dd = rng.uniform(0, 3, rows), rng.uniform(-1, 1, rows), rng.uniform(-1, 1, (rows, 2))
        dev = {k: ctx.upload(v) for k, v in dict(a=a, dz=dz, dagg=dagg, a1=a1, a2=a2, lse=lse, delta=delta, dd=dd, m=np.full((rows + 1, ld_m), 7.0),
                                                 q=np.full((rows + 1, ld_q), 7.0), da=np.full((rows + 1, ld_da), 7.0)).items()}
        ctx.check(lib.hnh_attn_add_scores_f64(ctx.h, dev["m"].ptr, ld_m, dev["a"].ptr, ld_a, dev["a1"].ptr, dev["a2"].ptr, rows, f, K.STREAM_COMPUTE), "scores")
        ctx.check(lib.hnh_attn_add_pack_f64(ctx.h, dev["q"].ptr, ld_q, dev["dz"].ptr, ld_dz, dev["m"].ptr, ld_m, dev["lse"].ptr, dev["delta"].ptr, rows, f,
                                            K.STREAM_COMPUTE), "pack")
        ctx.check(lib.hnh_attn_add_update_f64(ctx.h, dev["da"].ptr, ld_da, col0, dev["dagg"].ptr, f, dev["dd"].ptr, 2, dev["a1"].ptr, dev["a2"].ptr, rows, f,
                                              K.STREAM_COMPUTE), "update")
        gm, gq, gda = dev["m"].get(), dev["q"].get(), dev["da"].get()
        wm = R.scored(a[:, :f], a1, a2)
        assert np.array_equal(gm[:rows, :fp], wm[:, :fp]) and T.rel(gm[:rows, fp:fp + 2], wm[:, fp:]) <= T.TOL, f
        assert np.all(gm[:rows, fp + 2:] == 7.0) and np.all(gm[rows] == 7.0)
        wq = R.pack(dz[:, :f], gm[:rows, fp], lse, delta)
        assert np.array_equal(gq[:rows, :fp + 4], wq) and np.all(gq[:rows, fp + 4:] == 7.0) and np.all(gq[rows] == 7.0), f
        wda = dagg + np.outer(dd[:, 0], a1) + np.outer(dd[:, 1], a2)
        assert T.rel(gda[:rows, col0:col0 + f], wda) <= T.TOL
        assert np.all(gda[:rows, :col0] == 7.0) and np.all(gda[:rows, col0 + f:] == 7.0) and np.all(gda[rows] == 7.0)
        assert lib.hnh_attn_add_scores_f64(ctx.h, dev["m"].ptr, ld_m + 1, dev["a"].ptr, ld_a, dev["a1"].ptr, dev["a2"].ptr, rows, f, K.STREAM_COMPUTE) == 1
        for d in dev.values():
            d.free()


@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_wide_heads_are_refused_and_write_nothing(ctx, pas):
    for f in (257, 320):
        p = Problem(ctx, pas, f, m=128, ncols=96, degrees=np.full(128, 3))
        a, blk = p.args(), p.block()
        assert p.fn()(ctx.h, C.byref(blk), C.byref(a), K.FUSED_OUT_OVERWRITE, None, K.STREAM_COMPUTE) == K.ERR_UNSUPPORTED
        assert b"256" in ctx.lib.hnh_last_error(ctx.h)
        ctx.sync()
        assert np.array_equal(p.d["out"].get(), p.out0) and np.array_equal(p.d["vec"].get(), p.vec0) and np.array_equal(p.d["state"].get(), p.state0)
        assert p.fn()(ctx.h, C.byref(blk), C.byref(a), 4, None, K.STREAM_COMPUTE) == 1  # (an unknown flag, at any width)
        p.free()


@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_empty_block(ctx, pas):
    """rowptr == NULL: overwrite (and the forward finish) leave zeros in the pass's outputs, accumulate leaves everything alone."""
    f = 33
    p = Problem(ctx, pas, f, m=256, ncols=96, degrees=np.full(256, 2))
    a = p.args()
    none = K.CsrBlock(p.m, 0, -1, 0, 0, None, None, None)
    ctx.check(p.fn()(ctx.h, C.byref(none), C.byref(a), 0, None, K.STREAM_COMPUTE), "empty block, accumulate")
    ctx.sync()
    assert np.array_equal(p.d["out"].get(), p.out0) and np.array_equal(p.d["vec"].get(), p.vec0) and np.array_equal(p.d["state"].get(), p.state0)
    fl = K.FUSED_OUT_OVERWRITE | (K.ATTN_FINISH if pas == FWD else 0)
    ctx.check(p.fn()(ctx.h, C.byref(none), C.byref(a), fl, None, K.STREAM_COMPUTE), "empty block, overwrite")
    ctx.sync()
    out, vec, state = p.d["out"].get(), p.d["vec"].get(), p.d["state"].get()
    c0 = p.col0
    if pas != ROW:
        assert np.all(out[:p.m, c0:c0 + f] == 0.0) and np.array_equal(out[:, c0 + f:], p.out0[:, c0 + f:]) and np.array_equal(out[p.m], p.out0[p.m])
    if pas == FWD:
        assert np.all(state[2, :p.m] == 0.0) and np.all(state[1, :p.m] == 0.0) and np.all(np.isneginf(state[0, :p.m]))
    else:
        col = 0 if pas == ROW else 1
        assert np.all(vec[:p.m, col] == 0.0) and np.array_equal(vec[:, 1 - col], p.vec0[:, 1 - col])
    p.free()


# ------------------------------------------------------------------------------------------------ the operator
def hashed_weights(layers):
    return {(li, h): O.gat_weight(li, h, fin, fph) for li, (fin, fph, heads) in enumerate(layers) for h in range(heads)}


def setup(world, rows, cols, m, x, layers, weights, vectors, g_glob=None, **kw):
    sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
    d = H.DistributedSparse(world, "15d_fusion2", sp, layers[0][0], 1)
    gnn = H.GAT(d, layers, ALPHA, **kw)
    for k, w in weights.items():
        gnn.set_weight(*k, w)
    if vectors is not None:
        for k, (a1, a2) in vectors.items():
            gnn.set_attention_vectors(*k, a1, a2)
    d.setRValue(layers[0][0])
    subB = d.submatrices(H.BMAT)
    d.setRValue(layers[-1][1] * layers[-1][2])
    subA = d.submatrices(H.AMAT)
    x_d = H.Dense.create(world, *gnn.buffer_shape(0))
    x_d.upload(T.fill_local(subB, x_d.shape, x))
    g = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
    if g_glob is not None:
        g.upload(T.fill_local(subA, g.shape, g_glob))
    out = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
    dx = H.Dense.create(world, *gnn.buffer_shape(0))
    gnn.set_input(x_d)
    return dict(sp=sp, d=d, gnn=gnn, x=x_d, g=g, out=out, dx=dx, subA=subA, subB=subB)


def one_round(s, weights, additive):
    gnn = s["gnn"]
    gnn.forwardPass()
    gnn.get_output(s["out"])
    out = s["out"].download()
    gnn.backwardPass(s["g"])
    gnn.get_input_grad(s["dx"])
    r = dict(out=out, dx=s["dx"].download(), dw={k: gnn.weight_grad(*k) for k in weights})
    if additive:
        r["da"] = {k: gnn.attention_grad(*k) for k in weights}
    return r


def teardown(s):
    for k in ("x", "g", "out", "dx", "gnn", "d", "sp"):
        s[k].free()


def run_additive(world, rows, cols, m, x, layers, weights, vectors, g_glob, rounds=1):
    s = setup(world, rows, cols, m, x, layers, weights, vectors, g_glob, attention="softmax", score="additive")
    res = dict(subA=s["subA"], subB=s["subB"], rounds=[one_round(s, weights, True) for _ in range(rounds)])
    teardown(s)
    return res


def assembled(per_rank, k, m, layers):
    """The global output and dX of round k, and rank 0's replicated gradients (asserted equal on every rank)."""
    r0 = per_rank[0]["rounds"][k]
    for pr in per_rank:
        for key in r0["dw"]:
            assert np.array_equal(pr["rounds"][k]["dw"][key], r0["dw"][key]), "dW must be equal on every rank"
            assert all(np.array_equal(pr["rounds"][k]["da"][key][i], r0["da"][key][i]) for i in (0, 1)), "da1, da2 must be equal on every rank"
    hf = layers[-1][1] * layers[-1][2]
    out = T.assemble_dense([dict(o=pr["rounds"][k]["out"], subA=pr["subA"]) for pr in per_rank], "o", "subA", m, hf)
    dx = T.assemble_dense([dict(dx=pr["rounds"][k]["dx"], subB=pr["subB"]) for pr in per_rank], "dx", "subB", m, layers[0][0])
    return dict(out=out, dx=dx, dw=r0["dw"], da=r0["da"])


def check_against(got, want_out, want_dw, want_da, want_dx, label, ranks):
    errs = {"out": T.rel(got["out"], want_out), "dx": T.rel(got["dx"], want_dx)}
    for key in want_dw:
        assert np.abs(want_dw[key]).max() > 0 and np.abs(want_da[key][0]).max() > 0 and np.abs(want_da[key][1]).max() > 0
        errs[("dw",) + key] = T.rel(got["dw"][key], want_dw[key])
        errs[("da1",) + key] = T.rel(got["da"][key][0], want_da[key][0])
        errs[("da2",) + key] = T.rel(got["da"][key][1], want_da[key][1])
    worst = max(errs.values())
    T.record_observed("gat_additive", case=label, ranks=ranks, worst=worst)
    print("observed", label, ranks, "worst %.2e" % worst, "out %.2e dx %.2e" % (errs["out"], errs["dx"]))
    assert worst <= TOL, errs


def reference(rows, cols, m, x, layers, w, av, g):
    out = R.forward(rows, cols, m, x, layers, ALPHA, w, av)
    dw, da, dx = R.backward(rows, cols, m, x, layers, ALPHA, g, w, av)
    return out, dw, da, dx


def er8():
    case = T.case_inputs("er8_r16")
    return case["rows"], case["cols"], case["M"], case["A"] * T.GAT_INPUT_SCALE


ER8_RESULTS = {}


@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_additive_er8(p):
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w, av = hashed_weights(layers), R.vectors_of(layers)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 9) * 16.0
    per_rank = H.run_spmd(p, lambda wd: run_additive(wd, rows, cols, m, x, layers, w, av, g, rounds=2))
    got = assembled(per_rank, 0, m, layers)
    check_against(got, *reference(rows, cols, m, x, layers, w, av, g), "er8_r16 p%d" % p, p)
    again = assembled(per_rank, 1, m, layers)
    assert np.array_equal(got["out"], again["out"]) and np.array_equal(got["dx"], again["dx"]), "two rounds must be bit-identical"
    assert all(np.array_equal(got["dw"][k], again["dw"][k]) and np.array_equal(got["da"][k][0], again["da"][k][0]) for k in w)
    ER8_RESULTS[p] = got


def test_one_rank_and_eight_ranks_agree():
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w, av = hashed_weights(layers), R.vectors_of(layers)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 9) * 16.0
    res = {}
    for p in (1, 8):
        res[p] = ER8_RESULTS.get(p) or assembled(H.run_spmd(p, lambda wd: run_additive(wd, rows, cols, m, x, layers, w, av, g)), 0, m, layers)
    a, b = res[1], res[8]
    check_against(b, a["out"], a["dw"], a["da"], a["dx"], "er8_r16 p8 against p1", 8)


WIDE = {"benchmark widths": (1 << 12, [(256, 256, 1), (256, 128, 2), (256, 64, 3)]), "odd heads": (1 << 11, [(24, 33, 2), (66, 7, 3)])}


@pytest.mark.parametrize("p", [1, 4])
@pytest.mark.parametrize("shape", sorted(WIDE))
def test_additive_widths(shape, p):
    m, layers = WIDE[shape]
    rows, cols = H.generate_er(m, m, m * 16, 77)
    x = O.dense_fill(m, layers[0][0], 41) * 16.0
    w, av = hashed_weights(layers), R.vectors_of(layers, seed=5)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 3) * 64.0
    per_rank = H.run_spmd(p, lambda wd: run_additive(wd, rows, cols, m, x, layers, w, av, g))
    check_against(assembled(per_rank, 0, m, layers), *reference(rows, cols, m, x, layers, w, av, g), "%s p%d" % (shape, p), p)


@pytest.mark.parametrize("p", [1, 4])
def test_additive_rmat_hub_rows(p):
    m, layers = 1 << 13, [(64, 64, 2), (128, 32, 2)]
    rows, cols = H.generate_rmat(13, m * 16)
    assert np.bincount(rows, minlength=m).max() >= 512 and np.bincount(cols, minlength=m).max() >= 512
    x = O.dense_fill(m, 64, 8) * 8.0
    w, av = hashed_weights(layers), R.vectors_of(layers, seed=6)
    g = O.dense_fill(m, 64, 4) * 32.0
    per_rank = H.run_spmd(p, lambda wd: run_additive(wd, rows, cols, m, x, layers, w, av, g, rounds=2))
    got = assembled(per_rank, 0, m, layers)
    check_against(got, *reference(rows, cols, m, x, layers, w, av, g), "rmat hubs p%d" % p, p)
    again = assembled(per_rank, 1, m, layers)
    assert np.array_equal(got["dx"], again["dx"]) and all(np.array_equal(got["da"][k][1], again["da"][k][1]) for k in w), "a repeat must be bit-identical"


@pytest.mark.parametrize("backward", ["unfused", "fused"])
@pytest.mark.parametrize("p", [1, 4])
def test_score_dot_is_untouched_by_a_round_trip(p, backward):
    """dot -> additive -> dot on one object: the dot-product results are bit-identical before and after, and equal those of a GAT built
    without the new argument."""
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w, av = hashed_weights(layers), R.vectors_of(layers)
    g = O.dense_fill(m, 12, 9) * 16.0

    def trip(world):
        s = setup(world, rows, cols, m, x, layers, w, None, g, attention="softmax", backward=backward, score="dot")
        before = one_round(s, w, False)
        s["gnn"].set_score("additive")
        for k, (a1, a2) in av.items():
            s["gnn"].set_attention_vectors(*k, a1, a2)
        with pytest.raises(H.HnhError, match="forwardPass"):
            s["gnn"].backwardPass(s["g"])  # a change of score invalidates the stored forward pass
        mid = one_round(s, w, True)
        s["gnn"].set_score("dot")
        after = one_round(s, w, False)
        teardown(s)
        return before, mid, after

    def plain(world):
        s = setup(world, rows, cols, m, x, layers, w, None, g, attention="softmax", backward=backward)
        r = one_round(s, w, False)
        teardown(s)
        return r

    for (before, mid, after), old in zip(H.run_spmd(p, trip), H.run_spmd(p, plain)):
        for a in (after, old):
            assert np.array_equal(before["out"], a["out"]) and np.array_equal(before["dx"], a["dx"])
            assert all(np.array_equal(before["dw"][k], a["dw"][k]) for k in w)
        assert not np.array_equal(mid["out"], before["out"]), "the additive round computed something else"


SCHEDULE_NAMES = {"15d_sparse": "1.5D Sparse Shifting", "25d_dense_replicate": "2.5D Cannon's Algorithm Replicating Dense",
                  "15d_fusion1": "15d_fusion1", "15d_fusion2": "15d_fusion2"}


@pytest.mark.parametrize("alg,p,c,layers,attention,words", [
    ("15d_fusion1", 4, 2, [(16, 8, 2)], "softmax", None), ("15d_fusion2", 4, 2, [(16, 8, 2)], "softmax", None),
    ("15d_sparse", 2, 1, [(16, 8, 2)], "softmax", None), ("25d_dense_replicate", 4, 1, [(16, 8, 2)], "softmax", None),
    ("15d_fusion2", 2, 1, [(16, 8, 2)], "none", "attention mode softmax only"), ("15d_fusion2", 2, 1, [(16, 257, 1)], "softmax", "at most 256 features, not 257")])
def test_refusals_leave_nothing_in_flight(alg, p, c, layers, attention, words):
    rows, cols, m, _ = er8()
    words = "score additive.*" + (words or "%s.*c = %d" % (SCHEDULE_NAMES[alg], c))

    def rank(world):
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, alg, sp, 16, c)
        gnn = H.GAT(d, layers, ALPHA, attention=attention, score="additive")
        g = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
        with pytest.raises(H.HnhError, match=words):
            gnn.forwardPass()
        with pytest.raises(H.HnhError, match=words):
            gnn.backwardPass(g)
        world.sync()  # nothing was left in flight
        with pytest.raises(ValueError):
            gnn.set_score("bilinear")
        assert H.lib().hnh_gat_set_score(gnn.h, 7) != 0
        for h in (g, gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(p, rank))


def sgd(world, rows, cols, m, x, layers, target, steps, lr_scale):
    w, av = hashed_weights(layers), R.vectors_of(layers)
    s = setup(world, rows, cols, m, x, layers, w, av, None, attention="softmax", score="additive")
    gnn = s["gnn"]
    tgt = T.fill_local(s["subA"], gnn.buffer_shape(len(layers)), target)
    losses, lr = [], None
    for step in range(steps + 1):
        gnn.forwardPass()
        gnn.get_output(s["out"])
        diff = s["out"].download() - tgt
        losses.append(0.5 * float(np.sum(diff * diff)))
        if step == steps:
            break
        s["g"].upload(diff)
        gnn.backwardPass(s["g"])
        dw = {k: gnn.weight_grad(*k) for k in w}
        da = {k: gnn.attention_grad(*k) for k in w}
        if lr is None:  # the same on every rank: the gradients are replicated
            lr = R.sgd_step_size(lr_scale, w, av, dw, da)
        for k in w:
            w[k] = w[k] - lr * dw[k]
            av[k] = (av[k][0] - lr * da[k][0], av[k][1] - lr * da[k][1])
            gnn.set_weight(*k, w[k])
            gnn.set_attention_vectors(*k, *av[k])
    teardown(s)
    return losses, av


@pytest.mark.parametrize("p", [1, 4])
def test_sgd_lowers_the_loss(p):
    """Five steps on W, a1 and a2 with the step size of tests/test_gat_additive_cpu.py::test_the_reference_trains."""
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    target = O.dense_fill(m, 12, 21) * R.SGD_TARGET_SCALE
    per_rank = H.run_spmd(p, lambda wd: sgd(wd, rows, cols, m, x, layers, target, R.SGD_STEPS, R.SGD_LR_SCALE))
    loss = np.sum(np.array([pr[0] for pr in per_rank]), axis=0)
    print("losses", loss)
    assert all(loss[i + 1] < loss[i] for i in range(R.SGD_STEPS)), loss
    start = R.vectors_of(layers)
    for _, av in per_rank:
        assert all(np.abs(av[k][i] - start[k][i]).max() > 0 for k in start for i in (0, 1)), "a1 and a2 have moved"
