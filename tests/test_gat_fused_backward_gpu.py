"""The GAT's fused backward mode on the GPU (include/hnh_attn_grad.h, GAT backward mode "fused").

Kernel level, through ctypes: the row pass, the column pass and the pack kernel against numpy (tests/gat_pass_ref.py) at
every kind of width, on blocks with empty rows, hub rows and repeated pairs, with leading dimensions wider than the widths and guard
values around the output; their independence of how a row's nonzeros are split into launches (forced panels, every grouping of six
windows); overwrite against accumulate; the width limit; empty blocks.
Operator level: GAT(..., backward="fused") on 15d_fusion2, c = 1 over loopback ranks against the numpy definition
(tests/gat_ref.py) and against the un-fused pass of the same object, determinism, mode switches,
SGD, and the refusals.

Bounds: T.TOL = 1e-11 for the kernels with attention none (summation order only), 1e-10 with softmax (the bound of the softmax tests)
and for the operator (the TOL of test_gat_backward_gpu.py).  The observed worst cases are recorded with T.record_observed.

Observed on an MI355X (max |x - ref| / max |ref| per matrix): kernels <= 3.9e-15 with attention none, <= 6.2e-15 with softmax, over every
width and the R-MAT graph; the operator (worst of dW of every (layer, head) and dX, p = 1 .. 8) <= 3.8e-15 with attention none,
<= 1.8e-15 with softmax; fused against un-fused on the same object <= 9.7e-16."""
import ctypes as C
import itertools

import numpy as np
import pytest

import gat_gpu_harness as G
import gat_pass_ref as P
import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import ALPHA, NWIN, TOL, ctx, er8, graph, hashed_weights, hip_backend, mixed_degrees  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu
KTOL = {False: T.TOL, True: 1e-10}  # kernel level, by softmax
WIDTHS = [1, 7, 8, 16, 33, 64, 100, 101, 128, 200, 255, 256]


# ------------------------------------------------------------------------------------------------ kernels
class Problem:
    """One pass's operands on the device, with pitches wider than the widths and guards round the output: run() launches the pass
    (whole block, or one call per window group) and returns the output rows."""

    def __init__(self, ctx, column_side, softmax, f, m=2048, ncols=1536, seed=0, pad=None, degrees=None):
        self.ctx, self.column_side, self.softmax, self.f, self.m, self.ncols = ctx, column_side, softmax, f, m, ncols
        rng = np.random.default_rng(1000 * f + seed)
        deg = mixed_degrees(m, seed + f) if degrees is None else degrees
        self.rowptr, self.colidx, self.rows = graph(m, ncols, deg, seed + 1)
        cols = self.colidx.astype(np.int64)
        pad = (2 if f % 2 == 0 else 3) if pad is None else pad  # (even widths keep even pitches: the 16-byte instances)
        self.ld_x, self.ld_dz, self.ld_out = f + pad, f + 2 * pad, f + 3 * pad
        scale = 1.0 / np.sqrt(np.sqrt(f))  # scores of order one at every width
        self.x = rng.uniform(-1, 1, (m, self.ld_x)) * scale
        self.dz = rng.uniform(-1, 1, (m, self.ld_dz))
        self.a_cols = rng.uniform(-1, 1, (ncols, f)) * scale   # the gathered rows' A
        self.dz_cols = rng.uniform(-1, 1, (ncols, f))           # ... and dZ (column pass)
        e = np.einsum("ij,ij->i", self.x[self.rows, :f], self.a_cols[cols])
        s = R.leaky(e, ALPHA)
        self.lse = self.delta = None
        if softmax:  # a real log-sum-exp over the nonzeros that share the scalar (rows of S: the pass's rows / the gathered rows)
            owner, n_own = (cols, ncols) if column_side else (self.rows, m)
            _, self.lse = R.row_softmax(owner, n_own, s)
            self.delta = rng.uniform(-1, 1, n_own)
        if column_side:
            self.ld_y = P.fused_packed_width(f, softmax) + 4
            self.y = P.fused_pack(self.a_cols, self.dz_cols, self.lse, self.delta, ld=self.ld_y)
            self.y[np.isnan(self.y)] = 1e300  # beyond the packed width: never read
        else:
            self.ld_y = f + (4 if f % 2 == 0 else 5)
            self.y = np.full((ncols, self.ld_y), 1e300)
            self.y[:, :f] = self.a_cols
        self.out0 = rng.uniform(-1, 1, (m + 1, self.ld_out))
        self.d = {k: ctx.upload(v) for k, v in dict(rowptr=self.rowptr, colidx=np.concatenate([self.colidx, [0]]).astype(np.int32), x=self.x,
                                                   dz=self.dz, y=self.y, out=self.out0).items()}
        if softmax and not column_side:
            self.d["lse"], self.d["delta"] = ctx.upload(self.lse), ctx.upload(self.delta)
        self.split = None

    def args(self):
        d = self.d
        lse = d["lse"].ptr if "lse" in d else None
        delta = d["delta"].ptr if "delta" in d else None
        return K.AttnGrad(d["x"].ptr, self.ld_x, d["dz"].ptr, self.ld_dz, lse, delta, d["y"].ptr, self.ld_y, d["out"].ptr, self.ld_out, self.f,
                          int(self.softmax), ALPHA)

    def block(self):
        return K.CsrBlock(self.m, int(self.rowptr[-1]), self.ncols, int(np.diff(self.rowptr).max()), 0, self.d["rowptr"].ptr, self.d["colidx"].ptr, None)

    def fn(self):
        return self.ctx.lib.hnh_attn_grad_col_csr_p if self.column_side else self.ctx.lib.hnh_attn_grad_row_csr_p

    def run(self, overwrite=True, groups=None):
        ctx, lib, m = self.ctx, self.ctx.lib, self.m
        self.d["out"].set(self.out0)
        a, blk = self.args(), self.block()
        first = K.FUSED_OUT_OVERWRITE if overwrite else 0
        if groups is None:
            ctx.check(self.fn()(ctx.h, C.byref(blk), C.byref(a), first, None, K.STREAM_COMPUTE), "attn grad pass")
        else:
            if self.split is None:
                bounds = (C.c_int32 * (NWIN - 1))(*[int(self.ncols * (b + 1) / NWIN) for b in range(NWIN - 1)])
                self.split = K.DevArray(ctx, (NWIN - 1) * m, np.int32)
                ctx.check(lib.hnh_csr_window_bounds(ctx.h, m, self.d["rowptr"].ptr, self.d["colidx"].ptr, NWIN - 1, bounds, self.split.ptr,
                                                    K.STREAM_COMPUTE), "window bounds")
            sp = self.split.ptr
            for k, (w0, w1) in enumerate(groups):
                win = K.CsrWindow(None if w0 == 0 else sp + (w0 - 1) * m * 4, None if w1 == NWIN else sp + (w1 - 1) * m * 4, int(w1 == NWIN))
                ctx.check(self.fn()(ctx.h, C.byref(blk), C.byref(a), first if k == 0 else 0, C.byref(win), K.STREAM_COMPUTE), "attn grad window")
        ctx.sync()
        got = self.d["out"].get()
        assert np.array_equal(got[:, self.f:], self.out0[:, self.f:]), "columns beyond f are not written"
        assert np.array_equal(got[m], self.out0[m]), "the row past the last one is not written"
        return got[:m, :self.f]

    def want(self, overwrite=True):
        f, cols = self.f, self.colidx.astype(np.int64)
        out = np.zeros((self.m, f)) if overwrite else self.out0[:self.m, :f].copy()
        if self.column_side:
            return P.fused_col_pass(self.rows, cols, self.m, self.x[:, :f], self.y, f, self.softmax, ALPHA, out)
        return P.fused_row_pass(self.rows, cols, self.m, self.x[:, :f], self.dz[:, :f], self.y, ALPHA, self.lse, self.delta, out)

    def free(self):
        for v in self.d.values():
            v.free()
        if self.split is not None:
            self.split.free()


PASSES = [(cs, sm) for cs in (False, True) for sm in (False, True)]
PASS_IDS = ["%s-%s" % ("col" if cs else "row", "softmax" if sm else "none") for cs, sm in PASSES]


@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("column_side,softmax", PASSES, ids=PASS_IDS)
def test_pass_vs_numpy(ctx, column_side, softmax, f):
    """Overwrite and accumulate against numpy, guards untouched, empty rows zero under overwrite, a repeat bit-identical."""
    p = Problem(ctx, column_side, softmax, f)
    assert np.diff(p.rowptr).max() >= 1500 and np.count_nonzero(np.diff(p.rowptr) == 0) > 100
    got = p.run(True)
    want = p.want(True)
    empty = np.diff(p.rowptr) == 0
    assert np.all(got[empty] == 0.0) and np.abs(want).max() > 0
    errs = [T.rel(got, want)]
    assert np.array_equal(p.run(True), got), "a repeat must be bit-identical"
    acc = p.run(False)
    errs.append(T.rel(acc, p.want(False)))
    assert np.array_equal(acc[empty], p.out0[:p.m, :f][empty]), "accumulating leaves rows without nonzeros alone"
    p.free()
    T.record_observed("gat_fused_backward_kernel", case="%s %s f=%d" % ("col" if column_side else "row", "softmax" if softmax else "none", f),
                      worst=max(errs))
    assert max(errs) <= KTOL[softmax], errs


def compositions(n):
    """Every way to cut [0, n) into consecutive groups: what the adaptive walk can produce from n windows."""
    for k in range(n):
        for cuts in itertools.combinations(range(1, n), k):
            edges = (0,) + cuts + (n,)
            yield list(zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("f", [7, 64, 100, 128, 200, 255, 256])
@pytest.mark.parametrize("column_side,softmax", PASSES, ids=PASS_IDS)
def test_grouping_independence(ctx, column_side, softmax, f):
    """One launch against the six windows in every grouping (1 .. 6 launches, all 32 of them), overwriting and accumulating: the
    same bits, because every launch continues the row's sum nonzero by nonzero."""
    p = Problem(ctx, column_side, softmax, f, seed=3)
    for overwrite in (True, False):
        whole = p.run(overwrite)
        n = 0
        for groups in compositions(NWIN):
            assert np.array_equal(p.run(overwrite, groups), whole), groups
            n += 1
        assert n == 32
    assert T.rel(whole, p.want(False)) <= KTOL[softmax]
    p.free()


@pytest.mark.parametrize("f", [33, 64, 128, 256])
@pytest.mark.parametrize("column_side,softmax", PASSES, ids=PASS_IDS)
def test_forced_panels_are_bit_identical(monkeypatch, column_side, softmax, f):
    """Column panels (several launches over every row, hub rows after the last): the same bits as one launch."""
    ncols = 1536
    c1 = K.Ctx(0)
    p1 = Problem(c1, column_side, softmax, f, seed=5)
    one, want = p1.run(True), p1.want(True)
    p1.free()
    c1.close()
    gather_w = P.fused_packed_width(f, softmax) if column_side else f
    monkeypatch.setenv("HNH_PANEL_BYTES", str(ncols * gather_w * 8 / 5))
    monkeypatch.setenv("HNH_MAX_PANELS", "8")
    monkeypatch.setenv("HNH_PANELS_WITH_HUBS", "1")
    c5 = K.Ctx(0)
    p5 = Problem(c5, column_side, softmax, f, seed=5)
    # (hnh_panel_count speaks for the passes of hnh_kernels.h, whose rows end at 512 columns: asked at the nearest width it knows)
    assert c5.lib.hnh_panel_count(c5.h, p5.m, int(p5.rowptr[-1]), ncols, min(gather_w, 512), int(np.diff(p5.rowptr).max())) == 5
    five = p5.run(True)
    p5.free()
    c5.close()
    assert np.array_equal(one, five)
    assert T.rel(five, want) <= KTOL[softmax]


@pytest.mark.parametrize("softmax", [False, True])
def test_pack_kernel(ctx, softmax):
    lib = ctx.lib
    rng = np.random.default_rng(4)
    for f in WIDTHS:
        rows, ld_a, ld_dz = 301, f + 3, f + 5
        pw = P.fused_packed_width(f, softmax)
        ld_p = pw + 2
        a, dz = rng.uniform(-1, 1, (rows, ld_a)), rng.uniform(-1, 1, (rows, ld_dz))
        lse, delta = rng.uniform(0, 3, rows), rng.uniform(-1, 1, rows)
        da, ddz, dl, dd = ctx.upload(a), ctx.upload(dz), ctx.upload(lse), ctx.upload(delta)
        dp = ctx.upload(np.full((rows + 1, ld_p), 7.0))
        ctx.check(lib.hnh_attn_grad_pack_f64(ctx.h, dp.ptr, ld_p, da.ptr, ld_a, ddz.ptr, ld_dz, dl.ptr if softmax else None, dd.ptr if softmax else None,
                                             rows, f, K.STREAM_COMPUTE), "pack")
        got = dp.get()
        want = P.fused_pack(a[:, :f], dz[:, :f], lse if softmax else None, delta if softmax else None)
        assert np.array_equal(got[:rows, :pw], want) and np.all(got[:rows, pw:] == 7.0) and np.all(got[rows] == 7.0), f
        assert lib.hnh_attn_grad_pack_f64(ctx.h, dp.ptr, ld_p + 1, da.ptr, ld_a, ddz.ptr, ld_dz, None, None, rows, f, K.STREAM_COMPUTE) == 1  # odd pitch
        for d in (da, ddz, dl, dd, dp):
            d.free()


@pytest.mark.parametrize("column_side", [False, True], ids=["row", "col"])
def test_wide_heads_are_refused_and_write_nothing(ctx, column_side):
    for f in (257, 320, 512):
        p = Problem(ctx, column_side, True, f, m=128, ncols=96, degrees=np.full(128, 3))
        a, blk = p.args(), p.block()
        assert p.fn()(ctx.h, C.byref(blk), C.byref(a), K.FUSED_OUT_OVERWRITE, None, K.STREAM_COMPUTE) == K.ERR_UNSUPPORTED
        assert b"256" in ctx.lib.hnh_last_error(ctx.h)
        ctx.sync()
        assert np.array_equal(p.d["out"].get(), p.out0)
        assert p.fn()(ctx.h, C.byref(blk), C.byref(a), 4, None, K.STREAM_COMPUTE) == 1  # (an unknown flag, at any width)
        p.free()


@pytest.mark.parametrize("column_side", [False, True], ids=["row", "col"])
def test_empty_block(ctx, column_side):
    """rowptr == NULL: overwrite leaves zeros in the f columns of every row, accumulate leaves everything alone."""
    p = Problem(ctx, column_side, False, 33, m=256, ncols=96, degrees=np.full(256, 2))
    a = p.args()
    none = K.CsrBlock(p.m, 0, -1, 0, 0, None, None, None)
    ctx.check(p.fn()(ctx.h, C.byref(none), C.byref(a), 0, None, K.STREAM_COMPUTE), "empty block, accumulate")
    ctx.sync()
    assert np.array_equal(p.d["out"].get(), p.out0)
    ctx.check(p.fn()(ctx.h, C.byref(none), C.byref(a), K.FUSED_OUT_OVERWRITE, None, K.STREAM_COMPUTE), "empty block, overwrite")
    ctx.sync()
    got = p.d["out"].get()
    assert np.all(got[:p.m, :33] == 0.0) and np.array_equal(got[:, 33:], p.out0[:, 33:]) and np.array_equal(got[p.m], p.out0[p.m])
    p.free()


@pytest.mark.parametrize("column_side,softmax", PASSES, ids=PASS_IDS)
def test_rmat_hub_rows(ctx, column_side, softmax):
    """The R-MAT graph of test_backward_rmat_hub_rows: hub rows of S for the row pass, hub rows of S^T (hub columns) for the column pass."""
    m, f = 1 << 13, 64
    rows, cols = H.generate_rmat(13, m * 16)
    assert np.bincount(rows, minlength=m).max() >= 512 and np.bincount(cols, minlength=m).max() >= 512
    r, c = (cols, rows) if column_side else (rows, cols)
    order = np.lexsort((c, r))
    r, c = r[order].astype(np.int64), c[order].astype(np.int64)
    p = Problem(ctx, column_side, softmax, f, m=m, ncols=m, degrees=np.full(m, 2))
    # (the operands were drawn for another structure: swap in the R-MAT one and redo what depends on it)
    p.rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))]).astype(np.int32)
    p.colidx, p.rows = c.astype(np.int32), r
    for k in ("rowptr", "colidx"):
        p.d[k].free()
    p.d["rowptr"], p.d["colidx"] = ctx.upload(p.rowptr), ctx.upload(np.concatenate([p.colidx, [0]]).astype(np.int32))
    if softmax:
        s = R.leaky(np.einsum("ij,ij->i", p.x[r, :f], p.a_cols[c]), ALPHA)
        owner = c if column_side else r
        _, p.lse = R.row_softmax(owner, m, s)
        if column_side:
            p.y = P.fused_pack(p.a_cols, p.dz_cols, p.lse, p.delta, ld=p.ld_y)
            p.y[np.isnan(p.y)] = 1e300
            p.d["y"].set(p.y)
        else:
            p.d["lse"].set(p.lse)
    got = p.run(True)
    err = T.rel(got, p.want(True))
    assert np.array_equal(p.run(True), got), "a repeat must be bit-identical"
    p.free()
    T.record_observed("gat_fused_backward_kernel", case="rmat %s %s" % ("col" if column_side else "row", "softmax" if softmax else "none"), worst=err)
    assert err <= KTOL[softmax], err


# ------------------------------------------------------------------------------------------------ the operator
def later(attention, scale=40.0):
    """the scale of the weights after the first layer (the softmax keeps the later layers' inputs of order one by itself)"""
    return scale if attention == "none" else 1.0


def run_gat(world, alg, c, rows, cols, m, x, layers, weights, g_glob, attention, modes, ordinary_call=None):
    """Forward once, then one backward per entry of `modes` on the same object; returns this rank's blocks and every round's results."""
    s = G.setup(world, rows, cols, m, x, layers, weights, None, g_glob, alg=alg, c=c, attention=attention, backward=modes[0])
    gnn, d = s["gnn"], s["d"]
    res = dict(subA=s["subA"], subB=s["subB"], rounds=[])
    gnn.forwardPass()
    for k, mode in enumerate(modes):
        if k > 0:
            gnn.set_backward(mode)  # no new forward pass
        res["rounds"].append(G.one_round(s, weights, False, forward=False, out_after=True))
    if ordinary_call is not None:  # an ordinary call of the same operator afterwards: the landing buffers are in a usable shape
        r = ordinary_call["R"]
        d.setRValue(r)
        A, B = d.like_A_matrix(0.0), d.like_B_matrix(0.0)
        res["ord_subA"] = d.submatrices(H.AMAT)
        A.upload(T.fill_local(d.submatrices(H.AMAT), A.shape, ordinary_call["a"]))
        B.upload(T.fill_local(d.submatrices(H.BMAT), B.shape, ordinary_call["b"]))
        S, buf = d.like_S_values(1.0), d.like_S_values(0.0)
        d.sddmmA(A, B, S, buf)
        res["sddmm_sum"] = float(np.sum(buf.download()))
        d.fusedSpMM(A, B, S, buf, H.AMAT)
        res["fused"] = A.download()
        for h in (A, B, S, buf):
            h.free()
    G.teardown(s)
    return res


def check_round(per_rank, k, rows, cols, m, x, layers, weights, g_glob, attention, label):
    G.compare(G.assembled(per_rank, k, m, layers), G.reference(rows, cols, m, x, layers, weights, None, g_glob, attention=attention), "gat_fused_backward",
              label, len(per_rank), check=("dw", "dx"))


def fused_vs_unfused(per_rank, kf, ku, weights, label):
    """The fused round against the un-fused round of the same object on the same inputs."""
    worst = 0.0
    for pr in per_rank:
        a, b = pr["rounds"][kf], pr["rounds"][ku]
        worst = max([worst, T.rel(a["dx"], b["dx"])] + [T.rel(a["dw"][k], b["dw"][k]) for k in weights])
    T.record_observed("gat_fused_vs_unfused", case=label, ranks=len(per_rank), worst=worst)
    assert worst <= TOL, worst


@pytest.mark.parametrize("attention", ["none", "softmax"])
@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_fused_backward_er8(p, attention):
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w = hashed_weights(layers, later(attention))
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 9) * 16.0
    per_rank = H.run_spmd(p, lambda wd: run_gat(wd, "15d_fusion2", 1, rows, cols, m, x, layers, w, g, attention, ["fused", "unfused"]))
    check_round(per_rank, 0, rows, cols, m, x, layers, w, g, attention, "er8_r16 %s p%d" % (attention, p))
    fused_vs_unfused(per_rank, 0, 1, w, "er8_r16 %s p%d" % (attention, p))
    for pr in per_rank:
        assert np.array_equal(pr["rounds"][0]["out"], pr["rounds"][0]["out_after"]), "backward changed the forward output"


WIDE = {"benchmark widths": (1 << 12, [(256, 128, 2), (256, 64, 3)]), "a 256-feature head": (1 << 11, [(64, 256, 1)]),
        "odd heads": (1 << 11, [(24, 33, 2), (66, 7, 3)])}


@pytest.mark.parametrize("attention", ["none", "softmax"])
@pytest.mark.parametrize("p", [1, 4])
@pytest.mark.parametrize("shape", sorted(WIDE))
def test_fused_backward_widths(shape, p, attention):
    m, layers = WIDE[shape]
    rows, cols = H.generate_er(m, m, m * 16, 77)
    x = O.dense_fill(m, layers[0][0], 41) * 16.0
    w = hashed_weights(layers, later(attention, 8.0))
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 3) * 64.0
    per_rank = H.run_spmd(p, lambda wd: run_gat(wd, "15d_fusion2", 1, rows, cols, m, x, layers, w, g, attention, ["fused", "unfused"]))
    check_round(per_rank, 0, rows, cols, m, x, layers, w, g, attention, "%s %s p%d" % (shape, attention, p))
    fused_vs_unfused(per_rank, 0, 1, w, "%s %s p%d" % (shape, attention, p))


@pytest.mark.parametrize("attention", ["none", "softmax"])
@pytest.mark.parametrize("p", [1, 4])
def test_fused_backward_rmat_hub_rows(p, attention):
    m, layers = 1 << 13, [(64, 64, 2), (128, 32, 2)]
    rows, cols = H.generate_rmat(13, m * 16)
    assert np.bincount(rows, minlength=m).max() >= 512 and np.bincount(cols, minlength=m).max() >= 512
    x = O.dense_fill(m, 64, 8) * 8.0
    w = hashed_weights(layers, later(attention, 4.0))
    g = O.dense_fill(m, 64, 4) * 32.0
    per_rank = H.run_spmd(p, lambda wd: run_gat(wd, "15d_fusion2", 1, rows, cols, m, x, layers, w, g, attention, ["fused", "fused", "unfused"]))
    check_round(per_rank, 0, rows, cols, m, x, layers, w, g, attention, "rmat hubs %s p%d" % (attention, p))
    fused_vs_unfused(per_rank, 0, 2, w, "rmat hubs %s p%d" % (attention, p))
    for pr in per_rank:
        a, b = pr["rounds"][:2]
        assert np.array_equal(a["dx"], b["dx"]) and all(np.array_equal(a["dw"][k], b["dw"][k]) for k in w), "a repeat must be bit-identical"


@pytest.mark.parametrize("attention", ["none", "softmax"])
def test_two_rounds_are_bit_identical(attention):
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w = hashed_weights(layers, later(attention))
    g = O.dense_fill(m, 12, 9) * 16.0

    def two_rounds(wd):  # two forward + backward rounds
        a = run_gat(wd, "15d_fusion2", 1, rows, cols, m, x, layers, w, g, attention, ["fused"])
        b = run_gat(wd, "15d_fusion2", 1, rows, cols, m, x, layers, w, g, attention, ["fused"])
        return a["rounds"][0], b["rounds"][0]

    for a, b in H.run_spmd(4, two_rounds):
        assert np.array_equal(a["out"], a["out_after"]) and np.array_equal(b["out"], b["out_after"]), "backward changed the output"
        assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["dx"], b["dx"])
        assert all(np.array_equal(a["dw"][k], b["dw"][k]) for k in w)


@pytest.mark.parametrize("attention", ["none", "softmax"])
@pytest.mark.parametrize("p", [1, 4])
def test_mode_switches_leak_nothing(p, attention):
    """un-fused -> fused -> un-fused on one object: the un-fused results are those of a fresh default object, bit for bit (an explicit
    "unfused" included), and an ordinary sddmmA / fusedSpMM on the same operator afterwards still matches the oracle."""
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w = hashed_weights(layers, later(attention))
    g = O.dense_fill(m, 12, 9) * 16.0
    oc = dict(R=16, a=O.dense_fill(m, 16, 1), b=O.dense_fill(m, 16, 2))

    def default_object(world):  # as the parent's tests build it: no backward keyword at all
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, "15d_fusion2", sp, layers[0][0], 1)
        gnn = H.GAT(d, layers, ALPHA, attention=attention)
        for k, wk in w.items():
            gnn.set_weight(*k, wk)
        d.setRValue(layers[0][0])
        x_d = H.Dense.create(world, *gnn.buffer_shape(0))
        x_d.upload(T.fill_local(d.submatrices(H.BMAT), x_d.shape, x))
        d.setRValue(12)
        gg = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
        gg.upload(T.fill_local(d.submatrices(H.AMAT), gg.shape, g))
        dx = H.Dense.create(world, *gnn.buffer_shape(0))
        gnn.set_input(x_d)
        gnn.forwardPass()
        gnn.backwardPass(gg)
        gnn.get_input_grad(dx)
        res = dict(dx=dx.download(), dw={k: gnn.weight_grad(*k) for k in w})
        for h in (x_d, gg, dx, gnn, d, sp):
            h.free()
        return res

    fresh = H.run_spmd(p, default_object)
    per_rank = H.run_spmd(p, lambda wd: run_gat(wd, "15d_fusion2", 1, rows, cols, m, x, layers, w, g, attention, ["unfused", "fused", "unfused"],
                                                ordinary_call=oc))
    for pr, fr in zip(per_rank, fresh):
        for k in (0, 2):
            assert np.array_equal(pr["rounds"][k]["dx"], fr["dx"]) and all(np.array_equal(pr["rounds"][k]["dw"][q], fr["dw"][q]) for q in w)
    check_round(per_rank, 1, rows, cols, m, x, layers, w, g, attention, "switched %s p%d" % (attention, p))
    want, want_vals = O.fused_a(rows, cols, np.ones(len(rows)), oc["a"], oc["b"])
    fused = T.assemble_dense([dict(f=pr["fused"], subA=pr["ord_subA"]) for pr in per_rank], "f", "subA", m, 16)
    assert T.rel(fused, want) <= T.TOL
    assert abs(sum(pr["sddmm_sum"] for pr in per_rank) - float(np.sum(want_vals))) <= T.TOL * float(np.sum(np.abs(want_vals)))


@pytest.mark.parametrize("attention,tscale", [("none", 4.0), ("softmax", 0.05)])
@pytest.mark.parametrize("p", [1, 2])
def test_sgd_lowers_the_loss(p, attention, tscale):
    rows, cols, m, x = er8()
    target = O.dense_fill(m, 12, 21) * tscale
    w = hashed_weights(T.GAT_LAYERS, later(attention))
    per_rank = H.run_spmd(p, lambda wd: G.sgd(wd, rows, cols, m, x, T.GAT_LAYERS, target, 5, 0.02, w, attention=attention, backward="fused"))
    loss = np.sum(np.array([pr[0] for pr in per_rank]), axis=0)
    assert all(loss[i + 1] < loss[i] for i in range(5)), loss


SCHEDULE_NAMES = {"15d_sparse": "1.5D Sparse Shifting", "25d_dense_replicate": "2.5D Cannon's Algorithm Replicating Dense",
                  "15d_fusion1": "15d_fusion1", "15d_fusion2": "15d_fusion2"}


@pytest.mark.parametrize("alg,p,c,layers,words", [("15d_fusion1", 4, 2, [(16, 8, 2)], None), ("15d_fusion2", 4, 2, [(16, 8, 2)], None),
                                                  ("15d_sparse", 2, 1, [(16, 8, 2)], None), ("25d_dense_replicate", 4, 1, [(16, 8, 2)], None),
                                                  ("15d_fusion2", 2, 1, [(16, 320, 1)], "at most 256 features, not 320")])
def test_refusals_leave_nothing_in_flight(alg, p, c, layers, words):
    rows, cols, m, _ = er8()
    words = words or "fused backward.*%s.*c = %d" % (SCHEDULE_NAMES[alg], c)

    def rank(world):
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, alg, sp, 16, c)
        gnn = H.GAT(d, layers, ALPHA, backward="fused")
        g = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
        gnn.forwardPass()
        with pytest.raises(H.HnhError, match=words):
            gnn.backwardPass(g)
        world.sync()  # nothing was left in flight
        with pytest.raises(ValueError):
            gnn.set_backward("half-fused")
        for h in (g, gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(p, rank))
