"""The export of the GAT's attention coefficients on the GPU (include/hnh_attn_coef.h, GAT.attention_coefficients).

Kernel level, through ctypes: hnh_attn_coef_csr_p against the extended-precision numpy reference (tests/gat_coef_ref.py, coef_pass_ld) for the
three scores at widths 1, 7, 8, 33, 64, 100, 128, 200, 255, 256 on the harness's blocks (2048 x 1536, mixed_degrees: empty rows, rows of 200 -
300, hub rows of 600 and 1500, a planted repeated pair), operands at even and at odd column offsets, guard zones round `values`; row sums;
six column windows in every grouping and forced Infinity-Cache panels, bit for bit, and the sentinel in every nonzero of a window that was not
selected; the mask of include/hnh_attn_dropout.h (zero pattern == the host's keep test, kept entries == scale * a, a repeated pair, a row with
every edge dropped); scores far outside exp's range; rowptr == NULL and the width limit.
Operator level: GAT.attention_coefficients on 15d_fusion2, c = 1 over 1, 2, 4, 8 loopback ranks in every mode against the model's trace
through S_coordinates(), the stored output rebuilt from the downloaded coefficients, benchmark widths, an R-MAT graph with hub rows, and
non-interference with the forward and backward passes.

Bounds: FTOL = 1e-12 for the kernel against the longdouble reference (the float64 reference alone stays within FTOL / 10 on the same operands:
tests/test_gat_coef_cpu.py), 1e-11 for the row sums, TOL = 1e-10 for the operator; far outside exp's range 10 x the float64 reference's own
error against the longdouble one on the same inputs.  Observed worst cases go through T.record_observed.

Observed on an MI355X (max |x - ref| / max |ref|): the kernel <= 3.9e-15 over the three scores, every width and both alignments, 1.7e-16 under
the mask; at |z| = 800 dot 1.25e-13 (the float64 reference: 1.34e-13), additive 5.69e-14 (5.69e-14), gatv2 1.51e-13 (1.19e-13); the operator
<= 7.4e-16 on er8_r16 over p = 1 .. 8 in every mode, 7.5e-16 at a head of 256, 4.5e-16 on the R-MAT graph."""
import ctypes as C

import numpy as np
import pytest

import gat_coef_ref as CR
import gat_pass_ref as P
import gat_ref as R
import gat_v2_ref as V
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import (ALPHA, FTOL, GROUPINGS, NWIN, TOL, ctx, er8, graph, hashed_weights, hip_backend, mixed_degrees, one_round, setup,  # noqa: F401
                             teardown)
from oracle import oracle as O

pytestmark = pytest.mark.gpu
WIDTHS = [1, 7, 8, 33, 64, 100, 128, 200, 255, 256]
GUARD = 1e300   # beyond an operand's width: never read (a read would show as inf or NaN)
SENTINEL = -7.5  # what `values` and its guard zones hold before a launch: no coefficient is negative
M, NCOLS = 2048, 1536
BLOCKS = {}


def block(f, seed=0):
    """(rowptr, colidx, rows, cols) of the harness's block for width f, made once"""
    if (f, seed) not in BLOCKS:
        rowptr, colidx, rows = graph(M, NCOLS, mixed_degrees(M, seed + f), seed + 1)
        BLOCKS[(f, seed)] = (rowptr, colidx, rows, colidx.astype(np.int64))
    return BLOCKS[(f, seed)]


def padded(mat, ld, off):
    out = np.full((mat.shape[0], ld), GUARD)
    out[:, off:off + mat.shape[1]] = mat
    return out


class CoefProblem:
    """One launch's operands on the device.  odd=True puts X, Y and a at an odd column offset of an odd pitch (8-byte aligned only: the
    8-byte lanes) and `values` at an odd offset; otherwise offsets and pitches are even.  The packed pair of score additive keeps its
    16-byte alignment (the layout asks for it) at a pitch of 4.  drop = (seed, p): the mask, own rows from just below 2^31, gathered rows with
    scattered ids up to 2^32."""

    def __init__(self, ctx, score, f, seed=0, odd=False, big=0.0, drop=None):
        self.ctx, self.score, self.f, self.odd = ctx, score, f, odd
        self.rowptr, self.colidx, self.rows, self.cols = block(f, seed)
        self.nnz = int(self.rowptr[-1])
        o = self.o = CR.with_lse(CR.operands(score, f, self.rows, self.cols, M, NCOLS, seed, big), self.rows, self.cols, M, score, ALPHA)
        off = self.off = 1 if odd else 2
        ld = f + off + 1
        ld += int(ld % 2 != (1 if odd else 0))
        assert ld % 2 == (1 if odd else 0)
        self.guard = 3 if odd else 4
        host = dict(rowptr=self.rowptr, colidx=np.concatenate([self.colidx, [0]]).astype(np.int32), lse=o["lse"],
                    values=np.full(self.nnz + 2 * self.guard, SENTINEL))
        self.drop = self.ref_drop = None
        if score == "additive":
            self.row_id0 = (1 << 31) - M // 2
            self.ids = np.random.default_rng(99 + f + seed).permutation(np.arange(NCOLS, dtype=np.int64) * 2700001 + 17)
            assert (1 << 31) <= self.ids.max() < (1 << 32)
            pair = np.full((NCOLS, 4), GUARD)
            pair[:, 0], pair[:, 1] = o["y"], self.ids
            host.update(y=pair, s=o["x"])
            self.ld_y = 4
            if drop is not None:
                dseed, p = drop
                w2 = 2 * 65536 + 5
                self.drop = K.AttnDrop(dseed, w2, K.dropout_threshold(p), 1.0 / (1.0 - p), self.row_id0)
                self.ref_drop = (dseed, w2, p, np.arange(M, dtype=np.uint64) + np.uint64(self.row_id0), self.ids.astype(np.uint64))
        else:
            host.update(x=padded(o["x"], ld, off), y=padded(o["y"], ld, off))
            self.ld_x = self.ld_y = ld
            if score == "gatv2":
                host.update(a=np.concatenate([np.full(off, GUARD), o["a"], [GUARD]]))
        self.values0 = host["values"]
        self.d = {k: ctx.upload(v) for k, v in host.items()}
        self.split = None

    def args(self):
        d, a = self.d, K.AttnCoef()
        a.lse, a.f, a.score, a.leaky_alpha = d["lse"].ptr, self.f, CR.SCORE_CODE[self.score], ALPHA
        if self.score == "additive":
            a.s, a.Y, a.ld_y = d["s"].ptr, d["y"].ptr, self.ld_y
        else:
            a.X, a.ld_x, a.Y, a.ld_y = d["x"].ptr + 8 * self.off, self.ld_x, d["y"].ptr + 8 * self.off, self.ld_y
            if self.score == "gatv2":
                a.a = d["a"].ptr + 8 * self.off
        return a

    def blk(self):
        return K.CsrBlock(M, self.nnz, NCOLS, int(np.diff(self.rowptr).max()), 0, self.d["rowptr"].ptr, self.d["colidx"].ptr, None)

    def window_of(self):
        """the window of every nonzero"""
        bounds = np.array([int(NCOLS * (b + 1) / NWIN) for b in range(NWIN - 1)])
        return np.searchsorted(bounds, self.cols, side="right")

    def run(self, groups=None):
        """The values after one call over whole rows (groups None) or one call per window group; the guard zones are checked."""
        ctx, lib = self.ctx, self.ctx.lib
        self.d["values"].set(self.values0)
        a, b = self.args(), self.blk()
        vp = self.d["values"].ptr + 8 * self.guard
        dr = C.byref(self.drop) if self.drop is not None else None
        if groups is None:
            ctx.check(lib.hnh_attn_coef_csr_p(ctx.h, C.byref(b), vp, C.byref(a), dr, 0, None, K.STREAM_COMPUTE), "coef pass")
        else:
            if self.split is None:
                bounds = (C.c_int32 * (NWIN - 1))(*[int(NCOLS * (q + 1) / NWIN) for q in range(NWIN - 1)])
                self.split = K.DevArray(ctx, (NWIN - 1) * M, np.int32)
                ctx.check(lib.hnh_csr_window_bounds(ctx.h, M, self.d["rowptr"].ptr, self.d["colidx"].ptr, NWIN - 1, bounds, self.split.ptr, K.STREAM_COMPUTE),
                          "window bounds")
            sp = self.split.ptr
            for w0, w1 in groups:
                win = K.CsrWindow(None if w0 == 0 else sp + (w0 - 1) * M * 4, None if w1 == NWIN else sp + (w1 - 1) * M * 4, int(w1 == NWIN))
                ctx.check(lib.hnh_attn_coef_csr_p(ctx.h, C.byref(b), vp, C.byref(a), dr, 0, C.byref(win), K.STREAM_COMPUTE), "coef window")
        ctx.sync()
        v = self.d["values"].get()
        g = self.guard
        assert np.all(v[:g] == SENTINEL) and np.all(v[g + self.nnz:] == SENTINEL), "the guard zones round values are not written"
        return v[g:g + self.nnz]

    def want(self, drop=True):
        o = self.o
        return CR.coef_pass_ld(self.rows, self.cols, o["x"], o["y"], o["lse"], self.score, ALPHA, o["a"], self.ref_drop if drop else None)

    def want64(self):
        o = self.o
        return CR.coef_pass(self.rows, self.cols, o["x"], o["y"], o["lse"], self.score, ALPHA, o["a"])

    def free(self):
        for v in self.d.values():
            v.free()
        if self.split is not None:
            self.split.free()


def repeated_pair(p):
    pairs = p.rows.astype(np.int64) * NCOLS + p.cols
    e = int(np.nonzero(pairs[1:] == pairs[:-1])[0][0])
    return e, e + 1


# (the packed pair of score additive is 16-byte aligned by its layout: it has no odd offset to test)
@pytest.mark.parametrize("score,odd", [("dot", False), ("dot", True), ("gatv2", False), ("gatv2", True), ("additive", False)],
                         ids=lambda v: {False: "aligned", True: "odd"}.get(v, v) if isinstance(v, bool) else v)
def test_kernel_against_the_extended_reference(ctx, score, odd):
    worst = 0.0
    for f in WIDTHS:
        p = CoefProblem(ctx, score, f, odd=odd)
        got = p.run()
        again = p.run()
        assert np.array_equal(got, again), "a repeat must be bit-identical"
        err = float(T.rel(np.asarray(got, dtype=np.longdouble), p.want()))
        print("observed gat_coef kernel", score, f, "odd" if odd else "aligned", "%.2e" % err)
        worst = max(worst, err)
        assert np.all(got >= 0.0) and np.all(got <= 1.0 + 1e-12)
        assert err <= FTOL, (score, f, odd, err)
        sums = CR.row_sums(p.rows, M, got)
        live = np.diff(p.rowptr) > 0
        assert np.max(np.abs(sums[live] - 1.0)) <= 1e-11, (score, f, np.max(np.abs(sums[live] - 1.0)))
        e0, e1 = repeated_pair(p)
        assert got[e0] == got[e1], "the two copies of the repeated pair hold equal values"
        p.free()
    T.record_observed("gat_coef_kernel", case="%s %s" % (score, "odd" if odd else "aligned"), worst=worst)


@pytest.mark.parametrize("score,f", [("dot", 7), ("dot", 64), ("dot", 128), ("dot", 256), ("gatv2", 33), ("gatv2", 64), ("gatv2", 256), ("additive", 33)],
                         ids=lambda v: str(v))
def test_windows_in_every_grouping_are_bit_identical_and_leave_the_rest_alone(ctx, score, f):
    p = CoefProblem(ctx, score, f, seed=3, drop=(0xC0FFEE1234567890, 0.25) if score == "additive" else None)
    whole = p.run()
    for name, groups in GROUPINGS.items():
        if groups is not None:
            assert np.array_equal(p.run(groups), whole), name
    win = p.window_of()
    some = p.run([(1, 4), (5, 6)])
    picked = ((win >= 1) & (win < 4)) | (win == 5)
    assert picked.any() and (~picked).any()
    assert np.array_equal(some[picked], whole[picked]) and np.all(some[~picked] == SENTINEL), "the other windows' nonzeros keep their sentinel"
    p.free()


@pytest.mark.parametrize("score,f", [("dot", 7), ("dot", 128), ("dot", 256), ("gatv2", 64), ("gatv2", 200), ("additive", 33)], ids=lambda v: str(v))
def test_forced_panels_are_bit_identical(monkeypatch, score, f):
    c1 = K.Ctx(0)
    p1 = CoefProblem(c1, score, f, seed=5)
    one, want = p1.run(), p1.want()
    p1.free()
    c1.close()
    gather_w = 2 if score == "additive" else f
    monkeypatch.setenv("HNH_PANEL_BYTES", str(NCOLS * gather_w * 8 / 5))
    monkeypatch.setenv("HNH_MAX_PANELS", "8")
    monkeypatch.setenv("HNH_PANELS_WITH_HUBS", "1")
    c5 = K.Ctx(0)
    p5 = CoefProblem(c5, score, f, seed=5)
    assert c5.lib.hnh_panel_count(c5.h, M, p5.nnz, NCOLS, gather_w, int(np.diff(p5.rowptr).max())) == 5
    five = p5.run()
    p5.free()
    c5.close()
    assert np.array_equal(one, five)
    assert float(T.rel(np.asarray(five, dtype=np.longdouble), want)) <= FTOL


@pytest.mark.parametrize("rate", [0.6, 0.25])
def test_dropout_mask_of_the_additive_score(ctx, rate):
    seed = 0xC0FFEE1234567890
    for f in (7, 64, 256):
        p = CoefProblem(ctx, "additive", f, seed=1, drop=(seed, rate))
        got = p.run()
        keep = P.keep(seed, P.STREAM_ATTENTION, 2 * 65536 + 5, (p.rows.astype(np.uint64) + np.uint64(p.row_id0)), p.ids[p.cols].astype(np.uint64), rate)
        plain = p.want(drop=False)
        assert np.all(plain > 0), "no coefficient of these operands underflows: a zero is a dropped edge"
        assert np.array_equal(got != 0.0, keep), "the zero pattern is the host's keep test, bit for bit"
        err = float(T.rel(np.asarray(got, dtype=np.longdouble), p.want()))
        T.record_observed("gat_coef_kernel", case="additive drop %.2f f=%d" % (rate, f), worst=err)
        assert err <= FTOL, (f, err)
        e0, e1 = repeated_pair(p)
        assert got[e0] == got[e1] and keep[e0] == keep[e1], "both copies of a repeated pair share the mask"
        dropped_rows = np.bincount(p.rows, weights=keep, minlength=M) == 0
        live = np.diff(p.rowptr) > 0
        assert np.any(dropped_rows & live), "the block has a row whose edges are all dropped"
        assert np.all(CR.row_sums(p.rows, M, got)[dropped_rows] == 0.0)
        p.free()


@pytest.mark.parametrize("score", CR.SCORES)
def test_scores_far_outside_exps_range(ctx, score):
    """|z| > 700: every value finite and in [0, 1]; the kernel is allowed 10 x the error that the float64 reference itself has against the
    longdouble one on the same inputs (its summation order differs)."""
    p = CoefProblem(ctx, score, 6, seed=2, big=800.0)
    z = CR.scores(p.rows, p.cols, p.o["x"], p.o["y"], score, ALPHA if score == "gatv2" else 1.0, p.o["a"])  # (alpha 1: before the outer LeakyReLU)
    assert np.abs(z).max() > 700
    got = p.run()
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0) and np.all(got <= 1.0 + 1e-9)
    want = p.want()
    own = float(T.rel(np.asarray(p.want64(), dtype=np.longdouble), want))
    err = float(T.rel(np.asarray(got, dtype=np.longdouble), want))
    T.record_observed("gat_coef_far_range", score=score, kernel=err, float64_reference=own)
    print("observed gat_coef far range", score, "kernel %.2e float64 reference %.2e" % (err, own))
    assert own > 0 and err <= 10.0 * own, (err, own)
    p.free()


@pytest.mark.parametrize("score", CR.SCORES)
def test_empty_block_and_width_limit(ctx, score):
    p = CoefProblem(ctx, score, 33)
    a = p.args()
    vp = p.d["values"].ptr + 8 * p.guard
    none = K.CsrBlock(M, 0, -1, 0, 0, None, None, None)
    assert ctx.lib.hnh_attn_coef_csr_p(ctx.h, C.byref(none), vp, C.byref(a), None, 0, None, K.STREAM_COMPUTE) == 0
    b = p.blk()
    a.f = 257
    assert ctx.lib.hnh_attn_coef_csr_p(ctx.h, C.byref(b), vp, C.byref(a), None, 0, None, K.STREAM_COMPUTE) == K.ERR_UNSUPPORTED
    assert b"256" in ctx.lib.hnh_last_error(ctx.h)
    a.f = 33
    assert ctx.lib.hnh_attn_coef_csr_p(ctx.h, C.byref(b), vp, C.byref(a), None, 4, None, K.STREAM_COMPUTE) == 1  # an unknown flag
    if score != "additive":
        dr = K.AttnDrop(1, 0, K.dropout_threshold(0.5), 2.0, 0)
        assert ctx.lib.hnh_attn_coef_csr_p(ctx.h, C.byref(b), vp, C.byref(a), C.byref(dr), 0, None, K.STREAM_COMPUTE) == K.ERR_UNSUPPORTED
    ctx.sync()
    assert np.array_equal(p.d["values"].get(), p.values0), "nothing was written"
    p.free()


def test_scores_kernel_builds_s_and_the_packed_pair(ctx):
    rng = np.random.default_rng(4)
    for f in (1, 7, 64, 255, 256):
        rows, ld_a = 301, f + 3
        a_mat, a1, a2 = rng.uniform(-1, 1, (rows, ld_a)), rng.standard_normal(f), rng.standard_normal(f)
        dev = {k: ctx.upload(v) for k, v in dict(A=a_mat, a1=a1, a2=a2, s=np.full(rows + 1, 7.0), T=np.full((rows + 1, 4), 7.0)).items()}
        id0 = (1 << 40) + 3
        ctx.check(ctx.lib.hnh_attn_coef_scores_f64(ctx.h, dev["s"].ptr, dev["T"].ptr, 4, dev["A"].ptr, ld_a, dev["a1"].ptr, dev["a2"].ptr, rows, f, id0,
                                                   K.STREAM_COMPUTE), "coef scores")
        ctx.sync()
        s, t = dev["s"].get(), dev["T"].get()
        assert s[rows] == 7.0 and np.all(t[rows] == 7.0) and np.all(t[:, 2:] == 7.0)
        assert T.rel(s[:rows], a_mat[:, :f] @ a1) <= 1e-13 and T.rel(t[:rows, 0], a_mat[:, :f] @ a2) <= 1e-13
        assert np.array_equal(t[:rows, 1], np.arange(rows) + float(id0))
        # the sums of hnh_attn_add_scores_f64, bit for bit: the export sees the forward pass's s and t
        fp = f + (f & 1)
        mm = ctx.upload(np.zeros((rows, fp + 2)))
        ctx.check(ctx.lib.hnh_attn_add_scores_f64(ctx.h, mm.ptr, fp + 2, dev["A"].ptr, ld_a, dev["a1"].ptr, dev["a2"].ptr, rows, f, K.STREAM_COMPUTE), "scores")
        ctx.sync()
        m_host = mm.get().reshape(rows, fp + 2)
        assert np.array_equal(m_host[:, fp], s[:rows]) and np.array_equal(m_host[:, fp + 1], t[:rows, 0])
        mm.free()
        for d in dev.values():
            d.free()


# ------------------------------------------------------------------------------------------------ the operator
MODES = {"dot": dict(score="dot"), "additive": dict(score="additive"), "additive dropout": dict(score="additive", dropout=(0.6, 0.3), seed=11),
         "gatv2": dict(score="gatv2"), "gatv2 feature dropout": dict(score="gatv2", dropout=(0.0, 0.3), seed=11)}
ACTS = {"relu": "relu", "published": ("elu", "identity")}


def vectors_for(score, layers, seed=78):
    if score == "gatv2":
        return {k: (a, np.zeros_like(a)) for k, a in V.vectors_of(layers, seed=seed).items()}
    return R.vectors_of(layers) if score == "additive" else None


def export_all(world, rows, cols, m, x, layers, w, av, dropped=(False,), **kw):
    """forwardPass, then every (layer, head)'s coefficients with this rank's coordinates and the output"""
    s = setup(world, rows, cols, m, x, layers, w, av, None, attention="softmax", **kw)
    gnn, d = s["gnn"], s["d"]
    gnn.forwardPass()
    r0 = d.info()["R"]  # (what the forward pass left: the last head's width)
    res = dict(coords=d.S_coordinates(), subA=s["subA"], coef={})
    for li, (_, _, heads) in enumerate(layers):
        for h in range(heads):
            for dr in dropped:
                v = gnn.attention_coefficients(li, h, dropped=dr)
                res["coef"][(li, h, dr)] = v.download()
                v.free()
    assert d.info()["R"] == r0, "the operator's R is what it was"
    gnn.get_output(s["out"])
    res["out"] = s["out"].download()
    teardown(s)
    return res


def trace_for(score, rows, cols, m, x, layers, w, av, kw, acts):
    mode = dict(activations=acts)
    if "dropout" in kw:
        mode.update(rates=kw["dropout"], seed=kw["seed"])
    return CR.model_trace(score, rows, cols, m, x, layers, ALPHA, w, av if score != "gatv2" else {k: v[0] for k, v in av.items()}, **mode)


def check_export(per_rank, rows, cols, m, layers, tr, acts, label, ranks, dropped=(False,)):
    """Coverage, every (layer, head) against the model's trace through the coordinates, and the stored output rebuilt from the coefficients"""
    keys = rows * m + cols
    order = np.argsort(keys, kind="stable")
    assert len(np.unique(keys)) == len(keys)
    got_keys = np.concatenate([r["coords"][0] * m + r["coords"][1] for r in per_rank])
    assert np.array_equal(np.sort(got_keys), keys[order]), "the ranks' coordinates cover every edge once"
    pos = order[np.searchsorted(keys[order], got_keys)]  # position of every exported entry in the model's edge list
    names = R.activations_of(layers, acts)
    worst = 0.0
    hf_last = layers[-1][1] * layers[-1][2]
    out = T.assemble_dense([dict(o=r["out"], subA=r["subA"]) for r in per_rank], "o", "subA", m, hf_last)
    for (li, h), t in tr.items():
        f = layers[li][1]
        for dr in dropped:
            got = np.concatenate([r["coef"][(li, h, dr)] for r in per_rank])
            want = t["a"] * t["ck"] if (dr and t["ck"] is not None) else t["a"]
            worst = max(worst, float(T.rel(got, want[pos])))
        used = np.concatenate([r["coef"][(li, h, dropped[-1])] for r in per_rank])
        if t["ck"] is None or dropped[-1]:  # act(sum_j w_ij A_j) from the downloaded coefficients and the model's A: the stored output
            agg = np.zeros((m, f))
            np.add.at(agg, rows[pos], used[:, None] * t["A"][cols[pos]])
            worst = max(worst, float(T.rel(R.act(agg, names[li]), t["out"][:, h * f:(h + 1) * f])))
            if li == len(layers) - 1:
                worst = max(worst, float(T.rel(R.act(agg, names[li]), out[:, h * f:(h + 1) * f])))
    T.record_observed("gat_coef", case=label, ranks=ranks, worst=worst)
    print("observed gat_coef", label, ranks, "worst %.2e" % worst)
    assert worst <= TOL, (label, worst)


@pytest.mark.parametrize("acts", sorted(ACTS))
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_export_er8(p, mode, acts):
    rows, cols, m, x = er8()
    layers, kw = T.GAT_LAYERS, dict(MODES[mode])
    score = kw["score"]
    w, av = hashed_weights(layers), vectors_for(score, layers)
    dropped = (False, True) if kw.get("dropout", (0.0, 0.0))[0] > 0 else (False,)
    per_rank = H.run_spmd(p, lambda wd: export_all(wd, rows, cols, m, x, layers, w, av, dropped=dropped, activation=ACTS[acts], **kw))
    tr = trace_for(score, rows, cols, m, x, layers, w, av, kw, ACTS[acts])
    check_export(per_rank, rows, cols, m, layers, tr, ACTS[acts], "er8_r16 %s %s p%d" % (mode, acts, p), p, dropped)
    if mode == "additive":  # rate 0: `dropped` makes no difference
        again = H.run_spmd(p, lambda wd: export_all(wd, rows, cols, m, x, layers, w, av, dropped=(True,), activation=ACTS[acts], **kw))
        assert all(np.array_equal(a["coef"][k[:2] + (True,)], b["coef"][k]) for a, b in zip(again, per_rank) for k in b["coef"])


@pytest.mark.parametrize("p", [1, 4])
@pytest.mark.parametrize("score", CR.SCORES)
def test_export_at_a_benchmark_width(score, p):
    m, layers = 1 << 11, [(64, 256, 1)]
    rows, cols = H.generate_er(m, m, m * 16, 77)
    x = O.dense_fill(m, 64, 41) * 16.0
    w, av = hashed_weights(layers), vectors_for(score, layers, seed=5)
    per_rank = H.run_spmd(p, lambda wd: export_all(wd, rows, cols, m, x, layers, w, av, score=score, activation="identity"))
    tr = trace_for(score, rows, cols, m, x, layers, w, av, {}, "identity")
    check_export(per_rank, rows, cols, m, layers, tr, "identity", "head of 256 %s p%d" % (score, p), p)


@pytest.mark.parametrize("score", CR.SCORES)
def test_export_rmat_hub_rows(score):
    m, layers, p = 1 << 13, [(64, 64, 2), (128, 32, 2)], 4
    rows, cols = H.generate_rmat(13, m * 16)
    keys = np.unique(rows * m + cols)  # (the model's edge list: each pair once, as the coordinates are matched by key)
    rows, cols = keys // m, keys % m
    assert np.bincount(rows, minlength=m).max() >= 512
    x = O.dense_fill(m, 64, 8) * 8.0
    w, av = hashed_weights(layers), vectors_for(score, layers, seed=6)
    per_rank = H.run_spmd(p, lambda wd: export_all(wd, rows, cols, m, x, layers, w, av, score=score))
    tr = trace_for(score, rows, cols, m, x, layers, w, av, {}, "relu")
    check_export(per_rank, rows, cols, m, layers, tr, "relu", "rmat hubs %s p%d" % (score, p), p)


@pytest.mark.parametrize("mode", ["dot", "additive dropout", "gatv2"])
@pytest.mark.parametrize("p", [1, 4])
def test_export_does_not_interfere(p, mode):
    """forward -> export (every head) -> backward against forward -> backward on a fresh object: the output and every gradient bit-equal; a
    second export returns the same bits; an export after train_step without a new forward pass is refused."""
    rows, cols, m, x = er8()
    layers, kw = T.GAT_LAYERS, dict(MODES[mode], attention="softmax")
    score = kw["score"]
    w, av = hashed_weights(layers), vectors_for(score, layers)
    g = O.dense_fill(m, 12, 9) * 16.0
    learns = av is not None
    heads = [(li, h) for li, (_, _, nh) in enumerate(layers) for h in range(nh)]

    def with_export(world):
        s = setup(world, rows, cols, m, x, layers, w, av, g, **kw)
        gnn = s["gnn"]
        gnn.forwardPass()
        first = {}
        for k in heads:
            for dr in (False, True):
                v = gnn.attention_coefficients(*k, dropped=dr)
                first[k + (dr,)] = v.download()
                gnn.attention_coefficients(*k, out=v, dropped=dr)
                assert np.array_equal(v.download(), first[k + (dr,)]), "a second export returns the same bits"
                v.free()
        r = one_round(s, w, learns, forward=False)
        labels = np.arange(m, dtype=np.int32) % layers[-1][1]
        gnn.set_labels(labels, None, heads="mean")
        gnn.set_optimizer("sgd", 0.0)
        gnn.train_step()
        with pytest.raises(H.HnhError, match="attention_coefficients needs a forwardPass first"):
            gnn.attention_coefficients(0, 0)
        world.sync()
        teardown(s)
        return r

    def plain(world):
        s = setup(world, rows, cols, m, x, layers, w, av, g, **kw)
        r = one_round(s, w, learns)
        teardown(s)
        return r

    for a, b in zip(H.run_spmd(p, with_export), H.run_spmd(p, plain)):
        assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["dx"], b["dx"])
        assert all(np.array_equal(a["dw"][k], b["dw"][k]) for k in w)
        assert not learns or all(np.array_equal(a["da"][k][i], b["da"][k][i]) for k in w for i in (0, 1))
