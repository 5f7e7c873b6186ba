"""The per-edge bias of the GAT's score "transformer" on the GPU (include/hnh_attn_edge.h, GAT.set_edge_bias / edge_bias_from).

Kernel level, through ctypes, on the problems of tests/test_gat_qkv_gpu.py (mixed_degrees(1024, ..) blocks: empty rows, a repeated pair,
rows of 200 - 300, hub rows of 600 and 1500; a square block for the forward and the row pass, a 1024 x 768 block standing for S^T for the
column pass; guard zones round every output) with a bias uniform(-3, 3), distinct per nonzero (the two copies of the repeated pair differ),
between two sentinels of 1e300 that a read would show: the three passes against the pass references of tests/gat_edge_ref.py (the forward
pass against np.longdouble: output, lse and the biased scores) at widths 7, 33, 64, 100, 128, 200, 256 with operands at even and at odd
offsets; the finish with HNH_ATTN_ADDEND under relu, elu and identity at 7, 128, 256; a zero bias bit-identical to the plain entry point,
overwriting and accumulating; split independence bit for bit (one call per window, two uneven groupings of six windows, forced
Infinity-Cache panels) at 64 and 200; run-to-run bit identity; the width limit, bias == NULL, a finish without the last window (error
codes, nothing written); an empty block.
Operator level: GAT(..., attention="softmax", score="transformer") on 15d_fusion2, c = 1 with the bias of edge_bias_from, a hash of the
global (row, col), against the numpy model — output, every dW_v, dW_q, dW_k, db, dW_res and dX — on er8_r16 over 1, 2, 4, 8 loopback ranks
(plain layers and the published configuration), at heads of 256 and 33 on 2^12 vertices, on the R-MAT graph with hub rows; p = 8 against
p = 1; a bias on layer 0 only; clearing restores bit identity with an object that never had one; set_edge_bias after a forward pass makes
backwardPass refuse; b = log 2 on every edge equals no bias; five Adam steps through train_step follow the model; refusals on the device.

Bounds: FTOL = 1e-12 for the forward kernel against np.longdouble (1e-13 for its scores), TOL = 1e-10 for the backward kernels and the
operator (tests/gat_gpu_harness.py); the trajectory within 10 x the divergence of a reference run whose gradients are perturbed at 1e-10
(the rule of test_gat_train_gpu.py).  The observed worst cases are recorded with T.record_observed.

Observed on an MI355X (max |x - ref| / max |ref| per matrix): forward kernel <= 6.0e-16 over every width and both alignments (<= 2.9e-16 with
the addend), backward row pass <= 2.4e-15, column pass <= 4.1e-15; the operator (worst of the output, every dW_v, dW_q, dW_k, db, dW_res and
dX) <= 2.0e-15 over every case; the Adam trajectory 2.6e-14 in the parameters (bound 1.9e-8), 1.6e-16 in the loss (bound 7.4e-12)."""
import ctypes as C

import numpy as np
import pytest

import gat_edge_ref as E
import gat_pass_ref as P
import gat_qkv_ref as Q
import gat_ref as R
import hnh_testlib as T
import test_gat_qkv_gpu as QG
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
import gat_gpu_harness as G
from gat_gpu_harness import (ALPHA, COL, FTOL, FWD, GROUPINGS, PASS_NAMES, ROW, TOL, ctx, er8, errors, hashed_weights, hip_backend, same,  # noqa: F401
                             teardown)
from oracle import oracle as O

pytestmark = pytest.mark.gpu
WIDTHS = [7, 33, 64, 100, 128, 200, 256]
SENTINEL = 1e300  # round the bias vector: read as data it would send a score to +1e300
OFF = -1e300     # the documented switch-off value
PASSES = pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])


class EdgeProblem(QG.QKVProblem):
    """A QKVProblem with a bias per nonzero in the block's order.  zero=True: an all-zero bias (the plain pass's results, bit for bit);
    plain=True: the parent's entry point on the same operands."""

    def __init__(self, ctx, pas, f, zero=False, plain=False, off=None, **kw):
        super().__init__(ctx, pas, f, **kw)
        self.plain = plain
        rng = np.random.default_rng(77 + 1000 * f + pas)
        self.bias = np.zeros(self.nnz) if (zero or plain) else rng.uniform(-3, 3, self.nnz)
        if off is not None:  # entries switched off
            self.bias[off] = OFF
        rows, cols = self.rows, self.colidx.astype(np.int64)
        if not (zero or plain):
            _, _, copy = E.keys(rows, cols)
            twin = np.flatnonzero(copy == 1)
            assert len(twin) >= 1 and (off is not None or len(np.unique(self.bias)) == self.nnz), "a repeated pair, and its copies carry different values"
            # the softmax scalars of the biased scores: lse of the S rows (the gathered rows of the column pass)
            self.s = self.s + self.bias
            owner, n_own = (cols, self.ncols) if pas == COL else (rows, self.m)
            _, self.lse_in = R.row_softmax(owner, n_own, self.s)
            self.packed = P.fused_pack(self.y1, self.dz, self.lse_in, self.delta) if pas == COL else self.packed
            self.d["y"].free()
            self.d["y"] = ctx.upload(QG.padded(self.packed[:, :self.pw], self.ld_y, 0))
            if pas == ROW:
                self.d["lse_in"].free()
                self.d["lse_in"] = ctx.upload(self.lse_in)
        self.d["bias"] = ctx.upload(np.concatenate([[SENTINEL], self.bias, [SENTINEL]]))

    def bias_ptr(self):
        return self.d["bias"].ptr + 8

    def fn(self):
        if self.plain:
            return super().fn()
        lib = self.ctx.lib
        f = (lib.hnh_attn_qkv_bias_fwd_csr_p, lib.hnh_attn_qkv_bias_row_csr_p, lib.hnh_attn_qkv_bias_col_csr_p)[self.pas]
        return lambda h, blk, a, flags, win, stream: f(h, blk, a, self.bias_ptr(), flags, win, stream)

    def want(self, overwrite=True, act="relu", addend=False):
        f, m, cols, c0 = self.f, self.m, self.colidx.astype(np.int64), self.col0
        packed = np.nan_to_num(self.packed)
        if self.pas == FWD:
            o, lse, s = E.fwd_pass_ld(self.rows, cols, m, self.x, packed, f, self.scale, self.bias)
            return dict(out=R.act_ld(o + self.addend().astype(np.longdouble) if addend else o, act), lse=lse, values=s)
        base = None if overwrite else self.out0[:m, c0:c0 + f]
        if self.pas == ROW:
            return dict(out=E.row_pass(self.rows, cols, m, self.x, self.dz, self.lse_in, self.delta, packed, f, self.scale, self.bias, out=base))
        dk, dv = E.col_pass(self.rows, cols, m, self.x, self.x2, packed, f, self.scale, self.bias, out=base,
                            out2=None if overwrite else self.out20[:m, c0:c0 + f])
        return dict(out=dk, out2=dv)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd-offset"])
@pytest.mark.parametrize("f", WIDTHS)
@PASSES
def test_pass_vs_numpy(ctx, pas, f, odd):
    """Against the pass references (extended precision for the forward pass: output, lse and the biased scores), guards and sentinels
    untouched, rows without nonzeros zero, a repeat bit-identical, accumulate on top of overwrite for the backward passes; the bias matters."""
    p = EdgeProblem(ctx, pas, f, odd=odd)
    deg = np.diff(p.rowptr)
    assert deg.max() >= 1500 and np.count_nonzero(deg == 0) > 20 and np.count_nonzero((deg >= 200) & (deg <= 300)) >= 3 and 600 in deg
    act = "relu" if pas != FWD else ("relu", "elu", "identity")[f % 3]
    got, want = p.run(True, act=act), p.want(True, act=act)
    empty = deg == 0
    for k in got:
        if k not in ("state", "values"):
            assert np.all(got[k][empty] == 0.0), "rows without nonzeros: o = 0, lse = 0, sums = 0"
            assert np.all(np.isfinite(got[k])), "a sentinel read as data would show"
    assert all(np.abs(np.float64(v)).max() > 0 for v in want.values())
    errs = errors(got, want)
    assert same(p.run(True, act=act), got), "a repeat must be bit-identical"
    if pas != FWD:
        acc = p.run(False)
        errs.update({"acc " + k: v for k, v in errors(acc, p.want(False)).items()})
        for k, first in (("out", p.out0), ("out2", p.out20)):
            assert k not in acc or np.array_equal(acc[k][empty], first[:p.m, p.col0:p.col0 + f][empty]), "accumulating leaves rows without nonzeros alone"
    # the plain entry point on the same operands computes something else: the bias is not ignored
    p.plain = True
    other = p.run(True, act=act)
    assert T.rel(other["out"], got["out"]) > 1e-3
    p.free()
    T.record_observed("gat_edge_kernel", case="%s f=%d%s" % (PASS_NAMES[pas], f, " odd" if odd else ""), worst=max(errs.values()))
    print("observed", PASS_NAMES[pas], f, odd, errs)
    QG.assert_within(pas, errs)


@pytest.mark.parametrize("f", [7, 128, 256])
def test_forward_finish_with_addend(ctx, f):
    """HNH_ATTN_ADDEND on the finishing call: act(o + addend) under relu, elu and the identity against the extended-precision reference;
    lse, the row state and the scores do not see the flag; one call per window gives the same bits."""
    p = EdgeProblem(ctx, FWD, f, seed=4)
    errs = {}
    for act in ("relu", "elu", "identity"):
        got, want = p.run(True, act=act, addend=True), p.want(True, act=act, addend=True)
        errs.update({act + " " + k: v for k, v in errors(got, want).items()})
        assert np.all(np.isfinite(got["out"]))
        assert same(p.run(True, GROUPINGS["one call per window"], act=act, addend=True), got), "one call per window"
        plain = p.run(True, act=act)
        assert all(np.array_equal(plain[k], got[k]) for k in ("lse", "state", "values")), "lse, the row state and the scores do not see the flag"
        assert not np.array_equal(plain["out"], got["out"])
    p.free()
    T.record_observed("gat_edge_kernel", case="fwd addend f=%d" % f, worst=max(errs.values()))
    print("observed addend", f, errs)
    assert all(v <= QG.bound_of(FWD, k.split(" ", 1)[1]) for k, v in errs.items()), errs


@pytest.mark.parametrize("f", [7, 64, 128, 200, 256])
@PASSES
def test_zero_bias_is_bit_identical_to_the_plain_pass(ctx, pas, f):
    """bias = 0 on every nonzero against hnh_attn_qkv_* on the same operands: np.array_equal for everything the pass writes, overwriting and
    accumulating, whole and one call per window."""
    zero, plain = EdgeProblem(ctx, pas, f, zero=True, seed=6), EdgeProblem(ctx, pas, f, plain=True, seed=6)
    for overwrite in ((True,) if pas == FWD else (True, False)):
        for groups in (None, GROUPINGS["one call per window"]):
            a, b = zero.run(overwrite, groups, act="elu"), plain.run(overwrite, groups, act="elu")
            assert np.abs(b["out"]).max() > 0 and same(a, b), (overwrite, groups)
    zero.free()
    plain.free()


def switched_off_block(pas, f, m=1024, seed=9):
    """A designed block (QKVProblem's `given`) for the switch-off value, and the entries that carry it.  The rows of S are the block's rows
    (forward, row pass) or its columns (column pass, the block standing for S^T).  35 rows of S have a single edge, made by rows of length 1
    and by 35 more columns that occur once each; `off` holds the last entry of every row of S with two or more edges and the only entry
    of every second single-edge row."""
    ncols = 768 if pas == COL else m
    extra = 35
    deg = G.mixed_degrees(m, seed + f).copy()
    deg[100:100 + extra] = 1
    rowptr, colidx, rows = G.graph(m, ncols - extra, deg, seed + 1)
    cols = colidx.astype(np.int64)
    add_rows = 200 + 3 * np.arange(extra)  # one more entry, the row's largest column, for these block rows
    rows = np.concatenate([rows, add_rows])
    cols = np.concatenate([cols, ncols - extra + np.arange(extra)])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    owner, n_own = (cols, ncols) if pas == COL else (rows, m)
    odeg = np.bincount(owner, minlength=n_own)
    last = np.full(n_own, -1)
    last[owner] = np.arange(len(owner))  # (the last entry of every row of S in the block's order)
    single = np.flatnonzero(odeg == 1)
    assert len(single) >= extra and np.count_nonzero(odeg >= 2) > 500
    off = np.concatenate([last[odeg >= 2], last[single[::2]]])
    rng = np.random.default_rng(5000 + f + pas)
    given = (rowptr, cols.astype(np.int32), rows, rng.uniform(-1, 1, (m, f)), rng.uniform(-1, 1, (ncols, f)), Q.scale_of(f))
    return given, off, owner, odeg


@pytest.mark.parametrize("f", [33, 128])
@PASSES
def test_switched_off_edges(ctx, pas, f):
    """-1e300 on one edge of every row of S that has another edge, and on the only edge of single-edge rows: against the pass references,
    where exp underflows to an exact 0 or is exp(0) = 1.  The forward pass's online softmax rescales by exp(-1e300 - m) = 0 or meets the
    switched-off edge first and forgets it at the next; lse of a switched-off single edge is -1e300 exactly and the output is V_j; the
    backward passes give such an edge p = 1 and every other switched-off edge p = 0, to the bit of the reference's exp."""
    given, off, owner, odeg = switched_off_block(pas, f)
    p = EdgeProblem(ctx, pas, f, off=off, given=given)
    is_off = np.zeros(p.nnz, dtype=bool)
    is_off[off] = True
    alone = is_off & (odeg[owner] == 1)
    assert np.count_nonzero(alone) >= 15 and np.count_nonzero(is_off & ~alone) > 500
    got, want = p.run(True, act="identity"), p.want(True, act="identity")
    assert all(np.all(np.isfinite(v)) for k, v in got.items() if k != "state")
    errs = {k: T.rel(np.longdouble(got[k]), want[k]) for k in ("out", "out2") if k in got}
    if pas == FWD:
        gone = np.zeros(p.m, dtype=bool)
        gone[p.rows[alone]] = True
        assert np.all(got["lse"][gone] == OFF) and np.all(got["values"][is_off] == OFF)
        assert np.array_equal(got["out"][gone], p.v[p.colidx[alone]][np.argsort(p.rows[alone])]), "a switched-off single edge: p = 1, o = V_j"
        errs["lse"] = T.rel(np.longdouble(got["lse"][~gone]), want["lse"][~gone])
        errs["values"] = T.rel(np.longdouble(got["values"][~is_off]), want["values"][~is_off])
    else:
        # the same block without the switched-off edges of rows that keep another: the same sums
        keep = ~(is_off & ~alone)
        rows, cols = p.rows[keep], p.colidx.astype(np.int64)[keep]
        packed = np.nan_to_num(p.packed)
        if pas == ROW:
            less = dict(out=E.row_pass(rows, cols, p.m, p.x, p.dz, p.lse_in, p.delta, packed, f, p.scale, p.bias[keep]))
        else:
            dk, dv = E.col_pass(rows, cols, p.m, p.x, p.x2, packed, f, p.scale, p.bias[keep])
            less = dict(out=dk, out2=dv)
        errs.update({"removed " + k: T.rel(got[k], v) for k, v in less.items()})
    assert same(p.run(True, GROUPINGS["one call per window"], act="identity"), got), "one call per window"
    p.free()
    T.record_observed("gat_edge_kernel", case="%s f=%d switched off" % (PASS_NAMES[pas], f), worst=max(errs.values()))
    print("observed switched off", PASS_NAMES[pas], f, errs)
    assert all(v <= QG.bound_of(pas, k.replace("removed ", "")) for k, v in errs.items()), errs


SPLIT_CASES = [(pas, f) for pas in (FWD, ROW, COL) for f in (64, 200)]


@pytest.mark.parametrize("pas,f", SPLIT_CASES, ids=lambda v: str(v))
def test_grouping_independence(ctx, pas, f):
    """Whole rows, one call per window and two uneven groupings of six windows: the same bits, overwriting and accumulating: bias[e] is
    entry e of the block however the nonzero is reached."""
    p = EdgeProblem(ctx, pas, f, seed=3)
    for overwrite in ((True,) if pas == FWD else (True, False)):
        whole = p.run(overwrite, act="elu")
        for name, groups in GROUPINGS.items():
            assert same(p.run(overwrite, groups, act="elu"), whole), (name, overwrite)
    QG.assert_within(pas, errors(p.run(True, GROUPINGS["uneven a"], act="elu"), p.want(True, act="elu")))
    p.free()


@pytest.mark.parametrize("pas,f", SPLIT_CASES, ids=lambda v: str(v))
def test_forced_panels_are_bit_identical(monkeypatch, pas, f):
    """Column panels (several launches over every row, hub rows after the last): the same bits as one launch, and right."""
    ncols = 1536
    c1 = K.Ctx(0)
    p1 = EdgeProblem(c1, pas, f, ncols=ncols, seed=5)
    one, want = p1.run(True, act="elu"), p1.want(True, act="elu")
    p1.free()
    c1.close()
    gather_w = P.fused_packed_width(f, pas == COL)
    monkeypatch.setenv("HNH_PANEL_BYTES", str(ncols * gather_w * 8 / 5))
    monkeypatch.setenv("HNH_MAX_PANELS", "8")
    monkeypatch.setenv("HNH_PANELS_WITH_HUBS", "1")
    c5 = K.Ctx(0)
    p5 = EdgeProblem(c5, pas, f, ncols=ncols, seed=5)
    assert c5.lib.hnh_panel_count(c5.h, p5.m, p5.nnz, ncols, min(gather_w, 512), int(np.diff(p5.rowptr).max())) == 5
    five = p5.run(True, act="elu")
    p5.free()
    c5.close()
    assert same(one, five)
    QG.assert_within(pas, errors(five, want))


@PASSES
def test_bad_arguments_are_refused_and_write_nothing(ctx, pas):
    p = EdgeProblem(ctx, pas, 34)
    a, blk = p.args(), p.block()
    lib = ctx.lib
    raw = (lib.hnh_attn_qkv_bias_fwd_csr_p, lib.hnh_attn_qkv_bias_row_csr_p, lib.hnh_attn_qkv_bias_col_csr_p)[pas]
    call = lambda a, flags, win=None, bias=p.bias_ptr(): raw(ctx.h, C.byref(blk), C.byref(a), bias, flags, win, K.STREAM_COMPUTE)  # noqa: E731
    a.f = 257
    assert call(a, K.FUSED_OUT_OVERWRITE) == K.ERR_UNSUPPORTED
    assert b"256" in lib.hnh_last_error(ctx.h) and b"HNH_ATTN_QKV_MAX_F" in lib.hnh_last_error(ctx.h)
    assert call(a, K.FUSED_OUT_OVERWRITE, bias=None) == K.ERR_UNSUPPORTED, "the width limit comes first, with its own code"
    a.f = 34
    rc = call(a, K.FUSED_OUT_OVERWRITE, bias=None)
    assert rc not in (0, K.ERR_UNSUPPORTED) and b"null bias" in lib.hnh_last_error(ctx.h), "bias == NULL is an error, not the plain pass"
    assert call(a, 4) == 1  # an unknown flag
    if pas == FWD:
        win = K.CsrWindow(None, p.windows(), 0)
        assert call(a, K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH, C.byref(win)) == 1 and b"last window" in lib.hnh_last_error(ctx.h)
    else:
        assert call(a, K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH) == 1  # a backward pass has no finish
    ctx.sync()
    assert p.untouched()
    p.free()


@PASSES
def test_empty_block(ctx, pas):
    """rowptr == NULL: overwrite (and the forward finish) leave zeros in the pass's outputs, accumulate leaves everything alone."""
    p = EdgeProblem(ctx, pas, 33)
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
def bias_fn(salt=0):
    return lambda r, c: E.hash_bias(r, c, salt=salt)


def model_bias(rows, cols, layers, only=None):
    return {li: E.hash_bias(rows, cols) for li in range(len(layers)) if only is None or li == only}


def edge_setup(world, rows, cols, m, x, layers, w, wq, wk, g, bias=None, res_weights=None, edge_layer=None, edge_fn=None, **kw):
    s = QG.qkv_setup(world, rows, cols, m, x, layers, w, wq, wk, g, bias, res_weights, **kw)
    if edge_fn is not False:
        s["gnn"].edge_bias_from(edge_fn or bias_fn(), layer=edge_layer)
    return s


def run_edge(world, rows, cols, m, x, layers, w, wq, wk, g, rounds=1, bias=None, res_weights=None, **kw):
    s = edge_setup(world, rows, cols, m, x, layers, w, wq, wk, g, bias, res_weights, **kw)
    res = dict(subA=s["subA"], subB=s["subB"], rounds=[QG.qkv_round(s, w, bias, res_weights) for _ in range(rounds)])
    teardown(s)
    return res


def reference(rows, cols, m, x, layers, w, wq, wk, g, edge_bias, **mode):
    dw, dwq, dwk, db, dwr, dx, _ = E.backward(rows, cols, m, x, layers, g, w, wq, wk, edge_bias=edge_bias, **mode)
    return dict(out=E.forward(rows, cols, m, x, layers, w, wq, wk, edge_bias=edge_bias, **mode), dw=dw, dwq=dwq, dwk=dwk, db=db, dwr=dwr, dx=dx)


def check_against(got, want, label, ranks, tol=TOL):
    errs = {name: T.rel(got[name], want[name]) for name in ("out", "dx")}
    for name in QG.REPLICATED:
        assert got[name].keys() == want[name].keys(), name
        for key in want[name]:
            assert np.abs(want[name][key]).max() > 0, (name, key)
            errs[(name, key)] = T.rel(got[name][key], want[name][key])
    worst = max(errs.values())
    T.record_observed("gat_edge", case=label, ranks=ranks, worst=worst)
    print("observed gat_edge", label, ranks, "worst %.2e" % worst)
    assert worst <= tol, errs
    return worst


ER8_RESULTS = {}
CONFIGS = {"plain": dict(),
           "published": dict(activation=("elu", "identity"), residual="projection", bias=True, dropout=(0.0, 0.3), seed=11)}


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_edge_bias_er8(p, config):
    rows, cols, m, x, layers, w, wq, wk, g = QG.er8_problem()
    kw = CONFIGS[config]
    extra = dict(bias=QG._BIAS, res_weights=QG._WRES) if kw.get("bias") else {}
    per_rank = H.run_spmd(p, lambda wd: run_edge(wd, rows, cols, m, x, layers, w, wq, wk, g, rounds=2, **dict(kw, **extra)))
    got = QG.assembled(per_rank, 0, m, layers)
    eb = model_bias(rows, cols, layers)
    want = reference(rows, cols, m, x, layers, w, wq, wk, g, eb, **QG.ref_mode(kw))
    unbiased = QG.reference(rows, cols, m, x, layers, w, wq, wk, g, **QG.ref_mode(kw))
    assert T.rel(want["out"], unbiased["out"]) > 1e-3 and np.ptp(eb[0]) > 3.0, "the bias matters"
    check_against(got, want, "er8_r16 %s p%d" % (config, p), p)
    again = QG.assembled(per_rank, 1, m, layers)
    assert np.array_equal(got["out"], again["out"]) and np.array_equal(got["dx"], again["dx"]), "two rounds must be bit-identical"
    assert all(np.array_equal(got[name][k], again[name][k]) for name in QG.REPLICATED for k in got[name])
    ER8_RESULTS[(p, config)] = got


def test_one_rank_and_eight_ranks_agree():
    rows, cols, m, x, layers, w, wq, wk, g = QG.er8_problem()
    res = {}
    for p in (1, 8):
        res[p] = ER8_RESULTS.get((p, "plain")) or QG.assembled(H.run_spmd(p, lambda wd: run_edge(wd, rows, cols, m, x, layers, w, wq, wk, g)), 0, m, layers)
    check_against(res[8], res[1], "er8_r16 p8 against p1", 8)


WIDE = {"256": [(256, 256, 1), (256, 64, 2)], "33": [(24, 33, 2), (66, 7, 3)]}


@pytest.mark.parametrize("p", [1, 4])
@pytest.mark.parametrize("shape", sorted(WIDE))
def test_edge_bias_widths(shape, p):
    m, layers = 1 << 12, WIDE[shape]
    rows, cols = H.generate_er(m, m, m * 16, 77)
    x = O.dense_fill(m, layers[0][0], 41) * 16.0
    w = hashed_weights(layers)
    wq, wk = Q.qk_weights_of(layers, seed=5, scale=0.2)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 3) * 64.0
    kw = dict(activation=("elu",) * (len(layers) - 1) + ("identity",))
    per_rank = H.run_spmd(p, lambda wd: run_edge(wd, rows, cols, m, x, layers, w, wq, wk, g, **kw))
    check_against(QG.assembled(per_rank, 0, m, layers), reference(rows, cols, m, x, layers, w, wq, wk, g, model_bias(rows, cols, layers), **QG.ref_mode(kw)),
                  "heads of %s p%d" % (shape, p), p)


@pytest.mark.parametrize("p", [1, 4])
def test_edge_bias_rmat_hub_rows(p):
    m, layers = 1 << 13, [(64, 64, 2), (128, 32, 2)]
    rows, cols = H.generate_rmat(13, m * 16)
    assert np.bincount(rows, minlength=m).max() >= 512 and np.bincount(cols, minlength=m).max() >= 512
    x = O.dense_fill(m, 64, 8) * 8.0
    w = hashed_weights(layers)
    wq, wk = Q.qk_weights_of(layers, seed=6, scale=0.3)
    g = O.dense_fill(m, 64, 4) * 32.0
    per_rank = H.run_spmd(p, lambda wd: run_edge(wd, rows, cols, m, x, layers, w, wq, wk, g, rounds=2))
    got = QG.assembled(per_rank, 0, m, layers)
    check_against(got, reference(rows, cols, m, x, layers, w, wq, wk, g, model_bias(rows, cols, layers)), "rmat hubs p%d" % p, p)
    again = QG.assembled(per_rank, 1, m, layers)
    assert np.array_equal(got["dx"], again["dx"]) and all(np.array_equal(got[n][k], again[n][k]) for n in QG.REPLICATED for k in got[n])


@pytest.mark.parametrize("p", [1, 4])
def test_bias_on_layer_zero_only(p):
    rows, cols, m, x, layers, w, wq, wk, g = QG.er8_problem()
    per_rank = H.run_spmd(p, lambda wd: run_edge(wd, rows, cols, m, x, layers, w, wq, wk, g, edge_layer=0))
    want = reference(rows, cols, m, x, layers, w, wq, wk, g, model_bias(rows, cols, layers, only=0))
    both = reference(rows, cols, m, x, layers, w, wq, wk, g, model_bias(rows, cols, layers))
    assert T.rel(want["out"], both["out"]) > 1e-3
    check_against(QG.assembled(per_rank, 0, m, layers), want, "layer 0 only p%d" % p, p)


@pytest.mark.parametrize("p", [1, 4])
def test_clearing_restores_the_plain_results_and_a_new_bias_invalidates_the_forward_pass(p):
    """set, run, clear, run: bit-identical to an object that never had a bias; set_edge_bias after a forward pass makes backwardPass refuse
    until a new forward; a refused set_edge_bias leaves bias and stored pass as they were."""
    rows, cols, m, x, layers, w, wq, wk, g = QG.er8_problem()

    def trip(world):
        s = edge_setup(world, rows, cols, m, x, layers, w, wq, wk, g)
        gnn = s["gnn"]
        with_bias = QG.qkv_round(s, w)
        gnn.forwardPass()
        gnn.edge_bias_from(bias_fn(salt=5), layer=1)
        with pytest.raises(H.HnhError, match="forwardPass"):
            gnn.backwardPass(s["g"])
        other = QG.qkv_round(s, w)
        gnn.edge_bias_from(bias_fn())
        gnn.forwardPass()
        short = H.Vec.create(world, 3, 0.0)
        with pytest.raises(H.HnhError, match="like_S_values length"):
            gnn.set_edge_bias(0, short, short)
        short.free()
        gnn.backwardPass(s["g"])  # (the refused call invalidated nothing)
        back = QG.qkv_round(s, w)
        for li in range(len(layers)):
            gnn.set_edge_bias(li, None, None)
        with pytest.raises(H.HnhError, match="forwardPass"):
            gnn.backwardPass(s["g"])
        cleared = QG.qkv_round(s, w)
        teardown(s)
        return with_bias, other, back, cleared

    def never(world):
        return QG.run_qkv(world, rows, cols, m, x, layers, w, wq, wk, g)["rounds"][0]

    for (with_bias, other, back, cleared), plain in zip(H.run_spmd(p, trip), H.run_spmd(p, never)):
        for a, b, equal in ((cleared, plain, True), (back, with_bias, True), (with_bias, plain, False), (other, with_bias, False)):
            eq = np.array_equal(a["out"], b["out"]) and np.array_equal(a["dx"], b["dx"]) and all(
                np.array_equal(a[n][k], b[n][k]) for n in ("dw", "dwq", "dwk") for k in w)
            assert eq == equal


@pytest.mark.parametrize("p", [1, 4])
def test_a_constant_bias_changes_nothing(p):
    """b = log 2 on every edge: a row-constant bias, so every p_e, the output and every gradient are those of no bias, to rounding"""
    rows, cols, m, x, layers, w, wq, wk, g = QG.er8_problem()
    per_rank = H.run_spmd(p, lambda wd: run_edge(wd, rows, cols, m, x, layers, w, wq, wk, g, edge_fn=lambda r, c: np.full(r.shape, np.log(2.0))))
    check_against(QG.assembled(per_rank, 0, m, layers), QG.reference(rows, cols, m, x, layers, w, wq, wk, g), "log 2 everywhere p%d" % p, p)


def switched_off_problem():
    """er8 with five rows cut down to a single edge; -1e300 on the edge with the largest column of every row that has another column, and on
    the single edge of three of the five; a hash elsewhere.  A function of the global (row, col): both copies of a repeated pair get it."""
    rows, cols, m, x, layers, w, wq, wk, g = QG.er8_problem()
    rows, cols = np.asarray(rows), np.asarray(cols)
    cut = np.flatnonzero(np.bincount(rows, minlength=m) >= 3)[:5]
    keep = np.ones(len(rows), dtype=bool)
    for i in cut:
        keep[np.flatnonzero(rows == i)[1:]] = False
    rows, cols = rows[keep], cols[keep]
    top = np.full(m, -1)
    np.maximum.at(top, rows, cols)
    low = np.full(m, m)
    np.minimum.at(low, rows, cols)
    off_row = top > low  # rows that keep another column
    off_row[cut[:3]] = True
    fn = lambda r, c: np.where(off_row[r] & (c == top[r]), OFF, E.hash_bias(r, c))  # noqa: E731
    return rows, cols, m, x, layers, w, wq, wk, g, fn, cut


@pytest.mark.parametrize("p", [1, 4])
def test_switched_off_edges_through_the_operator(p):
    """Against the model with the same bias, and against the model WITHOUT a bias on the graph that lacks the switched-off edges of rows with
    another edge (the hash bias kept): forward and backward, a switched-off single edge keeping p = 1."""
    rows, cols, m, x, layers, w, wq, wk, g, fn, cut = switched_off_problem()
    b = fn(rows, cols)
    deg = np.bincount(rows, minlength=m)
    assert np.count_nonzero((b == OFF) & (deg[rows] == 1)) == 3 and np.count_nonzero((b == OFF) & (deg[rows] >= 2)) > 200
    kw = dict(activation=("elu", "identity"))
    per_rank = H.run_spmd(p, lambda wd: run_edge(wd, rows, cols, m, x, layers, w, wq, wk, g, edge_fn=fn, **kw))
    got = QG.assembled(per_rank, 0, m, layers)
    eb = {li: b for li in range(len(layers))}
    check_against(got, reference(rows, cols, m, x, layers, w, wq, wk, g, eb, **QG.ref_mode(kw)), "switched off p%d" % p, p)
    gone = (b == OFF) & (deg[rows] >= 2)
    b2 = np.where(b == OFF, 0.0, b)[~gone]  # (alone in its row any bias is a row constant)
    check_against(got, reference(rows[~gone], cols[~gone], m, x, layers, w, wq, wk, g, {li: b2 for li in range(len(layers))}, **QG.ref_mode(kw)),
                  "switched off p%d against the graph without" % p, p)


def test_refusals_on_the_device():
    rows, cols, m, _ = er8()

    def rank(world):
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, "15d_fusion2", sp, 16, 1)
        layers = [(16, 8, 2)]
        for score in ("dot", "additive", "gatv2"):
            gnn = H.GAT(d, layers, ALPHA, attention="softmax", score=score)
            gnn.edge_bias_from(bias_fn())
            g = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
            words = "edge bias of layer 0 supports score transformer only, not score %s" % score
            with pytest.raises(H.HnhError, match=words):
                gnn.forwardPass()
            with pytest.raises(H.HnhError, match=words):
                gnn.backwardPass(g)
            world.sync()  # nothing was left in flight
            gnn.set_edge_bias(0, None, None)
            gnn.forwardPass()  # ... and the score runs as before once the bias is cleared
            g.free()
            gnn.free()
        gnn = H.GAT(d, layers, ALPHA, attention="softmax", score="transformer")
        s, st = d.like_S_values(0.0), d.like_ST_values(0.0)
        with pytest.raises(H.HnhError, match="both orders"):
            gnn.set_edge_bias(0, s, None)
        with pytest.raises(H.HnhError, match="out of range"):
            gnn.set_edge_bias(1, s, st)
        with pytest.raises(ValueError, match="finite"):
            gnn.edge_bias_from(lambda r, c: np.full(r.shape, -np.inf))
        with pytest.raises(ValueError, match="largest edge bias of row .* every edge is switched off is not supported"):
            gnn.edge_bias_from(lambda r, c: np.where(r == r.min(), OFF, 0.0))
        world.sync()
        for h in (s, st, gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(2, rank))


# ------------------------------------------------------------------------------------------------ training
def device_train(world, pp, layers, wq, wk, steps):
    s = edge_setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["w"], wq, wk, None, activation=QG.PUBLISHED)
    gnn = s["gnn"]
    gnn.set_labels(pp["labels"], pp["mask"], heads="mean")
    opt = dict(QG.ADAM)
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
def test_adam_trajectory_with_an_edge_bias(p):
    """Five steps of train_step with a fixed edge bias: within 10 x the divergence of a reference run whose gradients are perturbed at
    1e-10, parameters bit-equal across ranks, and not the trajectory of the unbiased model."""
    layers, steps = T.GAT_LAYERS, 5
    pp = R.planted_partition(layers)
    wq, wk = Q.qk_weights_of(layers)
    eb = model_bias(pp["rows"], pp["cols"], layers)
    args = (pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["labels"], pp["mask"], "mean", pp["w"], wq, wk)
    ref = E.train(*args, QG.ADAM, steps, edge_bias=eb, activations=QG.PUBLISHED)
    per = E.train(*args, QG.ADAM, steps, edge_bias=eb, activations=QG.PUBLISHED, perturb=(1e-10, np.random.default_rng(7)))
    unbiased = Q.train(*args, QG.ADAM, steps, activations=QG.PUBLISHED)
    bound_p = 10.0 * E.parameter_divergence(per, ref)
    bound_l = 10.0 * float(np.max(np.abs(np.array(per[0]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    assert bound_p > 0 and bound_l > 0 and E.parameter_divergence(unbiased, ref) > 1e3 * bound_p
    per_rank = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, wq, wk, steps))
    r0 = per_rank[0]
    for pr in per_rank:
        assert pr["losses"] == r0["losses"] and pr["accs"] == r0["accs"]
        assert all(np.array_equal(pr[n][k], r0[n][k]) for n in ("w", "wq", "wk") for k in r0["w"]), "parameters are bit-equal across ranks"
    got_p = E.parameter_divergence((None, None, r0["w"], r0["wq"], r0["wk"]), ref[:5])
    got_l = float(np.max(np.abs(np.array(r0["losses"]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    T.record_observed("gat_edge_trajectory", ranks=p, parameters=got_p, parameters_bound=bound_p, loss=got_l, loss_bound=bound_l, first=r0["losses"][0],
                      last=r0["losses"][-1])
    print("observed gat_edge trajectory", p, "parameters %.2e (bound %.2e) loss %.2e (bound %.2e)" % (got_p, bound_p, got_l, bound_l), r0["losses"])
    assert got_p <= bound_p and got_l <= bound_l
    assert r0["accs"] == ref[1]
