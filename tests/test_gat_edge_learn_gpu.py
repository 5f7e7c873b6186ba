"""The learned per-edge bias of the GAT's score "transformer" on the GPU (include/hnh_attn_edge_grad.h, GAT.set_edge_bias_learned).

Kernel level, through ctypes, on test_gat_edge_gpu.EdgeProblem's blocks (empty rows, a repeated pair, rows of 200 - 300, hub rows of 600
and 1500; a square block for the row pass, a 1024 x 768 block standing for S^T for the column pass) with the gradient vector between two
guard zones of sentinels: hnh_attn_qkv_bias_grad_row_csr_p / _col_csr_p at widths 7, 33, 64, 100, 128, 200, 256 with operands at even and
at odd offsets: Out / Out2 np.array_equal to the BIAS entry point's on the same operands (overwriting and accumulating), dbias against
tests/gat_edge_learn_ref.py, accumulate = 1 onto a prefilled vector equal to the prefill plus the overwriting call's result to the bit;
split independence bit for bit, dbias included (one call per window, two uneven groupings, forced Infinity-Cache panels) at 64 and 200;
switched-off edges give an exact 0.0, and so does a single edge at -1e300 with integer operands (p = 1, <dZ, V> = delta); dbias == NULL is
refused behind the parents' refusals with nothing written; an empty block writes nothing.
Operator level: GAT.edge_bias_grad in both orders, matched to the numpy model through S_coordinates() / ST_coordinates(), on er8_r16
over 1, 2, 4, 8 loopback ranks with the asymmetric coordinate hash on every layer, every other gradient and the output np.array_equal to
the same object with the layers not learned; the two orders against each other; p = 8 against p = 1; heads of 256 and 33; the R-MAT graph
with hub rows; a bias learned on layer 0 only.  Five Adam steps through train_step with learned biases follow gat_edge_learn_ref.train,
switched-off entries staying -1e300 and an unlearned layer's bias staying as it was, to the bit.  Refusals on the device.

Bounds: TOL = 1e-10 for the backward kernels and the operator (tests/gat_gpu_harness.py, max |x - ref| / max |ref|); the two orders of one
gradient 1e-12 (the same expression from the same operands: only the butterfly's summation order can differ); the trajectory within 10 x
the divergence of a reference run whose gradients are perturbed at 1e-10 (the rule of test_gat_train_gpu.py), computed in the test.  The
observed worst cases are recorded with T.record_observed.

Observed on an MI355X (max |x - ref| / max |ref|): dbias of the row pass <= 6.4e-16 and of the column pass <= 8.1e-16 over every width and
both alignments; edge_bias_grad through the operator <= 1.2e-15 over every case, its two orders bit-equal in every case (recorded, not
asserted); the Adam trajectory 2.0e-15 (p = 1) and 1.7e-14 (p = 4) in the parameters, the biases included (bound 5.6e-6), 3.1e-16 in the
loss (bound 1.0e-10), the two orders of the trained bias bit-equal."""
import ctypes as C

import numpy as np
import pytest

import gat_edge_learn_ref as L
import gat_edge_ref as E
import gat_pass_ref as P
import gat_qkv_ref as Q
import gat_ref as R
import hnh_testlib as T
import test_gat_edge_gpu as EG
import test_gat_qkv_gpu as QG
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import ALPHA, COL, GROUPINGS, PASS_NAMES, ROW, TOL, ctx, er8, hashed_weights, hip_backend, same, teardown  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu
WIDTHS = [7, 33, 64, 100, 128, 200, 256]
OFF = EG.OFF
GUARD_N = 16        # entries of either guard zone round the gradient vector
GUARD = 7.25e77     # what they hold: a store would change it, an accumulating load-add-store too
ORDERS_TOL = 1e-12  # the S-order against the S^T-order gradient
PASSES = pytest.mark.parametrize("pas", [ROW, COL], ids=["row", "col"])


class GradProblem(EG.EdgeProblem):
    """An EdgeProblem with a gradient vector in the block's order, prefilled with uniform(-1, 1) between two guard zones, and the grad
    entry points.  accumulate: the entry point's argument; parent=True: the BIAS entry point on the same operands."""

    def __init__(self, ctx, pas, f, **kw):
        super().__init__(ctx, pas, f, **kw)
        assert pas in (ROW, COL)
        self.accumulate, self.parent = False, False
        self.pre = np.random.default_rng(31 + 7 * f + pas).uniform(-1, 1, self.nnz)
        self.db0 = np.concatenate([np.full(GUARD_N, GUARD), self.pre, np.full(GUARD_N, GUARD)])
        self.d["dbias"] = ctx.upload(self.db0)

    def dbias_ptr(self):
        return self.d["dbias"].ptr + 8 * GUARD_N

    def fn(self):
        if self.parent:
            return super().fn()
        lib = self.ctx.lib
        f = lib.hnh_attn_qkv_bias_grad_row_csr_p if self.pas == ROW else lib.hnh_attn_qkv_bias_grad_col_csr_p
        return lambda h, blk, a, flags, win, stream: f(h, blk, a, self.bias_ptr(), self.dbias_ptr(), int(self.accumulate), flags, win, stream)

    def reset(self):
        super().reset()
        self.d["dbias"].set(self.db0)

    def untouched(self):
        return super().untouched() and np.array_equal(self.d["dbias"].get(), self.db0)

    def collect(self):
        res = super().collect()
        db = self.d["dbias"].get()
        assert np.array_equal(db[:GUARD_N], self.db0[:GUARD_N]) and np.array_equal(db[-GUARD_N:], self.db0[-GUARD_N:]), "the guard zones are not written"
        res["dbias"] = db[GUARD_N:-GUARD_N]
        return res

    def run_as(self, overwrite=True, groups=None, accumulate=False, parent=False):
        self.accumulate, self.parent = accumulate, parent
        try:
            return self.run(overwrite, groups)
        finally:
            self.accumulate, self.parent = False, False

    def want_dbias(self):
        cols, packed = self.colidx.astype(np.int64), np.nan_to_num(self.packed)
        if self.pas == ROW:
            return L.row_pass(self.rows, cols, self.m, self.x, self.dz, self.lse_in, self.delta, packed, self.f, self.scale, self.bias)[1]
        return L.col_pass(self.rows, cols, self.m, self.x, self.x2, packed, self.f, self.scale, self.bias)[2]


def outputs_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("out", "out2") if k in b) and ("out2" in a) == ("out2" in b)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd-offset"])
@pytest.mark.parametrize("f", WIDTHS)
@PASSES
def test_grad_pass_vs_numpy(ctx, pas, f, odd):
    """Out / Out2 are the BIAS entry point's to the bit, overwriting and accumulating, whatever `accumulate` says; dbias against the
    reference; accumulate = 1 is the prefill plus the overwriting result to the bit; a repeat is bit-identical; guards untouched."""
    p = GradProblem(ctx, pas, f, odd=odd)
    deg = np.diff(p.rowptr)
    assert deg.max() >= 1500 and np.count_nonzero(deg == 0) > 20 and 600 in deg
    got = p.run_as(True)
    assert same(p.run_as(True), got), "a repeat must be bit-identical"
    for overwrite in (True, False):
        parent = p.run_as(overwrite, parent=True)
        assert np.array_equal(parent["dbias"], p.pre), "the BIAS entry point knows no dbias"
        for accumulate in (False, True):
            mine = p.run_as(overwrite, accumulate=accumulate)
            assert outputs_equal(mine, parent), (overwrite, accumulate)
            want = p.pre + got["dbias"] if accumulate else got["dbias"]
            assert np.array_equal(mine["dbias"], want), "accumulate is an argument of its own: HNH_FUSED_OUT_OVERWRITE governs Out alone"
    want = p.want_dbias()
    assert np.abs(want).max() > 0 and np.all(np.isfinite(got["dbias"]))
    err = T.rel(got["dbias"], want)
    p.free()
    T.record_observed("gat_edge_grad_kernel", case="%s f=%d%s" % (PASS_NAMES[pas], f, " odd" if odd else ""), worst=err)
    print("observed dbias", PASS_NAMES[pas], f, odd, "%.2e" % err)
    assert err <= TOL, err


SPLIT_CASES = [(pas, f) for pas in (ROW, COL) for f in (64, 200)]


@pytest.mark.parametrize("pas,f", SPLIT_CASES, ids=lambda v: str(v))
def test_grouping_independence(ctx, pas, f):
    """Whole rows, one call per window and two uneven groupings of six windows: the same bits, dbias included, overwriting and
    accumulating: every nonzero is visited by exactly one launch, which writes its entry and no other."""
    p = GradProblem(ctx, pas, f, seed=3)
    for overwrite in (True, False):
        for accumulate in (False, True):
            whole = p.run_as(overwrite, accumulate=accumulate)
            for name, groups in GROUPINGS.items():
                assert same(p.run_as(overwrite, groups, accumulate=accumulate), whole), (name, overwrite, accumulate)
    assert T.rel(p.run_as(True, GROUPINGS["uneven a"])["dbias"], p.want_dbias()) <= TOL
    p.free()


@pytest.mark.parametrize("pas,f", SPLIT_CASES, ids=lambda v: str(v))
def test_forced_panels_are_bit_identical(monkeypatch, pas, f):
    """Column panels (several launches over every row, hub rows in segments after the last): the same bits as one launch, and right."""
    ncols = 1536
    c1 = K.Ctx(0)
    p1 = GradProblem(c1, pas, f, ncols=ncols, seed=5)
    one, one_acc, want = p1.run_as(True), p1.run_as(False, accumulate=True), p1.want_dbias()
    p1.free()
    c1.close()
    gather_w = P.fused_packed_width(f, pas == COL)
    monkeypatch.setenv("HNH_PANEL_BYTES", str(ncols * gather_w * 8 / 5))
    monkeypatch.setenv("HNH_MAX_PANELS", "8")
    monkeypatch.setenv("HNH_PANELS_WITH_HUBS", "1")
    c5 = K.Ctx(0)
    p5 = GradProblem(c5, pas, f, ncols=ncols, seed=5)
    assert c5.lib.hnh_panel_count(c5.h, p5.m, p5.nnz, ncols, min(gather_w, 512), int(np.diff(p5.rowptr).max())) == 5
    five, five_acc = p5.run_as(True), p5.run_as(False, accumulate=True)
    p5.free()
    c5.close()
    assert same(one, five) and same(one_acc, five_acc)
    assert T.rel(five["dbias"], want) <= TOL


def integer_operands(p, alone):
    """dZ, V and delta of the problem replaced by small integers, delta of every single-edge row of S by its exact <dZ_i, V_j>: every sum
    is exact in any order, so the kernel's <dZ_i, V_j> - delta_i of such an edge is exactly 0."""
    rng = np.random.default_rng(99 + p.f)
    rows, cols = p.rows, p.colidx.astype(np.int64)
    p.dz = rng.integers(-4, 5, p.dz.shape).astype(np.float64)
    p.delta = rng.integers(-4, 5, p.delta.shape).astype(np.float64)
    if p.pas == ROW:
        p.v = rng.integers(-4, 5, p.v.shape).astype(np.float64)
        p.delta[rows[alone]] = np.einsum("ij,ij->i", p.dz[rows[alone]], p.v[cols[alone]])
        p.packed = P.fused_pack(p.y1, p.v)
        p.d["dz"].set(QG.padded(p.dz, p.ld_dz, p.off))
        p.d["delta"].set(p.delta)
    else:
        p.x2 = rng.integers(-4, 5, p.x2.shape).astype(np.float64)
        p.delta[cols[alone]] = np.einsum("ij,ij->i", p.x2[rows[alone]], p.dz[cols[alone]])
        p.packed = P.fused_pack(p.y1, p.dz, p.lse_in, p.delta)
        p.d["x2"].set(QG.padded(p.x2, p.ld_x2, p.off))
    p.d["y"].set(QG.padded(p.packed[:, :p.pw], p.ld_y, 0))


@pytest.mark.parametrize("f", [33, 128])
@PASSES
def test_switched_off_edges_have_gradient_zero(ctx, pas, f):
    """-1e300 on one edge of every row of S that has another edge: p_e = 0 and dbias[e] == 0.0 exactly.  On the only edge of a row:
    p_e = exp(0) = 1 and, with integer operands, <dZ_i, V_j> = delta_i to the bit, so dbias[e] == 0.0 exactly as well.  Everything else
    against the reference; accumulating leaves such entries at their prefill."""
    given, off, owner, odeg = EG.switched_off_block(pas, f)
    p = GradProblem(ctx, pas, f, off=off, given=given)
    is_off = np.zeros(p.nnz, dtype=bool)
    is_off[off] = True
    alone = is_off & (odeg[owner] == 1)
    assert np.count_nonzero(alone) >= 15 and np.count_nonzero(is_off & ~alone) > 500
    integer_operands(p, alone)
    got, want = p.run_as(True), p.want_dbias()
    assert outputs_equal(got, p.run_as(True, parent=True))
    assert np.all(got["dbias"][is_off & ~alone] == 0.0), "a switched-off edge next to another: gradient 0 exactly"
    assert np.all(got["dbias"][alone] == 0.0), "a single edge at -1e300: p = 1 and <dZ, V> = delta"
    assert np.all(want[is_off] == 0.0) and np.abs(want[~is_off]).max() > 0
    acc = p.run_as(True, accumulate=True)
    assert np.array_equal(acc["dbias"][is_off], p.pre[is_off]) and np.array_equal(acc["dbias"], p.pre + got["dbias"])
    assert same(p.run_as(True, GROUPINGS["one call per window"]), got), "one call per window"
    err = T.rel(got["dbias"], want)
    p.free()
    T.record_observed("gat_edge_grad_kernel", case="%s f=%d switched off" % (PASS_NAMES[pas], f), worst=err)
    assert err <= TOL, err


@PASSES
def test_bad_arguments_are_refused_and_write_nothing(ctx, pas):
    """the parents' refusals first and with their codes, then the null bias, then dbias == NULL: an error, never the BIAS pass"""
    p = GradProblem(ctx, pas, 34)
    a, blk = p.args(), p.block()
    lib = ctx.lib
    raw = lib.hnh_attn_qkv_bias_grad_row_csr_p if pas == ROW else lib.hnh_attn_qkv_bias_grad_col_csr_p

    def call(a, flags, bias=p.bias_ptr(), dbias=p.dbias_ptr(), accumulate=0):
        return raw(ctx.h, C.byref(blk), C.byref(a), bias, dbias, accumulate, flags, None, K.STREAM_COMPUTE)

    a.f = 257
    assert call(a, K.FUSED_OUT_OVERWRITE, dbias=None) == K.ERR_UNSUPPORTED, "the width limit comes first, with its own code"
    assert b"HNH_ATTN_QKV_MAX_F" in lib.hnh_last_error(ctx.h)
    a.f = 34
    assert call(a, 4, dbias=None) == 1  # an unknown flag
    assert call(a, K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH) == 1  # a backward pass has no finish
    rc = call(a, K.FUSED_OUT_OVERWRITE, bias=None, dbias=None)
    assert rc not in (0, K.ERR_UNSUPPORTED) and b"null bias" in lib.hnh_last_error(ctx.h)
    for accumulate in (0, 1):
        rc = call(a, K.FUSED_OUT_OVERWRITE, dbias=None, accumulate=accumulate)
        assert rc not in (0, K.ERR_UNSUPPORTED) and b"null dbias" in lib.hnh_last_error(ctx.h), "dbias == NULL is an error, not the BIAS pass"
    ctx.sync()
    assert p.untouched()
    p.free()


@PASSES
def test_empty_block(ctx, pas):
    """rowptr == NULL: no entry to address, no dbias is touched (or looked at); the outputs are the parents': zeros when overwriting"""
    p = GradProblem(ctx, pas, 33)
    a = p.args()
    none = K.CsrBlock(p.m, 0, -1, 0, 0, None, None, None)
    p.accumulate = True
    ctx.check(p.fn()(ctx.h, C.byref(none), C.byref(a), 0, None, K.STREAM_COMPUTE), "empty block, accumulate")
    ctx.sync()
    assert p.untouched()
    p.accumulate = False
    ctx.check(p.fn()(ctx.h, C.byref(none), C.byref(a), K.FUSED_OUT_OVERWRITE, None, K.STREAM_COMPUTE), "empty block, overwrite")
    raw = ctx.lib.hnh_attn_qkv_bias_grad_row_csr_p if pas == ROW else ctx.lib.hnh_attn_qkv_bias_grad_col_csr_p
    ctx.check(raw(ctx.h, C.byref(none), C.byref(a), None, None, 0, K.FUSED_OUT_OVERWRITE, None, K.STREAM_COMPUTE), "empty block, null vectors")
    ctx.sync()
    got = p.collect()
    assert np.all(got["out"] == 0.0) and (pas != COL or np.all(got["out2"] == 0.0))
    assert np.array_equal(got["dbias"], p.pre), "no nonzero, no gradient entry"
    p.free()


# ------------------------------------------------------------------------------------------------ the operator
def by_coordinates(rows, cols, vals):
    """(rows, cols, vals) sorted by (row, col, value): the copies of a repeated pair carry one bias under a function of the coordinates, so
    their gradients are one expression of the same operands and may be matched in any order"""
    order = np.lexsort((vals, cols, rows))
    return np.asarray(rows)[order], np.asarray(cols)[order], np.asarray(vals)[order]


def learn_round(s, w, learned, bias=None, res_weights=None):
    """one round with the layers of `learned` learned: qkv_round's results, the gradient and the bias of every learned layer in both orders"""
    gnn = s["gnn"]
    for li in learned:
        gnn.set_edge_bias_learned(li)
    r = QG.qkv_round(s, w, bias, res_weights)
    r["deb"] = {li: gnn.edge_bias_grad(li) for li in learned}
    r["eb"] = {li: gnn.get_edge_bias(li) for li in learned}
    return r


def run_learn(world, rows, cols, m, x, layers, w, wq, wk, g, learned, bias=None, res_weights=None, **kw):
    """this rank's coordinates in both orders, a round with no layer learned, then two rounds with `learned`"""
    s = EG.edge_setup(world, rows, cols, m, x, layers, w, wq, wk, g, bias, res_weights, **kw)
    srows, scols = s["d"].S_coordinates()
    tcols, trows = s["d"].ST_coordinates()  # (an entry (j, i) of S^T is the nonzero (i, j) of S: named by S's coordinates)
    fixed = QG.qkv_round(s, w, bias, res_weights)
    with pytest.raises(H.HnhError, match="no GAT edge-bias gradient of layer 0 yet"):
        s["gnn"].edge_bias_grad(0)
    res = dict(subA=s["subA"], subB=s["subB"], coords=((srows, scols), (trows, tcols)), fixed=fixed,
               rounds=[learn_round(s, w, learned, bias, res_weights) for _ in range(2)])
    teardown(s)
    return res


def gathered(per_rank, k, li, which):
    """the world's gradient of layer li in order `which`, sorted by S's coordinates"""
    rows = np.concatenate([pr["coords"][which][0] for pr in per_rank])
    cols = np.concatenate([pr["coords"][which][1] for pr in per_rank])
    vals = np.concatenate([pr["rounds"][k]["deb"][li][which] for pr in per_rank])
    return by_coordinates(rows, cols, vals)


def check_learned(per_rank, rows, cols, m, x, layers, w, wq, wk, g, learned, eb, label, ranks, **mode):
    """edge_bias_grad in both orders against the model through the coordinates (TOL); the orders against each other (ORDERS_TOL, bit
    equality recorded); every other result np.array_equal to the round with nothing learned, and the second round to the first"""
    want = E.backward(rows, cols, m, x, layers, g, w, wq, wk, edge_bias=eb, **mode)[6]
    worst, between, bit_equal = 0.0, 0.0, True
    for li in learned:
        wr, wc, wv = by_coordinates(rows, cols, want[li])
        assert np.abs(wv).max() > 0
        got = [gathered(per_rank, 0, li, which) for which in (0, 1)]
        for gr, gc, gv in got:
            assert np.array_equal(gr, wr) and np.array_equal(gc, wc), "every nonzero of S has one entry on one rank"
            worst = max(worst, T.rel(gv, wv))
        between = max(between, T.rel(got[0][2], got[1][2]))
        bit_equal = bit_equal and np.array_equal(got[0][2], got[1][2])
    for pr in per_rank:
        a, b, again = pr["fixed"], pr["rounds"][0], pr["rounds"][1]
        for other in (b, again):
            assert np.array_equal(a["out"], other["out"]) and np.array_equal(a["dx"], other["dx"]), "a learned bias changes no other result"
            assert all(np.array_equal(a[n][key], other[n][key]) for n in QG.REPLICATED for key in a[n])
        for li in learned:
            assert all(np.array_equal(b["deb"][li][k], again["deb"][li][k]) for k in (0, 1)), "two rounds must be bit-identical"
    T.record_observed("gat_edge_grad", case=label, ranks=ranks, worst=worst, orders=between, orders_bit_equal=bool(bit_equal))
    print("observed gat_edge_grad", label, ranks, "worst %.2e, S against S^T order %.2e, bit-equal %s" % (worst, between, bit_equal))
    assert worst <= TOL, worst
    assert between <= ORDERS_TOL, between


ER8_GRADS = {}


@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_edge_bias_grad_er8(p):
    rows, cols, m, x, layers, w, wq, wk, g = QG.er8_problem()
    learned = tuple(range(len(layers)))
    per_rank = H.run_spmd(p, lambda wd: run_learn(wd, rows, cols, m, x, layers, w, wq, wk, g, learned))
    eb = EG.model_bias(rows, cols, layers)
    assert not np.array_equal(E.hash_bias(rows, cols), E.hash_bias(cols, rows)), "the coordinate hash is asymmetric"
    check_learned(per_rank, rows, cols, m, x, layers, w, wq, wk, g, learned, eb, "er8_r16 p%d" % p, p)
    ER8_GRADS[p] = {li: [gathered(per_rank, 0, li, which)[2] for which in (0, 1)] for li in learned}
    for pr in per_rank:  # get_edge_bias hands out what edge_bias_from set, in both orders
        (sr, sc), (tr, tc) = pr["coords"]
        assert all(np.array_equal(pr["rounds"][0]["eb"][li][0], E.hash_bias(sr, sc)) and np.array_equal(pr["rounds"][0]["eb"][li][1], E.hash_bias(tr, tc))
                   for li in learned)


def test_one_rank_and_eight_ranks_agree():
    rows, cols, m, x, layers, w, wq, wk, g = QG.er8_problem()
    learned = tuple(range(len(layers)))
    for p in (1, 8):
        if p not in ER8_GRADS:
            per_rank = H.run_spmd(p, lambda wd: run_learn(wd, rows, cols, m, x, layers, w, wq, wk, g, learned))
            ER8_GRADS[p] = {li: [gathered(per_rank, 0, li, which)[2] for which in (0, 1)] for li in learned}
    worst = max(T.rel(ER8_GRADS[8][li][k], ER8_GRADS[1][li][k]) for li in learned for k in (0, 1))
    T.record_observed("gat_edge_grad", case="er8_r16 p8 against p1", ranks=8, worst=worst)
    assert worst <= TOL, worst


@pytest.mark.parametrize("p", [1, 4])
@pytest.mark.parametrize("shape", sorted(EG.WIDE))
def test_edge_bias_grad_widths(shape, p):
    m, layers = 1 << 12, EG.WIDE[shape]
    rows, cols = H.generate_er(m, m, m * 16, 77)
    x = O.dense_fill(m, layers[0][0], 41) * 16.0
    w = hashed_weights(layers)
    wq, wk = Q.qk_weights_of(layers, seed=5, scale=0.2)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 3) * 64.0
    kw = dict(activation=("elu",) * (len(layers) - 1) + ("identity",))
    learned = tuple(range(len(layers)))
    per_rank = H.run_spmd(p, lambda wd: run_learn(wd, rows, cols, m, x, layers, w, wq, wk, g, learned, **kw))
    check_learned(per_rank, rows, cols, m, x, layers, w, wq, wk, g, learned, EG.model_bias(rows, cols, layers), "heads of %s p%d" % (shape, p), p,
                  **QG.ref_mode(kw))


@pytest.mark.parametrize("p", [1, 4])
def test_edge_bias_grad_rmat_hub_rows(p):
    m, layers = 1 << 13, [(64, 64, 2), (128, 32, 2)]
    rows, cols = H.generate_rmat(13, m * 16)
    assert np.bincount(rows, minlength=m).max() >= 512 and np.bincount(cols, minlength=m).max() >= 512
    x = O.dense_fill(m, 64, 8) * 8.0
    w = hashed_weights(layers)
    wq, wk = Q.qk_weights_of(layers, seed=6, scale=0.3)
    g = O.dense_fill(m, 64, 4) * 32.0
    learned = (0, 1)
    per_rank = H.run_spmd(p, lambda wd: run_learn(wd, rows, cols, m, x, layers, w, wq, wk, g, learned))
    check_learned(per_rank, rows, cols, m, x, layers, w, wq, wk, g, learned, EG.model_bias(rows, cols, layers), "rmat hubs p%d" % p, p)


@pytest.mark.parametrize("p", [1, 4])
def test_bias_learned_on_layer_zero_only(p):
    """a bias on both layers, layer 0's learned: its gradient is right, layer 1 has none to hand out, and the published configuration
    (bias, projection, feature dropout) runs on top"""
    rows, cols, m, x, layers, w, wq, wk, g = QG.er8_problem()
    kw = EG.CONFIGS["published"]
    extra = dict(bias=QG._BIAS, res_weights=QG._WRES)

    def rank(world):
        s = EG.edge_setup(world, rows, cols, m, x, layers, w, wq, wk, g, **dict(kw, **extra))
        srows, scols = s["d"].S_coordinates()
        tcols, trows = s["d"].ST_coordinates()
        fixed = QG.qkv_round(s, w, QG._BIAS, QG._WRES)
        rounds = [learn_round(s, w, (0,), QG._BIAS, QG._WRES) for _ in range(2)]
        with pytest.raises(H.HnhError, match="no GAT edge-bias gradient of layer 1 yet"):
            s["gnn"].edge_bias_grad(1)
        res = dict(subA=s["subA"], subB=s["subB"], coords=((srows, scols), (trows, tcols)), fixed=fixed, rounds=rounds)
        teardown(s)
        return res

    per_rank = H.run_spmd(p, rank)
    check_learned(per_rank, rows, cols, m, x, layers, w, wq, wk, g, (0,), EG.model_bias(rows, cols, layers), "layer 0 only, published p%d" % p, p,
                  **QG.ref_mode(kw))


def test_refusals_on_the_device():
    rows, cols, m, _ = er8()

    def rank(world):
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, "15d_fusion2", sp, 16, 1)
        layers = [(16, 8, 2)]
        gnn = H.GAT(d, layers, ALPHA, attention="softmax", score="transformer")
        g = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
        with pytest.raises(H.HnhError, match="set_edge_bias_learned: layer 0 has no edge bias to learn"):
            gnn.set_edge_bias_learned(0)
        with pytest.raises(H.HnhError, match="get_edge_bias: layer 0 has no edge bias"):
            gnn.get_edge_bias(0)
        gnn.edge_bias_from(EG.bias_fn())
        gnn.set_edge_bias_learned(0)
        words = "no GAT edge-bias gradient of layer 0 yet"
        with pytest.raises(H.HnhError, match=words):
            gnn.edge_bias_grad(0)
        gnn.forwardPass()
        with pytest.raises(H.HnhError, match=words):
            gnn.edge_bias_grad(0)  # a forward pass is no backward pass
        gnn.backwardPass(g)
        assert all(len(v) == len(b) for v, b in zip(gnn.edge_bias_grad(0), gnn.get_edge_bias(0)))
        for score in ("dot", "additive", "gatv2"):  # another score: the layer's bias is refused by name, and the gradient is dropped
            gnn.set_score(score)
            refusal = "edge bias of layer 0 supports score transformer only, not score %s" % score
            with pytest.raises(H.HnhError, match=refusal):
                gnn.forwardPass()
            with pytest.raises(H.HnhError, match=refusal):
                gnn.backwardPass(g)
            with pytest.raises(H.HnhError, match=words):
                gnn.edge_bias_grad(0)
            world.sync()  # nothing was left in flight
        gnn.set_score("transformer")
        gnn.forwardPass()
        gnn.backwardPass(g)
        gnn.edge_bias_grad(0)
        gnn.set_edge_bias_learned(0, False)  # switching off drops the gradient
        with pytest.raises(H.HnhError, match=words):
            gnn.edge_bias_grad(0)
        gnn.set_edge_bias_learned(0)
        gnn.backwardPass(g)
        gnn.edge_bias_grad(0)
        gnn.set_edge_bias(0, None, None)  # clearing the bias clears the switch and drops the gradient
        with pytest.raises(H.HnhError, match=words):
            gnn.edge_bias_grad(0)
        with pytest.raises(H.HnhError, match="no edge bias to learn"):
            gnn.set_edge_bias_learned(0)
        gnn.forwardPass()
        gnn.backwardPass(g)  # ... and the plain score runs as before
        world.sync()
        for h in (g, gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(2, rank))


# ------------------------------------------------------------------------------------------------ training
def training_problem(layers):
    """The planted partition with the coordinate hash on every layer and -1e300 on the entry with the largest column of every row that has
    another column: a function of the global coordinates, so both copies of a repeated pair carry it"""
    pp = R.planted_partition(layers)
    rows, cols, m = np.asarray(pp["rows"]), np.asarray(pp["cols"]), pp["m"]
    top = np.full(m, -1)
    np.maximum.at(top, rows, cols)
    low = np.full(m, m)
    np.minimum.at(low, rows, cols)
    fns = [lambda r, c, li=li: np.where((c == top[r]) & (top[r] > low[r]), OFF, E.hash_bias(r, c, salt=li)) for li in range(len(layers))]
    return pp, fns


def device_train(world, pp, layers, wq, wk, fns, learned, steps):
    s = EG.edge_setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["w"], wq, wk, None, activation=QG.PUBLISHED, edge_fn=False)
    gnn = s["gnn"]
    for li, fn in enumerate(fns):
        gnn.edge_bias_from(fn, layer=li)
    for li in learned:
        gnn.set_edge_bias_learned(li)
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
    res["eb"] = {li: gnn.get_edge_bias(li) for li in range(len(layers))}
    srows, scols = s["d"].S_coordinates()
    tcols, trows = s["d"].ST_coordinates()
    res["coords"] = ((srows, scols), (trows, tcols))
    res["eval"] = gnn.evaluate()  # evaluate works unchanged on top
    teardown(s)
    return res


TRAIN_REFS = {}


def train_reference(learned, layers, steps):
    if learned not in TRAIN_REFS:
        pp, fns = training_problem(layers)
        wq, wk = Q.qk_weights_of(layers)
        rows, cols = np.asarray(pp["rows"]), np.asarray(pp["cols"])
        eb = {li: fn(rows, cols) for li, fn in enumerate(fns)}
        args = (rows, cols, pp["m"], pp["x"], layers, pp["labels"], pp["mask"], "mean", pp["w"], wq, wk)
        kw = dict(edge_bias=eb, learned=learned, activations=QG.PUBLISHED)
        TRAIN_REFS[learned] = (pp, fns, wq, wk, eb, L.train(*args, QG.ADAM, steps, **kw),
                               L.train(*args, QG.ADAM, steps, perturb=(1e-10, np.random.default_rng(7)), **kw),
                               E.train(*args, QG.ADAM, steps, edge_bias=eb, activations=QG.PUBLISHED))
    return TRAIN_REFS[learned]


def live_divergence(a, b, live):
    """parameter_divergence over W, W_q, W_k and the biases' entries that are not switched off (those are compared to the bit)"""
    worst = Q.parameter_divergence((None, None) + tuple(a[:3]), (None, None) + tuple(b[:3]))
    for li in b[3]:
        worst = max(worst, T.rel(a[3][li][live], b[3][li][live]))
    return worst


@pytest.mark.parametrize("learned", [(0, 1), (0,)], ids=["both layers", "layer 0"])
@pytest.mark.parametrize("p", [1, 4])
def test_adam_trajectory_with_learned_biases(p, learned):
    """Five steps of train_step with learned biases (weight decay on, which the biases do not see): within 10 x the divergence of a
    reference run whose gradients are perturbed at 1e-10; the loss falls; switched-off entries are still -1e300 and an unlearned layer's
    bias is what was set, to the bit, in both orders; not the trajectory of the fixed bias."""
    layers, steps = T.GAT_LAYERS, 5
    pp, fns, wq, wk, eb, ref, per, fixed = train_reference(learned, layers, steps)
    rows, cols = np.asarray(pp["rows"]), np.asarray(pp["cols"])
    is_off = eb[0] == OFF
    assert np.count_nonzero(is_off) > 100 and all(np.array_equal(b == OFF, is_off) for b in eb.values())
    sr, sc, live = by_coordinates(rows, cols, (~is_off).astype(np.float64))
    live = live > 0
    model = lambda res: (res[2], res[3], res[4], {li: by_coordinates(rows, cols, res[5][li])[2] for li in learned})  # noqa: E731
    bound_p = 10.0 * live_divergence(model(per), model(ref), live)
    bound_l = 10.0 * float(np.max(np.abs(np.array(per[0]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    assert bound_p > 0 and bound_l > 0
    assert Q.parameter_divergence((None, None) + tuple(fixed[2:5]), (None, None) + tuple(ref[2:5])) > 1e3 * bound_p, "learning the bias matters"
    per_rank = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, wq, wk, fns, learned, steps))
    r0 = per_rank[0]
    for pr in per_rank:
        assert pr["losses"] == r0["losses"] and pr["accs"] == r0["accs"] and pr["eval"] == r0["eval"]
        assert all(np.array_equal(pr[n][k], r0[n][k]) for n in ("w", "wq", "wk") for k in r0["w"]), "replicated parameters are bit-equal across ranks"
    got_p, orders, orders_equal = 0.0, 0.0, True
    for which in (0, 1):
        dev = {}
        for li in range(len(layers)):
            gr, gc, gv = by_coordinates(np.concatenate([pr["coords"][which][0] for pr in per_rank]),
                                        np.concatenate([pr["coords"][which][1] for pr in per_rank]),
                                        np.concatenate([pr["eb"][li][which] for pr in per_rank]))
            assert np.array_equal(gr, sr) and np.array_equal(gc, sc)
            assert np.array_equal(gv[~live], np.full(np.count_nonzero(~live), OFF)), "switched-off entries stay -1e300 to the bit"
            if li in learned:
                dev[li] = gv
            else:
                assert np.array_equal(gv, by_coordinates(rows, cols, eb[li])[2]), "an unlearned layer's bias is unchanged to the bit"
        got_p = max(got_p, live_divergence((r0["w"], r0["wq"], r0["wk"], dev), model(ref), live))
        if which == 0:
            first = dev
        else:
            orders = max(T.rel(dev[li][live], first[li][live]) for li in learned)
            orders_equal = all(np.array_equal(dev[li], first[li]) for li in learned)
    got_l = float(np.max(np.abs(np.array(r0["losses"]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    T.record_observed("gat_edge_learn_trajectory", ranks=p, learned=list(learned), parameters=got_p, parameters_bound=bound_p, loss=got_l,
                      loss_bound=bound_l, first=r0["losses"][0], last=r0["losses"][-1], orders=orders, orders_bit_equal=bool(orders_equal))
    print("observed gat_edge_learn trajectory", p, learned, "parameters %.2e (bound %.2e) loss %.2e (bound %.2e) orders %.2e bit-equal %s"
          % (got_p, bound_p, got_l, bound_l, orders, orders_equal), r0["losses"])
    assert got_p <= bound_p and got_l <= bound_l
    assert r0["losses"][-1] < r0["losses"][0] and all(b < a for a, b in zip(ref[0], ref[0][1:])), "the loss falls"
    assert r0["accs"] == ref[1]
