"""The GAT's additive (a1, a2) attention score on the GPU (include/hnh_attn_additive.h, GAT score "additive").

Kernel level, through ctypes: the forward pass against the extended-precision numpy reference (tests/gat_pass_ref.py, fwd_pass_ld),
the backward row and column passes against numpy, at widths 1, 2, 7, 16, 64, 100, 128, 200, 256 on blocks with empty rows, rows of 200 - 300,
hub rows of 600 and 1500 and repeated pairs, with pitches wider than the widths, an output block at an odd column offset of an odd
pitch, guard values around every output, and scores far outside exp's range (|z| about 800); their independence of how a row's
nonzeros are split into launches (whole rows, one call per window, two uneven groupings of six windows, forced Infinity-Cache panels),
bit for bit; the dense helpers; the width limit; empty blocks.
Operator level: GAT(..., attention="softmax", score="additive") on 15d_fusion2, c = 1 over 1, 2, 4, 8 loopback ranks against the numpy
definition (tests/gat_ref.py) — output, every dW, da1, da2 and dX — at the small shape, the benchmark widths and on an R-MAT graph with hub rows; p = 1
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

import gat_gpu_harness as G
import gat_pass_ref as P
import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import (ALPHA, COL, FTOL, FWD, GROUPINGS, PASS_NAMES, ROW, TOL, Problem, assembled, ctx, er8, errors, hashed_weights,  # noqa: F401
                             hip_backend, one_round, same, setup, teardown)
from oracle import oracle as O

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 7, 16, 64, 100, 128, 200, 256]
MODE = dict(attention="softmax", score="additive")


# ------------------------------------------------------------------------------------------------ kernels
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
    gather_w = P.packed_width(f) if pas == COL else P.scored_width(f)
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
        wm = P.scored(a[:, :f], a1, a2)
        assert np.array_equal(gm[:rows, :fp], wm[:, :fp]) and T.rel(gm[:rows, fp:fp + 2], wm[:, fp:]) <= T.TOL, f
        assert np.all(gm[:rows, fp + 2:] == 7.0) and np.all(gm[rows] == 7.0)
        wq = P.pack(dz[:, :f], gm[:rows, fp], lse, delta)
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
def run_additive(world, rows, cols, m, x, layers, weights, vectors, g_glob, rounds=1):
    return G.run_rounds(world, rows, cols, m, x, layers, weights, vectors, g_glob, rounds, **MODE)


def check_against(got, want, label, ranks):
    G.compare(got, want, "gat_additive", label, ranks)


def reference(rows, cols, m, x, layers, w, av, g):
    return G.reference(rows, cols, m, x, layers, w, av, g, **MODE)


ER8_RESULTS = {}


@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_additive_er8(p):
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w, av = hashed_weights(layers), R.vectors_of(layers)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 9) * 16.0
    per_rank = H.run_spmd(p, lambda wd: run_additive(wd, rows, cols, m, x, layers, w, av, g, rounds=2))
    got = assembled(per_rank, 0, m, layers)
    check_against(got, reference(rows, cols, m, x, layers, w, av, g), "er8_r16 p%d" % p, p)
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
    check_against(b, a, "er8_r16 p8 against p1", 8)


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
    check_against(assembled(per_rank, 0, m, layers), reference(rows, cols, m, x, layers, w, av, g), "%s p%d" % (shape, p), p)


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
    check_against(got, reference(rows, cols, m, x, layers, w, av, g), "rmat hubs p%d" % p, p)
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


@pytest.mark.parametrize("p", [1, 4])
def test_sgd_lowers_the_loss(p):
    """Five steps on W, a1 and a2 with the step size of tests/test_gat_additive_cpu.py::test_the_reference_trains."""
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    target = O.dense_fill(m, 12, 21) * R.SGD_TARGET_SCALE
    w, av = hashed_weights(layers), R.vectors_of(layers)
    per_rank = H.run_spmd(p, lambda wd: G.sgd(wd, rows, cols, m, x, layers, target, R.SGD_STEPS, R.SGD_LR_SCALE, w, av, **MODE))
    loss = np.sum(np.array([pr[0] for pr in per_rank]), axis=0)
    print("losses", loss)
    assert all(loss[i + 1] < loss[i] for i in range(R.SGD_STEPS)), loss
    start = R.vectors_of(layers)
    for _, av in per_rank:
        assert all(np.abs(av[k][i] - start[k][i]).max() > 0 for k in start for i in (0, 1)), "a1 and a2 have moved"
