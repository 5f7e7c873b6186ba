"""The GAT's dropout on the GPU (include/hnh_attn_dropout.h, GAT.set_dropout).

Kernel level, through ctypes: the device generator against numpy bit for bit; the three masked passes against the numpy reference
(tests/gat_pass_ref.py with `drop`; the forward pass against its extended-precision twin) at widths 1, 7, 33, 64, 100, 101, 128, 200, 255, 256 on the
blocks of gat_gpu_harness.Problem (empty rows, hub rows of 600 and 1500, repeated pairs, guards round every output) and on a block with
an R-MAT graph's degrees, with own-row ids that cross 2^31 and gathered-row ids that are a scattered relabelling; independence of
windows, groups of windows and forced Infinity-Cache panels, bit for bit; the helper kernels exactly.
Operator level: GAT(..., score="additive", dropout=(p, q), seed=s) on 15d_fusion2, c = 1 over 1, 2, 4, 8 loopback ranks against the numpy
definition (tests/gat_ref.py with rates) — output, every dW, da1, da2 and dX — at T.GAT_LAYERS, the benchmark widths and on an R-MAT graph with hub rows; 8 ranks
against 1; seeds; the refusal of a backward pass after a new seed; rates (0, 0) bit-identical to an object without dropout.

Bounds: those of test_gat_additive_gpu.py — 1e-12 for the forward kernel against the extended-precision reference, 1e-10 for the backward
kernels and the operator.  The observed worst cases are recorded with T.record_observed."""

import numpy as np
import pytest

import gat_gpu_harness as G
import gat_pass_ref as P
import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import (COL, FTOL, FWD, GROUPINGS, PASS_NAMES, ROW, TOL, DropProblem, assembled, ctx, er8, errors, hashed_weights,  # noqa: F401
                             hip_backend, one_round, same, setup, teardown)
from oracle import oracle as O

pytestmark = pytest.mark.gpu
WIDTHS = [1, 7, 33, 64, 100, 101, 128, 200, 255, 256]
MODE = dict(attention="softmax", score="additive")


# ------------------------------------------------------------------------------------------------ the generator
def test_device_words_match_numpy(ctx):
    n = 1000000
    rng = np.random.default_rng(21)
    gi, gj = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    gi[:4], gj[:4] = [0, 0xFFFFFFFF, 1 << 31, 5], [0, 0xFFFFFFFF, 7, 1 << 31]
    assert np.count_nonzero(gi >= 1 << 31) > n // 4 and np.count_nonzero(gj >= 1 << 31) > n // 4
    d_gi, d_gj, d_out = ctx.upload(gi), ctx.upload(gj), K.DevArray(ctx, n, np.uint32)
    for seed, w2, tag in ((0, 0, 0), (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 1), (0x0123456789ABCDEF, 3 * 65536 + 2, 0), (0x0123456789ABCDEF, 3, 1)):
        ctx.check(ctx.lib.hnh_dropout_words_u32(ctx.h, d_out.ptr, d_gi.ptr, d_gj.ptr, n, seed, w2, tag, K.STREAM_COMPUTE), "words")
        assert np.array_equal(d_out.get(), P.word(seed, tag, w2, gi, gj)), (seed, w2, tag)
    for d in (d_gi, d_gj, d_out):
        d.free()


# ------------------------------------------------------------------------------------------------ kernels
def check_pass(p, label):
    pas = p.pas
    deg = np.diff(p.rowptr)
    ck = p.factor()
    kept = np.bincount(p.rows, weights=ck > 0, minlength=p.m)
    assert 0.3 < np.count_nonzero(ck) / len(ck) < 0.5, "about 40 % of the edges are kept"
    got, want = p.run(True), p.want(True)
    empty, all_dropped = deg == 0, (deg > 0) & (kept == 0)
    assert np.count_nonzero(all_dropped) > 0
    for k in got:
        if k != "state":
            assert np.all(got[k][empty] == 0.0), "rows without nonzeros: o = 0, lse = 0, sums = 0"
    if pas == FWD:
        assert np.all(got["out"][all_dropped] == 0.0) and np.all(got["lse"][all_dropped] != 0.0), "every edge dropped: o = 0, lse kept"
    if pas == COL:
        assert np.all(got["out"][all_dropped] == 0.0)
    assert all(np.abs(np.float64(v)).max() > 0 for v in want.values())
    errs = errors(got, want)
    assert same(p.run(True), got), "a repeat must be bit-identical"
    if pas != FWD:
        acc = p.run(False)
        errs.update({"acc " + k: v for k, v in errors(acc, p.want(False)).items()})
    T.record_observed("gat_dropout_kernel", case=label, worst=max(errs.values()))
    print("observed", label, errs)
    assert max(errs.values()) <= (FTOL if pas == FWD else TOL), errs
    return got


@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_pass_vs_numpy(ctx, pas, f):
    p = DropProblem(ctx, pas, f)
    deg = np.diff(p.rowptr)
    assert deg.max() >= 1500 and np.count_nonzero(deg == 0) > 100 and 600 in deg
    got = check_pass(p, "%s f=%d" % (PASS_NAMES[pas], f))
    # the mask is a function of the seed: another seed gives other numbers, the plain entry point yet others
    p.drop.seed += 1
    assert not same(p.run(True), got)
    p.free()


@pytest.mark.parametrize("f", [64, 255])
@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_pass_on_rmat_degrees(ctx, pas, f):
    """A block with the row degrees of an R-MAT graph: hub rows of several hundred to thousands of nonzeros beside many short ones."""
    m = 2048
    rows, _ = H.generate_rmat(11, m * 24)
    deg = np.minimum(np.bincount(rows, minlength=m), 1536)
    assert deg.max() >= 600 and np.count_nonzero(deg >= 257) >= 8 and np.count_nonzero(deg <= 4) > 100
    p = DropProblem(ctx, pas, f, seed=7, degrees=deg)
    check_pass(p, "%s f=%d rmat" % (PASS_NAMES[pas], f))
    p.free()


@pytest.mark.parametrize("f", [7, 64, 128, 256])
@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_grouping_independence(ctx, pas, f):
    """Whole rows, one call per window and two uneven groupings of six windows: the same bits, overwriting and accumulating."""
    p = DropProblem(ctx, pas, f, seed=3)
    for overwrite in ((True,) if pas == FWD else (True, False)):
        whole = p.run(overwrite)
        for name, groups in GROUPINGS.items():
            assert same(p.run(overwrite, groups), whole), (name, overwrite)
    p.free()


@pytest.mark.parametrize("f", [64, 256])
@pytest.mark.parametrize("pas", [FWD, ROW, COL], ids=["fwd", "row", "col"])
def test_forced_panels_are_bit_identical(monkeypatch, pas, f):
    ncols = 1536
    c1 = K.Ctx(0)
    p1 = DropProblem(c1, pas, f, seed=5)
    one, want = p1.run(True), p1.want(True)
    p1.free()
    c1.close()
    gather_w = P.scored_width(f, ids=True)  # (= the packed width)
    monkeypatch.setenv("HNH_PANEL_BYTES", str(ncols * gather_w * 8 / 5))
    monkeypatch.setenv("HNH_MAX_PANELS", "8")
    monkeypatch.setenv("HNH_PANELS_WITH_HUBS", "1")
    c5 = K.Ctx(0)
    p5 = DropProblem(c5, pas, f, seed=5)
    assert c5.lib.hnh_panel_count(c5.h, p5.m, int(p5.rowptr[-1]), ncols, gather_w, int(np.diff(p5.rowptr).max())) == 5
    five = p5.run(True)
    p5.free()
    c5.close()
    assert same(one, five)
    assert max(errors(five, want).values()) <= (FTOL if pas == FWD else TOL)


def test_helper_kernels(ctx):
    lib = ctx.lib
    rng = np.random.default_rng(4)
    row_id0 = (1 << 32) - 301
    for f in WIDTHS:
        rows, fp = 301, f + (f & 1)
        ld_a, ld_m, ld_q, ld_dz = f + 3, fp + 6, fp + 6, f + 5
        a, dz = rng.uniform(-1, 1, (rows, ld_a)), rng.uniform(-1, 1, (rows, ld_dz))
        a1, a2 = rng.uniform(-1, 1, f), rng.uniform(-1, 1, f)
        lse, delta = rng.uniform(0, 3, rows), rng.uniform(-1, 1, rows)
        dev = {k: ctx.upload(v) for k, v in dict(a=a, dz=dz, a1=a1, a2=a2, lse=lse, delta=delta, m=np.full((rows + 1, ld_m), 7.0),
                                                 q=np.full((rows + 1, ld_q), 7.0)).items()}
        ctx.check(lib.hnh_attn_drop_scores_f64(ctx.h, dev["m"].ptr, ld_m, dev["a"].ptr, ld_a, dev["a1"].ptr, dev["a2"].ptr, rows, f, row_id0,
                                               K.STREAM_COMPUTE), "scores")
        ctx.check(lib.hnh_attn_drop_pack_f64(ctx.h, dev["q"].ptr, ld_q, dev["dz"].ptr, ld_dz, dev["m"].ptr, ld_m, dev["lse"].ptr, dev["delta"].ptr, rows, f,
                                             row_id0, K.STREAM_COMPUTE), "pack")
        gm, gq = dev["m"].get(), dev["q"].get()
        ids = row_id0 + np.arange(rows)
        wm = P.scored(a[:, :f], a1, a2, ids)
        assert np.array_equal(gm[:rows, :fp], wm[:, :fp]) and T.rel(gm[:rows, fp:fp + 2], wm[:, fp:fp + 2]) <= T.TOL, f
        assert np.array_equal(gm[:rows, fp + 2:fp + 4], wm[:, fp + 2:]) and np.all(gm[:rows, fp + 4:] == 7.0) and np.all(gm[rows] == 7.0), "ids exact, slot 3 zero"
        wq = P.pack(dz[:, :f], gm[:rows, fp], lse, delta, ids)
        assert np.array_equal(gq[:rows, :fp + 4], wq) and np.all(gq[:rows, fp + 4:] == 7.0) and np.all(gq[rows] == 7.0), f
        assert lib.hnh_attn_drop_scores_f64(ctx.h, dev["m"].ptr, fp + 2, dev["a"].ptr, ld_a, dev["a1"].ptr, dev["a2"].ptr, rows, f, row_id0, K.STREAM_COMPUTE) == 1
        assert lib.hnh_attn_drop_scores_f64(ctx.h, dev["m"].ptr, ld_m, dev["a"].ptr, ld_a, dev["a1"].ptr, dev["a2"].ptr, rows, f, row_id0 + 1, K.STREAM_COMPUTE) == 1, \
            "ids beyond 32 bits are refused"
        for d in dev.values():
            d.free()
    # the feature mask: dst = scale * mask o src, exactly; into another matrix with other pitches, and in place
    for rows, cols, q, layer in ((301, 33, 0.6, 0), (64, 256, 0.3, 2), (1, 1, 0.9, 1)):
        src = rng.uniform(-1, 1, (rows + 1, cols + 3))
        d_src, d_dst = ctx.upload(src), ctx.upload(np.full((rows + 1, cols + 5), 7.0))
        seed, scale = 0xFEEDFACE12345678, 1.0 / (1.0 - q)
        want = P.feature_factor(seed, layer, (rows, cols), q, row_id0) * src[:rows, :cols]
        assert np.array_equal(P.feature_factor(seed, layer, (rows, cols), q, row_id0) > 0, P.keep(seed, 1, layer, (row_id0 + np.arange(rows))[:, None],
                                                                                             np.arange(cols)[None, :], q))
        ctx.check(lib.hnh_feat_drop_f64(ctx.h, d_dst.ptr, cols + 5, d_src.ptr, cols + 3, rows, cols, row_id0, seed, layer, K.dropout_threshold(q), scale,
                                        K.STREAM_COMPUTE), "feat")
        got = d_dst.get()
        assert np.array_equal(got[:rows, :cols], want) and np.all(got[:rows, cols:] == 7.0) and np.all(got[rows] == 7.0)
        ctx.check(lib.hnh_feat_drop_f64(ctx.h, d_src.ptr, cols + 3, d_src.ptr, cols + 3, rows, cols, row_id0, seed, layer, K.dropout_threshold(q), scale,
                                        K.STREAM_COMPUTE), "feat in place")
        got = d_src.get()
        assert np.array_equal(got[:rows, :cols], want) and np.array_equal(got[:, cols:], src[:, cols:]) and np.array_equal(got[rows], src[rows])
        d_src.free()
        d_dst.free()


# ------------------------------------------------------------------------------------------------ the operator
def run_dropout(world, rows, cols, m, x, layers, weights, vectors, g_glob, configs, **kw):
    """One object, one round per (rates, seed) of configs."""
    s = setup(world, rows, cols, m, x, layers, weights, vectors, g_glob, **MODE, **kw)
    rounds = []
    for rates, seed in configs:
        if rates is not None:
            s["gnn"].set_dropout(rates[0], rates[1], seed)
        rounds.append(one_round(s, weights, True))
    res = dict(subA=s["subA"], subB=s["subB"], rounds=rounds)
    teardown(s)
    return res


def reference(rows, cols, m, x, layers, w, av, g, rates, seed):
    return G.reference(rows, cols, m, x, layers, w, av, g, rates=rates, seed=seed, **MODE)


def check_against(got, want, label, ranks):
    G.compare(got, want, "gat_additive", label, ranks)


CONFIGS = [((0.6, 0.6), 1), ((0.6, 0.0), 1), ((0.6, 0.6), 0xDEADBEEF00000002), ((0.6, 0.0), 0xDEADBEEF00000002), ((0.6, 0.6), 1)]
ER8_RESULTS = {}


@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_dropout_er8(p):
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w, av = hashed_weights(layers), R.vectors_of(layers)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 9) * 16.0
    per_rank = H.run_spmd(p, lambda wd: run_dropout(wd, rows, cols, m, x, layers, w, av, g, CONFIGS))
    got = [assembled(per_rank, k, m, layers) for k in range(len(CONFIGS))]
    for k, (rates, seed) in enumerate(CONFIGS[:4]):
        check_against(got[k], reference(rows, cols, m, x, layers, w, av, g, rates, seed), "er8_r16 p%d rates %s seed %x" % (p, rates, seed), p)
    assert np.array_equal(got[0]["out"], got[4]["out"]) and np.array_equal(got[0]["dx"], got[4]["dx"]), "the same seed gives the same bits"
    assert all(np.array_equal(got[0]["dw"][k], got[4]["dw"][k]) and np.array_equal(got[0]["da"][k][0], got[4]["da"][k][0]) for k in w)
    assert not np.array_equal(got[0]["out"], got[2]["out"]) and not np.array_equal(got[1]["out"], got[3]["out"]), "another seed gives another output"
    assert not np.array_equal(got[0]["out"], got[1]["out"])
    ER8_RESULTS[p] = got


def test_one_rank_and_eight_ranks_agree():
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w, av = hashed_weights(layers), R.vectors_of(layers)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 9) * 16.0
    res = {}
    for p in (1, 8):
        res[p] = ER8_RESULTS.get(p) or [assembled(H.run_spmd(p, lambda wd: run_dropout(wd, rows, cols, m, x, layers, w, av, g, CONFIGS[:2])), k, m, layers)
                                        for k in range(2)]
    for k in range(2):
        a, b = res[1][k], res[8][k]
        check_against(b, a, "er8_r16 p8 against p1 rates %s" % (CONFIGS[k][0],), 8)


BENCH_WIDTHS = (1 << 12, [(256, 256, 1), (256, 128, 2), (256, 64, 3)])


@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_dropout_benchmark_widths(p):
    m, layers = BENCH_WIDTHS
    rows, cols = H.generate_er(m, m, m * 16, 77)
    x = O.dense_fill(m, layers[0][0], 41) * 16.0
    w, av = hashed_weights(layers), R.vectors_of(layers, seed=5)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 3) * 64.0
    configs = [((0.6, 0.6), 5), ((0.6, 0.0), 5), ((0.6, 0.6), 6), ((0.6, 0.0), 6)] if p in (1, 8) else [((0.6, 0.6), 5), ((0.6, 0.0), 6)]
    per_rank = H.run_spmd(p, lambda wd: run_dropout(wd, rows, cols, m, x, layers, w, av, g, configs))
    for k, (rates, seed) in enumerate(configs):
        check_against(assembled(per_rank, k, m, layers), reference(rows, cols, m, x, layers, w, av, g, rates, seed),
                      "benchmark widths p%d rates %s seed %d" % (p, rates, seed), p)


@pytest.mark.parametrize("p", [1, 4])
def test_dropout_rmat_hub_rows(p):
    m, layers = 1 << 13, [(64, 64, 2), (128, 32, 2)]
    rows, cols = H.generate_rmat(13, m * 16)
    assert np.bincount(rows, minlength=m).max() >= 512 and np.bincount(cols, minlength=m).max() >= 512
    x = O.dense_fill(m, 64, 8) * 8.0
    w, av = hashed_weights(layers), R.vectors_of(layers, seed=6)
    g = O.dense_fill(m, 64, 4) * 32.0
    configs = [((0.6, 0.6), 9), ((0.6, 0.0), 9), ((0.6, 0.6), 9)]
    per_rank = H.run_spmd(p, lambda wd: run_dropout(wd, rows, cols, m, x, layers, w, av, g, configs))
    got = [assembled(per_rank, k, m, layers) for k in range(3)]
    for k in range(2):
        check_against(got[k], reference(rows, cols, m, x, layers, w, av, g, *configs[k]), "rmat hubs p%d rates %s" % (p, configs[k][0]), p)
    assert np.array_equal(got[0]["dx"], got[2]["dx"]) and all(np.array_equal(got[0]["da"][k][1], got[2]["da"][k][1]) for k in w), "a repeat must be bit-identical"


@pytest.mark.parametrize("p", [1, 4])
def test_a_new_seed_needs_a_new_forward_pass(p):
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w, av = hashed_weights(layers), R.vectors_of(layers)
    g = O.dense_fill(m, 12, 9) * 16.0

    def rank(world):
        s = setup(world, rows, cols, m, x, layers, w, av, g, attention="softmax", score="additive", dropout=(0.6, 0.6), seed=4)
        first = one_round(s, w, True)
        s["gnn"].set_dropout_seed(5)
        with pytest.raises(H.HnhError, match="forwardPass"):
            s["gnn"].backwardPass(s["g"])
        second = one_round(s, w, True)
        s["gnn"].set_dropout(0.6, 0.6, 4)
        with pytest.raises(H.HnhError, match="forwardPass"):
            s["gnn"].backwardPass(s["g"])
        third = one_round(s, w, True)
        teardown(s)
        return first, second, third

    for first, second, third in H.run_spmd(p, rank):
        assert not np.array_equal(first["out"], second["out"]) and not np.array_equal(first["dx"], second["dx"])
        assert np.array_equal(first["out"], third["out"]) and np.array_equal(first["dx"], third["dx"])
        assert all(np.array_equal(first["dw"][k], third["dw"][k]) for k in w)


@pytest.mark.parametrize("p", [1, 4])
def test_rates_zero_are_bit_identical_to_no_dropout(p):
    """dropout=(0, 0) with any seed, and (0, 0) after a round with dropout on the same object, against an object that never heard of it."""
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w, av = hashed_weights(layers), R.vectors_of(layers)
    g = O.dense_fill(m, 12, 9) * 16.0
    with_arg = H.run_spmd(p, lambda wd: run_dropout(wd, rows, cols, m, x, layers, w, av, g, [(None, 0), ((0.6, 0.6), 3), ((0.0, 0.0), 3)],
                                                    dropout=(0.0, 0.0), seed=77))
    plain = H.run_spmd(p, lambda wd: run_dropout(wd, rows, cols, m, x, layers, w, av, g, [(None, 0)]))
    for a, b in zip(with_arg, plain):
        want = b["rounds"][0]
        for k in (0, 2):
            got = a["rounds"][k]
            assert np.array_equal(got["out"], want["out"]) and np.array_equal(got["dx"], want["dx"])
            assert all(np.array_equal(got["dw"][key], want["dw"][key]) for key in w)
            assert all(np.array_equal(got["da"][key][i], want["da"][key][i]) for key in w for i in (0, 1))
        assert not np.array_equal(a["rounds"][1]["out"], want["out"])


def test_score_dot_refuses_attention_dropout_and_takes_feature_dropout():
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w = hashed_weights(layers)
    g = O.dense_fill(m, 12, 9) * 16.0

    def rank(world):
        s = setup(world, rows, cols, m, x, layers, w, None, g, attention="softmax", backward="fused", dropout=(0.6, 0.0), seed=2)
        with pytest.raises(H.HnhError, match=r"attention dropout.*score additive only.*score dot"):
            s["gnn"].forwardPass()
        world.sync()
        s["gnn"].set_dropout(0.0, 0.5, 2)
        r = one_round(s, w, False)
        res = dict(subA=s["subA"], subB=s["subB"], rounds=[r])
        teardown(s)
        return res

    per_rank = H.run_spmd(2, rank)
    dx = T.assemble_dense([dict(dx=pr["rounds"][0]["dx"], subB=pr["subB"]) for pr in per_rank], "dx", "subB", m, layers[0][0])
    mask = P.feature_factor(2, 0, x.shape, 0.5) > 0
    assert np.all(dx[~mask] == 0.0) and np.count_nonzero(dx[mask]) > 0.9 * np.count_nonzero(mask), "the input gradient carries layer 0's feature mask"
