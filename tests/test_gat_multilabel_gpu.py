"""The GAT's multi-label head on the GPU (include/hnh_train_multilabel.h; GAT.set_multilabel_targets / multilabel_counts, and loss / train_step
/ evaluate under the sigmoid head).

Kernel level, through ctypes.  hnh_bce_rows_f64 against the extended-precision numpy reference (tests/gat_multilabel_ref.py, bce_rows with
np.longdouble) for classes in {1, 2, 31, 32, 33, 64, 65, 121, 1000} x heads in {1, 3, 6}, with pitches wider than the row for out, G and
the target words, guard values round G, the four result words and the workspace, garbage in the unused bits of the last target word,
about 30 % of the rows masked out, every fifth row with logits in +-700 and rows of small integers that are the same in every head, so
that some head means are exactly 0 and must predict "absent"; more rows than one grid round takes and a row wider than
HNH_XENT_MAX_WIDTH; the argument refusals and a NaN.  Bounds: T.TOL (1e-11, the project's kernel bound) for loss_sum relatively and for G
normwise; tp / fp / fn exactly; masked-out rows of G exactly 0; a repeat bit-identical; G = null leaves G untouched and gives the same
results; G aliasing out gives the same bits; pos_weight = ones gives the bits of null.  Condition on the inputs, asserted: outside the
exact zeros |z| >= 1e-6 (a prediction must not hang on the last bit of a head mean).
Operator level, 15d_fusion2 with c = 1 on 1, 2, 4, 8 loopback ranks with the published activations (ELU, identity on the last layer: the
logits take both signs): loss with grad_out, then backwardPass, against the reference — loss, counts, G, every dW, da1, da2 and dX — for
score dot (backward unfused and fused) and score additive, heads "mean" and "concat", without and with pos_weight on the same object;
bound 1e-10, the operator bound of the other GAT tests; the counts exactly.
Trajectories: 10 train_steps with SGD with momentum and with Adam on 1 and 4 ranks against gat_multilabel_ref.train; the tolerance is
measured as tests/test_gat_train_gpu.py measures it: ten times the divergence of a reference run whose gradients are perturbed by 1e-10.
Parameters are bit-equal across ranks.
Head switching: set_multilabel_targets, then set_labels, then loss equals a fresh object that only called set_labels bit for bit, and the
other way round.
Learning: the planted tags of gat_multilabel_ref.planted_tags: the final train loss is at most half the first and the held-out micro-F1
at least 0.70 (tests/test_gat_multilabel_cpu.py derives the threshold from the reference's own run).

The observed errors and the measured bounds are recorded with T.record_observed."""
import numpy as np
import pytest

import gat_multilabel_ref as M
import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import ALPHA, TOL, ctx, er8, hashed_weights, hip_backend, setup, teardown  # noqa: F401

pytestmark = pytest.mark.gpu
GUARD = 7.0


# ------------------------------------------------------------------------------------------------ the loss kernel
def bce_inputs(rows, heads, classes, seed):
    """Logits (rows x heads * classes), 0/1 targets, a mask without about 30 % of the rows, class weights, and where z is exactly 0."""
    rng = np.random.default_rng(seed)
    n = heads * classes
    out = rng.uniform(-5.0, 5.0, (rows, n))
    big = np.arange(rows) % 5 == 1
    out[big] = rng.uniform(-700.0, 700.0, (np.count_nonzero(big), n))
    ints = np.arange(rows) % 11 == 3
    for r in np.flatnonzero(ints):
        vals = rng.integers(-2, 3, classes).astype(np.float64)  # (a fifth of them 0)
        if r % 22 == 3:
            vals[0] = 0.0
        out[r] = np.tile(vals, heads)
    inv_heads = 1.0 / heads
    z = out.reshape(rows, heads, classes).sum(axis=1) * inv_heads
    close = (np.abs(z) < 1e-3) & ~ints[:, None]
    out += np.tile(np.where(close, 0.01, 0.0), (1, heads))  # (move a random head mean away from 0: the condition below)
    z = out.reshape(rows, heads, classes).sum(axis=1) * inv_heads
    zero = z == 0.0
    assert np.all(np.abs(z[~zero]) >= 1e-6), "condition on the inputs: outside the exact zeros |z| >= 1e-6"
    assert not np.any(zero[~ints]) and np.count_nonzero(zero) > 0
    targets = rng.random((rows, classes)) < 0.4
    mask = rng.random(rows) >= 0.3
    pw = rng.uniform(0.0, 3.0, classes)
    return out, targets, mask, pw, zero


def run_bce(ctx, out, targets, mask, pw, heads, classes, inv_n, with_g=True, in_place=False, pad=(3, 5, 2)):
    rows, n = out.shape
    ld_out, ld_g, ld_t = n + pad[0], n + pad[1], (classes + 31) // 32 + pad[2]
    host = np.full((rows + 1, ld_out), np.nan)
    host[:rows, :n] = out
    need = int(ctx.lib.hnh_bce_rows_f64_workspace(rows))
    assert need > 0
    words = M.pack_bits(targets, ld_t, garbage=np.random.default_rng(rows + classes))
    assert np.array_equal(M.unpack_bits(words, classes), np.asarray(targets, dtype=bool))
    d_out, d_t, d_m = ctx.upload(host), ctx.upload(words), ctx.upload(np.ascontiguousarray(mask, dtype=np.uint8))
    d_pw = ctx.upload(np.ascontiguousarray(pw, dtype=np.float64)) if pw is not None else None
    d_g = ctx.upload(np.full((rows + 1, ld_g), GUARD))
    d_res, d_work = ctx.upload(np.full(6, GUARD)), ctx.upload(np.full(need + 2, GUARD))
    g_ptr, g_ld = (d_out.ptr, ld_out) if in_place else ((d_g.ptr if with_g else None), ld_g)
    rc = ctx.lib.hnh_bce_rows_f64(ctx.h, d_out.ptr, ld_out, d_t.ptr, ld_t, d_m.ptr, d_pw.ptr if d_pw else None, rows, heads, classes, inv_n, g_ptr, g_ld,
                                  d_res.ptr + 8, d_work.ptr + 8, need, K.STREAM_COMPUTE)
    ctx.check(rc, "hnh_bce_rows_f64")
    ctx.sync()
    res, work, g = d_res.get(), d_work.get(), (d_out.get() if in_place else d_g.get())
    assert res[0] == GUARD and res[5] == GUARD and work[0] == GUARD and work[-1] == GUARD, "guards round the result words and the workspace"
    if in_place:
        assert np.all(np.isnan(g[:rows, n:])) and np.all(np.isnan(g[rows]))
    elif with_g:
        assert np.all(g[:rows, n:] == GUARD) and np.all(g[rows] == GUARD), "guards round G"
    else:
        assert np.all(g == GUARD), "no gradient asked for: G untouched"
    for d in (d_out, d_t, d_m, d_g, d_res, d_work) + ((d_pw,) if d_pw else ()):
        d.free()
    return float(res[1]), float(res[2]), float(res[3]), float(res[4]), g[:rows, :n]


def reference(out, targets, mask, heads, inv_n, pw, chunk=20000):
    """bce_rows in np.longdouble over the masked-in rows, a block of them at a time; the other rows' G is 0 by definition"""
    live = np.flatnonzero(mask)
    parts = [M.bce_rows(out[live[a:a + chunk]], targets[live[a:a + chunk]], None, heads, inv_n, pw, np.longdouble) for a in range(0, len(live), chunk)]
    g = np.zeros(out.shape)
    g[live] = np.concatenate([np.float64(p[4]) for p in parts])
    return (sum(p[0] for p in parts), sum(p[1] for p in parts), sum(p[2] for p in parts), sum(p[3] for p in parts), g)


def same(a, b):
    return a[:4] == b[:4] and np.array_equal(a[4], b[4])


SHAPES = [(h, c) for c in (1, 2, 31, 32, 33, 64, 65, 121, 1000) for h in (1, 3, 6)]


@pytest.mark.parametrize("heads,classes", SHAPES)
def test_bce_kernel_vs_longdouble(ctx, heads, classes):
    rows = 301 if heads * classes > 512 else 1237
    out, targets, mask, pw, zero = bce_inputs(rows, heads, classes, seed=heads * 1000 + classes)
    inv_n = 1.0 / 137.0
    assert 0.6 * rows < np.count_nonzero(mask) < 0.8 * rows and np.any(zero[mask] & targets[mask]) and np.any(zero[mask] & ~targets[mask])
    worst = 0.0
    for weights in (None, pw):
        want = reference(out, targets, mask, heads, inv_n, weights)
        got = run_bce(ctx, out, targets, mask, weights, heads, classes, inv_n)
        assert np.all(got[4][~mask] == 0.0), "masked-out rows get G = 0"
        errs = dict(loss=abs(got[0] - float(want[0])) / float(want[0]), g=T.rel(got[4], want[4]))
        worst = max(worst, *errs.values())
        print("observed heads=%d classes=%d weighted=%s" % (heads, classes, weights is not None), errs, "tp fp fn", got[1:4], want[1:4])
        assert got[1:4] == tuple(float(v) for v in want[1:4]), "the counts are exact, and z == 0 predicts absent"
        assert max(errs.values()) <= T.TOL, errs
        assert same(run_bce(ctx, out, targets, mask, weights, heads, classes, inv_n), got), "a repeat must be bit-identical"
        assert run_bce(ctx, out, targets, mask, weights, heads, classes, inv_n, with_g=False)[:4] == got[:4]
        assert same(run_bce(ctx, out, targets, mask, weights, heads, classes, inv_n, in_place=True), got), "G may alias out"
        if weights is None:
            assert same(run_bce(ctx, out, targets, mask, np.ones(classes), heads, classes, inv_n), got), "pos_weight = ones gives the bits of null"
            assert got[3] >= np.count_nonzero(zero[mask] & targets[mask]) > 0
    T.record_observed("gat_multilabel_bce_kernel", case="heads=%d classes=%d" % (heads, classes), worst=worst)


@pytest.mark.parametrize("heads,classes,rows", [(1, 121, 140001), (6, 121, 40000), (1, 5000, 600)])
def test_bce_kernel_many_rows_and_wide_rows(ctx, heads, classes, rows):
    """More rows than one round of the grid takes, and a row beyond the softmax head's width limit."""
    assert rows > 2048 * 4 or heads * classes > K.XENT_MAX_WIDTH  # (2048 workgroups of 4 rows a round at this width)
    out, targets, mask, pw, _ = bce_inputs(rows, heads, classes, seed=rows)
    inv_n = 1.0 / (np.count_nonzero(mask) * classes)
    want = reference(out, targets, mask, heads, inv_n, pw)
    got = run_bce(ctx, out, targets, mask, pw, heads, classes, inv_n, pad=(1, 0, 0))
    errs = dict(loss=abs(got[0] - float(want[0])) / float(want[0]), g=T.rel(got[4], want[4]))
    T.record_observed("gat_multilabel_bce_kernel", case="heads=%d classes=%d rows=%d" % (heads, classes, rows), worst=max(errs.values()))
    print("observed", heads, classes, rows, errs)
    assert got[1:4] == tuple(float(v) for v in want[1:4]) and max(errs.values()) <= T.TOL, errs
    assert np.all(got[4][~mask] == 0.0)
    assert same(run_bce(ctx, out, targets, mask, pw, heads, classes, inv_n, pad=(1, 0, 0)), got)


def test_bce_kernel_refusals_and_nan(ctx):
    lib = ctx.lib
    d = ctx.upload(np.zeros(16))
    res = ctx.upload(np.full(4, GUARD))
    bad = [dict(heads=0), dict(classes=0), dict(heads=-1), dict(ld_out=7), dict(ld_g=7, g=True), dict(ld_t=1), dict(work=3), dict(rows=-1)]
    for kw in bad:  # the good call: 1 row of 2 heads x 4 classes... 40 classes for the target pitch
        a = dict(dict(heads=2, classes=4, ld_out=8, ld_g=8, g=False, ld_t=1, work=4, rows=1), **kw)
        if "ld_t" in kw:
            a.update(classes=40, ld_out=80)
        rc = lib.hnh_bce_rows_f64(ctx.h, d.ptr, a["ld_out"], d.ptr, a["ld_t"], d.ptr, None, a["rows"], a["heads"], a["classes"], 1.0, d.ptr if a["g"] else None,
                                  a["ld_g"], res.ptr, d.ptr, a["work"], K.STREAM_COMPUTE)
        assert rc == 1 and b"hnh_bce_rows_f64" in lib.hnh_last_error(ctx.h), kw
    ctx.sync()
    assert np.all(res.get() == GUARD) and np.all(d.get() == 0.0), "nothing was launched"
    # no rows: the four sums are zero
    ctx.check(lib.hnh_bce_rows_f64(ctx.h, None, 4, None, 1, None, None, 0, 1, 4, 1.0, None, 0, res.ptr, d.ptr, 4, K.STREAM_COMPUTE), "no rows")
    assert np.all(res.get() == 0.0)
    res.free()
    d.free()
    # a NaN in a masked-in row makes the loss NaN; in a masked-out row it is never read
    out, targets, mask, pw, _ = bce_inputs(50, 2, 5, seed=1)
    out[int(np.flatnonzero(~mask)[0]), 3] = np.nan
    clean = run_bce(ctx, out, targets, mask, pw, 2, 5, 0.1)
    assert np.isfinite(clean[0]) and np.all(np.isfinite(clean[4]))
    out[int(np.flatnonzero(mask)[0]), 3] = np.nan
    assert np.isnan(run_bce(ctx, out, targets, mask, pw, 2, 5, 0.1)[0])


# ------------------------------------------------------------------------------------------------ the operator: loss, then backwardPass
def er8_targets(classes, seed=3):
    _, _, m, _ = er8()
    rng = np.random.default_rng(seed)
    return rng.random((m, classes)) < 0.35, rng.random(m) < 0.5, rng.uniform(0.25, 3.0, classes)


def published(gnn, layers):
    for li in range(len(layers)):
        gnn.set_activation(li, M.PUBLISHED[li])


def bce_round(world, rows, cols, m, x, layers, w, av, targets, mask, pw, heads, **kw):
    """Both rounds on ONE object: without class weights, then with."""
    s = setup(world, rows, cols, m, x, layers, w, av, None, **kw)
    gnn = s["gnn"]
    published(gnn, layers)
    res = []
    for weights in (None, pw):
        gnn.set_multilabel_targets(targets, mask, heads=heads, pos_weight=weights)
        gnn.forwardPass()
        gnn.get_output(s["out"])
        loss, f1 = gnn.loss(None, s["g"])
        r = dict(out=s["out"].download(), g=s["g"].download(), loss=loss, f1=f1, counts=gnn.multilabel_counts())
        r["other"] = gnn.loss(~mask) + gnn.multilabel_counts()
        r["again"] = gnn.loss(None, s["g"]) + gnn.multilabel_counts()
        assert np.array_equal(s["g"].download(), r["g"]), "a repeat must be bit-identical"
        gnn.backwardPass(s["g"])
        gnn.get_input_grad(s["dx"])
        r.update(dx=s["dx"].download(), dw={k: gnn.weight_grad(*k) for k in w}, subA=s["subA"], subB=s["subB"])
        if av is not None:
            r["da"] = {k: gnn.attention_grad(*k) for k in w}
        res.append(r)
    teardown(s)
    return res


CONFIGS = {"dot unfused": dict(attention="softmax", backward="unfused"), "dot fused": dict(attention="softmax", backward="fused"),
           "additive": dict(attention="softmax", score="additive")}


@pytest.mark.parametrize("heads", ["mean", "concat"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_loss_then_backward_vs_reference(p, config, heads):
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    nh, classes = R.heads_of(layers, heads)
    targets, mask, pw = er8_targets(classes)
    w = hashed_weights(layers)
    av = R.vectors_of(layers) if config == "additive" else None
    mode = dict(attention="softmax", score="additive" if config == "additive" else "dot", activations=M.PUBLISHED)
    both = H.run_spmd(p, lambda wd: bce_round(wd, rows, cols, m, x, layers, w, av, targets, mask, pw, heads, **CONFIGS[config]))
    hf = layers[-1][1] * layers[-1][2]
    want_out = R.forward(rows, cols, m, x, layers, ALPHA, w, av, **mode)
    assert np.any(want_out > 0) and np.any(want_out < 0), "the logits take both signs"
    for k, weights in enumerate((None, pw)):
        per_rank = [pr[k] for pr in both]
        out = T.assemble_dense(per_rank, "out", "subA", m, hf)
        g = T.assemble_dense(per_rank, "g", "subA", m, hf)
        dx = T.assemble_dense(per_rank, "dx", "subB", m, layers[0][0])
        want_loss, want_f1, want_g, want_counts = M.bce(want_out, targets, mask, nh, weights)
        other_loss, other_f1, _, other_counts = M.bce(want_out, targets, ~mask, nh, weights)
        want_dw, want_da, want_dx = R.backward(rows, cols, m, x, layers, ALPHA, want_g, w, av, **mode)
        assert np.abs(want_g).max() > 0 and np.abs(want_dx).max() > 0 and min(want_counts) > 0
        r0 = per_rank[0]
        errs = {"out": T.rel(out, want_out), "g": T.rel(g, want_g), "dx": T.rel(dx, want_dx), "loss": abs(r0["loss"] - want_loss) / want_loss,
                "other loss": abs(r0["other"][0] - other_loss) / other_loss}
        for pr in per_rank:
            assert (pr["loss"], pr["f1"], pr["counts"], pr["other"]) == (r0["loss"], r0["f1"], r0["counts"], r0["other"]), "every rank returns the same scalars"
            assert pr["again"] == (r0["loss"], r0["f1"]) + r0["counts"]
            for key in w:
                assert np.array_equal(pr["dw"][key], r0["dw"][key])
        for key in w:
            assert np.abs(want_dw[key]).max() > 0
            errs[("dw",) + key] = T.rel(r0["dw"][key], want_dw[key])
            if want_da:
                errs[("da1",) + key] = T.rel(r0["da"][key][0], want_da[key][0])
                errs[("da2",) + key] = T.rel(r0["da"][key][1], want_da[key][1])
        worst = max(errs.values())
        T.record_observed("gat_multilabel_loss_backward", case="%s %s weighted=%s" % (config, heads, weights is not None), ranks=p, worst=worst)
        print("observed", config, heads, weights is not None, p, "worst %.2e" % worst, "loss %.6f micro-F1 %.4f" % (r0["loss"], r0["f1"]), r0["counts"])
        assert r0["counts"] == want_counts and r0["other"][2:] == other_counts, "the counts are exact"
        assert r0["f1"] == want_f1 and r0["other"][1] == other_f1
        assert worst <= TOL, errs


# ------------------------------------------------------------------------------------------------ trajectories
def device_train(world, pp, layers, heads, optimizer, steps, pw=None):
    s = setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["w"], pp["av"], None, attention="softmax", score="additive")
    gnn = s["gnn"]
    published(gnn, layers)
    gnn.set_multilabel_targets(pp["targets"], pp["mask"], heads=heads, pos_weight=pw)
    opt = dict(optimizer)
    gnn.set_optimizer(opt.pop("kind"), opt.pop("lr"), **opt)
    res = dict(losses=[], f1s=[])
    for _ in range(steps):
        loss, f1 = gnn.train_step()
        res["losses"].append(loss)
        res["f1s"].append(f1)
    res["last_counts"] = gnn.multilabel_counts()
    res["w"] = {k: gnn.get_weight(*k) for k in pp["w"]}
    res["av"] = {k: gnn.get_attention_vectors(*k) for k in pp["w"]}
    res["held"] = gnn.evaluate(~pp["mask"])
    res["held_counts"] = gnn.multilabel_counts()
    res["train"] = gnn.evaluate()
    teardown(s)
    return res


TRAJECTORIES = {"sgd": dict(kind="sgd", lr=0.05, momentum=0.9, weight_decay=5e-4), "adam": dict(kind="adam", lr=0.01, weight_decay=5e-4)}


@pytest.mark.parametrize("kind", sorted(TRAJECTORIES))
@pytest.mark.parametrize("p", [1, 4])
def test_trajectory_vs_reference(p, kind):
    layers = T.GAT_LAYERS
    pp = M.planted_tags(layers)
    pw = np.array([0.5, 1.0, 2.0, 3.0])
    args = (pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, pp["targets"], pp["mask"], "mean", pp["w"], pp["av"], TRAJECTORIES[kind], 10, pw)
    ref = M.train(*args)
    per = M.train(*args, perturb=(1e-10, np.random.default_rng(7)))
    div_p = R.parameter_divergence(per[2], per[3], ref[2], ref[3])
    div_l = float(np.max(np.abs(np.array(per[0]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    assert div_p > 0 and div_l > 0
    bound_p, bound_l = 10.0 * div_p, 10.0 * div_l
    per_rank = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, "mean", TRAJECTORIES[kind], 10, pw))
    r0 = per_rank[0]
    for pr in per_rank:
        assert pr["losses"] == r0["losses"] and pr["f1s"] == r0["f1s"] and pr["last_counts"] == r0["last_counts"]
        for k in r0["w"]:
            assert np.array_equal(pr["w"][k], r0["w"][k]), "parameters are bit-equal across ranks"
            assert np.array_equal(pr["av"][k][0], r0["av"][k][0]) and np.array_equal(pr["av"][k][1], r0["av"][k][1])
    got_p = R.parameter_divergence(r0["w"], r0["av"], ref[2], ref[3])
    got_l = float(np.max(np.abs(np.array(r0["losses"]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    T.record_observed("gat_multilabel_trajectory", case=kind, ranks=p, parameters=got_p, parameters_bound=bound_p, loss=got_l, loss_bound=bound_l)
    print("observed", kind, p, "parameters %.2e (bound %.2e) loss %.2e (bound %.2e)" % (got_p, bound_p, got_l, bound_l))
    assert got_p <= bound_p and got_l <= bound_l
    assert r0["f1s"] == ref[1], "micro-F1 of every step, exactly"
    assert all(np.abs(r0["w"][k] - pp["w"][k]).max() > 0 and np.abs(r0["av"][k][0] - pp["av"][k][0]).max() > 0 for k in pp["w"])
    held = M.evaluate(pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, pp["targets"], ~pp["mask"], "mean", ref[2], ref[3], pw)
    # (the parameters agree with the reference's to bound_p and the loss is smooth in them: 1e-6 is a loose bound)
    assert abs(r0["held"][0] - held[0]) <= 1e-6 * held[0] and r0["held"][1] == held[1] == M.micro_f1(*r0["held_counts"])


# ------------------------------------------------------------------------------------------------ switching between the heads
def switching(world, rows, cols, m, x, layers, w, targets, labels, mask, order):
    """order: the setters called before the loss, "t" = set_multilabel_targets, "l" = set_labels; the last one decides."""
    s = setup(world, rows, cols, m, x, layers, w, None, None, attention="softmax")
    gnn = s["gnn"]
    for what in order:
        if what == "t":
            gnn.set_multilabel_targets(targets, mask, pos_weight=[0.5, 1.0, 2.0, 3.0])
        else:
            gnn.set_labels(labels, mask)
    gnn.forwardPass()
    pair = gnn.loss(None, s["g"])
    res = dict(pair=pair, g=s["g"].download(), other=gnn.evaluate(~mask))
    teardown(s)
    return res


@pytest.mark.parametrize("last", ["l", "t"])
def test_the_most_recent_setter_decides_the_head(last):
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w = hashed_weights(layers)
    targets, mask, _ = er8_targets(4)
    labels = np.random.default_rng(3).integers(0, 4, m).astype(np.int32)
    first = "t" if last == "l" else "l"
    runs = {order: H.run_spmd(2, lambda wd: switching(wd, rows, cols, m, x, layers, w, targets, labels, mask, order)) for order in (first + last, last, last + first + last)}
    for order in (first + last, last + first + last):
        for a, b in zip(runs[order], runs[last]):
            assert a["pair"] == b["pair"] and a["other"] == b["other"] and np.array_equal(a["g"], b["g"]), "bit for bit the object that only knew one head"
    other = H.run_spmd(2, lambda wd: switching(wd, rows, cols, m, x, layers, w, targets, labels, mask, first))
    assert other[0]["pair"] != runs[last][0]["pair"] and not np.array_equal(other[0]["g"], runs[last][0]["g"]), "the two heads differ"


# ------------------------------------------------------------------------------------------------ learning
@pytest.mark.parametrize("p", [1, 4])
def test_the_device_learns_the_planted_tags(p):
    layers = T.GAT_LAYERS
    pp = M.planted_tags(layers)
    per_rank = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, "mean", M.LEARN_OPTIMIZER, M.LEARN_STEPS))
    r = per_rank[0]
    T.record_observed("gat_multilabel_learning", ranks=p, first=r["losses"][0], last=r["losses"][-1], held_out_micro_f1=r["held"][1])
    print("observed: loss %.3f -> %.3f, held-out loss %.3f micro-F1 %.3f, train micro-F1 %.3f" % (r["losses"][0], r["losses"][-1], r["held"][0], r["held"][1], r["train"][1]))
    assert r["losses"][-1] <= 0.5 * r["losses"][0], "the final train loss is at most half the first"
    assert r["held"][1] >= M.HELD_OUT_F1, "held-out micro-F1"
    assert all(pr["held"] == r["held"] and pr["losses"] == r["losses"] for pr in per_rank)
