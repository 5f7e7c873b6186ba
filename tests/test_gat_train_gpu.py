"""The GAT's training step on the GPU (include/hnh_train.h; GAT.set_labels / loss / set_optimizer / optimizer_step / train_step / evaluate).

Kernel level, through ctypes.  hnh_xent_rows_f64 against the extended-precision numpy reference (tests/gat_ref.py, xent_rows with
np.longdouble) for classes in {1, 2, 3, 7, 8, 40, 64, 65, 256, 1000} x heads in {1, 3, 8} within HNH_XENT_MAX_WIDTH, with pitches wider
than the row, guard values round G, the result words and the workspace, logits up to +-700, a share of unlabelled rows and rows with
exact ties (small integers, the same in every head, so the head mean ties exactly); more rows than one grid round takes; a label beyond
the classes; the width limit.  Bounds: T.TOL (1e-11, summation order only) for loss_sum and for G normwise, `correct` exactly, a repeat
bit-identical.  Condition on the inputs: outside the deliberate ties the top two logits differ by at least 1e-6.
hnh_optim_step_f64 against numpy with the same gradient bits: column blocks of a wider gradient, pitch-2 vectors, padded parameter
pitches, rows or cols equal to 1, and a table longer than one launch holds; bound T.TOL per tensor.
Operator level, 15d_fusion2 with c = 1 on 1, 2, 4, 8 loopback ranks: loss with grad_out, then backwardPass, against the reference — loss,
accuracy, G, every dW, da1, da2 and dX — for score dot (backward unfused and fused) and score additive, heads "mean" and "concat"; bound
1e-10, the operator bound of the other GAT tests.
Trajectories: K = 10 train_steps against gat_ref.train.  The tolerance is measured: the reference runs a second time with every
gradient perturbed by 1e-10 * max|g| * u (1e-10: the bound on one backward pass), and the device may differ from the reference by 10
times the divergence of that run (the factor covers kink crossings of ReLU / LeakyReLU).  SGD with momentum is the sharp check, Adam the
loose one (its first steps are ill-conditioned where |g| ~ eps).  Parameters are bit-equal across ranks; a run with dropout (0.6, 0.6)
uses the masks of seed0 + t; evaluate leaves rates and seed as they were.
Learning: the planted partition of gat_ref.planted_partition, Adam, 40 steps: the final train loss is at most half the first and
the held-out accuracy at least 0.8.
The optimizer state's lifecycle: Adam through a bias and a projection switched on after set_optimizer, the bias off and on again, a change
of score and a second set_optimizer, every parameter after every step against a numpy trajectory (test_optimizer_state_lifecycle).

The observed errors and the measured bounds are recorded with T.record_observed."""
import ctypes as C

import numpy as np
import pytest

import gat_ref as R
import gat_skip_ref as S
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import ALPHA, TOL, ctx, er8, hashed_weights, hip_backend, setup, teardown  # noqa: F401

pytestmark = pytest.mark.gpu
GUARD = 7.0


# ------------------------------------------------------------------------------------------------ the loss kernel
def xent_inputs(rows, heads, classes, seed):
    """Logits (rows x heads * classes), labels with about 30 % unlabelled rows, and the rows with deliberate exact ties."""
    rng = np.random.default_rng(seed)
    n = heads * classes
    out = rng.uniform(-5.0, 5.0, (rows, n))
    big = np.arange(rows) % 5 == 1
    out[big] = rng.uniform(-700.0, 700.0, (np.count_nonzero(big), n))
    ties = np.zeros(rows, dtype=bool)
    if classes >= 2:
        ties[np.arange(rows) % 11 == 3] = True
        for r in np.flatnonzero(ties):
            vals = rng.integers(-3, 3, classes).astype(np.float64)
            top = rng.choice(classes, size=min(classes, 2 + int(rng.integers(0, 2))), replace=False)
            vals[top] = 4.0  # two or three classes share the maximum
            out[r] = np.tile(vals, heads)
    labels = rng.integers(0, classes, rows).astype(np.int32)
    labels[rng.random(rows) < 0.3] = -1
    labels[rng.random(rows) < 0.05] = -5
    for r in np.flatnonzero(ties)[::2]:
        labels[r] = int(np.argmax(out[r, :classes]))  # half of the tied rows are "correct" only with the lowest-index rule
    z = out.reshape(rows, heads, classes).mean(axis=1)
    if classes >= 2:
        top2 = np.sort(z, axis=1)[:, -2:]
        assert np.all((top2[:, 1] - top2[:, 0])[~ties] >= 1e-6), "condition on the inputs: the top two logits differ outside the ties"
        assert np.all((top2[:, 1] == top2[:, 0])[ties])
    return out, labels, ties


def run_xent(ctx, out, labels, heads, classes, inv_n, with_g=True, in_place=False, pad=(3, 5)):
    rows, n = out.shape
    ld_out, ld_g = n + pad[0], n + pad[1]
    host = np.full((rows + 1, ld_out), np.nan)
    host[:rows, :n] = out
    need = int(ctx.lib.hnh_xent_rows_f64_workspace(rows))
    assert need > 0
    d_out, d_lab = ctx.upload(host), ctx.upload(np.ascontiguousarray(labels, dtype=np.int32))
    d_g = ctx.upload(np.full((rows + 1, ld_g), GUARD))
    d_res, d_work = ctx.upload(np.full(4, GUARD)), ctx.upload(np.full(need + 2, GUARD))
    g_ptr, g_ld = (d_out.ptr, ld_out) if in_place else ((d_g.ptr if with_g else None), ld_g)
    rc = ctx.lib.hnh_xent_rows_f64(ctx.h, d_out.ptr, ld_out, d_lab.ptr, rows, heads, classes, inv_n, g_ptr, g_ld, d_res.ptr + 8, d_work.ptr + 8, need,
                                   K.STREAM_COMPUTE)
    ctx.check(rc, "hnh_xent_rows_f64")
    ctx.sync()
    res, work, g = d_res.get(), d_work.get(), (d_out.get() if in_place else d_g.get())
    assert res[0] == GUARD and res[3] == GUARD and work[0] == GUARD and work[-1] == GUARD, "guards round the result words and the workspace"
    if in_place:
        assert np.all(np.isnan(g[:rows, n:])) and np.all(np.isnan(g[rows]))
    elif with_g:
        assert np.all(g[:rows, n:] == GUARD) and np.all(g[rows] == GUARD), "guards round G"
    else:
        assert np.all(g == GUARD), "no gradient asked for: G untouched"
    for d in (d_out, d_lab, d_g, d_res, d_work):
        d.free()
    return float(res[1]), float(res[2]), g[:rows, :n]


SHAPES = [(h, c) for c in (1, 2, 3, 7, 8, 40, 64, 65, 256, 1000) for h in (1, 3, 8) if h * c <= K.XENT_MAX_WIDTH]


@pytest.mark.parametrize("heads,classes", SHAPES)
def test_xent_kernel_vs_longdouble(ctx, heads, classes):
    rows = 301 if heads * classes > 512 else 1237
    out, labels, ties = xent_inputs(rows, heads, classes, seed=heads * 1000 + classes)
    inv_n = 1.0 / 137.0
    want_loss, want_correct, want_g = R.xent_rows(out, labels, heads, inv_n, np.longdouble)
    loss, correct, g = run_xent(ctx, out, labels, heads, classes, inv_n)
    live = labels >= 0
    assert 0.5 * rows < np.count_nonzero(live) < 0.8 * rows and (classes < 2 or np.count_nonzero(ties & live) > 5)
    assert np.all(g[~live] == 0.0), "unlabelled rows get G = 0"
    errs = dict(loss=abs(loss - float(want_loss)) / max(abs(float(want_loss)), 1e-300) if classes > 1 else abs(loss), g=T.rel(g, np.float64(want_g)))
    T.record_observed("gat_train_xent_kernel", case="heads=%d classes=%d" % (heads, classes), worst=max(errs.values()))
    print("observed heads=%d classes=%d" % (heads, classes), errs, "correct", correct, want_correct)
    assert correct == want_correct, "argmax with ties to the lowest index, exactly"
    assert max(errs.values()) <= T.TOL, errs
    again = run_xent(ctx, out, labels, heads, classes, inv_n)
    assert again[0] == loss and again[1] == correct and np.array_equal(again[2], g), "a repeat must be bit-identical"
    no_g = run_xent(ctx, out, labels, heads, classes, inv_n, with_g=False)
    assert no_g[0] == loss and no_g[1] == correct
    in_place = run_xent(ctx, out, labels, heads, classes, inv_n, in_place=True)
    assert in_place[0] == loss and np.array_equal(in_place[2], g), "G may alias out"


@pytest.mark.parametrize("heads,classes,rows", [(1, 7, 140001), (8, 7, 40000), (3, 512, 9000)])
def test_xent_kernel_many_rows(ctx, heads, classes, rows):
    """More rows than one round of the grid takes (short rows share a wave), and the benchmark's row width."""
    out, labels, _ = xent_inputs(rows, heads, classes, seed=rows)
    inv_n = 1.0 / np.count_nonzero(labels >= 0)
    want_loss, want_correct, want_g = R.xent_rows(out, labels, heads, inv_n, np.longdouble)
    loss, correct, g = run_xent(ctx, out, labels, heads, classes, inv_n, pad=(1, 0))
    errs = dict(loss=abs(loss - float(want_loss)) / abs(float(want_loss)), g=T.rel(g, np.float64(want_g)))
    T.record_observed("gat_train_xent_kernel", case="heads=%d classes=%d rows=%d" % (heads, classes, rows), worst=max(errs.values()))
    print("observed", heads, classes, rows, errs)
    assert correct == want_correct and max(errs.values()) <= T.TOL, errs
    again = run_xent(ctx, out, labels, heads, classes, inv_n, pad=(1, 0))
    assert again[0] == loss and np.array_equal(again[2], g)


def test_xent_kernel_refusals_and_bad_labels(ctx):
    lib = ctx.lib
    out, labels, _ = xent_inputs(50, 2, 5, seed=1)
    labels[[3, 17]] = [5, 99]  # beyond the classes: reported in the results, never read
    loss, correct, g = run_xent(ctx, out, labels, 2, 5, 0.1)
    assert np.isnan(loss) and correct == -2.0 and np.all(g[[3, 17]] == 0.0)
    d = ctx.upload(np.zeros(8))
    for heads, classes in ((1, K.XENT_MAX_WIDTH + 1), (8, 513)):
        assert lib.hnh_xent_rows_f64(ctx.h, d.ptr, heads * classes, d.ptr, 0, heads, classes, 1.0, None, 0, d.ptr, d.ptr, 8, K.STREAM_COMPUTE) == 1
        assert b"HNH_XENT_MAX_WIDTH" in lib.hnh_last_error(ctx.h)
    assert lib.hnh_xent_rows_f64(ctx.h, d.ptr, 3, d.ptr, 1, 1, 4, 1.0, None, 0, d.ptr, d.ptr, 8, K.STREAM_COMPUTE) == 1, "a pitch below the row"
    assert lib.hnh_xent_rows_f64(ctx.h, d.ptr, 4, d.ptr, 1, 1, 4, 1.0, None, 0, d.ptr, d.ptr, 2, K.STREAM_COMPUTE) == 1, "a short workspace"
    assert lib.hnh_xent_rows_f64(ctx.h, d.ptr, 4, d.ptr, 1, 0, 4, 1.0, None, 0, d.ptr, d.ptr, 8, K.STREAM_COMPUTE) == 1
    # no rows: both sums are zero
    res = ctx.upload(np.full(2, GUARD))
    ctx.check(lib.hnh_xent_rows_f64(ctx.h, None, 4, None, 0, 1, 4, 1.0, None, 0, res.ptr, d.ptr, 8, K.STREAM_COMPUTE), "no rows")
    assert np.all(res.get() == 0.0)
    res.free()
    d.free()


# ------------------------------------------------------------------------------------------------ the optimizer kernel
class OptimProblem:
    """Tensors as the GAT has them: per layer the heads' W (rows x f at a padded pitch) whose gradients are column blocks of one
    rows x H f matrix, and a1 / a2 (H f x 1) whose gradients interleave at pitch 2; plus shapes with rows or cols equal to 1."""

    def __init__(self, ctx, kind, seed=0):
        self.ctx, self.kind = ctx, kind
        rng = np.random.default_rng(seed)
        self.tensors, self.dev = [], []
        specs = [(16, 8, 2), (16, 4, 3), (40, 33, 9), (7, 1, 25), (1, 5, 6), (1, 1, 3)]  # (rows, f, heads): 48 W and 12 vectors = 60 tensors
        for rows, f, heads in specs:
            hf = heads * f
            gw = self.array(rng.standard_normal((rows, hf)) * 10.0 ** rng.integers(-6, 2))
            gv = self.array(rng.standard_normal((hf, 2)))
            for h in range(heads):
                pad = int(rng.integers(0, 3))
                p = self.array(np.where(np.arange(f + pad) < f, rng.standard_normal((rows, f + pad)), GUARD))
                self.add(p, f + pad, gw, h * f, hf, rows, f)
            for q in (0, 1):
                p = self.array(rng.standard_normal((hf, 1)))
                self.add(p, 1, gv, q, 2, hf, 1)
        assert len(self.tensors) > 1 * K.OPTIM_MAX_TENSORS and len(self.tensors) % K.OPTIM_MAX_TENSORS != 0, "longer than one launch holds"
        self.rng = rng

    def array(self, host):
        d = self.ctx.upload(np.ascontiguousarray(host, dtype=np.float64))
        self.dev.append(d)
        return dict(host=np.array(host, dtype=np.float64), dev=d)

    def add(self, p, ld_p, g, g_off, ld_g, rows, cols):
        m = self.array(np.zeros((rows, cols))) if self.kind == "adam" else None
        v = self.array(np.zeros((rows, cols)))
        self.tensors.append(dict(p=p, ld_p=ld_p, g=g, g_off=g_off, ld_g=ld_g, m=m, v=v, rows=rows, cols=cols))

    def new_gradients(self):
        seen = set()
        for t in self.tensors:
            if id(t["g"]) not in seen:
                seen.add(id(t["g"]))
                t["g"]["host"] = t["g"]["host"] * self.rng.uniform(0.5, 1.5) + 0.1 * self.rng.standard_normal(t["g"]["host"].shape)
                t["g"]["dev"].set(t["g"]["host"])

    def step(self, t_step, hyper):
        tab = (K.OptimTensor * len(self.tensors))()
        for k, t in enumerate(self.tensors):
            tab[k] = K.OptimTensor(t["p"]["dev"].ptr, t["ld_p"], t["g"]["dev"].ptr + 8 * t["g_off"], t["ld_g"], t["m"]["dev"].ptr if t["m"] else None,
                                   t["v"]["dev"].ptr, t["rows"], t["cols"])
        hy = K.Optim(K.OPTIM_ADAM if self.kind == "adam" else K.OPTIM_SGD, 0, hyper["lr"], hyper.get("beta1", 0.9), hyper.get("beta2", 0.999),
                     hyper.get("eps", 1e-8), hyper.get("momentum", 0.0), hyper.get("weight_decay", 0.0), 1.0 - hyper.get("beta1", 0.9) ** t_step,
                     1.0 - hyper.get("beta2", 0.999) ** t_step)
        self.ctx.check(self.ctx.lib.hnh_optim_step_f64(self.ctx.h, tab, len(self.tensors), C.byref(hy), K.STREAM_COMPUTE), "hnh_optim_step_f64")
        self.ctx.sync()
        worst = 0.0
        for t in self.tensors:  # the reference step on the host copies, then the comparison
            rows, cols = t["rows"], t["cols"]
            p = t["p"]["host"][:, :cols]
            g = t["g"]["host"][:, t["g_off"]:t["g_off"] + cols]
            if self.kind == "adam":
                kw = {k: hyper[k] for k in ("beta1", "beta2", "eps", "weight_decay") if k in hyper}
                newp, t["m"]["host"], t["v"]["host"] = R.adam_step(p, g, t["m"]["host"], t["v"]["host"], t_step, hyper["lr"], **kw)
            else:
                kw = {k: hyper[k] for k in ("momentum", "weight_decay") if k in hyper}
                newp, t["v"]["host"] = R.sgd_step(p, g, t["v"]["host"], hyper["lr"], **kw)
            t["p"]["host"][:, :cols] = newp
            got_p = t["p"]["dev"].get()
            assert np.all(got_p[:, cols:] == GUARD), "the parameter's pitch padding is untouched"
            errs = [T.rel(got_p[:, :cols], newp), T.rel(t["v"]["dev"].get(), t["v"]["host"])]
            if t["m"]:
                errs.append(T.rel(t["m"]["dev"].get(), t["m"]["host"]))
            worst = max(worst, *errs)
            assert max(errs) <= T.TOL, (rows, cols, t["ld_g"], errs)
        return worst

    def free(self):
        for d in self.dev:
            d.free()


@pytest.mark.parametrize("kind,hyper", [("adam", dict(lr=0.01, weight_decay=5e-4)), ("adam", dict(lr=0.003, beta1=0.8, beta2=0.99, eps=1e-6)),
                                        ("sgd", dict(lr=0.05, momentum=0.9, weight_decay=5e-4)), ("sgd", dict(lr=0.1))])
def test_optimizer_kernel_vs_numpy(ctx, kind, hyper):
    p = OptimProblem(ctx, kind, seed=len(hyper))
    assert any(t["rows"] == 1 for t in p.tensors) and any(t["cols"] == 1 for t in p.tensors) and any(t["ld_g"] == 2 for t in p.tensors)
    assert any(t["ld_p"] > t["cols"] for t in p.tensors) and any(t["g_off"] > 0 and t["ld_g"] > 2 for t in p.tensors)
    start = [t["p"]["host"].copy() for t in p.tensors]
    worst = 0.0
    for step in range(1, 5):
        worst = max(worst, p.step(step, hyper))
        p.new_gradients()
    assert all(np.abs(t["p"]["host"][:, :t["cols"]] - s[:, :t["cols"]]).max() > 0 for t, s in zip(p.tensors, start)), "every tensor has moved"
    T.record_observed("gat_train_optim_kernel", case="%s %s" % (kind, sorted(hyper.items())), worst=worst)
    print("observed", kind, hyper, "worst %.2e" % worst)
    p.free()


def test_optimizer_kernel_refusals(ctx):
    lib = ctx.lib
    d = ctx.upload(np.zeros(16))
    tab = (K.OptimTensor * 1)(K.OptimTensor(d.ptr, 2, d.ptr + 64, 2, None, d.ptr + 32, 2, 2))
    ok = K.Optim(K.OPTIM_SGD, 0, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.1, 0.001)
    ctx.check(lib.hnh_optim_step_f64(ctx.h, tab, 1, C.byref(ok), K.STREAM_COMPUTE), "sgd without m")
    ctx.check(lib.hnh_optim_step_f64(ctx.h, None, 0, C.byref(ok), K.STREAM_COMPUTE), "an empty table")
    adam = K.Optim(K.OPTIM_ADAM, 0, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.1, 0.001)
    assert lib.hnh_optim_step_f64(ctx.h, tab, 1, C.byref(adam), K.STREAM_COMPUTE) == 1, "Adam needs m"
    assert lib.hnh_optim_step_f64(ctx.h, tab, 1, C.byref(K.Optim(5, 0, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.1, 0.001)), K.STREAM_COMPUTE) == 1
    narrow = (K.OptimTensor * 1)(K.OptimTensor(d.ptr, 1, d.ptr + 64, 2, None, d.ptr + 32, 2, 2))
    assert lib.hnh_optim_step_f64(ctx.h, narrow, 1, C.byref(ok), K.STREAM_COMPUTE) == 1, "a pitch below the width"
    ctx.sync()
    d.free()


# ------------------------------------------------------------------------------------------------ the operator: loss, then backwardPass
def er8_labels(classes, seed=3):
    _, _, m, _ = er8()
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, classes, m).astype(np.int32)
    labels[rng.random(m) < 0.1] = -1
    return labels, rng.random(m) < 0.5


def loss_round(world, rows, cols, m, x, layers, w, av, labels, mask, heads, **kw):
    s = setup(world, rows, cols, m, x, layers, w, av, None, **kw)
    gnn = s["gnn"]
    gnn.set_labels(labels, mask, heads=heads)
    gnn.forwardPass()
    gnn.get_output(s["out"])
    loss, acc = gnn.loss(None, s["g"])
    r = dict(out=s["out"].download(), g=s["g"].download(), loss=loss, acc=acc, other=gnn.loss(~mask), again=gnn.loss(None, s["g"]))
    assert np.array_equal(s["g"].download(), r["g"]), "a repeat must be bit-identical"
    gnn.backwardPass(s["g"])
    gnn.get_input_grad(s["dx"])
    r.update(dx=s["dx"].download(), dw={k: gnn.weight_grad(*k) for k in w}, subA=s["subA"], subB=s["subB"])
    if av is not None:
        r["da"] = {k: gnn.attention_grad(*k) for k in w}
    teardown(s)
    return r


CONFIGS = {"dot unfused": dict(attention="softmax", backward="unfused"), "dot fused": dict(attention="softmax", backward="fused"),
           "additive": dict(attention="softmax", score="additive")}


@pytest.mark.parametrize("heads", ["mean", "concat"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_loss_then_backward_vs_reference(p, config, heads):
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    nh, classes = R.heads_of(layers, heads)
    labels, mask = er8_labels(classes)
    w = hashed_weights(layers)
    av = R.vectors_of(layers) if config == "additive" else None
    mode = dict(attention="softmax", score="additive" if config == "additive" else "dot")
    per_rank = H.run_spmd(p, lambda wd: loss_round(wd, rows, cols, m, x, layers, w, av, labels, mask, heads, **CONFIGS[config]))
    hf = layers[-1][1] * layers[-1][2]
    out = T.assemble_dense(per_rank, "out", "subA", m, hf)
    g = T.assemble_dense(per_rank, "g", "subA", m, hf)
    dx = T.assemble_dense(per_rank, "dx", "subB", m, layers[0][0])
    want_out = R.forward(rows, cols, m, x, layers, ALPHA, w, av, **mode)
    want_loss, want_acc, want_g = R.xent(want_out, labels, mask, nh)
    other_loss, other_acc, _ = R.xent(want_out, labels, ~mask, nh)
    want_dw, want_da, want_dx = R.backward(rows, cols, m, x, layers, ALPHA, want_g, w, av, **mode)
    assert np.abs(want_g).max() > 0 and np.abs(want_dx).max() > 0
    r0 = per_rank[0]
    errs = {"out": T.rel(out, want_out), "g": T.rel(g, want_g), "dx": T.rel(dx, want_dx), "loss": abs(r0["loss"] - want_loss) / want_loss,
            "other loss": abs(r0["other"][0] - other_loss) / other_loss}
    for pr in per_rank:
        assert (pr["loss"], pr["acc"], pr["other"], pr["again"]) == (r0["loss"], r0["acc"], r0["other"], (r0["loss"], r0["acc"])), "every rank returns the same scalars"
        for key in w:
            assert np.array_equal(pr["dw"][key], r0["dw"][key])
    for key in w:
        assert np.abs(want_dw[key]).max() > 0
        errs[("dw",) + key] = T.rel(r0["dw"][key], want_dw[key])
        if want_da:
            errs[("da1",) + key] = T.rel(r0["da"][key][0], want_da[key][0])
            errs[("da2",) + key] = T.rel(r0["da"][key][1], want_da[key][1])
    worst = max(errs.values())
    T.record_observed("gat_train_loss_backward", case="%s %s" % (config, heads), ranks=p, worst=worst)
    print("observed", config, heads, p, "worst %.2e" % worst, "loss %.6f acc %.4f" % (r0["loss"], r0["acc"]))
    assert r0["acc"] == want_acc and r0["other"][1] == other_acc
    assert worst <= TOL, errs


# ------------------------------------------------------------------------------------------------ trajectories
def device_train(world, pp, layers, heads, optimizer, steps, rates=(0.0, 0.0), seed0=0, probe_evaluate=False):
    s = setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["w"], pp["av"], None, attention="softmax", score="additive", dropout=rates,
              seed=seed0)
    gnn = s["gnn"]
    gnn.set_labels(pp["labels"], pp["mask"], heads=heads)
    opt = dict(optimizer)
    gnn.set_optimizer(opt.pop("kind"), opt.pop("lr"), **opt)
    res = dict(losses=[], accs=[])
    for _ in range(steps):
        loss, acc = gnn.train_step()
        res["losses"].append(loss)
        res["accs"].append(acc)
    res["w"] = {k: gnn.get_weight(*k) for k in pp["w"]}
    res["av"] = {k: gnn.get_attention_vectors(*k) for k in pp["w"]}
    res["held"] = gnn.evaluate(~pp["mask"])
    res["train"] = gnn.evaluate()
    if probe_evaluate:
        # evaluate left rates and seed as they were: the next forward pass has the masks of seed0 + steps, as one before evaluate had,
        # and the stored forward pass of evaluate (no dropout) is not offered to backwardPass
        with pytest.raises(H.HnhError, match="forwardPass"):
            gnn.backwardPass(s["g"])
        gnn.forwardPass()
        gnn.get_output(s["out"])
        res["out_after"] = s["out"].download()
        gnn.evaluate(~pp["mask"])
        gnn.forwardPass()
        gnn.get_output(s["out"])
        res["out_again"] = s["out"].download()
        gnn.set_dropout(0.0, 0.0, 0)
        gnn.forwardPass()
        gnn.get_output(s["out"])
        res["out_plain"] = s["out"].download()
        res["subA"] = s["subA"]
    teardown(s)
    return res


def measured_bounds(pp, layers, heads, optimizer, steps, rates=(0.0, 0.0), seed0=0):
    """(reference run, allowed parameter difference, allowed loss difference): 10 x the divergence of a reference run whose gradients are
    perturbed by 1e-10 * max|g| * u."""
    args = (pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, pp["labels"], pp["mask"], heads, pp["w"], pp["av"])
    ref = R.train(*args, optimizer, steps, rates, seed0)
    per = R.train(*args, optimizer, steps, rates, seed0, perturb=(1e-10, np.random.default_rng(7)))
    div_p = R.parameter_divergence(per[2], per[3], ref[2], ref[3])
    div_l = float(np.max(np.abs(np.array(per[0]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    assert div_p > 0 and div_l > 0
    return ref, 10.0 * div_p, 10.0 * div_l


TRAJECTORIES = {"sgd": dict(kind="sgd", lr=0.05, momentum=0.9, weight_decay=5e-4), "adam": dict(kind="adam", lr=0.01, weight_decay=5e-4)}


def check_trajectory(per_rank, ref, bound_p, bound_l, label, p):
    r0 = per_rank[0]
    for pr in per_rank:
        assert pr["losses"] == r0["losses"] and pr["accs"] == r0["accs"]
        for k in r0["w"]:
            assert np.array_equal(pr["w"][k], r0["w"][k]), "parameters are bit-equal across ranks"
            assert np.array_equal(pr["av"][k][0], r0["av"][k][0]) and np.array_equal(pr["av"][k][1], r0["av"][k][1])
    got_p = R.parameter_divergence(r0["w"], r0["av"], ref[2], ref[3])
    got_l = float(np.max(np.abs(np.array(r0["losses"]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    T.record_observed("gat_train_trajectory", case=label, ranks=p, parameters=got_p, parameters_bound=bound_p, loss=got_l, loss_bound=bound_l)
    print("observed", label, p, "parameters %.2e (bound %.2e) loss %.2e (bound %.2e)" % (got_p, bound_p, got_l, bound_l))
    assert got_p <= bound_p and got_l <= bound_l
    assert r0["accs"] == ref[1]


@pytest.mark.parametrize("heads", ["mean", "concat"])
@pytest.mark.parametrize("kind", sorted(TRAJECTORIES))
@pytest.mark.parametrize("p", [1, 4])
def test_trajectory_vs_reference(p, kind, heads):
    layers = T.GAT_LAYERS
    pp = R.planted_partition(layers)
    if heads == "concat":
        pp["labels"] = (pp["labels"] * 3 + np.arange(pp["m"]) % 3).astype(np.int32)  # 12 classes
    ref, bound_p, bound_l = measured_bounds(pp, layers, heads, TRAJECTORIES[kind], 10)
    per_rank = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, heads, TRAJECTORIES[kind], 10))
    check_trajectory(per_rank, ref, bound_p, bound_l, "%s %s" % (kind, heads), p)
    assert all(np.abs(per_rank[0]["w"][k] - pp["w"][k]).max() > 0 and np.abs(per_rank[0]["av"][k][0] - pp["av"][k][0]).max() > 0 for k in pp["w"])


@pytest.mark.parametrize("p", [1, 4])
def test_trajectory_with_dropout_uses_seed_plus_step(p):
    layers = T.GAT_LAYERS
    pp = R.planted_partition(layers)
    seed0, steps = 0xFFFFFFFFFFFFFFFD, 5  # (the seed wraps mod 2^64 on the way)
    opt = TRAJECTORIES["sgd"]
    ref, bound_p, bound_l = measured_bounds(pp, layers, "mean", opt, steps, (0.6, 0.6), seed0)
    per_rank = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, "mean", opt, steps, (0.6, 0.6), seed0, probe_evaluate=True))
    check_trajectory(per_rank, ref, bound_p, bound_l, "sgd with dropout", p)
    other = R.train(pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, pp["labels"], pp["mask"], "mean", pp["w"], pp["av"], opt, steps, (0.6, 0.6), seed0 + 1)
    assert abs(other[0][0] - per_rank[0]["losses"][0]) > 1e-6, "another seed0 gives another first loss"
    # evaluate: the numbers of a forward pass without dropout; rates and seed as they were afterwards
    # (the parameters agree with the reference's to bound_p, about 1e-10, and the loss is smooth in them: 1e-6 is a loose bound)
    held = R.evaluate(pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, pp["labels"], ~pp["mask"], "mean", ref[2], ref[3])
    assert abs(per_rank[0]["held"][0] - held[0]) <= 1e-6 * held[0] and per_rank[0]["held"][1] == held[1]
    for pr in per_rank:
        assert np.array_equal(pr["out_after"], pr["out_again"]) and not np.array_equal(pr["out_after"], pr["out_plain"])
    hf = layers[-1][1] * layers[-1][2]
    out = T.assemble_dense(per_rank, "out_after", "subA", pp["m"], hf)
    want = R.forward(pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, per_rank[0]["w"], per_rank[0]["av"], rates=(0.6, 0.6),
                     seed=(seed0 + steps) & 0xFFFFFFFFFFFFFFFF, **R.TRAINED)
    assert T.rel(out, want) <= TOL, "after evaluate the masks are those of the last step's seed"


# ------------------------------------------------------------------------------------------------ learning
@pytest.mark.parametrize("p", [1, 4])
def test_the_device_learns_the_planted_partition(p):
    layers = T.GAT_LAYERS
    pp = R.planted_partition(layers)
    per_rank = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, "mean", R.LEARN_OPTIMIZER, R.LEARN_STEPS))
    r = per_rank[0]
    T.record_observed("gat_train_learning", ranks=p, first=r["losses"][0], last=r["losses"][-1], held_out_accuracy=r["held"][1])
    print("observed: loss %.3f -> %.3f, held-out loss %.3f accuracy %.3f, train accuracy %.3f" % (r["losses"][0], r["losses"][-1], r["held"][0], r["held"][1], r["train"][1]))
    assert r["losses"][-1] <= 0.5 * r["losses"][0], "the final train loss is at most half the first"
    assert r["held"][1] >= 0.8, "held-out accuracy"
    assert all(pr["held"] == r["held"] and pr["losses"] == r["losses"] for pr in per_rank)


def test_refusals_on_the_device():
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w = hashed_weights(layers)
    labels, mask = er8_labels(4)

    def rank(world):
        s = setup(world, rows, cols, m, x, layers, w, None, None, attention="softmax")
        gnn = s["gnn"]
        with pytest.raises(H.HnhError, match="set_labels"):
            gnn.train_step()
        gnn.set_labels(labels, mask)
        with pytest.raises(H.HnhError, match="forwardPass"):
            gnn.loss()
        with pytest.raises(H.HnhError, match="set_optimizer"):
            gnn.train_step()
        gnn.set_optimizer("sgd", 0.01)
        with pytest.raises(H.HnhError, match="backwardPass since the last step"):
            gnn.optimizer_step()
        first = gnn.train_step()
        with pytest.raises(H.HnhError, match="backwardPass since the last step"):
            gnn.optimizer_step()  # train_step has used its gradients
        with pytest.raises(H.HnhError, match="forwardPass"):
            gnn.loss()  # the update invalidated the stored forward pass
        gnn.forwardPass()
        second = gnn.loss()
        world.sync()
        teardown(s)
        return first, second

    for first, second in H.run_spmd(2, rank):
        assert np.isfinite(first[0]) and np.isfinite(second[0]) and second[0] != first[0], "the step changed the parameters"


# ------------------------------------------------------------------------------------------------ the optimizer state's lifecycle
LIFECYCLE_LAYERS = [(16, 8, 2), (16, 4, 3)]
LIFECYCLE_ADAM = dict(kind="adam", lr=0.01, weight_decay=5e-4)
# what happens to the object, in order; ("steps", n) are n train_steps, and every parameter is compared after each of them
LIFECYCLE = [("optimizer",), ("steps", 2), ("bias", "b"), ("projection",), ("steps", 2), ("bias", None), ("steps", 1), ("bias", "b again"), ("steps", 1),
             ("gatv2",), ("steps", 1), ("optimizer",), ("steps", 1)]


def lifecycle_problem():
    rows, cols, m, x = er8()
    labels, mask = er8_labels(LIFECYCLE_LAYERS[-1][1])
    rng = np.random.default_rng(5)
    hf0 = LIFECYCLE_LAYERS[0][1] * LIFECYCLE_LAYERS[0][2]
    fin1, hf1 = LIFECYCLE_LAYERS[1][0], LIFECYCLE_LAYERS[1][1] * LIFECYCLE_LAYERS[1][2]
    return dict(rows=rows, cols=cols, m=m, x=x, labels=labels, mask=mask, w=hashed_weights(LIFECYCLE_LAYERS), av=R.vectors_of(LIFECYCLE_LAYERS),
                bias={"b": rng.uniform(-0.5, 0.5, hf0), "b again": rng.uniform(-0.5, 0.5, hf0)}, wr=rng.standard_normal((fin1, hf1)) / np.sqrt(fin1))


def lifecycle_reference(pp, perturb=None):
    """The parameters after every step, as (None, None, w, av, bias, W_res) for gat_skip_ref.parameter_divergence, under the rules of
    the optimizer's state: a tensor that becomes learned gets zero moments then and the bias correction of the global step count; a tensor
    that stops being learned keeps its moments for when it is learned again; set_optimizer drops every moment and the step count."""
    layers, opt = LIFECYCLE_LAYERS, dict(LIFECYCLE_ADAM)
    kind, lr = opt.pop("kind"), opt.pop("lr")
    params = {("w",) + k: v.copy() for k, v in pp["w"].items()}
    params.update({("a1",) + k: v[0].copy() for k, v in pp["av"].items()})
    params.update({("a2",) + k: v[1].copy() for k, v in pp["av"].items()})
    score, bias_on, projection, mom, var, t, snaps = "additive", False, False, {}, {}, 0, []
    for what in LIFECYCLE:
        if what[0] == "optimizer":
            mom, var, t = {}, {}, 0
        elif what[0] == "bias":
            bias_on = what[1] is not None
            if bias_on:
                params[("b", 0)] = pp["bias"][what[1]].copy()
        elif what[0] == "projection":
            projection, params[("wr", 1)] = True, pp["wr"].copy()
        elif what[0] == "gatv2":
            score = "gatv2"
        for _ in range(what[1] if what[0] == "steps" else 0):
            t += 1
            wt = {k: params[("w",) + k] for k in pp["w"]}
            at = {k: (params[("a1",) + k], params[("a2",) + k]) if score == "additive" else params[("a1",) + k] for k in pp["w"]}
            mode = dict(score=score, residual=("none", "projection" if projection else "none"), bias={0: params[("b", 0)]} if bias_on else None,
                        res_weights={1: params[("wr", 1)]} if projection else None)
            out = S.forward(pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, wt, at, **mode)
            _, _, g = R.xent(out, pp["labels"], pp["mask"], layers[-1][2])
            dw, da, db, dwr, _ = S.backward(pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, g, wt, at, **mode)
            grads = {("w",) + k: v for k, v in dw.items()}
            grads.update({("a1",) + k: v[0] if score == "additive" else v for k, v in da.items()})
            if score == "additive":
                grads.update({("a2",) + k: v[1] for k, v in da.items()})
            grads.update({("b", li): v for li, v in db.items()})
            grads.update({("wr", li): v for li, v in dwr.items()})
            for k, gk in grads.items():  # (exactly the learned tensors)
                if perturb is not None:
                    gk = gk + perturb[0] * np.max(np.abs(gk)) * perturb[1].uniform(-1.0, 1.0, gk.shape)
                if k not in mom:
                    mom[k], var[k] = np.zeros_like(params[k]), np.zeros_like(params[k])
                params[k], mom[k], var[k] = R.adam_step(params[k], gk, mom[k], var[k], t, lr, **opt)
            snaps.append((None, None, {k: params[("w",) + k].copy() for k in pp["w"]},
                          {k: (params[("a1",) + k].copy(), params[("a2",) + k].copy()) for k in pp["w"]},
                          {0: params[("b", 0)].copy()} if ("b", 0) in params else {}, {1: params[("wr", 1)].copy()} if projection else {}))
    return snaps


def lifecycle_device(world, pp):
    s = setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], LIFECYCLE_LAYERS, pp["w"], pp["av"], None, attention="softmax", score="additive")
    gnn = s["gnn"]
    gnn.set_labels(pp["labels"], pp["mask"], heads="mean")
    opt = dict(LIFECYCLE_ADAM)
    kind, lr = opt.pop("kind"), opt.pop("lr")
    bias_on, bias_seen, projection, snaps = False, False, False, []
    for what in LIFECYCLE:
        if what[0] == "optimizer":
            gnn.set_optimizer(kind, lr, **opt)
        elif what[0] == "bias":
            gnn.set_bias(0, None if what[1] is None else pp["bias"][what[1]])
            bias_on, bias_seen = what[1] is not None, True
        elif what[0] == "projection":
            gnn.set_residual(1, "projection")
            gnn.set_residual_weight(1, pp["wr"])
            projection = True
        elif what[0] == "gatv2":
            gnn.set_score("gatv2")
        for _ in range(what[1] if what[0] == "steps" else 0):
            gnn.train_step()
            # (a bias that is switched off is not handed out: it is what the last step it was learned in left)
            b = {} if not bias_seen else ({0: gnn.get_bias(0)} if bias_on else dict(snaps[-1][4]))
            snaps.append((None, None, {k: gnn.get_weight(*k) for k in pp["w"]}, {k: gnn.get_attention_vectors(*k) for k in pp["w"]}, b,
                          {1: gnn.get_residual_weight(1)} if projection else {}))
    teardown(s)
    return snaps


@pytest.mark.parametrize("p", [1, 4])
def test_optimizer_state_lifecycle(p):
    """Adam moments through a bias and a projection switched on after set_optimizer, the bias off and on again, a change of score and a
    second set_optimizer (LIFECYCLE): after EVERY train_step all parameters (W, a1, a2, bias, W_res) against the numpy trajectory of
    lifecycle_reference.  The metric and the tolerance are those of test_adam_trajectory_with_bias_and_residuals (tests/test_gat_skip_gpu.py):
    gat_skip_ref.parameter_divergence within 10 x the divergence of a reference run whose gradients are perturbed at 1e-10, here taken
    after every step (the largest so far: a difference once made stays in the moments).  A state that is lost, kept where it should be
    zeroed, or corrected with a step count of its own moves a parameter by a share of lr = 1e-2 in one step, five orders above the bound.
    Observed on the MI355X: at most 1.2e-15 at every step, p = 1 and p = 4 (bounds 6.2e-10 after the first step, 2.9e-8 .. 3.6e-8 after the others)."""
    pp = lifecycle_problem()
    ref = lifecycle_reference(pp)
    per = lifecycle_reference(pp, perturb=(1e-10, np.random.default_rng(7)))
    bounds = list(np.maximum.accumulate([10.0 * S.parameter_divergence(a, b) for a, b in zip(per, ref)]))
    assert len(ref) == 8 and all(b > 0 for b in bounds)
    per_rank = H.run_spmd(p, lambda wd: lifecycle_device(wd, pp))
    r0 = per_rank[0]
    for pr in per_rank:
        for a, b in zip(pr, r0):
            assert S.parameter_divergence(a, b) == 0.0 and S.parameter_divergence(b, a) == 0.0, "parameters are bit-equal across ranks"
    got = [S.parameter_divergence(a, b) for a, b in zip(r0, ref)]
    T.record_observed("gat_train_lifecycle", ranks=p, parameters=got, parameters_bound=bounds)
    print("observed lifecycle", p, " ".join("%.2e (bound %.2e)" % gb for gb in zip(got, bounds)))
    assert [set(x) for x in r0[-1][2:]] == [set(x) for x in ref[-1][2:]] and len(r0) == len(ref)
    assert all(g <= b for g, b in zip(got, bounds)), (got, bounds)
    # the sequence is telling: the bias moved while it was learned and stood still while it was off; a2 stands still under gatv2
    assert np.abs(ref[3][4][0] - pp["bias"]["b"]).max() > 0 and np.array_equal(ref[4][4][0], ref[3][4][0]) and np.abs(ref[5][4][0] - pp["bias"]["b again"]).max() > 0
    assert all(np.array_equal(ref[6][3][k][1], ref[5][3][k][1]) and np.abs(ref[6][3][k][0] - ref[5][3][k][0]).max() > 0 for k in pp["w"])
