"""Gradient clipping, AdamW and learning-rate schedules of the GAT's training step on the GPU (include/hnh_train_clip.h; GAT.set_grad_clip /
grad_norm / set_optimizer("adamw") / set_learning_rate / set_lr_schedule; tests/gat_clip_ref.py is the definition).

Kernel level, through ctypes.  hnh_grad_sumsq_f64 over the gradient tensors of test_gat_train_gpu.OptimProblem (60 tensors: two launches, the
second not full; column blocks at wide pitches, the pitch-2 interleave, rows or cols of 1) plus one tensor of 300 001 elements at an odd
base offset (the stride loop, the 8-byte loads) and two tensors without elements: with integer gradients in [-8, 8] every partial sum is
exact, so the result equals numpy's to the bit whatever the order; with normal gradients over scales 1e-6 .. 1e2 it lies within T.TOL of
np.longdouble; accumulate adds to the bit; a repeat gives the same bits; the guard words round the workspace and the result stay; refusals.
hnh_optim_step_clip_f64 on the same problem over four steps with new gradients against gat_clip_ref (Adam, SGD, AdamW; coef < 1 from two
nonzero sums) within T.TOL; with coef == 1 and with sumsq == NULL bit-equal to hnh_optim_step_f64 on a twin; AdamW without decay bit-equal
to Adam; the pitch padding keeps its guard value.
Operator level, 15d_fusion2 with c = 1 on loopback ranks: ten clipped steps (max_norm 0.2: some steps clip, some do not) with Adam, SGD
and AdamW against gat_clip_ref.train within the measured bound of test_gat_train_gpu (10 x the divergence of a reference run whose
gradients are perturbed at 1e-10), grad_norm() against the reference's norm within T.TOL, everything bit-equal across ranks; a run with
max_norm 1e300, and one with clipping switched on and off again, bit-equal to a run without; a cosine schedule with a warm-up and
set_learning_rate in mid-run against the reference with per-step rates; what the norm is made of on the full model (transformer score,
learned edge bias, layer norm, projection, bias); the multi-label head; refusals.

The observed errors and the measured bounds are recorded with T.record_observed.

Observed on an MI355X: the sum of squares exact on integers and 1.4e-16 from np.longdouble; the clipped step at most 5.9e-16 from the
reference; clipped trajectories at most 5.6e-16 in the parameters (bounds 8.8e-11 SGD, 6.7e-9 Adam, 1.3e-8 AdamW) and 4.8e-16 in the
losses, grad_norm() at most 2.9e-16 from the reference's norm; norm^2 of the full model against its parts 1.9e-16."""
import ctypes as C

import numpy as np
import pytest

import gat_clip_ref as CR
import gat_multilabel_ref as M
import gat_ref as R
import hnh_testlib as T
import test_gat_edge_learn_gpu as LG
import test_gat_norm_gpu as NG
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import ALPHA, ctx, hip_backend, setup, teardown  # noqa: F401
from test_gat_train_gpu import GUARD, OptimProblem, check_trajectory

pytestmark = pytest.mark.gpu
OFF = LG.OFF


# ------------------------------------------------------------------------------------------------ the sum of squares
class ClipProblem(OptimProblem):
    """OptimProblem with first moments for AdamW too, and the step through hnh_optim_step_clip_f64"""

    def add(self, p, ld_p, g, g_off, ld_g, rows, cols):
        m = self.array(np.zeros((rows, cols))) if self.kind in ("adam", "adamw") else None
        v = self.array(np.zeros((rows, cols)))
        self.tensors.append(dict(p=p, ld_p=ld_p, g=g, g_off=g_off, ld_g=ld_g, m=m, v=v, rows=rows, cols=cols))

    def gradient_arrays(self):
        seen = {}
        for t in self.tensors:
            seen.setdefault(id(t["g"]), t["g"])
        return list(seen.values())

    def table(self, full=True):
        tab = (K.OptimTensor * len(self.tensors))()
        for k, t in enumerate(self.tensors):
            g = t["g"]["dev"].ptr + 8 * t["g_off"]
            tab[k] = K.OptimTensor(t["p"]["dev"].ptr, t["ld_p"], g, t["ld_g"], t["m"]["dev"].ptr if t["m"] else None, t["v"]["dev"].ptr, t["rows"],
                                   t["cols"]) if full else K.OptimTensor(None, 0, g, t["ld_g"], None, None, t["rows"], t["cols"])
        return tab

    def hyper(self, t_step, hyper, kind=None):
        code = {"adam": K.OPTIM_ADAM, "sgd": K.OPTIM_SGD, "adamw": K.OPTIM_ADAMW}[kind or self.kind]
        return K.Optim(code, 0, hyper["lr"], hyper.get("beta1", 0.9), hyper.get("beta2", 0.999), hyper.get("eps", 1e-8), hyper.get("momentum", 0.0),
                       hyper.get("weight_decay", 0.0), 1.0 - hyper.get("beta1", 0.9) ** t_step, 1.0 - hyper.get("beta2", 0.999) ** t_step)

    def clip_step(self, t_step, hyper, sums, max_norm, kind=None):
        """one launch sequence of hnh_optim_step_clip_f64; sums = None: sumsq == NULL"""
        hy = self.hyper(t_step, hyper, kind)
        d = self.ctx.upload(np.array([GUARD] + list(sums or [0.0]) + [GUARD]))
        rc = self.ctx.lib.hnh_optim_step_clip_f64(self.ctx.h, self.table(), len(self.tensors), C.byref(hy), d.ptr + 8 if sums else None, len(sums or []),
                                                  max_norm, K.STREAM_COMPUTE)
        self.ctx.check(rc, "hnh_optim_step_clip_f64")
        self.ctx.sync()
        got = d.get()
        assert got[0] == GUARD and got[-1] == GUARD and (sums is None or list(got[1:-1]) == list(sums)), "the sums are read, never written"
        d.free()

    def state(self):
        return [(t["p"]["dev"].get(), t["m"]["dev"].get() if t["m"] else None, t["v"]["dev"].get()) for t in self.tensors]


def sumsq_extras(ctx, rng, integer):
    """one tensor of 300 001 elements at an odd base offset, and two tensors without elements"""
    n = 300001
    host = rng.integers(-8, 9, n + 1).astype(np.float64) if integer else rng.standard_normal(n + 1) * 3.0
    dev = ctx.upload(host)
    return dev, host[1:], [K.OptimTensor(None, 0, dev.ptr + 8, 1, None, None, n, 1), K.OptimTensor(None, 0, None, 5, None, None, 0, 5),
                           K.OptimTensor(None, 0, dev.ptr, 7, None, None, 3, 0)]


def run_sumsq(ctx, tab, n, accumulate=0, start=GUARD):
    need = int(ctx.lib.hnh_grad_sumsq_f64_workspace(tab, n))
    assert need > 0
    res, work = ctx.upload(np.array([GUARD, start, GUARD])), ctx.upload(np.full(need + 2, GUARD))
    ctx.check(ctx.lib.hnh_grad_sumsq_f64(ctx.h, tab, n, accumulate, res.ptr + 8, work.ptr + 8, need, K.STREAM_COMPUTE), "hnh_grad_sumsq_f64")
    ctx.sync()
    r, w = res.get(), work.get()
    assert r[0] == GUARD and r[2] == GUARD and w[0] == GUARD and w[-1] == GUARD, "guards round the result and the workspace"
    res.free()
    work.free()
    return float(r[1])


def sumsq_case(ctx, integer):
    p = ClipProblem(ctx, "sgd", seed=3)
    rng = np.random.default_rng(11)
    arrays = p.gradient_arrays()
    for j, g in enumerate(arrays):  # integers, or normal values at scales 1e-6 .. 1e2
        shape = g["host"].shape
        g["host"] = rng.integers(-8, 9, shape).astype(np.float64) if integer else rng.standard_normal(shape) * 10.0 ** (-6.0 + 8.0 * j / (len(arrays) - 1))
        g["dev"].set(g["host"])
    dev, big, extras = sumsq_extras(ctx, rng, integer)
    own = p.table(full=False)
    tab = (K.OptimTensor * (len(own) + 3))(*(list(own)[:40] + extras[:2] + list(own)[40:] + extras[2:]))
    parts = [t["g"]["host"][:, t["g_off"]:t["g_off"] + t["cols"]] for t in p.tensors] + [big]
    assert len(tab) == 63 and len(tab) > K.OPTIM_MAX_TENSORS and len(tab) % K.OPTIM_MAX_TENSORS != 0
    assert any(t["ld_g"] == 2 for t in p.tensors) and any(t["g_off"] > 0 and t["ld_g"] > 2 for t in p.tensors)
    assert any(t["rows"] == 1 for t in p.tensors) and any(t["cols"] == 1 for t in p.tensors)
    return p, dev, tab, parts


def test_sumsq_kernel_is_exact_on_integers(ctx):
    p, dev, tab, parts = sumsq_case(ctx, integer=True)
    want = float(sum(np.sum(np.square(a)) for a in parts))
    assert want > 1e6 and want == float(int(want))
    got = run_sumsq(ctx, tab, len(tab))
    assert got == want, "every partial sum is an integer below 2^53: exact in any order"
    assert run_sumsq(ctx, tab, len(tab)) == got
    assert run_sumsq(ctx, tab, len(tab), accumulate=1, start=1234.5) == 1234.5 + want
    # one launch's worth, a single tensor, nothing at all
    assert run_sumsq(ctx, tab, 5) == float(sum(np.sum(np.square(a)) for a in parts[:5]))
    assert run_sumsq(ctx, (K.OptimTensor * 1)(tab[40]), 1) == float(np.sum(np.square(parts[-1]))), "the long tensor alone"
    assert run_sumsq(ctx, (K.OptimTensor * 2)(tab[41], tab[62]), 2) == 0.0 and run_sumsq(ctx, None, 0) == 0.0
    assert run_sumsq(ctx, None, 0, accumulate=1, start=2.5) == 2.5
    dev.free()
    p.free()


def test_sumsq_kernel_vs_longdouble(ctx):
    p, dev, tab, parts = sumsq_case(ctx, integer=False)
    scales = sorted(float(np.abs(a).max()) for a in parts)
    assert scales[0] < 1e-4 and scales[-1] > 10.0, "gradients across many scales"
    want = sum(np.sum(np.square(a.astype(np.longdouble)), dtype=np.longdouble) for a in parts)
    got = run_sumsq(ctx, tab, len(tab))
    err = float(abs(np.longdouble(got) - want) / want)
    T.record_observed("gat_clip_sumsq_kernel", case="63 tensors", worst=err)
    print("observed sumsq against longdouble: %.2e" % err)
    assert err <= T.TOL
    assert run_sumsq(ctx, tab, len(tab)) == got, "a repeat must be bit-identical"
    first = run_sumsq(ctx, tab, 20)
    assert run_sumsq(ctx, tab, len(tab), accumulate=1, start=first) == first + got, "accumulate adds onto the earlier value to the bit"
    dev.free()
    p.free()


def test_sumsq_kernel_refusals(ctx):
    lib = ctx.lib
    d = ctx.upload(np.zeros(64))
    ok = (K.OptimTensor * 1)(K.OptimTensor(None, 0, d.ptr, 4, None, None, 3, 4))
    need = int(lib.hnh_grad_sumsq_f64_workspace(ok, 1))
    assert need >= 1
    ctx.check(lib.hnh_grad_sumsq_f64(ctx.h, ok, 1, 0, d.ptr + 256, d.ptr + 264, need, K.STREAM_COMPUTE), "p, m and v may be null")
    assert lib.hnh_grad_sumsq_f64(ctx.h, ok, 1, 0, d.ptr + 256, d.ptr + 264, need - 1, K.STREAM_COMPUTE) == 1, "a short workspace"
    assert lib.hnh_grad_sumsq_f64(ctx.h, ok, 1, 0, None, d.ptr + 264, need, K.STREAM_COMPUTE) == 1, "a null result"
    assert lib.hnh_grad_sumsq_f64(ctx.h, ok, 1, 0, d.ptr + 256, None, need, K.STREAM_COMPUTE) == 1, "a null workspace"
    narrow = (K.OptimTensor * 1)(K.OptimTensor(None, 0, d.ptr, 3, None, None, 3, 4))
    assert lib.hnh_grad_sumsq_f64_workspace(narrow, 1) < 0
    assert lib.hnh_grad_sumsq_f64(ctx.h, narrow, 1, 0, d.ptr + 256, d.ptr + 264, 64, K.STREAM_COMPUTE) == 1, "a pitch below the width"
    null_g = (K.OptimTensor * 1)(K.OptimTensor(None, 0, None, 4, None, None, 3, 4))
    assert lib.hnh_grad_sumsq_f64(ctx.h, null_g, 1, 0, d.ptr + 256, d.ptr + 264, 64, K.STREAM_COMPUTE) == 1, "a null gradient with elements"
    assert lib.hnh_grad_sumsq_f64(ctx.h, None, 1, 0, d.ptr + 256, d.ptr + 264, 64, K.STREAM_COMPUTE) == 1, "a null table"
    ctx.sync()
    d.free()


# ------------------------------------------------------------------------------------------------ the clipped optimizer step
SUMS, MAX_NORM = [30.0, 6.0], 1.5  # norm 6: coef about 0.25
KERNEL_CASES = [("adam", dict(lr=0.01, weight_decay=5e-4)), ("sgd", dict(lr=0.05, momentum=0.9, weight_decay=5e-4)), ("adamw", dict(lr=0.01, weight_decay=0.01)),
                ("adamw", dict(lr=0.003, beta1=0.8, beta2=0.99, eps=1e-6, weight_decay=0.1))]


@pytest.mark.parametrize("kind,hyper", KERNEL_CASES)
def test_clip_step_kernel_vs_numpy(ctx, kind, hyper):
    p = ClipProblem(ctx, kind, seed=len(hyper))
    coef = min(1.0, MAX_NORM / (np.sqrt(SUMS[0] + SUMS[1]) + 1e-6))
    assert 0.2 < coef < 0.3
    start = [t["p"]["host"].copy() for t in p.tensors]
    worst = 0.0
    for step in range(1, 5):
        p.clip_step(step, hyper, SUMS, MAX_NORM)
        for t in p.tensors:
            cols = t["cols"]
            g = coef * t["g"]["host"][:, t["g_off"]:t["g_off"] + cols]
            old = t["p"]["host"][:, :cols]
            if kind == "sgd":
                newp, t["v"]["host"] = R.sgd_step(old, g, t["v"]["host"], hyper["lr"], **{k: hyper[k] for k in ("momentum", "weight_decay") if k in hyper})
            else:
                kw = {k: hyper[k] for k in ("beta1", "beta2", "eps", "weight_decay") if k in hyper}
                newp, t["m"]["host"], t["v"]["host"] = (R.adam_step if kind == "adam" else CR.adamw_step)(old, g, t["m"]["host"], t["v"]["host"], step, hyper["lr"], **kw)
            t["p"]["host"][:, :cols] = newp
            got_p = t["p"]["dev"].get()
            assert np.all(got_p[:, cols:] == GUARD), "the parameter's pitch padding is untouched"
            errs = [T.rel(got_p[:, :cols], newp), T.rel(t["v"]["dev"].get(), t["v"]["host"])] + ([T.rel(t["m"]["dev"].get(), t["m"]["host"])] if t["m"] else [])
            worst = max(worst, *errs)
            assert max(errs) <= T.TOL, (step, t["rows"], cols, t["ld_g"], errs)
        p.new_gradients()
    assert all(np.abs(t["p"]["host"][:, :t["cols"]] - s[:, :t["cols"]]).max() > 0 for t, s in zip(p.tensors, start)), "every tensor has moved"
    T.record_observed("gat_clip_step_kernel", case="%s %s" % (kind, sorted(hyper.items())), worst=worst)
    print("observed clip step", kind, hyper, "worst %.2e" % worst)
    p.free()


def same_state(a, b):
    return all(np.array_equal(x, y) for ta, tb in zip(a, b) for x, y in zip(ta, tb) if x is not None)


@pytest.mark.parametrize("kind,hyper", KERNEL_CASES[:2])
@pytest.mark.parametrize("sums", [None, [1e-4, 2e-4]], ids=["null sumsq", "coef 1"])
def test_clip_step_with_coef_one_is_the_parent_to_the_bit(ctx, kind, hyper, sums):
    twin, mine = OptimProblem(ctx, kind, seed=5), ClipProblem(ctx, kind, seed=5)
    for step in range(1, 4):
        twin.step(step, hyper)  # hnh_optim_step_f64
        mine.clip_step(step, hyper, sums, 1e300 if sums is None else 0.5)  # (norm about 0.017 below max_norm 0.5: coef == 1)
        theirs = [(t["p"]["dev"].get(), t["m"]["dev"].get() if t["m"] else None, t["v"]["dev"].get()) for t in twin.tensors]
        assert same_state(mine.state(), theirs), "p, m and v bit-identical to hnh_optim_step_f64's"
        twin.new_gradients()
        mine.new_gradients()  # (the same generator state: the same gradients)
    assert all(np.array_equal(a["g"]["host"], b["g"]["host"]) for a, b in zip(twin.tensors, mine.tensors))
    twin.free()
    mine.free()


@pytest.mark.parametrize("sums,max_norm", [(None, 0.0), (SUMS, MAX_NORM)], ids=["unclipped", "clipped"])
def test_adamw_without_decay_is_adam_to_the_bit(ctx, sums, max_norm):
    hyper = dict(lr=0.01, weight_decay=0.0)
    a, b = ClipProblem(ctx, "adam", seed=9), ClipProblem(ctx, "adamw", seed=9)
    for step in range(1, 4):
        a.clip_step(step, hyper, sums, max_norm)
        b.clip_step(step, hyper, sums, max_norm)
        assert same_state(a.state(), b.state())
        a.new_gradients()
        b.new_gradients()
    a.free()
    b.free()


def test_clip_step_kernel_refusals(ctx):
    lib = ctx.lib
    d = ctx.upload(np.ones(16))
    tab = (K.OptimTensor * 1)(K.OptimTensor(d.ptr, 2, d.ptr + 64, 2, None, d.ptr + 32, 2, 2))
    sgd = K.Optim(K.OPTIM_SGD, 0, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.1, 0.001)
    ctx.check(lib.hnh_optim_step_clip_f64(ctx.h, tab, 1, C.byref(sgd), d.ptr + 96, 2, 1.0, K.STREAM_COMPUTE), "sgd without m")
    ctx.check(lib.hnh_optim_step_clip_f64(ctx.h, None, 0, C.byref(sgd), None, 0, 0.0, K.STREAM_COMPUTE), "an empty table")
    for kind in (K.OPTIM_ADAM, K.OPTIM_ADAMW):
        hy = K.Optim(kind, 0, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.1, 0.001)
        assert lib.hnh_optim_step_clip_f64(ctx.h, tab, 1, C.byref(hy), None, 0, 0.0, K.STREAM_COMPUTE) == 1, "Adam and AdamW need m"
    assert lib.hnh_optim_step_clip_f64(ctx.h, tab, 1, C.byref(K.Optim(3, 0, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.1, 0.001)), None, 0, 0.0, K.STREAM_COMPUTE) == 1
    for nsums, max_norm in ((0, 1.0), (K.CLIP_MAX_SUMS + 1, 1.0), (2, -1.0), (2, float("nan"))):
        assert lib.hnh_optim_step_clip_f64(ctx.h, tab, 1, C.byref(sgd), d.ptr + 96, nsums, max_norm, K.STREAM_COMPUTE) == 1, (nsums, max_norm)
    assert lib.hnh_optim_step_f64(ctx.h, tab, 1, C.byref(K.Optim(K.OPTIM_ADAMW, 0, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.1, 0.001)), K.STREAM_COMPUTE) == 1, \
        "the parent entry point does not know AdamW"
    ctx.sync()
    d.free()


# ------------------------------------------------------------------------------------------------ trajectories
MAX_NORM_TRAINED = 0.2
# the reference's norms under max_norm 0.2, steps 1 - 10 (computed on the CPU):
#   adam   0.2033 0.1987 0.1930 0.1925 0.2031 0.2145 0.2286 0.2416 0.2503 0.2605
#   sgd    0.2033 0.2066 0.2044 0.2022 0.2011 0.2012 0.1978 0.1986 0.1962 0.1935
#   adamw  0.2033 0.1991 0.1914 0.1932 0.2042 0.2156 0.2301 0.2424 0.2522 0.2616
OPTIMIZERS = {"adam": dict(kind="adam", lr=0.01, weight_decay=5e-4), "sgd": dict(kind="sgd", lr=0.05, momentum=0.9),
              "adamw": dict(kind="adamw", lr=0.01, weight_decay=0.01)}
SCHEDULE = dict(kind="cosine", W=3, T=8, min_factor=0.1)


def device_train(world, pp, layers, optimizer, steps, max_norm=None, schedule=None, lr_at=None, clip_then_off=False):
    s = setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["w"], pp["av"], None, attention="softmax", score="additive")
    gnn = s["gnn"]
    gnn.set_labels(pp["labels"], pp["mask"], heads="mean")
    opt = dict(optimizer)
    gnn.set_optimizer(opt.pop("kind"), opt.pop("lr"), **opt)
    if clip_then_off:
        gnn.set_grad_clip(0.2)
    gnn.set_grad_clip(max_norm)
    if schedule:
        gnn.set_lr_schedule(schedule["kind"], schedule["W"], schedule["T"], schedule["min_factor"])
    res = dict(losses=[], accs=[], norms=[], rates=[])
    for t in range(1, steps + 1):
        if lr_at and t in lr_at:
            gnn.set_learning_rate(lr_at[t])
        res["rates"].append(gnn.learning_rate())
        loss, acc = gnn.train_step()
        res["losses"].append(loss)
        res["accs"].append(acc)
        if max_norm:
            res["norms"].append(gnn.grad_norm())
    res["w"] = {k: gnn.get_weight(*k) for k in pp["w"]}
    res["av"] = {k: gnn.get_attention_vectors(*k) for k in pp["w"]}
    teardown(s)
    return res


def measured_bounds(pp, layers, optimizer, steps, **kw):
    """test_gat_train_gpu.measured_bounds with the trainer of gat_clip_ref: (reference run, allowed parameter difference, allowed loss
    difference), 10 x the divergence of a reference run whose gradients are perturbed by 1e-10 * max|g| * u."""
    args = (pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, pp["labels"], pp["mask"], "mean", pp["w"], pp["av"], optimizer, steps)
    ref = CR.train(*args, **kw)
    per = CR.train(*args, perturb=(1e-10, np.random.default_rng(7)), **kw)
    div_p = R.parameter_divergence(per[2], per[3], ref[2], ref[3])
    div_l = float(np.max(np.abs(np.array(per[0]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    assert div_p > 0 and div_l > 0
    return ref, 10.0 * div_p, 10.0 * div_l


@pytest.mark.parametrize("kind", sorted(OPTIMIZERS))
@pytest.mark.parametrize("p", [1, 4])
def test_clipped_trajectory_vs_reference(p, kind):
    layers = T.GAT_LAYERS
    pp = R.planted_partition(layers)
    ref, bound_p, bound_l = measured_bounds(pp, layers, OPTIMIZERS[kind], 10, max_norm=MAX_NORM_TRAINED)
    norms = np.array(ref[4])
    # the condition on the reference's own clipped run: steps that clip, steps that do not, none at the threshold
    assert np.count_nonzero(norms > MAX_NORM_TRAINED) >= 2 and np.count_nonzero(norms < MAX_NORM_TRAINED) >= 2, norms
    assert np.all(np.abs(norms - MAX_NORM_TRAINED) > 1e-3 * MAX_NORM_TRAINED), norms
    unclipped = CR.train(pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, pp["labels"], pp["mask"], "mean", pp["w"], pp["av"], OPTIMIZERS[kind], 10)
    assert R.parameter_divergence(unclipped[2], unclipped[3], ref[2], ref[3]) > 1e3 * bound_p, "clipping matters"
    per_rank = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, OPTIMIZERS[kind], 10, max_norm=MAX_NORM_TRAINED))
    check_trajectory(per_rank, ref, bound_p, bound_l, "clipped %s" % kind, p)
    r0 = per_rank[0]
    assert all(pr["norms"] == r0["norms"] for pr in per_rank), "grad_norm() is bit-equal across ranks"
    err = float(np.max(np.abs(np.array(r0["norms"]) - norms) / norms))
    T.record_observed("gat_clip_grad_norm", case=kind, ranks=p, worst=err, last=abs(r0["norms"][-1] - norms[-1]) / norms[-1])
    print("observed grad_norm", kind, p, "%.2e" % err, r0["norms"])
    assert abs(r0["norms"][-1] - norms[-1]) <= T.TOL * norms[-1]


def same_run(a, b):
    return a["losses"] == b["losses"] and a["accs"] == b["accs"] and all(
        np.array_equal(a["w"][k], b["w"][k]) and np.array_equal(a["av"][k][0], b["av"][k][0]) and np.array_equal(a["av"][k][1], b["av"][k][1]) for k in a["w"])


@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("p", [1, 4])
def test_clipping_that_never_clips_changes_no_bit(p, kind):
    layers = T.GAT_LAYERS
    pp = R.planted_partition(layers)
    plain = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, OPTIMIZERS[kind], 5))
    huge = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, OPTIMIZERS[kind], 5, max_norm=1e300))
    off_again = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, OPTIMIZERS[kind], 5, clip_then_off=True))
    for a, b, c in zip(plain, huge, off_again):
        assert same_run(a, b), "max_norm 1e300: losses and every parameter bit-equal to a run without clipping"
        assert same_run(a, c), "clipping switched on and off again before the first step"
        assert len(b["norms"]) == 5 and all(0.1 < n < 0.4 for n in b["norms"]) and not a["norms"] and not c["norms"]
    assert all(np.abs(plain[0]["w"][k] - pp["w"][k]).max() > 0 for k in pp["w"])


def test_schedule_and_set_learning_rate_vs_reference():
    layers, p, steps = T.GAT_LAYERS, 4, 10
    pp = R.planted_partition(layers)
    for label, kw in (("cosine with warm-up", dict(schedule=SCHEDULE)), ("set_learning_rate at step 5", dict(lr_at={5: 0.03}))):
        ref, bound_p, bound_l = measured_bounds(pp, layers, OPTIMIZERS["adam"], steps, **kw)
        fixed = CR.train(pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, pp["labels"], pp["mask"], "mean", pp["w"], pp["av"], OPTIMIZERS["adam"], steps)
        assert R.parameter_divergence(fixed[2], fixed[3], ref[2], ref[3]) > 1e3 * bound_p, "the rate matters"
        per_rank = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, OPTIMIZERS["adam"], steps, **kw))
        check_trajectory(per_rank, ref, bound_p, bound_l, label, p)
        sched = kw.get("schedule")
        want = [(0.03 if "lr_at" in kw and t >= 5 else 0.01) * (CR.lr_factor(sched["kind"], t, sched["W"], sched["T"], sched["min_factor"]) if sched else 1.0)
                for t in range(1, steps + 1)]
        assert np.allclose(per_rank[0]["rates"], want, rtol=1e-15, atol=0.0), (per_rank[0]["rates"], want)
    assert want[4] == 0.03 and want[3] == 0.01


# ------------------------------------------------------------------------------------------------ what the norm is made of
def full_model_problem():
    """test_gat_norm_gpu's training problem with score transformer (W_q, W_k, a bias, a projection, layer norm on both layers) and, on
    layer 0, a learned edge bias that is -1e300 on the entry with the largest column of every row that has another column"""
    norms = ("layer", "layer")
    pp, p = NG.train_problem("transformer", norms)
    rows, cols, m = np.asarray(pp["rows"]), np.asarray(pp["cols"]), pp["m"]
    top, low = np.full(m, -1), np.full(m, m)
    np.maximum.at(top, rows, cols)
    np.minimum.at(low, rows, cols)
    return pp, p, norms, lambda r, c: np.where((c == top[r]) & (top[r] > low[r]), OFF, LG.E.hash_bias(r, c))


def full_model_rank(world, pp, p, norms, fn):
    s = setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], NG.TRAIN_LAYERS, p["w"], None, None, attention="softmax", score="transformer",
              activation=NG.PUBLISHED, residual=NG.TRAIN_RESIDUAL, bias=True, norm=norms)
    gnn = s["gnn"]
    NG.configure(gnn, p, "transformer")
    gnn.edge_bias_from(fn, layer=0)
    gnn.set_edge_bias_learned(0)
    gnn.set_labels(pp["labels"], pp["mask"], heads="mean")
    gnn.set_optimizer("adam", 0.01, weight_decay=5e-4)
    with pytest.raises(H.HnhError, match="grad_norm needs"):
        gnn.grad_norm()
    gnn.set_grad_clip(1e300)
    gnn.train_step()
    res = dict(norm=gnn.grad_norm())
    rep = [gnn.weight_grad(*k) for k in p["w"]] + [gnn.query_weight_grad(*k) for k in p["w"]] + [gnn.key_weight_grad(*k) for k in p["w"]]
    rep += [gnn.residual_weight_grad(li) for li in p["wr"]] + [gnn.bias_grad(li) for li in p["bias"]]
    rep += [g for li in p["gamma"] for g in gnn.norm_grad(li)]
    res["replicated"] = rep
    res["edge"] = gnn.edge_bias_grad(0)
    gnn.set_grad_clip(0.5 * res["norm"])
    res["norms"] = []
    for _ in range(3):
        gnn.train_step()
        res["norms"].append(gnn.grad_norm())
    res["p"] = NG.read_parameters(gnn, p)
    res["eb"] = gnn.get_edge_bias(0)
    srows, scols = s["d"].S_coordinates()
    tcols, trows = s["d"].ST_coordinates()
    res["coords"] = ((srows, scols), (trows, tcols))
    teardown(s)
    return res


def test_what_the_norm_is_made_of():
    pp, p, norms, fn = full_model_problem()
    per_rank = H.run_spmd(4, lambda wd: full_model_rank(wd, pp, p, norms, fn))
    r0 = per_rank[0]
    for pr in per_rank:
        assert pr["norm"] == r0["norm"] and pr["norms"] == r0["norms"], "grad_norm() is bit-equal across ranks"
        assert all(np.array_equal(a, b) for a, b in zip(pr["replicated"], r0["replicated"]))
        assert NG.same_parameters(pr["p"], r0["p"]), "replicated parameters stay bit-equal across ranks under clipping"
    replicated = sum(float(np.sum(np.square(g.astype(np.longdouble)))) for g in r0["replicated"])
    edge = sum(float(np.sum(np.square(pr["edge"][0].astype(np.longdouble)))) for pr in per_rank)
    edge_t = sum(float(np.sum(np.square(pr["edge"][1].astype(np.longdouble)))) for pr in per_rank)
    assert replicated > 0 and edge > 1e-6 * replicated and abs(edge_t - edge) <= 1e-9 * edge, "the S^T copy holds the same numbers"
    err = abs(r0["norm"] ** 2 - (replicated + edge)) / (replicated + edge)
    T.record_observed("gat_clip_norm_parts", ranks=4, worst=err, replicated=replicated, edge=edge)
    print("observed norm^2 %.6e = replicated %.6e + edge bias %.6e to %.2e" % (r0["norm"] ** 2, replicated, edge, err))
    assert err <= T.TOL, "replicated tensors once, the S-order edge-bias gradient over the ranks, the S^T copy not at all"
    assert all(n > 0.5 * r0["norm"] for n in r0["norms"]), "the three steps at half the norm all clip"
    # both copies of the trained bias: the same numbers through the coordinates, the switched-off entries untouched
    both = []
    for which in (0, 1):
        both.append(LG.by_coordinates(np.concatenate([pr["coords"][which][0] for pr in per_rank]), np.concatenate([pr["coords"][which][1] for pr in per_rank]),
                                      np.concatenate([pr["eb"][which] for pr in per_rank])))
    rows, cols = np.asarray(pp["rows"]), np.asarray(pp["cols"])
    sr, sc, start = LG.by_coordinates(rows, cols, fn(rows, cols))
    off = start == OFF
    assert np.count_nonzero(off) > 100
    for gr, gc, gv in both:
        assert np.array_equal(gr, sr) and np.array_equal(gc, sc)
        assert np.array_equal(gv[off], np.full(np.count_nonzero(off), OFF)), "an entry at -1e300 is still -1e300 to the bit"
        assert np.abs(gv[~off] - start[~off]).max() > 0, "the bias was trained"
    assert T.rel(both[1][2][~off], both[0][2][~off]) <= 1e-12, "the two copies of the bias agree"


# ------------------------------------------------------------------------------------------------ the multi-label head; refusals
def test_clipped_step_under_the_multilabel_head():
    layers = T.GAT_LAYERS
    pp = M.planted_tags(layers)

    def rank(world):
        s = setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["w"], pp["av"], None, attention="softmax", score="additive", activation=M.PUBLISHED)
        gnn = s["gnn"]
        gnn.set_multilabel_targets(pp["targets"], pp["mask"], heads="mean")
        gnn.set_optimizer("adamw", 0.02, weight_decay=0.01)
        gnn.set_grad_clip(0.05)
        res = gnn.train_step(), gnn.grad_norm(), gnn.train_step()
        teardown(s)
        return res

    per_rank = H.run_spmd(2, rank)
    (loss, f1), norm, (loss2, _) = per_rank[0]
    assert per_rank[1] == per_rank[0] and np.isfinite(loss) and 0.0 <= f1 <= 1.0 and norm > 0 and np.isfinite(loss2) and loss2 != loss


def test_refusals_on_the_device():
    layers = T.GAT_LAYERS
    pp = R.planted_partition(layers)

    def rank(world):
        s = setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["w"], pp["av"], None, attention="softmax", score="additive")
        gnn = s["gnn"]
        gnn.set_labels(pp["labels"], pp["mask"])
        gnn.set_optimizer("adam", 0.01)
        with pytest.raises(H.HnhError, match="grad_norm needs"):
            gnn.grad_norm()
        first = gnn.train_step()
        with pytest.raises(H.HnhError, match="grad_norm needs"):
            gnn.grad_norm()  # (a step without clipping leaves no norm)
        for bad in (-0.5, float("nan"), float("inf")):
            with pytest.raises(H.HnhError, match="set_grad_clip needs a finite max_norm >= 0"):
                gnn.set_grad_clip(bad)
        for args in (("linear", 4, 4, 0.0), ("cosine", 0, 0, 0.0), ("cosine", 0, 4, 1.01), ("constant", -2, 0, 0.0)):
            with pytest.raises(H.HnhError, match="set_lr_schedule"):
                gnn.set_lr_schedule(*args)
        second = gnn.train_step()  # the refused calls left the object as it was: no clipping, the constant rate
        assert gnn.learning_rate() == 0.01
        gnn.set_grad_clip(0.2)
        with pytest.raises(H.HnhError, match="backwardPass since the last step"):
            gnn.optimizer_step()
        third = gnn.train_step()
        norm = gnn.grad_norm()
        teardown(s)
        return first, second, third, norm

    for first, second, third, norm in H.run_spmd(2, rank):
        assert np.isfinite(first[0]) and second[0] != first[0] and third[0] != second[0] and 0.1 < norm < 0.4
