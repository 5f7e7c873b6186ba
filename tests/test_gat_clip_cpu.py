"""Gradient clipping, AdamW and learning-rate schedules of the GAT's training step without a GPU (include/hnh_train_clip.h; GAT.set_grad_clip
/ grad_norm / set_optimizer("adamw") / set_learning_rate / learning_rate / set_lr_schedule; tests/gat_clip_ref.py is the definition).

The definition against torch on CPU tensors in float64, an independent implementation, over five steps on a handful of random tensors:
clip_coef against torch.nn.utils.clip_grad_norm_, adamw_step against torch.optim.AdamW, L2 Adam behind clipping against torch.optim.Adam
behind clip_grad_norm_; bound 1e-14 relative (both sides round a few times per element and step; the update is lr times a number of order
one).  lr_factor against its closed form at t = 1, W, W + 1, T, T + 1, and its continuity at W and T.  The optional kernel group: declared
== bound == exported by the HIP library with those argtypes, disjoint from every other header and table, absent from both CPU test doubles,
hnh_train.h as it was.  The host calls.  On the second test double (which has hnh_train.h but not the new group) with 2 loopback ranks:
the refusals of set_grad_clip and set_lr_schedule, the refusals of train_step / optimizer_step under clipping and under adamw naming a
symbol of the group and its header, the same object then training bit for bit like one that never heard of clipping, and learning_rate()
through a warm-up of 3 in a linear schedule of 6 and through set_learning_rate.

Observed here: clip 2.6e-16, AdamW 4.6e-17, clipped Adam 9.2e-17 against torch."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import gat_clip_ref as CR
import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared
import gat_gpu_harness as G  # (the functions only: its hip_backend / ctx fixtures are not imported)

GROUP = {"hnh_grad_sumsq_f64_workspace", "hnh_grad_sumsq_f64", "hnh_optim_step_clip_f64"}
HOST_CALLS = ("hnh_gat_set_grad_clip", "hnh_gat_grad_norm", "hnh_gat_set_learning_rate", "hnh_gat_learning_rate", "hnh_gat_set_lr_schedule")
TORCH_TOL = 1e-14
SHAPES = [(7, 5), (1, 9), (33,), (4, 1), (16, 8)]


def tensors(seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s) for s in SHAPES], rng


# ------------------------------------------------------------------------------------------------ the definition against torch
@pytest.mark.parametrize("max_norm", [0.5, 3.0, 1e3])
def test_clip_coef_is_clip_grad_norm(max_norm):
    grads, _ = tensors(1)
    params = [torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = torch.tensor(g)
    total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    coef = CR.clip_coef(grads, max_norm)
    assert abs(total - CR.grad_norm(grads)) <= TORCH_TOL * total
    assert (coef < 1.0) == (total > max_norm) and (max_norm < 1e3 or coef == 1.0)
    worst = max(T.rel(coef * g, p.grad.numpy()) for p, g in zip(params, grads))
    print("observed clip against torch: %.2e" % worst)
    assert worst <= TORCH_TOL
    assert CR.clip_coef(grads, None) == 1.0 and CR.clip_coef(grads, 0.0) == 1.0


def run_against_torch(kind, hyper, max_norm):
    """Five steps with new gradients each: the definition next to torch.optim, (worst difference, whether every / no step clipped)"""
    start, rng = tensors(2)
    params = [torch.nn.Parameter(torch.tensor(p)) for p in start]
    make = {"adamw": torch.optim.AdamW, "adam": torch.optim.Adam}[kind]
    opt = make(params, lr=hyper["lr"], betas=(hyper["beta1"], hyper["beta2"]), eps=hyper["eps"], weight_decay=hyper["weight_decay"])
    mine = [p.copy() for p in start]
    mom, var = [np.zeros_like(p) for p in start], [np.zeros_like(p) for p in start]
    step = {"adamw": CR.adamw_step, "adam": R.adam_step}[kind]
    worst, clipped = 0.0, []
    for t in range(1, 6):
        grads = [rng.standard_normal(p.shape) * (0.1 if t % 2 else 10.0) for p in start]  # (global norms of about 1.4 and 140)
        for p, g in zip(params, grads):
            p.grad = torch.tensor(g)
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        coef = CR.clip_coef(grads, max_norm)
        clipped.append(coef < 1.0)
        for k, g in enumerate(grads):
            mine[k], mom[k], var[k] = step(mine[k], coef * g, mom[k], var[k], t, hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"], hyper["weight_decay"])
        worst = max(worst, max(T.rel(a, p.detach().numpy()) for a, p in zip(mine, params)))
    assert all(np.abs(a - s).max() > 1e-3 for a, s in zip(mine, start)), "every tensor has moved"
    return worst, clipped


HYPER = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05)


def test_adamw_step_is_torch_adamw():
    worst, _ = run_against_torch("adamw", HYPER, None)
    print("observed AdamW against torch: %.2e" % worst)
    assert worst <= TORCH_TOL
    # decoupled: not Adam with the L2 term
    p, g, z = np.ones(3), np.full(3, 0.5), np.zeros(3)
    assert np.abs(CR.adamw_step(p, g, z, z, 1, 0.1, weight_decay=0.3)[0] - R.adam_step(p, g, z, z, 1, 0.1, weight_decay=0.3)[0]).max() > 1e-3
    for a, b in zip(CR.adamw_step(p, g, z, z, 1, 0.1, weight_decay=0.0), R.adam_step(p, g, z, z, 1, 0.1)):
        assert np.array_equal(a, b), "AdamW without decay is Adam"


def test_clipped_l2_adam_is_torch_adam_behind_clip_grad_norm():
    worst, clipped = run_against_torch("adam", HYPER, 4.0)
    print("observed clipped Adam against torch: %.2e" % worst, clipped)
    assert any(clipped) and not all(clipped), "steps that clip and steps that do not"
    assert worst <= TORCH_TOL
    worst, clipped = run_against_torch("adamw", HYPER, 4.0)
    assert any(clipped) and worst <= TORCH_TOL


# ------------------------------------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("kind", CR.SCHEDULES)
def test_lr_factor_closed_form_and_continuity(kind):
    W, total, f = 5, 17, 0.1
    assert CR.lr_factor(kind, 1, W, total, f) == 1 / 5 and CR.lr_factor(kind, W, W, total, f) == 1.0
    after = CR.lr_factor(kind, W + 1, W, total, f)
    at_end, beyond = CR.lr_factor(kind, total, W, total, f), CR.lr_factor(kind, total + 1, W, total, f)
    if kind == "constant":
        assert after == at_end == beyond == 1.0 and CR.lr_factor(kind, 10 ** 6, W, total, f) == 1.0
    else:
        want = 1.0 - 0.9 / 12 if kind == "linear" else 0.1 + 0.9 * 0.5 * (1.0 + math.cos(math.pi / 12))
        assert abs(after - want) <= 1e-15 and abs(at_end - f) <= 1e-15 and beyond == f
        assert all(CR.lr_factor(kind, t, W, total, f) > CR.lr_factor(kind, t + 1, W, total, f) for t in range(W, total)), "it descends"
    # continuity: one step on either side of W and of T moves the factor by no more than the steepest slope allows
    slope = max(1.0 / W, (1.0 - f) * (math.pi / 2 if kind == "cosine" else 1.0) / (total - W))
    for t in (W - 1, W, total - 1, total):
        assert abs(CR.lr_factor(kind, t + 1, W, total, f) - CR.lr_factor(kind, t, W, total, f)) <= slope + 1e-15
    # no warm-up: the first step has the full rate
    first = CR.lr_factor(kind, 1, 0, total, f)
    assert first == 1.0 if kind == "constant" else CR.lr_factor(kind, 2, 0, total, f) < first < 1.0
    assert CR.lr_factor("constant", 1) == 1.0


# ------------------------------------------------------------------------------------------------ the group and the host calls
def test_clip_kernels_are_an_optional_group():
    names = declared("hnh_train_clip.h")
    assert names == GROUP
    assert names == set(K.TRAIN_CLIP_SIGNATURES), names ^ set(K.TRAIN_CLIP_SIGNATURES)
    headers = [h for h in os.listdir(os.path.join(ROOT, "include")) if h.endswith(".h") and h != "hnh_train_clip.h"]
    assert "hnh_train.h" in headers and "hnh_train_multilabel.h" in headers and len(headers) >= 16
    for header in headers:
        assert not names & declared(header), header
    tables = [n for n in dir(K) if n.endswith("SIGNATURES") and n != "TRAIN_CLIP_SIGNATURES"]
    assert "TRAIN_SIGNATURES" in tables and "SIGNATURES" in tables and len(tables) >= 16
    for table in tables:
        assert not names & set(getattr(K, table)), table
    assert not names & set(H.SIGNATURES)
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.TRAIN_CLIP_SIGNATURES[n][1] and getattr(lib, n).restype == K.TRAIN_CLIP_SIGNATURES[n][0]
    for path in (T.ORACLE_BACKEND, T.ORACLE_GAT_BACKEND):
        dbl = C.CDLL(path)
        for n in names:
            assert not hasattr(dbl, n), "the CPU test double %s does not export %s" % (os.path.basename(path), n)
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works
    assert declared("hnh_train.h") == set(K.TRAIN_SIGNATURES) == {"hnh_xent_rows_f64_workspace", "hnh_xent_rows_f64", "hnh_optim_step_f64"}, "hnh_train.h is as it was"
    assert C.sizeof(K.OptimTensor) == 64 and C.sizeof(K.Optim) == 72, "the structs of hnh_train.h are as they were"
    txt = open(os.path.join(ROOT, "include", "hnh_train_clip.h")).read()
    assert re.search(r"#define HNH_OPTIM_ADAMW 2\b", txt) and K.OPTIM_ADAMW == 2 and "not finite" in txt and "clip_grad_norm_" in txt
    assert int(re.search(r"#define HNH_CLIP_MAX_SUMS (\d+)", txt).group(1)) == K.CLIP_MAX_SUMS


def test_host_calls_declared_and_exported():
    for n in HOST_CALLS:
        assert n in declared("hnh_dist.h") and n in H.SIGNATURES and hasattr(H.lib(), n), n
    for name in ("set_grad_clip", "grad_norm", "set_learning_rate", "learning_rate", "set_lr_schedule"):
        assert callable(getattr(H.GAT, name))
    assert H.GAT.OPTIMIZER == {"adam": 0, "sgd": 1, "adamw": 2} and H.GAT.LR_SCHEDULE == {"constant": 0, "linear": 1, "cosine": 2}
    txt = open(os.path.join(ROOT, "include", "hnh_dist.h")).read()
    for name, value in (("HNH_GAT_OPTIMIZER_ADAMW", 2), ("HNH_GAT_LR_CONSTANT", 0), ("HNH_GAT_LR_LINEAR", 1), ("HNH_GAT_LR_COSINE", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), txt), name


# ------------------------------------------------------------------------------------------------ on the second test double
@pytest.fixture
def gat_double():
    assert H.load_backend(T.ORACLE_GAT_BACKEND) == "oracle-cpu-test-double-gat"
    yield
    H.load_backend(T.ORACLE_BACKEND)  # the modules after this one find the plain double, as before


def test_clipping_on_the_second_test_double(gat_double):
    layers = T.GAT_LAYERS
    pp = R.planted_partition(layers)
    named = r"GAT (gradient clipping|adamw) needs the kernel (hnh_[a-z0-9_]+).*include/hnh_train_clip\.h"
    adam = dict(weight_decay=5e-4)

    def plain(world):
        """three steps of an object that never heard of clipping"""
        s = G.setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["w"], None, None, attention="softmax")
        gnn = s["gnn"]
        gnn.set_labels(pp["labels"], pp["mask"])
        gnn.set_optimizer("adam", 0.01, **adam)
        res = dict(steps=[gnn.train_step() for _ in range(3)], w={k: gnn.get_weight(*k) for k in pp["w"]})
        G.teardown(s)
        return res

    def rank(world):
        s = G.setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["w"], None, None, attention="softmax")
        gnn = s["gnn"]
        gnn.set_labels(pp["labels"], pp["mask"])
        with pytest.raises(H.HnhError, match="set_optimizer first"):
            gnn.learning_rate()
        with pytest.raises(H.HnhError, match="set_optimizer first"):
            gnn.set_learning_rate(0.1)
        gnn.set_optimizer("adam", 0.01, **adam)
        with pytest.raises(H.HnhError, match="grad_norm needs"):
            gnn.grad_norm()
        # refused, and the object stays as it was: without clipping and without a schedule, the next step trains
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(H.HnhError, match="set_grad_clip needs a finite max_norm >= 0"):
                gnn.set_grad_clip(bad)
        for args in (("linear", 3, 3, 0.0), ("cosine", 5, 2, 0.0), ("linear", 0, 0, 0.0), ("constant", -1, 0, 0.0), ("cosine", 0, 4, 1.5),
                     ("linear", 0, 4, -0.1), ("constant", 0, 0, float("nan")), ("linear", 1, -4, 0.5)):
            with pytest.raises(H.HnhError, match="set_lr_schedule"):
                gnn.set_lr_schedule(*args)
        with pytest.raises(ValueError, match="schedule must be one of"):
            gnn.set_lr_schedule("exponential")
        assert H.lib().hnh_gat_set_lr_schedule(gnn.h, 7, 0, 0, 0.0) != 0
        with pytest.raises(H.HnhError, match="finite lr"):
            gnn.set_learning_rate(-0.5)
        assert gnn.learning_rate() == 0.01
        # under clipping train_step and optimizer_step name a symbol of the group and its header, before anything is launched: seed and
        # step count stay, no forward pass is stored
        gnn.set_grad_clip(0.2)
        seen = set()
        for call in (gnn.train_step, gnn.optimizer_step):
            with pytest.raises(H.HnhError, match=named) as e:
                call()
            seen.add(re.search(named, str(e.value)).groups())
        with pytest.raises(H.HnhError, match="forwardPass"):
            gnn.loss()
        with pytest.raises(H.HnhError, match="grad_norm needs"):
            gnn.grad_norm()
        gnn.set_grad_clip(None)
        gnn.set_optimizer("adamw", 0.01, weight_decay=0.01)
        for call in (gnn.train_step, gnn.optimizer_step):
            with pytest.raises(H.HnhError, match=named) as e:
                call()
            seen.add(re.search(named, str(e.value)).groups())
        assert {w for w, _ in seen} == {"gradient clipping", "adamw"} and {n for _, n in seen} <= GROUP
        gnn.set_grad_clip(0.2)
        gnn.set_optimizer("adam", 0.01, **adam)  # (leaves the clip setting in place)
        with pytest.raises(H.HnhError, match=named):
            gnn.train_step()
        # the same object without the feature: what an object that never heard of it returns, bit for bit
        gnn.set_grad_clip(None)
        res = dict(steps=[gnn.train_step() for _ in range(3)], w={k: gnn.get_weight(*k) for k in pp["w"]})
        # learning_rate() step by step: a warm-up of 3 in a linear schedule of 6 down to 0.25; set_optimizer restarts t and keeps the schedule
        gnn.set_lr_schedule("linear", 3, 6, 0.25)
        gnn.set_optimizer("adam", 0.01, **adam)
        rates = []
        for t in range(1, 9):
            rates.append(gnn.learning_rate())
            if t == 5:
                gnn.set_learning_rate(0.02)  # the step count survives: the factor goes on from t = 5
                assert gnn.learning_rate() == 0.02 * CR.lr_factor("linear", 5, 3, 6, 0.25)
            gnn.train_step()
        res["rates"] = rates
        gnn.set_lr_schedule()  # back to the default
        res["rate_after"] = gnn.learning_rate()
        G.teardown(s)
        return res

    per_rank, want = H.run_spmd(2, rank), H.run_spmd(2, plain)
    for got, ref in zip(per_rank, want):
        assert got["steps"] == ref["steps"] and all(np.isfinite(v) for st in got["steps"] for v in st)
        assert all(np.array_equal(got["w"][k], ref["w"][k]) for k in pp["w"]) and any(np.abs(got["w"][k] - pp["w"][k]).max() > 0 for k in pp["w"])
        base = [0.01] * 5 + [0.02] * 3  # (the rate of step 5 was read before set_learning_rate)
        want_rates = [b * CR.lr_factor("linear", t, 3, 6, 0.25) for t, b in zip(range(1, 9), base)]
        assert np.allclose(got["rates"], want_rates, rtol=1e-15, atol=0.0), (got["rates"], want_rates)
        assert got["rates"][2] == 0.01 and got["rates"][4] < 0.01 and got["rates"][7] == 0.02 * 0.25 and got["rate_after"] == 0.02
