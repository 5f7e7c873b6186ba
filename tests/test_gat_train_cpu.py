"""The GAT's training step without a GPU: the numpy definition of the loss (tests/gat_ref.py) against central finite differences
for heads "mean" and "concat" and against its extended-precision twin; Adam and SGD against a second, scalar-loop restatement; the
optional kernel group of include/hnh_train.h (declared == bound == exported by the HIP library, disjoint from the six existing tables and
headers, absent from the CPU test double); the host calls; on the test double, loss and train_step name a kernel of the group and its
header, bad labels, an empty mask and a missing optimizer are refused, and the same object then runs the plain GAT bit for bit; and the
learning problem of the GPU test meets its conditions on the reference.

Observed here: loss gradient against finite differences <= 2.2e-8 of its largest entry (bound 1e-6, the bound of the other
finite-difference tests); float64 against longdouble within 1e-14; the vectorised optimizers against the scalar loops within 1e-15."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared, make_gat, plain_output

GROUP = {"hnh_xent_rows_f64_workspace", "hnh_xent_rows_f64", "hnh_optim_step_f64"}
HOST_CALLS = ("hnh_gat_get_weight", "hnh_gat_get_attn_vectors", "hnh_gat_set_labels", "hnh_gat_loss", "hnh_gat_set_optimizer",
              "hnh_gat_optimizer_step", "hnh_gat_train_step", "hnh_gat_evaluate")


def xent_problem(heads, classes, rows=40, seed=0):
    rng = np.random.default_rng(seed + 10 * heads + classes)
    out = rng.uniform(-2, 3, (rows, heads * classes))
    labels = rng.integers(0, classes, rows)
    labels[::7] = -1
    mask = rng.random(rows) < 0.6
    return out, labels, mask


@pytest.mark.parametrize("heads,classes", [(3, 4), (1, 12), (8, 7), (1, 1), (2, 1)])
def test_loss_gradient_matches_finite_differences(heads, classes):
    """ "mean" is heads > 1, "concat" heads = 1.  The loss is smooth in `out`: no margin condition."""
    out, labels, mask = xent_problem(heads, classes)
    loss, acc, g = R.xent(out, labels, mask, heads)
    live = mask & (labels >= 0)
    assert 5 < np.count_nonzero(live) < len(live) and 0.0 <= acc <= 1.0
    assert np.all(g[~live] == 0.0) and (classes == 1 or np.all(g[live] != 0.0))
    step, worst = 1e-6, 0.0
    rng = np.random.default_rng(1)
    probes = [(int(r), int(c)) for r in np.flatnonzero(live)[:6] for c in rng.integers(0, heads * classes, 3)] + [(int(np.flatnonzero(~live)[0]), 0)]
    for idx in probes:
        plus, minus = out.copy(), out.copy()
        plus[idx] += step
        minus[idx] -= step
        fd = (R.xent(plus, labels, mask, heads)[0] - R.xent(minus, labels, mask, heads)[0]) / (2 * step)
        worst = max(worst, abs(fd - g[idx]))
    scale = max(np.abs(g).max(), 1e-300)
    print("observed heads=%d classes=%d: %.2e" % (heads, classes, worst / scale))
    assert classes == 1 or worst / scale <= 1e-6
    if classes == 1:
        assert loss == 0.0 and acc == 1.0 and np.all(g == 0.0), "one class: nothing to learn"
    # rows sum to zero over the classes of every head block, and the twin agrees
    assert np.abs(g.reshape(len(out), heads, classes).sum(axis=2)).max() <= 1e-16
    loss_ld, acc_ld, g_ld = R.xent_ld(out, labels, mask, heads)
    assert g_ld.dtype == np.longdouble and acc_ld == acc and abs(float(loss_ld) - loss) <= 1e-14 * max(1.0, abs(loss)) and T.rel(np.float64(g_ld), g) <= 1e-14


def test_loss_ties_extremes_and_masks():
    # ties go to the lowest index; the head mean of small integers is exact
    out = np.array([[1.0, 3.0, 3.0, 0.0] * 2, [2.0, 2.0, 2.0, 2.0] * 2, [0.0, 1.0, 5.0, 5.0] * 2])
    for labels, want in (([1, 0, 2], 3), ([2, 1, 3], 0)):
        assert R.xent_rows(out, np.array(labels), 2, 1.0)[1] == want
    # logits of +-700 neither overflow nor lose the small classes
    big = np.array([[700.0, -700.0, 699.0], [-700.0, -700.0, -700.0]])
    loss_sum, correct, g = R.xent_rows(big, np.array([2, 1]), 1, 0.5)
    assert np.isfinite(loss_sum) and np.all(np.isfinite(g)) and correct == 0
    assert abs(loss_sum - (1.0 + math.log1p(math.exp(-1.0)) + math.log(3.0))) <= 1e-12
    with pytest.raises(AssertionError):
        R.xent(big, np.array([-1, -1]), None, 1)  # no labelled row
    assert R.heads_of(T.GAT_LAYERS, "mean") == (3, 4) and R.heads_of(T.GAT_LAYERS, "concat") == (1, 12)


def scalar_adam(p, g, m, v, t, lr, beta1, beta2, eps, wd):
    p, m, v = p.copy(), m.copy(), v.copy()
    for i in np.ndindex(p.shape):
        gd = g[i] + wd * p[i]
        m[i] = beta1 * m[i] + (1.0 - beta1) * gd
        v[i] = beta2 * v[i] + (1.0 - beta2) * gd * gd
        mhat = m[i] / (1.0 - math.pow(beta1, t))
        vhat = v[i] / (1.0 - math.pow(beta2, t))
        p[i] = p[i] - lr * mhat / (math.sqrt(vhat) + eps)
    return p, m, v


def scalar_sgd(p, g, v, lr, momentum, wd):
    p, v = p.copy(), v.copy()
    for i in np.ndindex(p.shape):
        v[i] = momentum * v[i] + (g[i] + wd * p[i])
        p[i] = p[i] - lr * v[i]
    return p, v


def test_optimizers_against_scalar_loops():
    rng = np.random.default_rng(2)
    p0 = rng.standard_normal((5, 3))
    pa, ma, va = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    pb, mb, vb = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    ps, vs, pt, vt = p0.copy(), np.zeros_like(p0), p0.copy(), np.zeros_like(p0)
    for t in range(1, 6):
        g = rng.standard_normal(p0.shape) * 10.0 ** rng.integers(-9, 2)
        pa, ma, va = R.adam_step(pa, g, ma, va, t, 0.01, 0.9, 0.999, 1e-8, 5e-4)
        pb, mb, vb = scalar_adam(pb, g, mb, vb, t, 0.01, 0.9, 0.999, 1e-8, 5e-4)
        ps, vs = R.sgd_step(ps, g, vs, 0.05, 0.9, 5e-4)
        pt, vt = scalar_sgd(pt, g, vt, 0.05, 0.9, 5e-4)
        for a, b in ((pa, pb), (ma, mb), (va, vb), (ps, pt), (vs, vt)):
            assert T.rel(a, b) <= 1e-15, t
    assert np.abs(pa - p0).max() > 0.01 and np.abs(ps - p0).max() > 0.01
    # Adam's first step is lr * sign(g) wherever |g| >> eps
    p1, _, _ = R.adam_step(p0, np.full_like(p0, 3.0), np.zeros_like(p0), np.zeros_like(p0), 1, 0.01)
    assert np.allclose(p0 - p1, 0.01, rtol=1e-6)


def test_train_kernels_are_an_optional_group():
    names = declared("hnh_train.h")
    assert names == GROUP
    assert names == set(K.TRAIN_SIGNATURES), names ^ set(K.TRAIN_SIGNATURES)
    for header in ("hnh_kernels.h", "hnh_grad.h", "hnh_attention.h", "hnh_attn_grad.h", "hnh_attn_additive.h", "hnh_attn_dropout.h"):
        assert not names & declared(header), header
    for table in (K.SIGNATURES, K.GRAD_SIGNATURES, K.ATTN_SIGNATURES, K.ATTN_GRAD_SIGNATURES, K.ATTN_ADD_SIGNATURES, K.ATTN_DROP_SIGNATURES):
        assert not names & set(table), "disjoint from the six existing tables"
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.TRAIN_SIGNATURES[n][1]
    dbl = C.CDLL(T.ORACLE_BACKEND)
    for n in names:
        assert not hasattr(dbl, n), "the CPU test double does not export %s" % n
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works
    assert C.sizeof(K.OptimTensor) == 64 and C.sizeof(K.Optim) == 72
    txt = open(ROOT + "/include/hnh_train.h").read()
    assert re.search(r"#define HNH_XENT_MAX_WIDTH %d\b" % K.XENT_MAX_WIDTH, txt) and re.search(r"#define HNH_OPTIM_MAX_TENSORS %d\b" % K.OPTIM_MAX_TENSORS, txt)
    assert "ReLU" in txt and "average" in txt, "the header states the known deviation"


def test_host_calls_declared_and_exported():
    for n in HOST_CALLS:
        assert n in declared("hnh_dist.h") and n in H.SIGNATURES and hasattr(H.lib(), n), n
    for name in ("get_weight", "get_attention_vectors", "set_labels", "loss", "set_optimizer", "optimizer_step", "train_step", "evaluate"):
        assert callable(getattr(H.GAT, name))


def test_training_on_the_test_double():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")
    m = case["M"]
    rng = np.random.default_rng(0)
    labels = rng.integers(0, 4, m)
    mask = rng.random(m) < 0.3
    named = r"training needs the kernel (hnh_[a-z0-9_]+).*include/hnh_train\.h"

    def rank(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1)
        g = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.forwardPass()
        # nothing set yet: refused before the kernel group is looked at
        for call in (gnn.loss, gnn.train_step, gnn.evaluate):
            with pytest.raises(H.HnhError, match="set_labels"):
                call()
        # bad labels, an empty mask, wrong lengths: refused, and the object stays without labels
        bad = labels.copy()
        bad[np.flatnonzero(mask)[0]] = 4
        with pytest.raises(H.HnhError, match=r"label 4 of row \d+ is out of range: 4 classes"):
            gnn.set_labels(bad, mask, heads="mean")
        with pytest.raises(H.HnhError, match="no labelled row"):
            gnn.set_labels(labels, np.zeros(m, dtype=bool))
        with pytest.raises(H.HnhError, match="no labelled row"):
            gnn.set_labels(np.full(m, -1), None)
        with pytest.raises(H.HnhError, match="%d entries, not %d" % (m, m - 1)):
            gnn.set_labels(labels[:-1])
        with pytest.raises(ValueError):
            gnn.set_labels(labels, mask[:-1])
        with pytest.raises(ValueError):
            gnn.set_labels(labels, mask, heads="sum")
        with pytest.raises(H.HnhError, match="set_labels"):
            gnn.loss()
        gnn.set_labels(labels, mask, heads="mean")
        gnn.set_labels(labels + 8, mask, heads="concat")  # 12 classes
        gnn.set_labels(labels, mask)
        # labels but no optimizer: train_step and optimizer_step say so; loss names the missing kernel
        with pytest.raises(H.HnhError, match="set_optimizer"):
            gnn.train_step()
        with pytest.raises(H.HnhError, match="set_optimizer"):
            gnn.optimizer_step()
        for bad_opt in (dict(kind="adam", lr=-1.0), dict(kind="adam", lr=0.01, beta1=1.0), dict(kind="sgd", lr=0.01, momentum=1.5),
                        dict(kind="adam", lr=float("nan"))):
            with pytest.raises(H.HnhError, match="set_optimizer needs"):
                gnn.set_optimizer(**bad_opt)
        with pytest.raises(ValueError):
            gnn.set_optimizer("lion", 0.01)
        assert H.lib().hnh_gat_set_optimizer(gnn.h, 7, 0.01, 0.9, 0.999, 1e-8, 0.0, 0.0) != 0
        gnn.set_optimizer("adam", 0.01, weight_decay=5e-4)
        seen = set()
        for call in (gnn.loss, lambda: gnn.loss(~mask, g), gnn.train_step, gnn.evaluate, lambda: gnn.evaluate(~mask)):
            with pytest.raises(H.HnhError, match=named) as e:
                call()
            seen.add(re.search(named, str(e.value)).group(1))
        assert seen and seen <= GROUP
        with pytest.raises(H.HnhError, match="backwardPass since the last step|hnh_optim_step_f64"):
            gnn.optimizer_step()
        gnn.set_optimizer("sgd", 0.05, momentum=0.9)
        with pytest.raises(H.HnhError, match=named):
            gnn.train_step()
        # parameters can be read back, and the process and the operator live on: the plain GAT on the same object
        w00 = gnn.get_weight(0, 0)
        a1, a2 = gnn.get_attention_vectors(1, 2)
        assert w00.shape == gnn.weight_shape(0, 0) and np.all(a1 == 0.0) and np.all(a2 == 0.0)
        gnn.set_weight(0, 0, w00 + 1.0)
        assert np.array_equal(gnn.get_weight(0, 0), w00 + 1.0)
        gnn.set_weight(0, 0, w00)
        gnn.forwardPass()
        out = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.get_output(out)
        res = out.download()
        for h in (out, g, gnn, d, sp):
            h.free()
        return res

    per_rank, want = H.run_spmd(2, rank), H.run_spmd(2, lambda world: plain_output(world, case))
    assert all(np.isfinite(r).all() for r in per_rank) and all(np.array_equal(a, b) for a, b in zip(per_rank, want))


def test_the_reference_learns_the_planted_partition():
    """The conditions the GPU test asserts for the device, here for the reference: the final train loss is at most half the first, the
    held-out accuracy at least 0.8.  Observed: 1.378 -> 0.089, monotonically; held-out accuracy 0.964."""
    layers = T.GAT_LAYERS
    pp = R.planted_partition(layers)
    assert pp["m"] == 256 and len(pp["rows"]) == 256 * 13 and 50 < np.count_nonzero(pp["mask"]) < 110
    losses, accs, w, av = R.train(pp["rows"], pp["cols"], pp["m"], pp["x"], layers, T.GAT_ALPHA, pp["labels"], pp["mask"], "mean", pp["w"], pp["av"],
                                  R.LEARN_OPTIMIZER, R.LEARN_STEPS)
    held = R.evaluate(pp["rows"], pp["cols"], pp["m"], pp["x"], layers, T.GAT_ALPHA, pp["labels"], ~pp["mask"], "mean", w, av)
    print("observed: loss %.3f -> %.3f, held-out loss %.3f accuracy %.3f" % (losses[0], losses[-1], held[0], held[1]))
    assert losses[-1] <= 0.5 * losses[0] and held[1] >= 0.8
    assert losses[-1] <= 0.1 * losses[0] and held[1] >= 0.95, "the margin the generator was chosen for"


def test_reference_trajectory_is_stable_under_gradient_perturbations():
    """The measured tolerance of the GPU trajectories: gradients perturbed by 1e-10 * max|g| move the parameters after 10 steps by about
    1e-11 (SGD with momentum) and 1e-9 (Adam, whose first steps are ill-conditioned where |g| ~ eps)."""
    layers = T.GAT_LAYERS
    pp = R.planted_partition(layers)
    args = (pp["rows"], pp["cols"], pp["m"], pp["x"], layers, T.GAT_ALPHA, pp["labels"], pp["mask"], "mean", pp["w"], pp["av"])
    for opt, bound in ((dict(kind="sgd", lr=0.05, momentum=0.9), 1e-9), (dict(kind="adam", lr=0.01), 1e-6)):
        a = R.train(*args, opt, 10)
        b = R.train(*args, opt, 10, perturb=(1e-10, np.random.default_rng(7)))
        div = R.parameter_divergence(b[2], b[3], a[2], a[3])
        print("observed", opt["kind"], "%.2e" % div)
        assert 0.0 < div <= bound
    # dropout: step t uses seed0 + t, so two runs agree and another seed0 does not
    d1 = R.train(*args, dict(kind="sgd", lr=0.05), 3, rates=(0.6, 0.6), seed0=5)
    d2 = R.train(*args, dict(kind="sgd", lr=0.05), 3, rates=(0.6, 0.6), seed0=5)
    d3 = R.train(*args, dict(kind="sgd", lr=0.05), 3, rates=(0.6, 0.6), seed0=6)
    assert d1[0] == d2[0] and d1[0] != d3[0]
