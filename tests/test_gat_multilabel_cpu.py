"""The GAT's multi-label head without a GPU (GAT.set_multilabel_targets, include/hnh_train_multilabel.h; tests/gat_multilabel_ref.py is the
definition): the reference's gradient against central finite differences; loss and gradient at logits of +-700 against np.longdouble, with
and without pos_weight; all-ones weights equal to no weights bit for bit; the bit packing round trip; micro-F1 against a scalar loop; the
optional kernel group (declared == bound == exported by the HIP library with those argtypes, disjoint from every other header and table,
absent from the CPU test double); the host calls; on the test double with 2 loopback ranks every refusal of set_multilabel_targets, then
loss / train_step / evaluate name the missing kernel and the new header, and the same object then runs the plain GAT bit for bit; and the
learning problem of the GPU test meets its conditions on the reference.

Observed here: gradient against finite differences <= 8e-9 of its largest entry (bound 1e-6, the bound of the other finite-difference
tests); float64 against longdouble at +-700 within 2e-16."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gat_multilabel_ref as M
import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared, make_gat, plain_output

GROUP = {"hnh_bce_rows_f64_workspace", "hnh_bce_rows_f64"}
HOST_CALLS = ("hnh_gat_set_multilabel_targets", "hnh_gat_multilabel_counts")


def problem(heads, classes, rows=24, seed=0):
    rng = np.random.default_rng(seed + 10 * heads + classes)
    out = rng.uniform(-3, 3, (rows, heads * classes))
    targets = rng.random((rows, classes)) < 0.4
    mask = rng.random(rows) < 0.6
    return out, targets, mask, rng.uniform(0.0, 3.0, classes)


@pytest.mark.parametrize("heads,classes", [(1, 1), (2, 1), (3, 4), (1, 33), (6, 121)])
@pytest.mark.parametrize("weighted", [False, True])
def test_gradient_matches_finite_differences(heads, classes, weighted):
    out, targets, mask, pw = problem(heads, classes)
    pw = pw if weighted else None
    loss, f1, g, counts = M.bce(out, targets, mask, heads, pw)
    assert 5 < np.count_nonzero(mask) < len(mask) and 0.0 <= f1 <= 1.0 and sum(counts) <= np.count_nonzero(mask) * classes
    assert np.all(g[~mask] == 0.0) and np.all(g[mask] != 0.0)
    step, worst = 1e-4, 0.0  # (the loss is smooth: the truncation error is of order step^2, the rounding error of order 1e-16 / step)
    rng = np.random.default_rng(1)
    probes = [(int(r), int(c)) for r in np.flatnonzero(mask)[:6] for c in rng.integers(0, heads * classes, 3)] + [(int(np.flatnonzero(~mask)[0]), 0)]
    for idx in probes:
        plus, minus = out.copy(), out.copy()
        plus[idx] += step
        minus[idx] -= step
        fd = (M.bce(plus, targets, mask, heads, pw)[0] - M.bce(minus, targets, mask, heads, pw)[0]) / (2 * step)
        worst = max(worst, abs(fd - g[idx]))
    print("observed heads=%d classes=%d weighted=%s: %.2e" % (heads, classes, weighted, worst / np.abs(g).max()))
    assert worst / np.abs(g).max() <= 1e-6
    # every head block carries the same gradient, and the loss is torch's BCEWithLogitsLoss(pos_weight), mean reduction, restated
    assert all(np.array_equal(g[:, :classes], g[:, h * classes:(h + 1) * classes]) for h in range(heads))
    z = out.reshape(len(out), heads, classes).mean(axis=1)[mask]
    y, w = targets[mask].astype(float), (np.ones(classes) if pw is None else pw)
    sig = 1.0 / (1.0 + np.exp(-z))
    assert abs(loss - np.mean(-w * y * np.log(sig) - (1 - y) * np.log(1 - sig))) <= 1e-13 * loss


@pytest.mark.parametrize("weighted", [False, True])
def test_extreme_logits_against_longdouble(weighted):
    """Logits of +-700 (exp(700) overflows nothing here, exp(-700) is 1e-304): loss and gradient stay finite and agree with the twin."""
    rng = np.random.default_rng(3)
    heads, classes, rows = 2, 5, 12
    out = np.where(rng.random((rows, heads * classes)) < 0.5, 700.0, -700.0) + rng.uniform(-1, 1, (rows, heads * classes))
    out[0] = 700.0
    out[1] = -700.0
    out[2] = np.tile([700.0, -700.0, 0.0, 1e-300, -1e-300], heads)
    targets = rng.random((rows, classes)) < 0.5
    targets[0], targets[1] = [1, 0, 1, 0, 1], [1, 0, 1, 0, 1]
    pw = rng.uniform(0.0, 4.0, classes) if weighted else None
    got = M.bce_rows(out, targets, None, heads, 0.01, pw)
    want = M.bce_rows(out, targets, None, heads, 0.01, pw, np.longdouble)
    assert want[4].dtype == np.longdouble and np.isfinite(got[0]) and np.all(np.isfinite(got[4])) and got[0] > 700.0
    assert got[1:4] == want[1:4]
    errs = abs(got[0] - float(want[0])) / float(want[0]), T.rel(got[4], np.float64(want[4]))
    print("observed weighted=%s: loss %.2e g %.2e" % (weighted, errs[0], errs[1]))
    assert max(errs) <= 1e-14
    # a confident right answer costs nothing, a confident wrong one |z| w; z == 0 predicts "absent"
    one = M.bce_rows(np.array([[700.0, -700.0, 0.0]]), np.array([[1, 0, 1]]), None, 1, 1.0)
    assert abs(one[0] - np.log(2.0)) <= 1e-15 and one[1:4] == (1, 0, 1)
    wrong = M.bce_rows(np.array([[700.0, -700.0]]), np.array([[0, 1]]), None, 1, 1.0, np.array([1.0, 2.5]))
    assert wrong[0] == 700.0 + 2.5 * 700.0 and wrong[1:4] == (0, 1, 1) and np.allclose(wrong[4], [[1.0, -2.5]], rtol=1e-15)


def test_all_ones_weights_equal_no_weights_bit_for_bit():
    for heads, classes in ((1, 1), (3, 4), (6, 121)):
        out, targets, mask, _ = problem(heads, classes, seed=4)
        out[::5] *= 200.0
        a = M.bce_rows(out, targets, mask, heads, 1.0 / 77.0, None)
        b = M.bce_rows(out, targets, mask, heads, 1.0 / 77.0, np.ones(classes))
        assert a[:4] == b[:4] and np.array_equal(a[4], b[4])


@pytest.mark.parametrize("classes", [31, 32, 33, 64, 65])
def test_bit_packing_round_trip(classes):
    rng = np.random.default_rng(classes)
    t = rng.random((19, classes)) < 0.5
    t[0], t[1] = True, False
    words = (classes + 31) // 32
    plain = M.pack_bits(t)
    assert plain.dtype == np.uint32 and plain.shape == (19, words) and np.array_equal(M.unpack_bits(plain, classes), t)
    for r, c in ((0, 0), (5, classes - 1), (7, classes // 2)):  # bit (c % 32) of word c / 32, against a scalar restatement
        assert bool((int(plain[r, c // 32]) >> (c % 32)) & 1) == bool(t[r, c])
    assert int(plain[0, -1]) == (1 << ((classes - 1) % 32 + 1)) - 1 and not plain[1].any(), "nothing beyond the classes is set"
    wide = M.pack_bits(t, words + 2, garbage=rng)
    assert wide.shape == (19, words + 2) and np.array_equal(M.unpack_bits(wide, classes), t)
    assert classes % 32 == 0 or np.any(wide[:, words - 1] >> np.uint32(classes % 32)), "the unused bits of the last word hold garbage"


def test_micro_f1_against_a_scalar_loop():
    rng = np.random.default_rng(6)
    out = rng.uniform(-2, 2, (30, 7))
    out[3, 2] = 0.0
    targets = rng.random((30, 7)) < 0.3
    mask = rng.random(30) < 0.7
    tp = fp = fn = 0
    for r in range(30):
        for c in range(7):
            if mask[r]:
                pred = out[r, c] > 0.0
                tp += int(pred and targets[r, c])
                fp += int(pred and not targets[r, c])
                fn += int(not pred and targets[r, c])
    loss, f1, _, counts = M.bce(out, targets, mask, 1)
    assert counts == (tp, fp, fn) and tp > 0 and fp > 0 and fn > 0
    assert f1 == 2.0 * tp / (2 * tp + fp + fn) == M.micro_f1(tp, fp, fn)
    assert abs(f1 - 2.0 / (1.0 / (tp / (tp + fp)) + 1.0 / (tp / (tp + fn)))) <= 1e-15, "the harmonic mean of micro precision and recall"
    # nothing predicted and nothing present: 0.0, not a division by zero
    none = M.bce(-np.ones((4, 3)), np.zeros((4, 3), dtype=bool), None, 1)
    assert none[1] == 0.0 and none[3] == (0, 0, 0) and M.micro_f1(0, 0, 0) == 0.0
    assert M.micro_f1(5, 0, 0) == 1.0 and M.micro_f1(0, 3, 0) == 0.0


def test_multilabel_kernels_are_an_optional_group():
    names = declared("hnh_train_multilabel.h")
    assert names == GROUP
    assert names == set(K.MULTILABEL_SIGNATURES), names ^ set(K.MULTILABEL_SIGNATURES)
    headers = [h for h in os.listdir(os.path.join(ROOT, "include")) if h.endswith(".h") and h != "hnh_train_multilabel.h"]
    assert "hnh_train.h" in headers and "hnh_kernels.h" in headers and len(headers) >= 15
    for header in headers:
        assert not names & declared(header), header
    tables = [n for n in dir(K) if n.endswith("SIGNATURES") and n != "MULTILABEL_SIGNATURES"]
    assert "TRAIN_SIGNATURES" in tables and "SIGNATURES" in tables and len(tables) >= 15
    for table in tables:
        assert not names & set(getattr(K, table)), table
    assert not names & set(H.SIGNATURES)
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.MULTILABEL_SIGNATURES[n][1] and getattr(lib, n).restype == K.MULTILABEL_SIGNATURES[n][0]
    dbl = C.CDLL(T.ORACLE_BACKEND)
    for n in names:
        assert not hasattr(dbl, n), "the CPU test double does not export %s" % n
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works
    assert declared("hnh_train.h") == set(K.TRAIN_SIGNATURES), "hnh_train.h is as it was"


def test_host_calls_declared_and_exported():
    for n in HOST_CALLS:
        assert n in declared("hnh_dist.h") and n in H.SIGNATURES and hasattr(H.lib(), n), n
    for name in ("set_multilabel_targets", "multilabel_counts"):
        assert callable(getattr(H.GAT, name))
    assert H.GAT.HEADS == {"mean": 0, "concat": 1}
    for name in ("loss", "train_step", "evaluate"):
        assert "micro-F1" in getattr(H.GAT, name).__doc__ and "accuracy" in getattr(H.GAT, name).__doc__


def test_multilabel_on_the_test_double():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")
    m = case["M"]
    rng = np.random.default_rng(0)
    targets = rng.random((m, 4)) < 0.4
    wide = rng.random((m, 12)) < 0.4
    mask = rng.random(m) < 0.3
    labels = rng.integers(0, 4, m)
    named = r"training needs the kernel (hnh_bce_[a-z0-9_]+).*include/hnh_train_multilabel\.h"

    two = np.ascontiguousarray(targets, dtype=np.uint8)
    two[5, 3] = 2

    def raw_targets(gnn, t):  # (the host layer's own check of the bytes, past the Python layer's)
        H._check(H.lib().hnh_gat_set_multilabel_targets(gnn.h, t.ctypes.data, t.size, t.shape[1], None, 0, 0, None), "gat_set_multilabel_targets")

    def rank(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1)
        g = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.forwardPass()
        refused = [
            # a target value other than 0 and 1, named with its row and class
            (ValueError, r"target 2 of row 5, class 3 is neither 0 nor 1", lambda: gnn.set_multilabel_targets(np.where((np.arange(m)[:, None] == 5) & (np.arange(4) == 3), 2, targets), mask)),
            (ValueError, r"target 0.5 of row 7, class 0 is neither 0 nor 1", lambda: gnn.set_multilabel_targets(np.where((np.arange(m)[:, None] == 7) & (np.arange(4) == 0), 0.5, targets), mask)),
            (H.HnhError, r"target 2 of row 5, class 3 is neither 0 nor 1", lambda: raw_targets(gnn, two)),
            # wrong lengths: rows of the targets, of the mask, of pos_weight; a wrong shape
            (H.HnhError, r"needs %d x 4 = %d targets, not %d" % (m, 4 * m, 4 * (m - 1)), lambda: gnn.set_multilabel_targets(targets[:-1])),
            (ValueError, "differ in length", lambda: gnn.set_multilabel_targets(targets, mask[:-1])),
            (ValueError, "one entry per class", lambda: gnn.set_multilabel_targets(targets, mask, pos_weight=np.ones(5))),
            (ValueError, "two-dimensional", lambda: gnn.set_multilabel_targets(targets[:, 0])),
            (ValueError, "heads must be one of", lambda: gnn.set_multilabel_targets(targets, mask, heads="sum")),
            # a mask that selects no row
            (H.HnhError, "mask selects no row", lambda: gnn.set_multilabel_targets(targets, np.zeros(m, dtype=bool))),
            # a class count that does not match the heads mode
            (H.HnhError, r"12 classes, but heads mode 0 of the last layer gives 4", lambda: gnn.set_multilabel_targets(wide, mask, heads="mean")),
            (H.HnhError, r"4 classes, but heads mode 1 of the last layer gives 12", lambda: gnn.set_multilabel_targets(targets, mask, heads="concat")),
            # a pos_weight that is negative or not finite
            (H.HnhError, r"pos_weight -1.0+ of class 2 is negative or not finite", lambda: gnn.set_multilabel_targets(targets, mask, pos_weight=[1, 1, -1, 1])),
            (H.HnhError, r"pos_weight .* of class 0 is negative or not finite", lambda: gnn.set_multilabel_targets(targets, mask, pos_weight=[np.inf, 1, 1, 1])),
            (H.HnhError, r"pos_weight .* of class 3 is negative or not finite", lambda: gnn.set_multilabel_targets(targets, mask, pos_weight=[1, 1, 1, np.nan])),
        ]
        for exc, match, call in refused:
            with pytest.raises(exc, match=match):
                call()
            # a refused call leaves the object as it was: still without a head
            with pytest.raises(H.HnhError, match="set_labels"):
                gnn.loss()
            with pytest.raises(H.HnhError, match="set_multilabel_targets first"):
                gnn.multilabel_counts()
        assert H.lib().hnh_gat_set_multilabel_targets(gnn.h, None, 4 * m, 4, None, 0, 0, None) != 0
        assert H.lib().hnh_gat_set_multilabel_targets(gnn.h, np.zeros(4 * m, dtype=np.uint8).ctypes.data, 4 * m, 4, np.ones(m, dtype=np.uint8).ctypes.data, m - 1, 0, None) != 0
        assert H.lib().hnh_gat_set_multilabel_targets(gnn.h, np.zeros(4 * m, dtype=np.uint8).ctypes.data, 4 * m, 4, None, 0, 7, None) != 0
        # accepted: bool and 0/1 integers, with and without mask and weights, both heads modes
        gnn.set_multilabel_targets(wide, mask, heads="concat", pos_weight=np.linspace(0.0, 3.0, 12))
        gnn.set_multilabel_targets(targets.astype(np.int64))
        gnn.set_multilabel_targets(targets, mask, pos_weight=[0.5, 1, 2, 0])
        assert gnn.multilabel_counts() == (0, 0, 0)
        # a refusal now leaves the sigmoid head in place
        with pytest.raises(H.HnhError, match="mask selects no row"):
            gnn.set_multilabel_targets(targets, np.zeros(m, dtype=bool))
        # the head is set but no optimizer: train_step says so; loss and evaluate name the missing kernel and the new header
        with pytest.raises(H.HnhError, match="set_optimizer"):
            gnn.train_step()
        gnn.set_optimizer("adam", 0.01, weight_decay=5e-4)
        seen = set()
        for call in (gnn.loss, lambda: gnn.loss(~mask, g), gnn.train_step, gnn.evaluate, lambda: gnn.evaluate(~mask)):
            with pytest.raises(H.HnhError, match=named) as e:
                call()
            seen.add(re.search(named, str(e.value)).group(1))
        assert seen and seen <= GROUP
        # set_labels switches back: the softmax head's group is named again; and forth
        gnn.set_labels(labels, mask)
        with pytest.raises(H.HnhError, match=r"training needs the kernel hnh_xent_[a-z0-9_]+.*include/hnh_train\.h"):
            gnn.loss()
        with pytest.raises(H.HnhError, match="set_multilabel_targets first"):
            gnn.multilabel_counts()
        with pytest.raises(H.HnhError, match="neither 0 nor 1"):
            raw_targets(gnn, two)
        with pytest.raises(H.HnhError, match=r"hnh_xent_"):
            gnn.evaluate()  # (the refused call left the softmax head in place)
        gnn.set_multilabel_targets(targets, mask)
        with pytest.raises(H.HnhError, match=named):
            gnn.train_step()
        # the process and the operator live on: the plain GAT on the same object
        gnn.forwardPass()
        out = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.get_output(out)
        res = out.download()
        for h in (out, g, gnn, d, sp):
            h.free()
        return res

    per_rank, want = H.run_spmd(2, rank), H.run_spmd(2, lambda world: plain_output(world, case))
    assert all(np.isfinite(r).all() for r in per_rank) and all(np.array_equal(a, b) for a, b in zip(per_rank, want))


def test_the_reference_learns_the_planted_tags():
    """The conditions the GPU test asserts for the device, here for the reference: the final train loss is at most half the first, the
    held-out micro-F1 at least M.HELD_OUT_F1 = 0.70.  Observed: loss 0.746 -> 0.247; held-out micro-F1 0.751 (0.751 - 0.05 = 0.701, rounded
    down to a multiple of 0.05: 0.70)."""
    layers = T.GAT_LAYERS
    pp = M.planted_tags(layers)
    per_vertex = pp["targets"].sum(axis=1)
    assert pp["m"] == 256 and pp["targets"].shape == (256, 4) and len(pp["rows"]) == 256 * 13 and 100 < np.count_nonzero(pp["mask"]) < 156
    assert np.count_nonzero(per_vertex >= 2) > 64 and np.count_nonzero(per_vertex == 0) > 10, "several tags per vertex, and vertices without any"
    losses, f1s, w, av = M.train(pp["rows"], pp["cols"], pp["m"], pp["x"], layers, T.GAT_ALPHA, pp["targets"], pp["mask"], "mean", pp["w"], pp["av"],
                                 M.LEARN_OPTIMIZER, M.LEARN_STEPS)
    held = M.evaluate(pp["rows"], pp["cols"], pp["m"], pp["x"], layers, T.GAT_ALPHA, pp["targets"], ~pp["mask"], "mean", w, av)
    print("observed: loss %.3f -> %.3f, micro-F1 %.3f -> %.3f, held-out loss %.3f micro-F1 %.3f" % (losses[0], losses[-1], f1s[0], f1s[-1], held[0], held[1]))
    assert losses[-1] <= 0.5 * losses[0] and held[1] >= M.HELD_OUT_F1
