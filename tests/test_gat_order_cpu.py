"""The GAT's backward pass, softmax attention, fused backward and training step on the CPU, under the stream-order checker.

The second CPU test double (oracle/liboracle_backend_gat.so, oracle/hnh_oracle_gat_groups.h) has the four optional kernel groups these
paths need, so GAT::backwardPass in both backward modes, the softmax pipeline (products and scores of head j + 1 on the auxiliary stream
beside the pass of head j), attn_walk over walk_merged and the training step run here with every call's exact bytes and a vector clock
per stream watched (oracle/hnh_stream_order.h): a missing event wait is a RACE, an operand that runs past the end of its block (a pitch
or a packed width one column short) a MISUSE.  On one GPU either shows by luck of timing, or not at all.

Every configuration: one forward + backward round on er8_r16 with T.GAT_LAYERS and hashed weights against the numpy definition
(tests/gat_ref.py) within gat_gpu_harness.TOL, the gradients replicated bit for bit on every rank, a second round of the same object
with the same bits, an empty checker report, and more than 500 accesses watched.  Where a mode does not support a grid the documented
refusal is asserted.  Training: three train_steps (cross-entropy head; SGD with momentum, Adam) against the trajectory of gat_ref within
the measured bound of tests/test_gat_train_gpu.py (ten times the divergence of a reference run whose gradients are perturbed by 1e-10).

Sensitivity (test_the_checker_sees_the_gat_protocol): with every event wait ignored by the checker during the GAT's own passes the same
runs are reported as racy.  Observed: the p = 1 softmax forward pass 1547 reports with one pass per chunk and 1547 with every query answering
"not yet", all between the aux and the compute stream; the p = 4 softmax fused round 4604 and 3076 reports, hnh_attn_softmax_csr_p and
hnh_attn_grad_{row,col}_csr_p among them (the first at line 60 of the 115 lines the 16 KiB report keeps).
Observed errors against the reference: at most 1.5e-15 (attention none) and 1.3e-15 (softmax) over every grid; trajectories at most 2.7e-15 in
the parameters (bounds 5.4e-11 with SGD, 2.9e-9 with Adam) and 8.0e-16 in the losses (bound 1.1e-12)."""
import ctypes
import os

import numpy as np
import pytest

import gat_gpu_harness as G  # (the functions only: its hip_backend / ctx fixtures are not imported)
import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import api as H
from oracle import oracle as O

TOL, ALPHA = G.TOL, G.ALPHA


@pytest.fixture(scope="module")
def checker():
    assert H.load_backend(T.ORACLE_GAT_BACKEND) == "oracle-cpu-test-double-gat"
    lib = ctypes.CDLL(T.ORACLE_GAT_BACKEND)
    lib.hnh_oracle_order_report.restype = ctypes.c_long
    lib.hnh_oracle_order_accesses.restype = ctypes.c_long
    lib.hnh_oracle_order_enable(1)

    class Checker:
        def drain(self):
            """(reports since the last drain, their text): races and MISUSE reports alike"""
            buf = ctypes.create_string_buffer(16384)
            n = lib.hnh_oracle_order_report(buf, 16384)
            return n, buf.value.decode()

        def accesses(self):
            return lib.hnh_oracle_order_accesses()
    c = Checker()
    before, text = c.drain()
    assert before == 0, "reports left behind by earlier tests of this process:\n" + text
    yield c
    H.load_backend(T.ORACLE_BACKEND)  # the modules after this one find the plain double, as before


@pytest.fixture(autouse=True)
def fresh_report(checker):
    """What a failed test left in the report stays that test's failure."""
    checker.drain()
    yield


def problem(attention):
    rows, cols, m, x = G.er8()
    layers = T.GAT_LAYERS
    w = G.hashed_weights(layers, 40.0 if attention == "none" else 1.0)  # (the softmax keeps the later layers' inputs of order one itself)
    g = O.dense_fill(m, layers[-1][1] * layers[-1][2], 9) * 16.0
    return rows, cols, m, x, layers, w, g


def two_rounds(checker, alg, p, c, attention, backward, label):
    """Two forward + backward rounds of one object on p loopback ranks: the reference, the replicated gradients, the same bits twice,
    an empty report, more than 500 accesses watched."""
    rows, cols, m, x, layers, w, g = problem(attention)
    before = checker.accesses()
    per_rank = H.run_spmd(p, lambda wd: G.run_rounds(wd, rows, cols, m, x, layers, w, None, g, rounds=2, alg=alg, c=c, attention=attention,
                                                     backward=backward))
    assert checker.drain() == (0, "")
    assert checker.accesses() - before > 500  # (the run was actually watched)
    got = G.assembled(per_rank, 0, m, layers)  # (asserts dW equal on every rank)
    G.compare(got, G.reference(rows, cols, m, x, layers, w, None, g, attention=attention), "gat_order_cpu", label, p, check=("out", "dw", "dx"))
    assert np.abs(got["dx"]).max() > 0
    G.assembled(per_rank, 1, m, layers)
    for pr in per_rank:
        a, b = pr["rounds"]
        assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["dx"], b["dx"]) and all(np.array_equal(a["dw"][k], b["dw"][k]) for k in w), \
            "a second round of the same object must give the same bits"


MODES = [(a, b) for a in ("none", "softmax") for b in ("unfused", "fused")]
MODE_IDS = ["%s-%s" % m for m in MODES]


@pytest.mark.parametrize("attention,backward", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("p", [1, 4, 8])
def test_fusion2_round_is_race_free(checker, p, attention, backward):
    """15d_fusion2, c = 1: every mode.  attn_walk over walk_merged (own block, then the landed chunks in windows), the head pipeline."""
    two_rounds(checker, "15d_fusion2", p, 1, attention, backward, "15d_fusion2 p%d %s %s" % (p, attention, backward))


@pytest.mark.parametrize("env", [{"HNH_RING_MODE": "relay"}, {"HNH_WINDOW_MERGE": "0"}, {"HNH_ORACLE_EVENTS_PENDING": "1"}],
                         ids=["relay-ring", "one-pass-per-chunk", "queries-answer-not-yet"])
@pytest.mark.parametrize("backward", ["unfused", "fused"])
def test_fusion2_softmax_variants_are_race_free(checker, monkeypatch, backward, env):
    """Softmax on p = 4 with the relay ring instead of the mesh fetch, with one windowed pass per chunk, and on the adaptive path with every
    completion query answering "not yet" (ordering rests on the event waits alone)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    two_rounds(checker, "15d_fusion2", 4, 1, "softmax", backward, "15d_fusion2 p4 softmax %s %s" % (backward, sorted(env.items())))


FUSION1_GRIDS = [(4, 1), (4, 2), (6, 2), (9, 3), (8, 2)]


@pytest.mark.parametrize("env", [{}, {"HNH_FUSION1_MESH": "0"}], ids=["mesh", "rings"])
@pytest.mark.parametrize("p,c", FUSION1_GRIDS)
def test_fusion1_unfused_round_is_race_free(checker, monkeypatch, p, c, env):
    """15d_fusion1 supports attention none with the un-fused backward pass at every c: seven operator calls per head, the weight-gradient
    contraction and its all-reduce, with the mesh reduce-scatter and with the accumulator rings."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    two_rounds(checker, "15d_fusion1", p, c, "none", "unfused", "15d_fusion1 p%d c%d %s" % (p, c, sorted(env.items())))


@pytest.mark.parametrize("p,c", FUSION1_GRIDS)
def test_unsupported_grids_refuse_and_leave_nothing_racing(checker, p, c):
    """Softmax attention and the fused backward pass belong to 15d_fusion2 with c = 1: elsewhere forwardPass / backwardPass refuse with
    the documented words, nothing is left in flight, and the operator lives on."""
    alg = "15d_fusion1"
    rows, cols, m, x, layers, w, g = problem("none")

    def rank(world):
        s = G.setup(world, rows, cols, m, x, layers, w, None, g, alg=alg, c=c, attention="softmax")
        gnn = s["gnn"]
        with pytest.raises(H.HnhError, match="softmax"):
            gnn.forwardPass()
        world.sync()
        gnn.set_attention("none")
        gnn.set_backward("fused")
        gnn.forwardPass()
        with pytest.raises(H.HnhError, match="fused backward.*15d_fusion1.*c = %d" % c):
            gnn.backwardPass(s["g"])
        world.sync()
        gnn.set_backward("unfused")
        gnn.backwardPass(s["g"])  # the operator lives on
        res = {k: gnn.weight_grad(*k) for k in w}
        G.teardown(s)
        return res

    per_rank = H.run_spmd(p, rank)
    assert all(np.array_equal(pr[k], per_rank[0][k]) and np.abs(pr[k]).max() > 0 for pr in per_rank for k in w)
    assert checker.drain() == (0, "")


def test_fusion2_with_replication_refuses(checker):
    rows, cols, m, x, layers, w, g = problem("none")

    def rank(world):
        s = G.setup(world, rows, cols, m, x, layers, w, None, g, alg="15d_fusion2", c=2, attention="softmax", backward="fused")
        with pytest.raises(H.HnhError, match="softmax"):
            s["gnn"].forwardPass()
        s["gnn"].set_attention("none")
        s["gnn"].forwardPass()
        with pytest.raises(H.HnhError, match="fused backward.*15d_fusion2.*c = 2"):
            s["gnn"].backwardPass(s["g"])
        world.sync()
        G.teardown(s)
        return True
    assert all(H.run_spmd(4, rank))
    assert checker.drain() == (0, "")


# ------------------------------------------------------------------------------------------------ training
OPTIMIZERS = {"sgd": dict(kind="sgd", lr=0.05, momentum=0.9, weight_decay=5e-4), "adam": dict(kind="adam", lr=0.01, weight_decay=5e-4)}
STEPS = 3


def reference_trajectory(pp, layers, optimizer, perturb=None):
    """STEPS steps of gat_ref (forward, xent, backward with attention softmax and the dot score; sgd_step / adam_step): (losses, accuracies,
    W).  perturb = (scale, rng) adds scale * max|g| * u to every gradient, as gat_ref.train does for its measured bound."""
    nh, _ = R.heads_of(layers, "mean")
    opt = dict(optimizer)
    kind, lr = opt.pop("kind"), opt.pop("lr")
    w = {k: v.copy() for k, v in pp["w"].items()}
    mom, var = {k: np.zeros_like(v) for k, v in w.items()}, {k: np.zeros_like(v) for k, v in w.items()}
    losses, accs = [], []
    for t in range(1, STEPS + 1):
        out = R.forward(pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, w, None, attention="softmax")
        loss, acc, g = R.xent(out, pp["labels"], pp["mask"], nh)
        losses.append(float(loss))
        accs.append(float(acc))
        dw, _, _ = R.backward(pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, g, w, None, attention="softmax")
        for k in w:
            gk = dw[k]
            if perturb is not None:
                gk = gk + perturb[0] * np.max(np.abs(gk)) * perturb[1].uniform(-1.0, 1.0, gk.shape)
            if kind == "adam":
                w[k], mom[k], var[k] = R.adam_step(w[k], gk, mom[k], var[k], t, lr, **opt)
            else:
                w[k], var[k] = R.sgd_step(w[k], gk, var[k], lr, **opt)
    return losses, accs, w


def device_train(world, pp, layers, optimizer, backward):
    s = G.setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["w"], None, None, attention="softmax", backward=backward)
    gnn = s["gnn"]
    gnn.set_labels(pp["labels"], pp["mask"], heads="mean")
    opt = dict(optimizer)
    gnn.set_optimizer(opt.pop("kind"), opt.pop("lr"), **opt)
    res = dict(losses=[], accs=[])
    for _ in range(STEPS):
        loss, acc = gnn.train_step()
        res["losses"].append(loss)
        res["accs"].append(acc)
    res["w"] = {k: gnn.get_weight(*k) for k in pp["w"]}
    G.teardown(s)
    return res


@pytest.mark.parametrize("backward", ["unfused", "fused"])
@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("p", [1, 4])
def test_training_steps_are_race_free(checker, p, kind, backward):
    """Three train_steps (forward, hnh_xent_rows_f64, backward, hnh_optim_step_f64 on the device; one host synchronisation per step) with
    softmax attention: the trajectory of gat_ref within the measured bound, parameters bit-equal across ranks, an empty report."""
    layers = T.GAT_LAYERS
    pp = R.planted_partition(layers)
    ref = reference_trajectory(pp, layers, OPTIMIZERS[kind])
    per = reference_trajectory(pp, layers, OPTIMIZERS[kind], perturb=(1e-10, np.random.default_rng(7)))
    div_p = max(float(np.max(np.abs(per[2][k] - ref[2][k])) / np.max(np.abs(ref[2][k]))) for k in ref[2])
    div_l = float(np.max(np.abs(np.array(per[0]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    assert div_p > 0 and div_l > 0
    before = checker.accesses()
    per_rank = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, OPTIMIZERS[kind], backward))
    assert checker.drain() == (0, "")
    assert checker.accesses() - before > 500
    r0 = per_rank[0]
    for pr in per_rank:
        assert pr["losses"] == r0["losses"] and pr["accs"] == r0["accs"]
        assert all(np.array_equal(pr["w"][k], r0["w"][k]) for k in r0["w"]), "parameters are bit-equal across ranks"
    got_p = max(float(np.max(np.abs(r0["w"][k] - ref[2][k])) / np.max(np.abs(ref[2][k]))) for k in ref[2])
    got_l = float(np.max(np.abs(np.array(r0["losses"]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    T.record_observed("gat_order_cpu_trajectory", case="%s %s" % (kind, backward), ranks=p, parameters=got_p, parameters_bound=10 * div_p, loss=got_l,
                      loss_bound=10 * div_l)
    print("observed trajectory", kind, backward, p, "parameters %.2e (bound %.2e) loss %.2e (bound %.2e)" % (got_p, 10 * div_p, got_l, 10 * div_l))
    assert got_p <= 10.0 * div_p and got_l <= 10.0 * div_l
    assert r0["accs"] == ref[1]
    assert all(np.abs(r0["w"][k] - pp["w"][k]).max() > 0 for k in pp["w"]), "every weight has moved"


# ------------------------------------------------------------------------------------------------ sensitivity
DROP = "HNH_ORDER_CHECK_DROP_WAITS"


def with_dropped_waits(world, body):
    """body() with every hnh_event_wait ignored by the checker, on every rank at once: the set-up before it keeps its waits, so the
    report (16 KiB of text) holds the races of the GAT's own passes and not thousands from the redistribution of the matrix."""
    world.sync()
    world.barrier()
    if world.rank == 0:
        os.environ[DROP] = "1"
    world.barrier()
    try:
        return body()
    finally:
        world.sync()
        world.barrier()
        if world.rank == 0:
            os.environ.pop(DROP, None)
        world.barrier()


def forward_only(world, rows, cols, m, x, layers, w):
    s = G.setup(world, rows, cols, m, x, layers, w, None, None, attention="softmax")

    def body():
        s["gnn"].forwardPass()
        s["gnn"].get_output(s["out"])
        return dict(subA=s["subA"], out=s["out"].download())
    res = with_dropped_waits(world, body)
    G.teardown(s)
    return res


def fused_round(world, rows, cols, m, x, layers, w, g):
    s = G.setup(world, rows, cols, m, x, layers, w, None, g, alg="15d_fusion2", c=1, attention="softmax", backward="fused")
    res = dict(subA=s["subA"], subB=s["subB"], rounds=[with_dropped_waits(world, lambda: G.one_round(s, w, False))])
    G.teardown(s)
    return res


@pytest.mark.parametrize("windows", ["one pass per chunk", "adaptive, every query answers not yet"])
def test_the_checker_sees_the_gat_protocol(checker, monkeypatch, windows):
    """So that silence above means something: with every hnh_event_wait ignored BY THE CHECKER (the double computes as ever) the p = 1
    softmax forward pass is racy between the auxiliary and the compute stream (ev_gemm / ev_head of the head pipeline), and the p = 4
    softmax fused round is racy at the attention entry points (the chunk-arrival waits of walk_merged).  In both variants of
    tests/test_stream_order_cpu.py: one windowed pass per chunk, and the adaptive path with every completion query answering "not yet".
    Observed counts: the module docstring.  Asserted: at least one report each, and the names."""
    if windows == "one pass per chunk":
        monkeypatch.setenv("HNH_WINDOW_MERGE", "0")
    else:
        monkeypatch.setenv("HNH_ORACLE_EVENTS_PENDING", "1")
    rows, cols, m, x, layers, w, g = problem("softmax")
    want = R.forward(rows, cols, m, x, layers, ALPHA, w, None, attention="softmax")
    try:
        per_rank = H.run_spmd(1, lambda wd: forward_only(wd, rows, cols, m, x, layers, w))
        n1, text1 = checker.drain()
        assert T.rel(T.assemble_dense(per_rank, "out", "subA", m, want.shape[1]), want) <= TOL  # (the arithmetic does not depend on the checker)
        per_rank = H.run_spmd(4, lambda wd: fused_round(wd, rows, cols, m, x, layers, w, g))
        n4, text4 = checker.drain()
    finally:
        os.environ.pop(DROP, None)
    G.compare(G.assembled(per_rank, 0, m, layers), G.reference(rows, cols, m, x, layers, w, None, g, attention="softmax"), "gat_order_cpu",
              "dropped waits " + windows, 4, check=("out", "dw", "dx"))
    print("observed reports with the waits dropped (%s): p = 1 forward %d, p = 4 fused round %d" % (windows, n1, n4))
    assert n1 >= 1 and " aux)" in text1, (n1, text1[:2000])
    assert n4 >= 1 and ("hnh_attn_grad_" in text4 or "hnh_attn_softmax_csr_p" in text4), (n4, text4[:2000])
    assert checker.drain()[0] == 0
