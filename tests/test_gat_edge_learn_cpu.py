"""The learned per-edge bias of the GAT's score "transformer" without a GPU (include/hnh_attn_edge_grad.h, GAT.set_edge_bias_learned): the
pass twins of tests/gat_edge_learn_ref.py (the grad entry points as numpy, one head overwriting and the next accumulating) against the
dL/db_e of gat_edge_ref.backward, which that module's own test checks against finite differences; the optional kernel group (declared ==
bound == exported by the HIP library, disjoint from every other header and table, absent from the CPU test double); the C ABI; on the test
double every refusal by name (learned without a bias, the missing group, the getters before a backward pass, clearing the bias clears the
switch), with the plain GAT on the same object bit-equal afterwards to one that never heard of it; the model's loss falls when the bias
alone is trained; and entries at -1e300 stay -1e300 to the bit under Adam and SGD with weight decay on the other tensors.

Bounds: the passes against the definition 1e-11 (T.TOL, the by_passes convention of test_gat_edge_cpu.py)."""
import ctypes as C
import re

import numpy as np
import pytest

import gat_edge_learn_ref as L
import gat_edge_ref as E
import gat_qkv_ref as Q
import gat_ref as R
import hnh_testlib as T
import test_gat_edge_cpu as EC
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared, make_gat, plain_output

GROUP = {"hnh_attn_qkv_bias_grad_row_csr_p", "hnh_attn_qkv_bias_grad_col_csr_p"}
LAYERS = T.GAT_LAYERS
OFF = -1e300


@pytest.mark.parametrize("config", ["relu", "published"])
def test_pass_twins_equal_the_definition(config):
    mode = EC.CONFIGS[config]
    rows, cols, m, x, w, wq, wk, eb, g = EC.fd_inputs(mode)
    want = E.backward(rows, cols, m, x, LAYERS, g, w, wq, wk, edge_bias=eb, **mode)[6]
    got = L.bias_grad_by_passes(rows, cols, m, x, LAYERS, g, w, wq, wk, edge_bias=eb, **mode)
    assert got.keys() == want.keys() == set(range(len(LAYERS)))
    worst = 0.0
    for li in want:
        assert np.abs(want[li]).max() > 0
        for which in (0, 1):
            worst = max(worst, T.rel(got[li][which], want[li]))
    T.record_observed("gat_edge_learn_passes", case=config, worst=worst)
    assert worst <= T.TOL, worst


def test_pass_twins_overwrite_and_accumulate():
    """dbias=None overwrites, dbias=v returns v + the head's value; the other results are gat_edge_ref's, to the bit"""
    rows, cols, m, x, w, wq, wk, eb, g = EC.fd_inputs(EC.CONFIGS["relu"])
    f = LAYERS[0][1]
    sc = Q.scale_of(f)
    qm, km, vm = x @ wq[(0, 0)], x @ wk[(0, 0)], x @ w[(0, 0)]
    rng = np.random.default_rng(1)
    dz, delta = rng.uniform(-1, 1, (m, f)), rng.uniform(-1, 1, m)
    kv = np.nan_to_num(Q.P.fused_pack(km, vm))
    _, lse, _, p = E.fwd_pass(rows, cols, m, qm, kv, f, sc, eb[0])
    pre = rng.uniform(-1, 1, len(rows))
    dq, db = L.row_pass(rows, cols, m, qm, dz, lse, delta, kv, f, sc, eb[0])
    dq2, db2 = L.row_pass(rows, cols, m, qm, dz, lse, delta, kv, f, sc, eb[0], dbias=pre)
    assert np.array_equal(dq, E.row_pass(rows, cols, m, qm, dz, lse, delta, kv, f, sc, eb[0])) and np.array_equal(dq, dq2)
    assert np.array_equal(db2, pre + db)
    assert T.rel(db, p * (np.einsum("ij,ij->i", dz[rows], vm[cols]) - delta[rows])) <= 1e-13
    packed = Q.P.fused_pack(qm, dz, lse, delta)
    dk, dv, dbc = L.col_pass(cols, rows, m, km, vm, packed, f, sc, eb[0])
    dk2, dv2, dbc2 = L.col_pass(cols, rows, m, km, vm, packed, f, sc, eb[0], dbias=pre)
    want = E.col_pass(cols, rows, m, km, vm, packed, f, sc, eb[0])
    assert np.array_equal(dk, want[0]) and np.array_equal(dv, want[1]) and np.array_equal(dk, dk2) and np.array_equal(dv, dv2)
    assert np.array_equal(dbc2, pre + dbc) and T.rel(dbc, db) <= 1e-13, "the column pass computes the same expression"


def test_edge_grad_kernels_are_an_optional_group():
    names = declared("hnh_attn_edge_grad.h")
    assert names == GROUP
    assert names == set(K.EDGE_GRAD_SIGNATURES), names ^ set(K.EDGE_GRAD_SIGNATURES)
    for header in ("hnh_kernels.h", "hnh_grad.h", "hnh_attention.h", "hnh_attn_grad.h", "hnh_attn_additive.h", "hnh_attn_dropout.h", "hnh_train.h",
                   "hnh_attn_v2.h", "hnh_attn_coef.h", "hnh_gat_skip.h", "hnh_attn_qkv.h", "hnh_attn_edge.h"):
        assert not names & declared(header), header
    for table in (K.SIGNATURES, K.AIDS_SIGNATURES, K.GRAD_SIGNATURES, K.ATTN_SIGNATURES, K.ATTN_GRAD_SIGNATURES, K.ATTN_ADD_SIGNATURES,
                  K.ATTN_DROP_SIGNATURES, K.TRAIN_SIGNATURES, K.V2_SIGNATURES, K.ATTN_COEF_SIGNATURES, K.SKIP_SIGNATURES, K.QKV_SIGNATURES,
                  K.EDGE_SIGNATURES):
        assert not names & set(table), "disjoint from the existing tables"
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.EDGE_GRAD_SIGNATURES[n][1]
        parent = K.EDGE_SIGNATURES[n.replace("_grad", "")][1]
        assert K.EDGE_GRAD_SIGNATURES[n][1] == parent[:4] + [C.c_void_p, C.c_int32] + parent[4:], "the parent's arguments plus dbias and accumulate"
    dbl = C.CDLL(T.ORACLE_BACKEND)
    for n in names:
        assert not hasattr(dbl, n), "the CPU test double does not export %s" % n
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works
    assert C.sizeof(K.AttnQKV) == 168, "struct hnh_attn_qkv is unchanged"
    txt = open(ROOT + "/include/hnh_attn_edge_grad.h").read()
    assert "168 bytes" in txt and "no atomics" in txt and "accumulate" in txt
    assert "hnh_attn_edge_grad.h" in open(ROOT + "/include/hnh_attn_edge.h").read(), "the bias's header points at its gradient's"


def test_host_wiring():
    txt = open(ROOT + "/include/hnh_dist.h").read()
    assert re.search(r"int hnh_gat_set_edge_bias_learned\(hnh_gat\* g, int layer, int on\);", txt)
    assert re.search(r"int hnh_gat_get_edge_bias\(hnh_gat\* g, int layer, int which, hnh_vec\* out\);", txt)
    assert re.search(r"int hnh_gat_get_edge_bias_grad\(hnh_gat\* g, int layer, int which, hnh_vec\* out\);", txt)
    assert H.SIGNATURES["hnh_gat_set_edge_bias_learned"] == (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32])
    for n in ("hnh_gat_get_edge_bias", "hnh_gat_get_edge_bias_grad"):
        assert H.SIGNATURES[n] == (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p])
    assert all(hasattr(H.GAT, n) for n in ("set_edge_bias_learned", "get_edge_bias", "edge_bias_grad"))
    gat = open(ROOT + "/distributed_sddmm_amd/csrc/host/gat.hpp").read()
    assert "THE BIAS IS NEVER DECAYED" in gat and "PARAM_EDGE_BIAS_S" in gat and "PARAM_EDGE_BIAS_ST" in gat


def on_the_double(spoil, ranks=1, bias=True):
    """A transformer GAT on the test double, with an edge bias on layer 0 when `bias`; spoil(gnn, d, world) holds the refusals; then bias
    and switch are cleared and the plain GAT on the same object is bit-equal to an object that never heard of either."""
    case = T.case_inputs("er8_r16")

    def rank(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, attention="softmax", score="transformer")
        if bias:
            gnn.edge_bias_from(lambda r, c: E.hash_bias(r, c), layer=0)
        spoil(gnn, d, world)
        gnn.set_edge_bias(0, None, None)
        gnn.set_score("dot")
        gnn.set_attention("none")
        gnn.forwardPass()
        out = H.Dense.create(world, *gnn.buffer_shape(len(LAYERS)))
        gnn.get_output(out)
        res = out.download()
        for h in (out, gnn, d, sp):
            h.free()
        return res

    got = H.run_spmd(ranks, rank)
    want = H.run_spmd(ranks, lambda world: plain_output(world, case))
    assert all(np.isfinite(a).all() and np.array_equal(a, b) for a, b in zip(got, want))


def test_learned_without_a_bias_is_refused_by_name():
    H.load_backend(T.ORACLE_BACKEND)

    def spoil(gnn, d, world):
        for layer in (0, 1):
            with pytest.raises(H.HnhError, match=r"set_edge_bias_learned: layer %d has no edge bias to learn" % layer):
                gnn.set_edge_bias_learned(layer)
        gnn.set_edge_bias_learned(0, False)  # switching off what is off is allowed
        with pytest.raises(H.HnhError, match="layer index 2 out of range"):
            gnn.set_edge_bias_learned(len(LAYERS))
        with pytest.raises(H.HnhError, match="get_edge_bias: layer 0 has no edge bias"):
            gnn.get_edge_bias(0)
        with pytest.raises(H.HnhError, match=r"score transformer.*hnh_attn_qkv_fwd_csr_p"):
            gnn.forwardPass()  # nothing was set: the plain score's own refusal on the test double

    on_the_double(spoil, bias=False)


def test_a_learned_bias_on_the_test_double_names_the_missing_group():
    H.load_backend(T.ORACLE_BACKEND)

    def spoil(gnn, d, world):
        gnn.set_edge_bias_learned(0)
        g = H.Dense.create(world, *gnn.buffer_shape(len(LAYERS)))
        with pytest.raises(H.HnhError, match=r"learned edge bias needs the kernel hnh_attn_qkv_bias_grad_row_csr_p.*include/hnh_attn_edge_grad\.h"):
            gnn.backwardPass(g)
        with pytest.raises(H.HnhError, match=r"edge bias.*hnh_attn_qkv_bias_fwd_csr_p.*include/hnh_attn_edge\.h"):
            gnn.forwardPass()  # a forward pass needs the bias's own group alone
        gnn.set_edge_bias_learned(0, False)
        with pytest.raises(H.HnhError, match=r"edge bias.*hnh_attn_qkv_bias_fwd_csr_p.*include/hnh_attn_edge\.h"):
            gnn.backwardPass(g)  # ... and so does the backward pass of a bias that is not learned
        g.free()

    on_the_double(spoil, ranks=2)


def test_the_getters_before_a_backward_pass():
    H.load_backend(T.ORACLE_BACKEND)

    def spoil(gnn, d, world):
        rows, cols = d.S_coordinates()
        trows, tcols = d.ST_coordinates()
        s, st = gnn.get_edge_bias(0)  # the bias as it stands: what edge_bias_from set, in both orders
        assert np.array_equal(s, E.hash_bias(rows, cols)) and np.array_equal(st, E.hash_bias(tcols, trows))
        words = r"no GAT edge-bias gradient of layer 0 yet: call backwardPass with set_edge_bias_learned"
        with pytest.raises(H.HnhError, match=words):
            gnn.edge_bias_grad(0)  # not learned
        gnn.set_edge_bias_learned(0)
        with pytest.raises(H.HnhError, match=words):
            gnn.edge_bias_grad(0)  # learned, no backward pass yet
        with pytest.raises(H.HnhError, match="layer index 5 out of range"):
            gnn.edge_bias_grad(5)
        gnn.set_edge_bias(0, None, None)  # clearing the bias clears the switch
        with pytest.raises(H.HnhError, match="no edge bias to learn"):
            gnn.set_edge_bias_learned(0)
        gnn.edge_bias_from(lambda r, c: E.hash_bias(r, c), layer=0)
        with pytest.raises(H.HnhError, match=r"hnh_attn_qkv_bias_fwd_csr_p.*include/hnh_attn_edge\.h"):
            gnn.forwardPass()

    on_the_double(spoil)


# ------------------------------------------------------------------------------------------------ the model that learns its bias
ADAM = dict(kind="adam", lr=0.05, weight_decay=5e-4)


def planted(off=False):
    pp = R.planted_partition(LAYERS)
    wq, wk = Q.qk_weights_of(LAYERS)
    rows, cols = np.asarray(pp["rows"]), np.asarray(pp["cols"])
    eb = {li: E.hash_bias(rows, cols, salt=li) for li in range(len(LAYERS))}
    is_off = np.zeros(len(rows), dtype=bool)
    if off:  # the entry with the largest column of every row that has another column
        top = np.full(pp["m"], -1)
        np.maximum.at(top, rows, cols)
        low = np.full(pp["m"], pp["m"])
        np.minimum.at(low, rows, cols)
        is_off = (cols == top[rows]) & (top[rows] > low[rows])
        assert np.count_nonzero(is_off) > 100
        eb = {li: np.where(is_off, OFF, b) for li, b in eb.items()}
    args = (rows, cols, pp["m"], pp["x"], LAYERS, pp["labels"], pp["mask"], "mean", pp["w"], wq, wk)
    return args, eb, is_off


def test_the_loss_falls_when_only_the_bias_is_trained():
    args, eb, _ = planted()
    losses, _, w, wq, wk, got = L.train(*args, ADAM, 8, edge_bias=eb, learned=(0, 1), train_others=False, activations=("elu", "identity"))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] < 0.97 * losses[0], losses
    assert all(np.array_equal(w[k], args[8][k]) and np.array_equal(wq[k], args[9][k]) for k in w), "nothing else moved"
    assert all(T.rel(got[li], eb[li]) > 1e-3 for li in eb), "both biases moved"
    # a layer that is not learned keeps its bias to the bit
    _, _, _, _, _, one = L.train(*args, ADAM, 3, edge_bias=eb, learned=(0,), activations=("elu", "identity"))
    assert np.array_equal(one[1], eb[1]) and not np.array_equal(one[0], eb[0])


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_switched_off_entries_stay_switched_off_to_the_bit(kind):
    """weight_decay > 0 on every other tensor; the bias is not decayed: gradient 0, moments 0, value -1e300 (decay would give
    -1e300 (1 - lr wd) under SGD, and a gradient of -5e296 and a step of lr under Adam, which -1e300 absorbs: the SGD case tells)"""
    args, eb, is_off = planted(off=True)
    opt = ADAM if kind == "adam" else dict(kind="sgd", lr=0.05, momentum=0.9, weight_decay=5e-4)
    rows, cols, m, x = args[:4]
    g0 = R.xent(E.forward(rows, cols, m, x, LAYERS, args[8], args[9], args[10], edge_bias=eb), args[5], args[6], R.heads_of(LAYERS, "mean")[0])[2]
    deb = E.backward(rows, cols, m, x, LAYERS, g0, args[8], args[9], args[10], edge_bias=eb)[6]
    assert all(np.all(deb[li][is_off] == 0.0) and np.abs(deb[li][~is_off]).max() > 0 for li in deb), "p_e = 0 exactly: gradient 0 in every head"
    losses, _, _, _, _, got = L.train(*args, opt, 5, edge_bias=eb, learned=(0, 1))
    for li in eb:
        assert np.array_equal(got[li][is_off], np.full(np.count_nonzero(is_off), OFF))
        assert np.all(np.isfinite(got[li])) and not np.array_equal(got[li][~is_off], eb[li][~is_off])
    assert losses[-1] < losses[0]
