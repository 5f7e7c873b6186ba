"""The GAT's score "transformer" without a GPU: the numpy definition (tests/gat_qkv_ref.py) against central finite differences in every
parameter and the input, its pass-level restatement on the packed operands against the definition, uniform attention at W_q = 0, the
tied-weights identity against gat_ref's dot-product softmax, scores beyond +-800, the optional kernel group of include/hnh_attn_qkv.h
(declared == bound == exported by the HIP library, disjoint from every other table, absent from the CPU test double, the struct's size), the
host calls, and on the test double: the score names a kernel of the new group and its header, every unsupported shape is refused by name
before any launch, and a plain GAT on the same object runs as before.

Bounds: finite differences with step 1e-6 and bound 1e-6; the passes against the definition 1e-11 (T.TOL); "same maths, other summation
order" 1e-13."""
import ctypes as C
import re

import numpy as np
import pytest

import gat_qkv_ref as Q
import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared, fd_problem, make_gat, plain_output

GROUP = {"hnh_attn_qkv_fwd_csr_p", "hnh_attn_qkv_row_csr_p", "hnh_attn_qkv_col_csr_p"}
STEP = 1e-6
LAYERS = T.GAT_LAYERS


def skip_parameters(seed=12):
    """a bias on both layers and W_res of a projection on both, of order one over sqrt(fan-in)"""
    rng = np.random.default_rng(seed)
    bias = {li: rng.standard_normal(fph * heads) * 0.5 for li, (fin, fph, heads) in enumerate(LAYERS)}
    res_weights = {li: rng.standard_normal((fin, fph * heads)) / np.sqrt(fin) for li, (fin, fph, heads) in enumerate(LAYERS)}
    return dict(residual="projection", bias=bias, res_weights=res_weights)


CONFIGS = {"relu": dict(activations="relu"), "published": dict(activations=("elu", "identity")),
           "bias + projection": dict(activations=("elu", "relu"), **skip_parameters())}


def fd_inputs(mode):
    """fd_problem() with W_q, W_k of the usual scale and x drawn again from the first seed at which every activation's input lies at least
    200 steps from 0 (the score has no kink): the condition is asserted."""
    rows, cols, m, x, w, _, g = fd_problem()
    wq, wk = Q.qk_weights_of(LAYERS, scale=2.0)
    for seed in range(200):
        xs = np.random.default_rng(2000 + seed).uniform(-1, 1, x.shape)
        if np.abs(Q.pre_activations(rows, cols, m, xs, LAYERS, w, wq, wk, **mode)).min() >= 200 * STEP:
            return rows, cols, m, xs, w, wq, wk, g
    raise AssertionError("no seed keeps every kink 200 steps away")


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_reference_backward_matches_finite_differences(config):
    mode = CONFIGS[config]
    rows, cols, m, x, w, wq, wk, g = fd_inputs(mode)
    dws, dwqs, dwks, dbs, dwrs, dx = Q.backward(rows, cols, m, x, LAYERS, g, w, wq, wk, **mode)

    def loss(p):
        kw = dict(mode)
        if "bias" in mode:
            kw.update(bias=p["b"], res_weights=p["wr"])
        return float(np.sum(g * Q.forward(rows, cols, m, p["x"], LAYERS, p["w"], p["wq"], p["wk"], **kw)))

    def margin_ok(p, steps=100):
        kw = dict(mode)
        if "bias" in mode:
            kw.update(bias=p["b"], res_weights=p["wr"])
        return np.abs(Q.pre_activations(rows, cols, m, p["x"], LAYERS, p["w"], p["wq"], p["wk"], **kw)).min() >= steps * STEP

    base = dict(x=x, w=w, wq=wq, wk=wk, b=mode.get("bias"), wr=mode.get("res_weights"))
    assert margin_ok(base), "every activation's input is at least 100 steps from a kink"
    grads = dict(w=dws, wq=dwqs, wk=dwks, b=dbs, wr=dwrs)
    for name in ("w", "wq", "wk"):
        assert all(np.abs(d).max() > 0 for d in grads[name].values()), "the gradients must not be vacuous"
    assert np.count_nonzero(dx) > dx.size // 2

    def fd_of(name, key, probes):
        out = []
        for idx in probes:
            vals = []
            for h in (STEP, -STEP):
                p = dict(base)
                if key is None:
                    p[name] = base[name].copy()
                    p[name][idx] += h
                else:
                    p[name] = dict(base[name])
                    p[name][key] = base[name][key].copy()
                    p[name][key][idx] += h
                assert margin_ok(p, steps=99)
                vals.append(loss(p))
            out.append((vals[0] - vals[1]) / (2 * STEP))
        return np.array(out)

    rng = np.random.default_rng(3)
    worst = 0.0
    for name in ("w", "wq", "wk") + (("b", "wr") if "bias" in mode else ()):  # every tensor of every (layer, head) / layer
        for key, t in base[name].items():
            probes = [tuple(0 for _ in t.shape), tuple(s - 1 for s in t.shape)] + [tuple(rng.integers(0, s) for s in t.shape) for _ in range(3)]
            an = np.array([grads[name][key][idx] for idx in probes])
            err = np.max(np.abs(fd_of(name, key, probes) - an)) / np.max(np.abs(an))
            worst = max(worst, err)
            assert err <= 1e-6, (name, key, err)
    probes = [(0, 0), (m - 1, x.shape[1] - 1)] + [tuple(rng.integers(0, s) for s in x.shape) for _ in range(4)]
    an = np.array([dx[idx] for idx in probes])
    err = np.max(np.abs(fd_of("x", None, probes) - an)) / np.max(np.abs(an))
    T.record_observed("gat_qkv_fd", case=config, worst=max(worst, err))
    assert err <= 1e-6, err


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_passes_with_the_packed_operands_equal_the_definition(config):
    mode = CONFIGS[config]
    rows, cols, m, x, w, wq, wk, g = fd_inputs(mode)
    want = Q.backward(rows, cols, m, x, LAYERS, g, w, wq, wk, **mode)
    got = Q.backward(rows, cols, m, x, LAYERS, g, w, wq, wk, by_passes=True, **mode)
    for gd, wd in zip(got[:5], want[:5]):
        assert gd.keys() == wd.keys()
        for k in wd:
            assert T.rel(gd[k], wd[k]) <= T.TOL, k
    assert T.rel(got[5], want[5]) <= T.TOL
    assert T.rel(Q.forward(rows, cols, m, x, LAYERS, w, wq, wk, by_passes=True, **mode), Q.forward(rows, cols, m, x, LAYERS, w, wq, wk, **mode)) <= T.TOL
    # the forward pass as the kernel takes it, and its extended-precision twin
    fin, f, _ = LAYERS[0]
    kv = np.nan_to_num(Q.P.fused_pack(x @ wk[(0, 0)], x @ w[(0, 0)]))
    o, lse, s, _ = Q.fwd_pass(rows, cols, m, x @ wq[(0, 0)], kv, f, Q.scale_of(f))
    o_ld, lse_ld, s_ld = Q.fwd_pass_ld(rows, cols, m, x @ wq[(0, 0)], kv, f, Q.scale_of(f))
    assert o_ld.dtype == np.longdouble
    assert T.rel(np.float64(o_ld), o) <= 1e-13 and T.rel(np.float64(lse_ld), lse) <= 1e-13 and T.rel(np.float64(s_ld), s) <= 1e-13


@pytest.mark.parametrize("activations", ["relu", "elu", "identity"])
def test_zero_query_weights_give_uniform_attention(activations):
    """W_q = 0: every score is 0, so the output is act(mean of V_j over the row's nonzeros, with multiplicity), and dQ = dK = 0: the
    stationary point the README warns about."""
    rows, cols, m, x, w, _, g = fd_problem()
    layers = LAYERS[:1]
    _, wk = Q.qk_weights_of(layers)
    wq = {k: np.zeros_like(v) for k, v in wk.items()}
    out = Q.forward(rows, cols, m, x, layers, w, wq, wk, activations=activations)
    deg = np.bincount(rows, minlength=m)
    for h in range(layers[0][2]):
        v = x @ w[(0, h)]
        mean = np.zeros_like(v)
        np.add.at(mean, rows, v[cols])
        mean[deg > 0] /= deg[deg > 0][:, None]
        f = layers[0][1]
        assert T.rel(out[:, h * f:(h + 1) * f], R.act(mean, activations)) <= 1e-13
    gl = np.random.default_rng(2).uniform(-1, 1, out.shape)
    _, dwq, dwk, _, _, _ = Q.backward(rows, cols, m, x, layers, gl, w, wq, {k: np.zeros_like(v) for k, v in wk.items()}, activations=activations)
    assert all(np.all(d == 0.0) for d in dwq.values()) and all(np.all(d == 0.0) for d in dwk.values()), "W_q = W_k = 0 is a stationary point of both"


@pytest.mark.parametrize("f", [16, 64])
def test_tied_weights_equal_the_dot_product_softmax(f):
    """W_k = W_v = W and W_q = W / scale: s_ij = <A_i, A_j>, which is gat_ref's score dot under attention softmax with alpha = 1.0 (the
    LeakyReLU is the identity).  scale is a power of two at these widths, so the tie is exact in the inputs.  Then dW_dot = dW_v + dW_k +
    dW_q / scale."""
    rows, cols, m, x, _, _, _ = fd_problem()
    layers = [(16, f, 2), (2 * f, f, 1)]
    rng = np.random.default_rng(f)
    w = {(li, h): rng.standard_normal((fin, fph)) / np.sqrt(fin * np.sqrt(fph)) for li, (fin, fph, heads) in enumerate(layers) for h in range(heads)}
    scale = Q.scale_of(f)
    assert scale in (0.25, 0.125)
    wq = {k: v / scale for k, v in w.items()}
    g = np.random.default_rng(1).uniform(-1, 1, (m, f))
    for acts in ("relu", ("elu", "identity")):
        out = Q.forward(rows, cols, m, x, layers, w, wq, w, activations=acts)
        want = R.forward(rows, cols, m, x, layers, 1.0, w, attention="softmax", score="dot", activations=acts)
        assert np.abs(want).max() > 0 and T.rel(out, want) <= 1e-13
        dw, dwq, dwk, _, _, dx = Q.backward(rows, cols, m, x, layers, g, w, wq, w, activations=acts)
        dw_dot, _, dx_dot = R.backward(rows, cols, m, x, layers, 1.0, g, w, attention="softmax", score="dot", activations=acts)
        for k in w:
            assert T.rel(dw[k] + dwk[k] + dwq[k] / scale, dw_dot[k]) <= 1e-13, k
        assert T.rel(dx, dx_dot) <= 1e-13


def test_forward_is_finite_far_outside_exps_range():
    from oracle import oracle as O
    rows, cols = O.erdos_renyi(6, 8)
    m, f = 64, 6
    rng = np.random.default_rng(1)
    qm, km, vm = rng.uniform(-1, 1, (m, f)) * 700, rng.uniform(-1, 1, (m, f)), rng.uniform(-1, 1, (m, f))
    kv = np.nan_to_num(Q.P.fused_pack(km, vm))
    o, lse, s, _ = Q.fwd_pass(rows, cols, m, qm, kv, f, 1.0)
    assert s.max() > 800 and s.min() < -800 and np.all(np.isfinite(o)) and np.all(np.isfinite(lse))
    o_ld, lse_ld, _ = Q.fwd_pass_ld(rows, cols, m, qm, kv, f, 1.0)
    assert T.rel(o, np.float64(o_ld)) <= 1e-12 and T.rel(lse, np.float64(lse_ld)) <= 1e-12


def test_qkv_kernels_are_an_optional_group():
    names = declared("hnh_attn_qkv.h")
    assert names == GROUP
    assert names == set(K.QKV_SIGNATURES), names ^ set(K.QKV_SIGNATURES)
    for header in ("hnh_kernels.h", "hnh_grad.h", "hnh_attention.h", "hnh_attn_grad.h", "hnh_attn_additive.h", "hnh_attn_dropout.h", "hnh_train.h",
                   "hnh_attn_v2.h", "hnh_attn_coef.h", "hnh_gat_skip.h"):
        assert not names & declared(header), header
    for table in (K.SIGNATURES, K.AIDS_SIGNATURES, K.GRAD_SIGNATURES, K.ATTN_SIGNATURES, K.ATTN_GRAD_SIGNATURES, K.ATTN_ADD_SIGNATURES,
                  K.ATTN_DROP_SIGNATURES, K.TRAIN_SIGNATURES, K.V2_SIGNATURES, K.ATTN_COEF_SIGNATURES, K.SKIP_SIGNATURES):
        assert not names & set(table), "disjoint from the existing tables"
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.QKV_SIGNATURES[n][1]
    dbl = C.CDLL(T.ORACLE_BACKEND)
    for n in names:
        assert not hasattr(dbl, n), "the CPU test double does not export %s" % n
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works
    assert C.sizeof(K.AttnQKV) == 168  # struct hnh_attn_qkv: nineteen pointers and pitches, an int (padded), a double
    assert K.AttnQKV.scale.offset == 160 and K.AttnQKV.f.offset == 152
    txt = open(ROOT + "/include/hnh_attn_qkv.h").read()
    assert re.search(r"#define HNH_ATTN_QKV_MAX_F %d\b" % K.ATTN_QKV_MAX_F, txt) and K.ATTN_QKV_MAX_F == 256
    assert "168 bytes" in txt


def test_host_wiring():
    txt = open(ROOT + "/include/hnh_dist.h").read()
    assert re.search(r"#define HNH_GAT_SCORE_TRANSFORMER 3\b", txt) and re.search(r"#define HNH_GAT_SCORE_GATV2 2\b", txt)
    for n in ("hnh_gat_set_qk_weight", "hnh_gat_get_qk_weight", "hnh_gat_get_qk_weight_grad"):
        assert n in txt and n in H.SIGNATURES
    assert H.GAT.SCORE == {"dot": 0, "additive": 1} and H.GAT.SCORE_V2 == {"gatv2": 2}, "the existing tables are unchanged"
    assert H.GAT.SCORE_QKV == {"transformer": 3}
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, attention="softmax")
        gnn.set_score("transformer")
        with pytest.raises(ValueError, match="additive.*dot.*gatv2.*transformer"):
            gnn.set_score("bilinear")
        assert H.lib().hnh_gat_set_score(gnn.h, 3) == 0 and H.lib().hnh_gat_set_score(gnn.h, 7) != 0
        # W_q and W_k: zero until set, read back as set, refused by shape, head and selector
        shape = gnn.weight_shape(1, 2)
        assert np.all(gnn.get_query_weight(1, 2) == 0.0) and np.all(gnn.get_key_weight(1, 2) == 0.0)
        wq, wk = np.random.default_rng(0).uniform(-1, 1, (2,) + shape)
        gnn.set_query_weight(1, 2, wq)
        gnn.set_key_weight(1, 2, wk)
        assert np.array_equal(gnn.get_query_weight(1, 2), wq) and np.array_equal(gnn.get_key_weight(1, 2), wk)
        assert np.all(gnn.get_query_weight(1, 1) == 0.0)
        with pytest.raises(ValueError):
            gnn.set_query_weight(1, 2, wq[:, :-1])
        with pytest.raises(H.HnhError):
            gnn.get_key_weight(1, 3)
        assert H.lib().hnh_gat_get_qk_weight(gnn.h, 1, 3, 1, wq.ctypes.data) != 0 and b"head index 3 out of range" in H.lib().hnh_host_last_error()
        assert H.lib().hnh_gat_set_qk_weight(gnn.h, 0, 0, 2, wq.ctypes.data) != 0, "the selector is 0 or 1"
        with pytest.raises(H.HnhError, match="no GAT query/key weight gradient yet.*score transformer"):
            gnn.query_weight_grad(0, 0)
        for h in (gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(1, rank))


def refused(case, words, ranks=1, alg="15d_fusion2", c=1, layers=None, backward=True, call=None, **kw):
    """forwardPass (and backwardPass) of a transformer GAT raise HnhError matching `words` (call: another entry point to try instead); the
    same object then runs a plain GAT whose output is bit-equal to that of an object that never heard of the score (schedules on which
    the plain GAT is the reference's only)."""
    def rank(world):
        sp, d, gnn = make_gat(world, case, alg, c, layers=layers, **dict(dict(attention="softmax", score="transformer"), **kw))
        with pytest.raises(H.HnhError, match=words) as e:
            (call or (lambda g: g.forwardPass()))(gnn)
        msg = str(e.value)
        if backward and call is None:
            g = H.Dense.create(world, *gnn.buffer_shape(len(layers or LAYERS)))
            with pytest.raises(H.HnhError, match=words):
                gnn.backwardPass(g)
            g.free()
        res = None
        if layers is None and alg == "15d_fusion2" and c == 1:
            gnn.set_score("dot")  # the process and the operator live on: the plain GAT on the same object
            gnn.set_attention("none")
            gnn.set_dropout(0.0, 0.0, 0)
            gnn.forwardPass()
            out = H.Dense.create(world, *gnn.buffer_shape(len(LAYERS)))
            gnn.get_output(out)
            res = out.download()
            out.free()
        for h in (gnn, d, sp):
            h.free()
        return msg, res

    per_rank = H.run_spmd(ranks, rank)
    if per_rank[0][1] is not None:
        want = H.run_spmd(ranks, lambda world: plain_output(world, case))
        assert all(np.isfinite(r[1]).all() and np.array_equal(r[1], b) for r, b in zip(per_rank, want))
    return per_rank[0][0]


def test_transformer_on_the_test_double_names_the_missing_kernel():
    H.load_backend(T.ORACLE_BACKEND)
    msg = refused(T.case_inputs("er8_r16"), r"transformer.*hnh_attn_qkv_[a-z0-9_]+.*include/hnh_attn_qkv\.h", ranks=2)
    assert re.search(r"hnh_attn_qkv_[a-z0-9_]+", msg).group(0) in GROUP


def test_transformer_refuses_attention_none_and_attention_dropout():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")
    refused(case, "score transformer.*attention mode softmax only.*attention mode none", attention="none")
    refused(case, "attention dropout.*transformer", dropout=(0.25, 0.0), seed=3)


@pytest.mark.parametrize("alg,p,c,name", [("15d_fusion1", 4, 2, "15d_fusion1"), ("15d_fusion2", 4, 2, "15d_fusion2")])
def test_transformer_refuses_unsupported_schedules(alg, p, c, name):
    H.load_backend(T.ORACLE_BACKEND)
    refused(T.case_inputs("er8_r16"), "score transformer.*%s.*c = %d" % (name, c), ranks=p, alg=alg, c=c, layers=[(16, 8, 2)])


def test_transformer_refuses_wide_heads_and_accepts_256():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")
    refused(case, "score transformer.*at most 256 features, not 257", layers=[(16, 257, 1)])
    refused(case, r"hnh_attn_qkv_fwd_csr_p.*include/hnh_attn_qkv\.h", layers=[(16, 256, 1)])


def test_attention_coefficients_refuse_the_score_by_name():
    H.load_backend(T.ORACLE_BACKEND)
    refused(T.case_inputs("er8_r16"), "attention_coefficients does not support score transformer", call=lambda g: g.attention_coefficients(0, 0))


def test_the_reference_trains():
    """The condition on the inputs of the GPU test's Adam run: the numpy reference's own loss on the planted partition falls, and every W_q and
    W_k moves."""
    pp = R.planted_partition(LAYERS)
    wq, wk = Q.qk_weights_of(LAYERS)
    res = Q.train(pp["rows"], pp["cols"], pp["m"], pp["x"], LAYERS, pp["labels"], pp["mask"], "mean", pp["w"], wq, wk, R.LEARN_OPTIMIZER, 10,
                  activations=("elu", "identity"))
    losses = res[0]
    assert losses[-1] < losses[0], losses
    assert all(np.abs(res[3][k] - wq[k]).max() > 0 and np.abs(res[4][k] - wk[k]).max() > 0 for k in wq)
