"""The per-edge bias of the GAT's score "transformer" without a GPU (include/hnh_attn_edge.h, GAT.set_edge_bias): the numpy definition
(tests/gat_edge_ref.py) against central finite differences in W_v, W_q, W_k, the input and the bias itself (db_e = g_e / scale: a check of
p_e, which nothing exports); b = 0 equals tests/gat_qkv_ref.py exactly; a row-constant bias leaves the output alone and moves lse by the
constant; b = log w equals an explicitly weighted softmax; -1e300 on one edge equals the model on the graph without that edge; two copies
of a repeated pair with different values; the pass-level restatement against the definition; the optional kernel group (declared ==
bound == exported by the HIP library, disjoint from every other header and table, absent from the CPU test double, struct hnh_attn_qkv
still 168 bytes); the C ABI; and on the test double: a biased forward pass names a kernel of the group and its header, wrong lengths, a
layer out of range and one null of the two are refused by name and leave the object usable, scores dot, additive and gatv2 with a bias
set are refused by name, and after clearing the plain GAT on the same object is bit-equal to an object that never heard of it.

Bounds: finite differences with step 1e-6 and bound 1e-6; the passes against the definition 1e-11 (T.TOL); "same maths, other summation
order" 1e-13."""
import ctypes as C
import re

import numpy as np
import pytest

import gat_edge_ref as E
import gat_qkv_ref as Q
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared, fd_problem, make_gat, plain_output

GROUP = {"hnh_attn_qkv_bias_fwd_csr_p", "hnh_attn_qkv_bias_row_csr_p", "hnh_attn_qkv_bias_col_csr_p"}
STEP = 1e-6
LAYERS = T.GAT_LAYERS


def edge_biases(rows, cols, seed=21):
    """one bias per layer in [-3, 3), distinct per entry: the two copies of the repeated pair differ"""
    rng = np.random.default_rng(seed)
    eb = {li: rng.uniform(-3, 3, len(rows)) for li in range(len(LAYERS))}
    r, c, copy = E.keys(rows, cols)
    assert copy.max() == 1, "fd_problem has one repeated pair"
    twin = np.flatnonzero(copy == 1)[0]
    first = np.flatnonzero((r == r[twin]) & (c == c[twin]) & (copy == 0))[0]
    assert all(b[twin] != b[first] for b in eb.values())
    return eb


def skip_parameters(seed=12):
    rng = np.random.default_rng(seed)
    bias = {li: rng.standard_normal(fph * heads) * 0.5 for li, (fin, fph, heads) in enumerate(LAYERS)}
    res_weights = {li: rng.standard_normal((fin, fph * heads)) / np.sqrt(fin) for li, (fin, fph, heads) in enumerate(LAYERS)}
    return dict(residual="projection", bias=bias, res_weights=res_weights)


CONFIGS = {"relu": dict(activations="relu"), "published": dict(activations=("elu", "identity")),
           "bias + projection": dict(activations=("elu", "relu"), **skip_parameters())}


def fd_inputs(mode):
    """fd_problem() with W_q, W_k, an edge bias on both layers, and x drawn again from the first seed at which every activation's input lies
    at least 200 steps from 0: the condition is asserted."""
    rows, cols, m, x, w, _, g = fd_problem()
    wq, wk = Q.qk_weights_of(LAYERS, scale=2.0)
    eb = edge_biases(rows, cols)
    for seed in range(200):
        xs = np.random.default_rng(2000 + seed).uniform(-1, 1, x.shape)
        if np.abs(E.pre_activations(rows, cols, m, xs, LAYERS, w, wq, wk, edge_bias=eb, **mode)).min() >= 200 * STEP:
            return rows, cols, m, xs, w, wq, wk, eb, g
    raise AssertionError("no seed keeps every kink 200 steps away")


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_reference_backward_matches_finite_differences(config):
    mode = CONFIGS[config]
    rows, cols, m, x, w, wq, wk, eb, g = fd_inputs(mode)
    dws, dwqs, dwks, dbs, dwrs, dx, debs = E.backward(rows, cols, m, x, LAYERS, g, w, wq, wk, edge_bias=eb, **mode)
    plain = Q.backward(rows, cols, m, x, LAYERS, g, w, wq, wk, **mode)
    assert T.rel(dx, plain[5]) > 1e-3, "the bias changes the gradients"

    def kwargs(p):
        kw = dict(mode, edge_bias=p["eb"])
        if "bias" in mode:
            kw.update(bias=p["b"], res_weights=p["wr"])
        return kw

    def loss(p):
        return float(np.sum(g * E.forward(rows, cols, m, p["x"], LAYERS, p["w"], p["wq"], p["wk"], **kwargs(p))))

    def margin_ok(p, steps=100):
        return np.abs(E.pre_activations(rows, cols, m, p["x"], LAYERS, p["w"], p["wq"], p["wk"], **kwargs(p))).min() >= steps * STEP

    base = dict(x=x, w=w, wq=wq, wk=wk, eb=eb, b=mode.get("bias"), wr=mode.get("res_weights"))
    assert margin_ok(base)
    grads = dict(w=dws, wq=dwqs, wk=dwks, eb=debs, b=dbs, wr=dwrs)
    for name in ("w", "wq", "wk", "eb"):
        assert all(np.abs(d).max() > 0 for d in grads[name].values()), "the gradients must not be vacuous"

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
    twin = int(np.flatnonzero(E.keys(rows, cols)[2] == 1)[0])
    for name in ("w", "wq", "wk", "eb") + (("b", "wr") if "bias" in mode else ()):
        for key, t in base[name].items():
            probes = [tuple(0 for _ in t.shape), tuple(s - 1 for s in t.shape)] + [tuple(rng.integers(0, s) for s in t.shape) for _ in range(3)]
            if name == "eb":
                probes.append((twin,))  # the second copy of the repeated pair has a derivative of its own
            an = np.array([grads[name][key][idx] for idx in probes])
            err = np.max(np.abs(fd_of(name, key, probes) - an)) / np.max(np.abs(an))
            worst = max(worst, err)
            assert err <= 1e-6, (name, key, err)
    probes = [(0, 0), (m - 1, x.shape[1] - 1)] + [tuple(rng.integers(0, s) for s in x.shape) for _ in range(4)]
    an = np.array([dx[idx] for idx in probes])
    err = np.max(np.abs(fd_of("x", None, probes) - an)) / np.max(np.abs(an))
    T.record_observed("gat_edge_fd", case=config, worst=max(worst, err))
    assert err <= 1e-6, err


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_zero_bias_equals_the_plain_model_exactly(config):
    mode = CONFIGS[config]
    rows, cols, m, x, w, wq, wk, _, g = fd_inputs(mode)
    zero = {li: np.zeros(len(rows)) for li in range(len(LAYERS))}
    assert np.array_equal(E.forward(rows, cols, m, x, LAYERS, w, wq, wk, edge_bias=zero, **mode), Q.forward(rows, cols, m, x, LAYERS, w, wq, wk, **mode))
    assert np.array_equal(E.forward(rows, cols, m, x, LAYERS, w, wq, wk, **mode), Q.forward(rows, cols, m, x, LAYERS, w, wq, wk, **mode))
    got = E.backward(rows, cols, m, x, LAYERS, g, w, wq, wk, edge_bias=zero, **mode)
    want = Q.backward(rows, cols, m, x, LAYERS, g, w, wq, wk, **mode)
    for gd, wd in zip(got[:5], want[:5]):
        assert gd.keys() == wd.keys() and all(np.array_equal(gd[k], wd[k]) for k in wd)
    assert np.array_equal(got[5], want[5])


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_passes_with_the_packed_operands_equal_the_definition(config):
    mode = CONFIGS[config]
    rows, cols, m, x, w, wq, wk, eb, g = fd_inputs(mode)
    want = E.backward(rows, cols, m, x, LAYERS, g, w, wq, wk, edge_bias=eb, **mode)
    got = E.backward(rows, cols, m, x, LAYERS, g, w, wq, wk, edge_bias=eb, by_passes=True, **mode)
    for gd, wd in zip(got[:5], want[:5]):
        assert gd.keys() == wd.keys()
        for k in wd:
            assert T.rel(gd[k], wd[k]) <= T.TOL, k
    assert T.rel(got[5], want[5]) <= T.TOL
    fin, f, _ = LAYERS[0]
    kv = np.nan_to_num(Q.P.fused_pack(x @ wk[(0, 0)], x @ w[(0, 0)]))
    o, lse, s, _ = E.fwd_pass(rows, cols, m, x @ wq[(0, 0)], kv, f, Q.scale_of(f), eb[0])
    o_ld, lse_ld, s_ld = E.fwd_pass_ld(rows, cols, m, x @ wq[(0, 0)], kv, f, Q.scale_of(f), eb[0])
    assert o_ld.dtype == np.longdouble
    assert T.rel(np.float64(o_ld), o) <= 1e-13 and T.rel(np.float64(lse_ld), lse) <= 1e-13 and T.rel(np.float64(s_ld), s) <= 1e-13
    o0, lse0, s0, _ = Q.fwd_pass(rows, cols, m, x @ wq[(0, 0)], kv, f, Q.scale_of(f))
    assert T.rel(s - eb[0], s0) <= 1e-13 and T.rel(o, o0) > 1e-3


def test_row_constant_bias_moves_lse_alone():
    """b_e = c_i for every entry of row i: p is unchanged, so is the output (1e-13), and lse_i moves by c_i."""
    rows, cols, m, x, w, _, g = fd_problem()
    layers = LAYERS[:1]
    wq, wk = Q.qk_weights_of(layers, scale=2.0)
    c = np.random.default_rng(8).uniform(-5, 5, m)
    out0, tr0 = Q.forward(rows, cols, m, x, layers, w, wq, wk, keep_trace=True)
    out1, tr1 = E.forward(rows, cols, m, x, layers, w, wq, wk, edge_bias={0: c[rows]}, keep_trace=True)
    assert np.abs(out0).max() > 0 and T.rel(out1, out0) <= 1e-13
    live = np.bincount(rows, minlength=m) > 0
    for h0, h1 in zip(tr0[0][3], tr1[0][3]):
        assert np.max(np.abs((h1[4] - h0[4])[live] - c[live])) <= 1e-13 * np.abs(c).max()
    gl = np.random.default_rng(2).uniform(-1, 1, out0.shape)
    b0 = Q.backward(rows, cols, m, x, layers, gl, w, wq, wk)
    b1 = E.backward(rows, cols, m, x, layers, gl, w, wq, wk, edge_bias={0: c[rows]})
    assert all(T.rel(b1[i][k], b0[i][k]) <= 1e-12 for i in range(3) for k in b0[i]) and T.rel(b1[5], b0[5]) <= 1e-12


def test_log_weights_are_the_weighted_softmax():
    """b = log w: a_e = w_e exp(s_e) / sum_e' w_e' exp(s_e'), written out"""
    rows, cols, m, x, w, _, _ = fd_problem()
    layers = LAYERS[:1]
    fin, f, heads = layers[0]
    wq, wk = Q.qk_weights_of(layers, scale=2.0)
    wt = np.random.default_rng(4).uniform(0.05, 20.0, len(rows))
    out = E.forward(rows, cols, m, x, layers, w, wq, wk, edge_bias={0: np.log(wt)}, activations="identity")
    for h in range(heads):
        qm, km, vm = x @ wq[(0, h)], x @ wk[(0, h)], x @ w[(0, h)]
        num = wt * np.exp(Q.scale_of(f) * np.einsum("ij,ij->i", qm[rows], km[cols]))
        den = np.bincount(rows, weights=num, minlength=m)
        want = np.zeros((m, f))
        np.add.at(want, rows, (num / den[rows])[:, None] * vm[cols])
        assert np.abs(want).max() > 0 and T.rel(out[:, h * f:(h + 1) * f], want) <= 1e-13


def test_a_very_negative_bias_removes_the_edge():
    """-1e300 on one entry of every row with two or more entries (one of them a copy of the repeated pair): the model on the graph without
    those entries, forward and backward, to the bit in p (exp underflows to an exact 0)."""
    rows, cols, m, x, w, _, g = fd_problem()
    wq, wk = Q.qk_weights_of(LAYERS, scale=2.0)
    deg = np.bincount(rows, minlength=m)
    off = np.zeros(len(rows), dtype=bool)
    for i in np.flatnonzero(deg >= 2):
        off[np.flatnonzero(rows == i)[-1]] = True
    assert off[-1], "the appended copy of the repeated pair is switched off, its first copy stays"
    eb = {li: np.where(off, -1e300, 0.0) for li in range(len(LAYERS))}
    mode = dict(activations=("elu", "identity"))
    out = E.forward(rows, cols, m, x, LAYERS, w, wq, wk, edge_bias=eb, **mode)
    want = Q.forward(rows[~off], cols[~off], m, x, LAYERS, w, wq, wk, **mode)
    assert np.all(np.isfinite(out)) and T.rel(out, want) <= 1e-13 and T.rel(out, Q.forward(rows, cols, m, x, LAYERS, w, wq, wk, **mode)) > 1e-3
    got = E.backward(rows, cols, m, x, LAYERS, g, w, wq, wk, edge_bias=eb, **mode)
    ref = Q.backward(rows[~off], cols[~off], m, x, LAYERS, g, w, wq, wk, **mode)
    assert all(T.rel(got[i][k], ref[i][k]) <= 1e-13 for i in range(3) for k in ref[i]) and T.rel(got[5], ref[5]) <= 1e-13
    assert all(np.all(d[off] == 0.0) for d in got[6].values())
    # alone in its row it is the row's only edge: p = 1, like any single edge
    single = np.flatnonzero(deg == 1)
    if len(single):
        e = np.flatnonzero(rows == single[0])[0]
        eb1 = {0: np.zeros(len(rows))}
        eb1[0][e] = -1e300
        a = E.forward(rows, cols, m, x, LAYERS[:1], w, wq, wk, edge_bias=eb1)
        assert np.array_equal(a[single[0]], Q.forward(rows, cols, m, x, LAYERS[:1], w, wq, wk)[single[0]])


def test_keys_and_hash_bias():
    rows, cols = np.array([3, 1, 3, 3, 1]), np.array([2, 0, 2, 5, 0])
    assert np.array_equal(E.keys(rows, cols)[2], [0, 0, 1, 0, 1])
    assert np.array_equal(E.bias_of(lambda r, c, k: r * 100 + c * 10 + k, rows, cols), [320, 100, 321, 350, 101])
    b = E.hash_bias(np.arange(1000), np.arange(1000)[::-1])
    assert b.min() >= -2 and b.max() < 2 and len(np.unique(b)) > 500
    assert np.array_equal(b, E.hash_bias(np.arange(1000).astype(np.int32), np.arange(1000)[::-1].copy()))


def test_edge_kernels_are_an_optional_group():
    names = declared("hnh_attn_edge.h")
    assert names == GROUP
    assert names == set(K.EDGE_SIGNATURES), names ^ set(K.EDGE_SIGNATURES)
    for header in ("hnh_kernels.h", "hnh_grad.h", "hnh_attention.h", "hnh_attn_grad.h", "hnh_attn_additive.h", "hnh_attn_dropout.h", "hnh_train.h",
                   "hnh_attn_v2.h", "hnh_attn_coef.h", "hnh_gat_skip.h", "hnh_attn_qkv.h"):
        assert not names & declared(header), header
    for table in (K.SIGNATURES, K.AIDS_SIGNATURES, K.GRAD_SIGNATURES, K.ATTN_SIGNATURES, K.ATTN_GRAD_SIGNATURES, K.ATTN_ADD_SIGNATURES,
                  K.ATTN_DROP_SIGNATURES, K.TRAIN_SIGNATURES, K.V2_SIGNATURES, K.ATTN_COEF_SIGNATURES, K.SKIP_SIGNATURES, K.QKV_SIGNATURES):
        assert not names & set(table), "disjoint from the existing tables"
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.EDGE_SIGNATURES[n][1]
        parent = K.QKV_SIGNATURES[n.replace("_bias", "")][1]
        assert K.EDGE_SIGNATURES[n][1] == parent[:3] + [C.c_void_p] + parent[3:], "the parent's arguments plus the bias"
    dbl = C.CDLL(T.ORACLE_BACKEND)
    for n in names:
        assert not hasattr(dbl, n), "the CPU test double does not export %s" % n
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works
    assert C.sizeof(K.AttnQKV) == 168, "struct hnh_attn_qkv is unchanged"
    txt = open(ROOT + "/include/hnh_attn_edge.h").read()
    assert "168 bytes" in txt and "-inf is NOT supported" in txt and "-1e300" in txt


def test_host_wiring():
    txt = open(ROOT + "/include/hnh_dist.h").read()
    assert re.search(r"int hnh_gat_set_edge_bias\(hnh_gat\* g, int layer, const hnh_vec\* s, const hnh_vec\* st\);", txt)
    assert H.SIGNATURES["hnh_gat_set_edge_bias"] == (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p])
    assert hasattr(H.GAT, "set_edge_bias") and hasattr(H.GAT, "edge_bias_from")


def biased(case, words, ranks=1, score="transformer", spoil=None, **kw):
    """A GAT with an edge bias on layer 0 (edge_bias_from of a hash of the coordinates), then `spoil(gnn, d)` if given, which must raise
    HnhError matching `words`; otherwise forwardPass and backwardPass must.  Then the bias is cleared and the plain GAT on the same object
    is bit-equal to an object that never heard of it."""
    def rank(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, **dict(dict(attention="softmax", score=score), **kw))
        gnn.edge_bias_from(lambda r, c: E.hash_bias(r, c), layer=0)
        if spoil is not None:
            with pytest.raises(H.HnhError, match=words) as e:
                spoil(gnn, d)
        else:
            with pytest.raises(H.HnhError, match=words) as e:
                gnn.forwardPass()
            g = H.Dense.create(world, *gnn.buffer_shape(len(LAYERS)))
            with pytest.raises(H.HnhError, match=words):
                gnn.backwardPass(g)
            g.free()
        msg = str(e.value)
        gnn.set_edge_bias(0, None, None)
        gnn.set_edge_bias(0, None, None)  # clearing twice is clearing
        gnn.set_score("dot")
        gnn.set_attention("none")
        gnn.forwardPass()
        out = H.Dense.create(world, *gnn.buffer_shape(len(LAYERS)))
        gnn.get_output(out)
        res = out.download()
        for h in (out, gnn, d, sp):
            h.free()
        return msg, res

    per_rank = H.run_spmd(ranks, rank)
    want = H.run_spmd(ranks, lambda world: plain_output(world, case))
    assert all(np.isfinite(r[1]).all() and np.array_equal(r[1], b) for r, b in zip(per_rank, want))
    return per_rank[0][0]


def test_a_biased_pass_on_the_test_double_names_the_missing_kernel():
    H.load_backend(T.ORACLE_BACKEND)
    msg = biased(T.case_inputs("er8_r16"), r"edge bias.*hnh_attn_qkv_bias_[a-z0-9_]+.*include/hnh_attn_edge\.h", ranks=2)
    assert re.search(r"hnh_attn_qkv_bias_[a-z0-9_]+", msg).group(0) in GROUP


@pytest.mark.parametrize("score", ["dot", "additive", "gatv2"])
def test_other_scores_refuse_an_edge_bias_by_name(score):
    H.load_backend(T.ORACLE_BACKEND)
    biased(T.case_inputs("er8_r16"), r"edge bias of layer 0 supports score transformer only, not score %s\b.*include/hnh_attn_edge\.h" % score, score=score)


def _wrong_length(which):
    def spoil(gnn, d):
        s, st = d.like_S_values(0.0), d.like_ST_values(0.0)
        n = [len(s), len(st)]
        n[which] += 1
        vs = [H.Vec.create(s.w, k, 0.0) for k in n]
        try:
            gnn.set_edge_bias(0, vs[0], vs[1])
        finally:
            for v in vs + [s, st]:
                v.free()
    return spoil


def _one_null(gnn, d):
    s = d.like_S_values(0.0)
    try:
        gnn.set_edge_bias(0, s, None)
    finally:
        s.free()


def _other_null(gnn, d):
    st = d.like_ST_values(0.0)
    try:
        gnn.set_edge_bias(1, None, st)
    finally:
        st.free()


def _layer_out_of_range(gnn, d):
    s, st = d.like_S_values(0.0), d.like_ST_values(0.0)
    try:
        gnn.set_edge_bias(len(LAYERS), s, st)
    finally:
        s.free()
        st.free()


@pytest.mark.parametrize("spoil,words", [
    (_one_null, "set_edge_bias needs the bias in both orders.*like_ST_values vector is null"),
    (_other_null, "set_edge_bias needs the bias in both orders.*like_S_values vector is null"),
    (_layer_out_of_range, "layer index %d out of range" % len(LAYERS)),
    (_wrong_length(0), r"set_edge_bias needs a vector of like_S_values length: \d+ entries, not \d+"),
    (_wrong_length(1), r"set_edge_bias needs a vector of like_ST_values length: \d+ entries, not \d+")],
    ids=["st null", "s null", "layer", "s length", "st length"])
def test_bad_arguments_are_refused_by_name_and_leave_the_object_usable(spoil, words):
    """... and leave the bias that was set before in place: the next forward pass still asks for the group's kernels"""
    H.load_backend(T.ORACLE_BACKEND)

    def spoil_then_forward(gnn, d):
        try:
            spoil(gnn, d)
        except H.HnhError:
            with pytest.raises(H.HnhError, match=r"edge bias.*hnh_attn_qkv_bias_fwd_csr_p"):
                gnn.forwardPass()  # layer 0 still has its bias
            raise

    biased(T.case_inputs("er8_r16"), words, spoil=spoil_then_forward)


def test_edge_bias_from_refuses_rows_that_are_switched_off_entirely():
    """a row of several edges whose largest bias lies beyond +-EDGE_BIAS_ROW_MAX: the backward pass could not recompute its coefficients
    (include/hnh_attn_edge.h, Magnitudes); a single edge may carry anything finite; nothing is set by a refused call"""
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")
    assert H.GAT.EDGE_BIAS_ROW_MAX == 1e6 and "+-1e6" in open(ROOT + "/include/hnh_attn_edge.h").read()

    def rank(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, attention="softmax", score="transformer")
        rows, cols = d.S_coordinates()
        deg = np.bincount(rows)
        full = int(np.flatnonzero(deg >= 2)[0])
        for value in (-1e300, 2e6):
            with pytest.raises(ValueError, match="largest edge bias of row %d" % full):
                gnn.edge_bias_from(lambda r, c: np.where(r == full, value, 0.0))
        with pytest.raises(H.HnhError, match=r"score transformer.*hnh_attn_qkv_fwd_csr_p"):
            gnn.forwardPass()  # no bias was set: the plain score's own refusal on the test double
        top = np.full(len(deg), -1)
        np.maximum.at(top, rows, cols)
        gnn.edge_bias_from(lambda r, c: np.where(c == top[r], 0.5, -1e300))  # every row keeps an edge of moderate bias
        with pytest.raises(H.HnhError, match=r"edge bias.*hnh_attn_qkv_bias_fwd_csr_p"):
            gnn.forwardPass()
        for h in (gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(1, rank))
