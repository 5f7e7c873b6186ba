"""The GAT's bias and skip connections without a GPU (GAT.set_bias / set_residual, include/hnh_gat_skip.h; tests/gat_skip_ref.py is the
definition).

* Residual "none" and no bias: gat_skip_ref computes gat_ref's (scores dot and additive, with and without dropout) and gat_v2_ref's
  forward and backward bit for bit on the siblings' fd_problem.
* The reference backward against central finite differences on the three-layer model (12, 8, 2) projection, (16, 8, 2) identity,
  (16, 5, 3) projection, a bias on every layer, activations elu, elu, identity, score additive and gatv2: every dW, da, db, dW_res and
  probes of dX at the siblings' step and bound (1e-6, 1e-6), the LeakyReLU inputs at least 100 steps from 0.  Checked on the inputs: a
  quarter of the hidden pre-activations negative, every gradient with a nonzero entry, |r + b| > |o| on a tenth of the units at least (a
  backward pass that forgets to take the addend out of the recovered pre-activation fails: test_forgetting_the_addend_fails).
* The recovery: dZ (phi^{-1}(out) - addend) from the stored output, as hnh_skip_grad_cols_f64 forms it, over the sibling test's range of o
  and addends in [-2, 2], against np.longdouble from the true o (see test_recovery_with_an_addend for the bound).
* Declarations: the group is declared in include/hnh_gat_skip.h, bound, exported by the HIP library and absent from hnh_kernels.h and
  from the CPU test double; the pinned struct sizes are unchanged; on the test double forwardPass with a bias or a residual raises,
  naming the missing symbol, before anything runs; identity at mismatched widths, attention none, a wrong schedule, bad layers, bad mode
  names and wrong shapes raise; an object with everything off behaves as before."""
import ctypes as C

import numpy as np
import pytest

import gat_ref as R
import gat_skip_ref as S
import gat_v2_ref as V
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared, fd_problem, make_gat, plain_output

LAYERS = [(12, 8, 2), (16, 8, 2), (16, 5, 3)]
RESIDUAL = ("projection", "identity", "projection")
ACTS = ("elu", "elu", "identity")
STEP = 1e-6


def same_dicts(a, b):
    return a.keys() == b.keys() and all(all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) if isinstance(a[k], tuple) else np.array_equal(a[k], b[k])
                                        for k in a)


# ------------------------------------------------------------------------------------------------ reduction to the existing references
@pytest.mark.parametrize("score", ["dot", "additive", "gatv2"])
@pytest.mark.parametrize("rates,seed", [((0.0, 0.0), 0), ((0.6, 0.3), 2)], ids=["no-dropout", "dropout"])
def test_everything_off_is_the_existing_reference_bit_for_bit(score, rates, seed):
    rows, cols, m, x, w, av, g = fd_problem()
    layers, alpha = T.GAT_LAYERS, T.GAT_ALPHA
    if score != "additive":
        rates = (0.0, rates[1])  # (attention dropout: score additive only)
    for acts in (None, ("elu", "identity")):
        kw = dict(rates=rates, seed=seed, activations=acts)
        if score == "gatv2":
            want_out = V.forward(rows, cols, m, x, layers, alpha, w, av, **kw)
            want = V.backward(rows, cols, m, x, layers, alpha, g, w, av, **kw)
        else:
            vec = av if score == "additive" else None
            want_out = R.forward(rows, cols, m, x, layers, alpha, w, vec, attention="softmax", score=score, **kw)
            want = R.backward(rows, cols, m, x, layers, alpha, g, w, vec, attention="softmax", score=score, **kw)
        for off in (dict(), dict(residual="none", bias=None), dict(residual=("none", "none"), bias={})):
            vec = av if score != "dot" else None
            assert np.array_equal(S.forward(rows, cols, m, x, layers, alpha, w, vec, score=score, **kw, **off), want_out)
            dw, da, db, dwr, dx = S.backward(rows, cols, m, x, layers, alpha, g, w, vec, score=score, **kw, **off)
            assert same_dicts(dw, want[0]) and same_dicts(da, want[1]) and np.array_equal(dx, want[2]) and db == {} and dwr == {}


# ------------------------------------------------------------------------------------------------ finite differences
def fd_model(score):
    """fd_problem's graph under the three-layer model; x, the parameters, the biases and W_res drawn from the first seed at which every
    LeakyReLU input is at least 200 steps from 0 (score gatv2 has one per edge and feature)."""
    rows, cols, m, _, _, _, _ = fd_problem()
    g = np.random.default_rng(9).uniform(-1, 1, (m, LAYERS[-1][1] * LAYERS[-1][2]))
    for seed in range(400):
        rng = np.random.default_rng(2000 + seed)
        x = rng.uniform(-1, 1, (m, LAYERS[0][0]))
        w = {(li, h): rng.standard_normal((fin, fph)) / np.sqrt(fin) for li, (fin, fph, heads) in enumerate(LAYERS) for h in range(heads)}
        av = {(li, h): (rng.standard_normal(fph), rng.standard_normal(fph)) for li, (fin, fph, heads) in enumerate(LAYERS) for h in range(heads)}
        if score == "gatv2":
            av = {k: v[0] for k, v in av.items()}
        bias = {li: rng.uniform(-1, 1, fph * heads) for li, (fin, fph, heads) in enumerate(LAYERS)}
        wr = {li: rng.standard_normal((fin, fph * heads)) / np.sqrt(fin) for li, (fin, fph, heads) in enumerate(LAYERS) if RESIDUAL[li] == "projection"}
        mode = dict(score=score, activations=ACTS, residual=RESIDUAL)
        pre = S.pre_activations(rows, cols, m, x, LAYERS, T.GAT_ALPHA, w, av, bias=bias, res_weights=wr, **mode)
        if min(np.abs(k).min() for k, _, _ in pre) >= 200 * STEP:
            return rows, cols, m, x, w, av, bias, wr, g, mode
    raise AssertionError("no seed keeps every LeakyReLU input 200 steps from 0")


def check_conditions(pre, grads):
    hidden = np.concatenate([(o + add).reshape(-1) for _, o, add in pre[:-1]])
    share = np.count_nonzero(hidden < 0) / hidden.size
    o_all, add_all = (np.concatenate([p[i].reshape(-1) for p in pre]) for i in (1, 2))
    dominated = np.count_nonzero(np.abs(add_all) > np.abs(o_all)) / o_all.size
    print("negative share of the hidden pre-activations %.3f, share of units with |r + b| > |o| %.3f" % (share, dominated))
    assert share >= 0.25 and dominated >= 0.10
    dw, da, db, dwr, dx = grads
    flat = list(dw.values()) + [v for p in da.values() for v in (p if isinstance(p, tuple) else (p,))] + list(db.values()) + list(dwr.values()) + [dx]
    assert all(np.abs(v).max() > 0 for v in flat), "every gradient has a nonzero entry"
    assert set(db) == {0, 1, 2} and set(dwr) == {0, 2}


def fd_check(score, backward):
    """central differences of L = <g, out> against `backward`'s gradients: the worst relative error over every parameter tensor and dX"""
    rows, cols, m, x, w, av, bias, wr, g, mode = fd_model(score)
    alpha = T.GAT_ALPHA

    def fwd(ww, aa, bb, rr, xx, **kw):
        return S.forward(rows, cols, m, xx, LAYERS, alpha, ww, aa, bias=bb, res_weights=rr, **mode, **kw)

    def loss(*p):
        return float(np.sum(g * fwd(*p)))

    def margin_ok(ww, aa, bb, rr, xx, steps=100):
        pre = S.pre_activations(rows, cols, m, xx, LAYERS, alpha, ww, aa, bias=bb, res_weights=rr, **mode)
        return min(np.abs(k).min() for k, _, _ in pre) >= steps * STEP

    base = (w, av, bias, wr, x)
    assert margin_ok(*base)
    grads = backward(rows, cols, m, x, LAYERS, alpha, g, w, av, bias=bias, res_weights=wr, **mode)
    check_conditions(S.pre_activations(rows, cols, m, x, LAYERS, alpha, w, av, bias=bias, res_weights=wr, **mode), grads)
    dw, da, db, dwr, dx = grads
    rng = np.random.default_rng(3)
    errs = {}

    def fd_of(slot, key, which, probes):
        res = []
        for idx in probes:
            pair = []
            for h in (STEP, -STEP):
                p = list(base)
                if slot == 4:
                    p[4] = x.copy()
                    p[4][idx] += h
                else:
                    p[slot] = dict(base[slot])
                    if which is None:
                        p[slot][key] = base[slot][key].copy()
                        p[slot][key][idx] += h
                    else:
                        vecs = [v.copy() for v in base[slot][key]]
                        vecs[which][idx] += h
                        p[slot][key] = tuple(vecs)
                assert margin_ok(*p, steps=99)
                pair.append(loss(*p))
            res.append((pair[0] - pair[1]) / (2 * STEP))
        return np.array(res)

    def probes_of(shape, n=3):
        return [tuple(0 for _ in shape), tuple(s - 1 for s in shape)] + [tuple(int(rng.integers(0, s)) for s in shape) for _ in range(n)]

    for key, wk in w.items():
        pr = probes_of(wk.shape)
        an = np.array([dw[key][i] for i in pr])
        errs[("dw",) + key] = np.max(np.abs(fd_of(0, key, None, pr) - an)) / np.max(np.abs(dw[key]))
    for key, v in av.items():
        for which in ((0, 1) if isinstance(v, tuple) else (None,)):
            an = da[key] if which is None else da[key][which]
            pr = [(i,) for i in range(len(an))]
            errs[("da", which) + key] = np.max(np.abs(fd_of(1, key, which, pr) - an)) / np.max(np.abs(an))
    for li, b in bias.items():
        pr = [(i,) for i in range(len(b))]
        errs[("db", li)] = np.max(np.abs(fd_of(2, li, None, pr) - db[li])) / np.max(np.abs(db[li]))
    for li, r in wr.items():
        pr = probes_of(r.shape, 6)
        an = np.array([dwr[li][i] for i in pr])
        errs[("dwr", li)] = np.max(np.abs(fd_of(3, li, None, pr) - an)) / np.max(np.abs(dwr[li]))
    pr = probes_of(x.shape, 6)
    an = np.array([dx[i] for i in pr])
    errs["dx"] = np.max(np.abs(fd_of(4, None, None, pr) - an)) / np.max(np.abs(dx))
    return errs


@pytest.mark.parametrize("score", ["additive", "gatv2"])
def test_reference_backward_matches_finite_differences(score):
    errs = fd_check(score, S.backward)
    print("observed worst finite-difference error (%s) %.2e" % (score, max(errs.values())))
    assert max(errs.values()) <= 1e-6, errs


def test_forgetting_the_addend_fails():
    """The same check on a backward pass whose delta is taken against the recovered pre-activation o + r + b instead of o
    (gat_skip_ref.backward(forget_addend=True), the mistake a backward pass without hnh_skip_grad_cols_f64 would make): it must miss the
    bound by far, or the model above would not tell the two apart."""
    errs = fd_check("additive", lambda *a, **kw: S.backward(*a, forget_addend=True, **kw))
    print("a backward pass that forgets the addend: worst finite-difference error %.2e" % max(errs.values()))
    assert max(errs.values()) > 1e-3


# ------------------------------------------------------------------------------------------------ the recovery
def recovery_inputs():
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-300, -1e-300, 1e-17, -1e-17])
    rng = np.random.default_rng(0)
    return np.concatenate([np.linspace(-800.0, 5.0, 20001), tiny, rng.uniform(-1e-3, 1e-3, 2000), -np.logspace(-16, 2.9, 2000),
                           np.array([-36.0, -36.7368005696771, -37.0, -37.5, -40.0, -745.0, -746.0])])


@pytest.mark.parametrize("name", ["elu", "identity", "relu"])
def test_recovery_with_an_addend(name):
    """pre = o + addend in fp64 (what the finishing launch forms), out = phi(pre), then dZ / G and dZ (phi^{-1}(out) - addend) / G from out
    and the addend alone, against np.longdouble from the TRUE o: dZ_true = phi'(o + addend), term_true = dZ_true o.

    The bound.  The sibling's 1e-13 covers the recovery of the pre-activation from the stored output.  New here: the forward sum
    o + addend is rounded once (relative 2^-53 of |pre| <= |o| + |addend|), and subtracting the addend from the recovered value gives
    that rounding back as an ABSOLUTE error of o, weighted by dZ <= 1.  Where dZ is of order one (pre > -1, say) |o| <= 1 + max|addend|,
    so the sibling's bound scales by (1 + max|addend|); where |o| is large, dZ = exp(pre) is tiny and the product stays far below.
    Observed here: elu dZ/G 1.1e-16, term/G 2.0e-15; identity term/G 1.1e-13 (o reaches 800 there: 800 * 2^-53 = 8.9e-14 from the one
    rounding of the forward sum, which no backward pass can undo; within 3e-13); relu 4.4e-16."""
    ld = np.longdouble
    o = recovery_inputs()
    rng = np.random.default_rng(1)
    addend = rng.uniform(-2.0, 2.0, o.shape)
    addend[:50] = 0.0
    addend[50:60] = [2.0, -2.0, 1.0, -1.0, 0.5, -0.0, 1e-300, -1e-300, 2.0, -2.0]
    pre = o + addend
    out = R.act(pre, name)
    assert not np.any(np.isnan(out))
    if name == "elu":
        assert np.count_nonzero(out == -1.0) > 0, "saturated units are part of the sample"
    g = np.ones_like(o)
    dz, term = S.stored_grad(g[None, :].T, out[None, :].T, name, addend[None, :].T)
    dz = dz[:, 0]
    assert not np.any(np.isnan(dz)) and not np.any(np.isnan(term))
    pre_ld = o.astype(ld) + addend.astype(ld)
    if name == "elu":
        want_dz = np.where(pre_ld > 0, ld(1), np.exp(np.minimum(pre_ld, 0)))
    else:
        want_dz = np.ones_like(pre_ld) if name == "identity" else np.where(pre > 0, ld(1), ld(0))  # (relu: the side the fp64 forward took)
    dz_err = float(np.max(np.abs(dz.astype(ld) - want_dz)))
    term_err = float(np.max(np.abs(term.astype(ld) - want_dz * o.astype(ld))))
    bound = 1e-13 * (1.0 + np.abs(addend).max())
    print("observed absolute errors (%s): dZ/G %.2e, dZ o/G %.2e, bound %.2e" % (name, dz_err, term_err, bound))
    assert dz_err <= bound and term_err <= bound
    # the extended twin of the helper agrees, and dZ is the sibling helper's
    dz_l, term_l = S.stored_grad(g[None, :].T, out[None, :].T, name, addend[None, :].T, ld)
    assert dz_l.dtype == ld and np.max(np.abs(dz_l[:, 0] - dz)) <= 1e-13 and np.max(np.abs(term_l - term)) <= bound
    assert np.array_equal(dz, R.stored_grad(g[None, :].T, out[None, :].T, name)[0][:, 0]), "dZ depends on G and out only"


def test_stored_grad_equals_the_definition_on_the_model():
    rows, cols, m, x, w, av, bias, wr, g, mode = fd_model("additive")
    _, trace = S.forward(rows, cols, m, x, LAYERS, T.GAT_ALPHA, w, av, bias=bias, res_weights=wr, keep_trace=True, **mode)
    res = S.residuals_of(LAYERS, RESIDUAL)
    for li, (_, fph, heads) in enumerate(LAYERS):
        xd, _, out, heads_t = trace[li]
        add = S.addend_of(xd, li, res, bias, wr)
        gg = np.random.default_rng(li).uniform(-1, 1, out.shape)
        for h in range(heads):
            sl = slice(h * fph, (h + 1) * fph)
            o = heads_t[h][3]
            dz_s, dl_s = S.stored_grad(gg[:, sl], out[:, sl], ACTS[li], add[:, sl])
            dz_t, _ = R.true_grad(gg[:, sl], o + add[:, sl], out[:, sl], ACTS[li])
            assert np.max(np.abs(dz_s - dz_t)) <= 1e-13 and np.max(np.abs(dl_s - np.sum(dz_t * o, axis=1))) <= 1e-13 * fph * (1 + np.abs(add).max())


# ------------------------------------------------------------------------------------------------ declarations and refusals
SKIP_SYMBOLS = ("hnh_skip_addend_cols_f64", "hnh_skip_grad_cols_f64", "hnh_colsum_f64_workspace", "hnh_colsum_f64")
HOST_CALLS = ("hnh_gat_set_residual", "hnh_gat_set_residual_weight", "hnh_gat_get_residual_weight", "hnh_gat_get_residual_weight_grad", "hnh_gat_set_bias",
              "hnh_gat_get_bias", "hnh_gat_get_bias_grad")


def test_new_symbols_are_declared_bound_and_exported():
    lib = K.load()  # the HIP library: dlopen needs no GPU
    double = C.CDLL(T.ORACLE_BACKEND)
    for n in SKIP_SYMBOLS:
        assert n in declared("hnh_gat_skip.h") and n in K.SKIP_SIGNATURES and n not in K.SIGNATURES
        assert getattr(lib, n).argtypes == K.SKIP_SIGNATURES[n][1]
        assert n not in declared("hnh_kernels.h") and not hasattr(double, n), "the group stays out of hnh_kernels.h and of the CPU test double"
    assert set(K.SKIP_SIGNATURES) == set(SKIP_SYMBOLS)
    for n in HOST_CALLS:
        assert n in declared("hnh_dist.h") and n in H.SIGNATURES and hasattr(H.lib(), n)
    txt = open(ROOT + "/include/hnh_gat_skip.h").read()
    assert "#define HNH_ATTN_ADDEND 0x%xu" % K.ATTN_ADDEND in txt and K.ATTN_ADDEND == 0x40
    used = K.FUSED_VALUES_OVERWRITE | K.FUSED_OUT_OVERWRITE | K.FUSED_LEAKY_RELU | K.ATTN_FINISH | K.ATTN_ACT_ELU | K.ATTN_ACT_IDENTITY | 0x100 | 0x200 | (0x1f << 16)
    assert K.ATTN_ADDEND & used == 0
    dist = open(ROOT + "/include/hnh_dist.h").read()
    for name, code in H.GAT.RESIDUAL.items():
        assert "#define HNH_GAT_RESIDUAL_%s %d" % (name.upper(), code) in dist
    assert C.sizeof(K.AttnAdd) == 144 and C.sizeof(K.AttnState) == 48 and C.sizeof(K.AttnV2) == 152, "no struct changes size"


def test_bias_and_residual_on_the_test_double():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")
    layers = [(16, 8, 2), (16, 4, 3)]  # (layer 0: input_features == heads * features_per_head)
    nl = len(layers)

    def rank(world):
        for bad in (dict(residual="skip"), dict(residual=("identity",)), dict(bias=(True,)), dict(residual=("none", "identity"))):
            with pytest.raises((ValueError, H.HnhError)):  # (the last: layer 1 has 16 inputs and 12 outputs, refused by the library)
                make_gat(world, case, "15d_fusion2", 1, layers=layers, **bad)
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, layers=layers, attention="softmax", bias=(True, False))
        g = H.Dense.create(world, *gnn.buffer_shape(nl))
        for call in (gnn.forwardPass, lambda: gnn.backwardPass(g)):
            with pytest.raises(H.HnhError, match=r"bias of layer 0.*hnh_skip_addend_cols_f64.*include/hnh_gat_skip\.h"):
                call()
        gnn.set_bias(0, None)
        gnn.set_residual(1, "projection")
        with pytest.raises(H.HnhError, match=r"residual projection of layer 1.*hnh_skip_addend_cols_f64"):
            gnn.forwardPass()
        gnn.set_residual(1, "none")
        gnn.set_residual(0, "identity")
        with pytest.raises(H.HnhError, match=r"residual identity of layer 0.*hnh_skip_addend_cols_f64"):
            gnn.forwardPass()
        gnn.set_attention("none")
        with pytest.raises(H.HnhError, match=r"residual identity of layer 0.*attention mode softmax only"):
            gnn.forwardPass()
        world.sync()  # nothing was launched
        with pytest.raises(H.HnhError, match=r"residual identity of layer 1.*input_features"):
            gnn.set_residual(1, "identity")
        assert H.lib().hnh_gat_set_residual(gnn.h, 1, 1) != 0
        for bad in ("skip", "", None, 1):
            with pytest.raises(ValueError):
                gnn.set_residual(0, bad)
        for layer in (-1, 2, 7):
            for call in (lambda: gnn.set_residual(layer, "projection"), lambda: gnn.set_bias(layer, np.zeros(16)), lambda: gnn.get_bias(layer),
                         lambda: gnn.bias_grad(layer), lambda: gnn.set_residual_weight(layer, np.zeros((16, 16))), lambda: gnn.get_residual_weight(layer),
                         lambda: gnn.residual_weight_grad(layer)):
                with pytest.raises(ValueError):
                    call()
            assert H.lib().hnh_gat_set_residual(gnn.h, layer, 2) != 0 and H.lib().hnh_gat_set_bias(gnn.h, layer, None) != 0
            buf = np.zeros(16 * 16)
            for name in ("hnh_gat_get_bias", "hnh_gat_get_bias_grad", "hnh_gat_get_residual_weight", "hnh_gat_get_residual_weight_grad", "hnh_gat_set_residual_weight"):
                assert getattr(H.lib(), name)(gnn.h, layer, buf.ctypes.data) != 0, "a layer out of range is refused by the C ABI too"
        assert H.lib().hnh_gat_set_residual(gnn.h, 0, 3) != 0 and H.lib().hnh_gat_set_residual(gnn.h, 0, -1) != 0
        for shape in ((15,), (16, 1), (17,)):
            with pytest.raises(ValueError):
                gnn.set_bias(0, np.zeros(shape))
        for shape in ((16, 12), (12, 16), (16 * 16,)):
            with pytest.raises(ValueError):
                gnn.set_residual_weight(0, np.zeros(shape))
        # parameters can be set and read back without a kernel of the group
        b = np.arange(16.0)
        gnn.set_bias(0, b)
        assert np.array_equal(gnn.get_bias(0), b)
        gnn.set_bias(0, None)
        with pytest.raises(H.HnhError, match="no bias"):
            gnn.get_bias(0)
        with pytest.raises(H.HnhError, match="no residual weight"):
            gnn.get_residual_weight(0)  # (layer 0 was never a projection)
        gnn.set_residual(1, "projection")
        assert np.all(gnn.get_residual_weight(1) == 0.0), "W_res is zero until set"
        wr = np.arange(16.0 * 12).reshape(16, 12)
        gnn.set_residual_weight(1, wr)
        assert np.array_equal(gnn.get_residual_weight(1), wr)
        for call in (lambda: gnn.bias_grad(0), lambda: gnn.residual_weight_grad(1)):
            with pytest.raises(H.HnhError, match="gradient yet"):
                call()
        for h in (g, gnn, d, sp):
            h.free()
        # the wrong schedule names itself
        sp, d, gnn = make_gat(world, case, "15d_fusion1", 1, layers=layers, attention="softmax", bias=True)
        with pytest.raises(H.HnhError, match=r"bias of layer 0.*15d_fusion1.*c = 1"):
            gnn.forwardPass()
        for h in (gnn, d, sp):
            h.free()
        return True

    def everything_off(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, residual="none", bias=False)
        gnn.set_bias(0, np.ones(T.GAT_LAYERS[0][1] * T.GAT_LAYERS[0][2]))
        gnn.set_residual(1, "projection")
        gnn.set_bias(0, None)  # switched on and off again: the plain GAT (attention none), on the test double
        gnn.set_residual(1, "none")
        gnn.forwardPass()
        out = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.get_output(out)
        res = out.download()
        for h in (out, gnn, d, sp):
            h.free()
        return res

    assert all(H.run_spmd(2, rank))
    got, want = H.run_spmd(2, everything_off), H.run_spmd(2, lambda world: plain_output(world, case))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
