"""The GAT's per-layer output activation without a GPU (GAT.set_activation; tests/gat_ref.py with `activations` is the definition).

* With "relu" on every layer, spelled out or left out, the reference computes the recorded results of the dropout reference it replaced
  (tests/golden/gat_ref_pinned.npz), with and without dropout.
* The reference backward against central finite differences on a two-layer model ("elu", then "identity"), rates (0, 0), for every dW, da1,
  da2 and dX at the sibling tests' step and bound (1e-6); the inputs are signed and at least a quarter of the hidden aggregates are negative.
  ELU is differentiable at 0 and the identity everywhere, so only the LeakyReLU inputs need the siblings' margin from 0.
* "identity" on the last layer with heads "mean": the loss is the cross-entropy of the mean of the raw head aggregates, the published
  output layer.
* The recovery from the stored output (out -> dZ / G and dZ o / G, what hnh_act_grad_cols_f64 computes) over o in [-800, 5] with +-0,
  the subnormal neighbourhood and |o| < 1e-3, against np.longdouble from the TRUE o: no NaN, absolute error <= 1e-13.
* The new symbols are declared, bound and exported; the structs keep their sizes; the CPU test double lacks hnh_act_grad_cols_f64, a
  non-ReLU layer on it is refused by forwardPass with that name before anything runs, bad names and layers raise, and the all-relu object
  behaves as before."""
import ctypes as C

import numpy as np
import pytest

import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared, fd_problem, make_gat, pinned_error, plain_output

ACTS = ("elu", "identity")  # the finite-difference model: hidden ELU, raw output
MODE = dict(attention="softmax", score="additive")
DOT = dict(attention="softmax", score="dot")


def test_all_relu_is_the_dropout_reference_bit_for_bit():
    rows, cols, m, x, w, av, g = fd_problem()
    layers, alpha = T.GAT_LAYERS, T.GAT_ALPHA
    for rates, seed, config in (((0.0, 0.0), 0, "softmax_additive"), ((0.6, 0.3), 2, "softmax_additive_dropout")):
        for acts in (None, "relu", ("relu", "relu")):
            kw = dict(MODE, rates=rates, seed=seed, activations=acts)
            out = R.forward(rows, cols, m, x, layers, alpha, w, av, **kw)
            assert pinned_error(config, out, *R.backward(rows, cols, m, x, layers, alpha, g, w, av, **kw)) <= 1e-13
    other = R.forward(rows, cols, m, x, layers, alpha, w, av, activations=ACTS, **MODE)
    assert not np.array_equal(other, R.forward(rows, cols, m, x, layers, alpha, w, av, **MODE)) and other.min() < 0
    assert pinned_error("softmax_additive_elu_identity", other, *R.backward(rows, cols, m, x, layers, alpha, g, w, av, activations=ACTS, **MODE)) <= 1e-13


def test_reference_backward_matches_finite_differences():
    rows, cols, m, x, w, av, g = fd_problem()  # (x uniform in [-1, 1], W normal: signed)
    layers, alpha, step = T.GAT_LAYERS, T.GAT_ALPHA, 1e-6
    hidden = np.concatenate([o.reshape(-1) for _, o in R.pre_activations(rows, cols, m, x, layers, alpha, w, av, activations=ACTS, **MODE)[0]])
    share = np.count_nonzero(hidden < 0) / hidden.size
    print("negative share of the hidden aggregates: %.3f" % share)
    assert share >= 0.25
    dws, das, dx = R.backward(rows, cols, m, x, layers, alpha, g, w, av, activations=ACTS, **MODE)

    def loss(ww, aa, xx):
        return float(np.sum(g * R.forward(rows, cols, m, xx, layers, alpha, ww, aa, activations=ACTS, **MODE)))

    def margin_ok(ww, aa, xx, steps=100):  # the LeakyReLU inputs stay on their side of 0 (the activations here are smooth)
        z = np.concatenate([z for layer in R.pre_activations(rows, cols, m, xx, layers, alpha, ww, aa, activations=ACTS, **MODE) for z, _ in layer])
        return np.abs(z).min() >= steps * step

    assert margin_ok(w, av, x)
    assert all(np.abs(a).max() > 0 and np.abs(b).max() > 0 for a, b in das.values())
    assert np.count_nonzero(dx) > dx.size // 2 and all(np.abs(d).max() > 0 for d in dws.values()), "the gradients must not be vacuous"

    def fd_of(perturb, probes):
        res = []
        for idx in probes:
            plus, minus = perturb(idx, step), perturb(idx, -step)
            assert margin_ok(*plus, steps=99) and margin_ok(*minus, steps=99)
            res.append((loss(*plus) - loss(*minus)) / (2 * step))
        return np.array(res)

    worst = 0.0
    rng = np.random.default_rng(3)
    for key, wk in w.items():
        probes = [(0, 0), (wk.shape[0] - 1, wk.shape[1] - 1)] + [tuple(rng.integers(0, s) for s in wk.shape) for _ in range(3)]

        def perturb(idx, h, key=key, wk=wk):
            ww = dict(w)
            ww[key] = wk.copy()
            ww[key][idx] += h
            return ww, av, x

        an = np.array([dws[key][idx] for idx in probes])
        err = np.max(np.abs(fd_of(perturb, probes) - an)) / np.max(np.abs(an))
        worst = max(worst, err)
        assert err <= 1e-6, (key, err)
    for key, (a1, a2) in av.items():
        for which in (0, 1):
            def perturb(idx, h, key=key, which=which):
                aa = dict(av)
                pair = [av[key][0].copy(), av[key][1].copy()]
                pair[which][idx] += h
                aa[key] = tuple(pair)
                return w, aa, x

            an = das[key][which]
            err = np.max(np.abs(fd_of(perturb, list(range(len(a1)))) - an)) / np.max(np.abs(an))
            worst = max(worst, err)
            assert err <= 1e-6, (key, which, err)
    probes = [(0, 0), (m - 1, x.shape[1] - 1)] + [tuple(rng.integers(0, s) for s in x.shape) for _ in range(4)]

    def perturb_x(idx, h):
        xx = x.copy()
        xx[idx] += h
        return w, av, xx

    an = np.array([dx[idx] for idx in probes])
    err = np.max(np.abs(fd_of(perturb_x, probes) - an)) / np.max(np.abs(an))
    print("observed worst finite-difference error %.2e" % max(worst, err))
    assert err <= 1e-6, err


def test_score_dot_reference_matches_the_softmax_reference_and_finite_differences():
    """score "dot": all-relu equals the recorded results of the softmax reference that tests/gat_ref.py replaced (1e-13: same maths, the
    matrix products' summation order may differ); elu / identity against central differences on two weights and two inputs."""
    rows, cols, m, x, w, _, g = fd_problem()
    layers, alpha, step = T.GAT_LAYERS, T.GAT_ALPHA, 1e-6
    assert pinned_error("softmax_dot", R.forward(rows, cols, m, x, layers, alpha, w, **DOT), *R.backward(rows, cols, m, x, layers, alpha, g, w, **DOT)) <= 1e-13
    dws, _, dx = R.backward(rows, cols, m, x, layers, alpha, g, w, activations=ACTS, **DOT)
    assert pinned_error("softmax_dot_elu_identity", R.forward(rows, cols, m, x, layers, alpha, w, activations=ACTS, **DOT), dws, {}, dx) <= 1e-13

    def loss(ww, xx):
        return float(np.sum(g * R.forward(rows, cols, m, xx, layers, alpha, ww, activations=ACTS, **DOT)))

    for key in ((0, 1), (1, 2)):
        for idx in ((0, 0), (3, 2)):
            wp, wm = dict(w), dict(w)
            wp[key], wm[key] = w[key].copy(), w[key].copy()
            wp[key][idx] += step
            wm[key][idx] -= step
            fd = (loss(wp, x) - loss(wm, x)) / (2 * step)
            assert abs(fd - dws[key][idx]) <= 1e-6 * np.abs(dws[key]).max(), (key, idx)
    for idx in ((0, 0), (17, 5)):
        xp, xm = x.copy(), x.copy()
        xp[idx] += step
        xm[idx] -= step
        assert abs((loss(w, xp) - loss(w, xm)) / (2 * step) - dx[idx]) <= 1e-6 * np.abs(dx).max(), idx


def test_identity_output_with_mean_heads_is_the_published_output_layer():
    layers = T.GAT_LAYERS
    pp = R.planted_partition(layers)
    args = (pp["rows"], pp["cols"], pp["m"], pp["x"], layers, T.GAT_ALPHA, pp["w"], pp["av"])
    out = R.forward(*args, activations=ACTS, **MODE)
    raw = [o for _, o in R.pre_activations(*args, activations=ACTS, **MODE)[-1]]
    nh = layers[-1][2]
    assert len(raw) == nh and min(o.min() for o in raw) < 0, "the raw class logits are signed"
    mean_raw = sum(raw) / nh
    loss, acc, _ = R.xent(out, pp["labels"], pp["mask"], nh)
    want, want_acc, _ = R.xent(mean_raw, pp["labels"], pp["mask"], 1)
    assert abs(loss - want) <= 1e-14 * abs(want) and acc == want_acc
    relu_loss, _, _ = R.xent(R.forward(*args, activations=("elu", "relu"), **MODE), pp["labels"], pp["mask"], nh)
    assert abs(relu_loss - want) > 1e-3, "a ReLU on the output layer computes another loss"


def recovery_inputs():
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-300, -1e-300, 1e-17, -1e-17])
    rng = np.random.default_rng(0)
    return np.concatenate([np.linspace(-800.0, 5.0, 20001), tiny, rng.uniform(-1e-3, 1e-3, 2000), -np.logspace(-16, 2.9, 2000),
                           np.array([-36.0, -36.7368005696771, -37.0, -37.5, -40.0, -745.0, -746.0])])


def test_recovery_from_the_stored_output():
    """out = elu(o) in fp64, then dZ / G and dZ o / G from out alone, against the true o in np.longdouble.  Absolute errors observed
    here: forward 5.6e-17, dZ / G 8.3e-17, dZ o / G 2.0e-15."""
    ld = np.longdouble
    o = recovery_inputs()
    out = R.act(o, "elu")
    assert not np.any(np.isnan(out)) and np.count_nonzero(out == -1.0) > 0, "saturated units are part of the sample"
    fwd_err = np.max(np.abs(out.astype(ld) - R.act_ld(o, "elu")))
    g = np.ones_like(o)
    dz, term = R.stored_grad(g[None, :].T, out[None, :].T, "elu")  # one column per row: delta_r is the row's single term
    dz = dz[:, 0]
    assert not np.any(np.isnan(dz)) and not np.any(np.isnan(term))
    want_dz = np.where(o > 0, ld(1), np.exp(np.minimum(o, 0).astype(ld)))
    dz_err = np.max(np.abs(dz.astype(ld) - want_dz))
    term_err = np.max(np.abs(term.astype(ld) - want_dz * o.astype(ld)))
    print("observed absolute errors: forward %.2e, dZ/G %.2e, dZ o/G %.2e" % (fwd_err, dz_err, term_err))
    assert fwd_err <= 1e-13 and dz_err <= 1e-13 and term_err <= 1e-13
    assert np.all(dz[out == -1.0] == 0.0) and np.all(term[out == -1.0] == 0.0)
    # the extended twin of the helper agrees with it, and identity / relu are exact
    dz_l, term_l = R.stored_grad_ld(g[None, :].T, out[None, :].T, "elu")
    assert dz_l.dtype == ld and np.max(np.abs(dz_l[:, 0] - dz)) <= 1e-13 and np.max(np.abs(term_l - term)) <= 1e-13
    for name in ("relu", "identity"):
        a, b = R.stored_grad(g[None, :].T, R.act(o, name)[None, :].T, name)
        want = np.where(o > 0, 1.0, 0.0) if name == "relu" else np.ones_like(o)
        assert np.array_equal(a[:, 0], want) and np.array_equal(b, want * o * (1.0 if name == "identity" else (o > 0)))


def test_stored_grad_equals_true_grad_on_the_model():
    rows, cols, m, x, w, av, g = fd_problem()
    _, trace = R.forward(rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, w, av, activations=("elu", "elu"), keep_trace=True, **MODE)
    for li, (_, fph, heads) in enumerate(T.GAT_LAYERS):
        out = trace[li][2]
        gg = np.random.default_rng(li).uniform(-1, 1, out.shape)
        for h in range(heads):
            sl = slice(h * fph, (h + 1) * fph)
            a = R.stored_grad(gg[:, sl], out[:, sl], "elu")
            b = R.true_grad(gg[:, sl], trace[li][3][h][3], out[:, sl], "elu")
            assert np.max(np.abs(a[0] - b[0])) <= 1e-13 and np.max(np.abs(a[1] - b[1])) <= 1e-13 * fph


def test_new_symbols_are_declared_bound_and_exported():
    assert "hnh_act_grad_cols_f64" in declared("hnh_grad.h") and "hnh_act_grad_cols_f64" in K.GRAD_SIGNATURES
    lib = K.load()  # the HIP library: dlopen needs no GPU
    assert lib.hnh_act_grad_cols_f64.argtypes == K.GRAD_SIGNATURES["hnh_act_grad_cols_f64"][1]
    assert "hnh_gat_set_activation" in declared("hnh_dist.h") and "hnh_gat_set_activation" in H.SIGNATURES and hasattr(H.lib(), "hnh_gat_set_activation")
    assert not hasattr(C.CDLL(T.ORACLE_BACKEND), "hnh_act_grad_cols_f64"), "the CPU test double does not export it"
    txt = open(ROOT + "/include/hnh_attention.h").read()
    assert "#define HNH_ATTN_ACT_ELU 0x%xu" % K.ATTN_ACT_ELU in txt and "#define HNH_ATTN_ACT_IDENTITY 0x%xu" % K.ATTN_ACT_IDENTITY in txt
    used = K.FUSED_VALUES_OVERWRITE | K.FUSED_OUT_OVERWRITE | K.FUSED_LEAKY_RELU | K.ATTN_FINISH | 0x100 | 0x200 | (0x1f << 16)
    assert K.ATTN_ACT_ELU & K.ATTN_ACT_IDENTITY == 0 and (K.ATTN_ACT_ELU | K.ATTN_ACT_IDENTITY) & used == 0 and max(K.ATTN_ACT_ELU, K.ATTN_ACT_IDENTITY) < 0x100
    assert (K.ACT_RELU, K.ACT_ELU, K.ACT_IDENTITY) == (0, 1, 2) == tuple(H.GAT.ACTIVATION[n] for n in ("relu", "elu", "identity"))
    assert C.sizeof(K.AttnAdd) == 144 and C.sizeof(K.AttnState) == 48, "no struct changes size"


def test_activation_on_the_test_double():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        with pytest.raises(ValueError):
            make_gat(world, case, "15d_fusion2", 1, activation="gelu")
        with pytest.raises(ValueError):
            make_gat(world, case, "15d_fusion2", 1, activation=("elu",))  # one name per layer: two layers
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, attention="softmax", activation=("elu", "identity"))
        g = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        for call in (gnn.forwardPass, lambda: gnn.backwardPass(g)):
            with pytest.raises(H.HnhError, match=r"activation elu of layer 0.*hnh_act_grad_cols_f64.*include/hnh_grad\.h"):
                call()
        gnn.set_activation(0, "relu")
        with pytest.raises(H.HnhError, match=r"activation identity of layer 1.*hnh_act_grad_cols_f64"):
            gnn.forwardPass()
        gnn.set_attention("none")
        with pytest.raises(H.HnhError, match=r"activation identity of layer 1.*attention mode softmax only"):
            gnn.forwardPass()
        world.sync()  # nothing was launched
        for bad in ("gelu", "", None):
            with pytest.raises(ValueError):
                gnn.set_activation(0, bad)
        for layer in (-1, 2, 7):
            with pytest.raises(ValueError):
                gnn.set_activation(layer, "elu")
            assert H.lib().hnh_gat_set_activation(gnn.h, layer, 1) != 0, "a layer out of range is refused by the C ABI too"
        assert H.lib().hnh_gat_set_activation(gnn.h, 0, 3) != 0 and H.lib().hnh_gat_set_activation(gnn.h, 0, -1) != 0
        gnn.set_activation(1, "relu")  # the process and the operator live on: the plain GAT on the same object
        gnn.forwardPass()
        out = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.get_output(out)
        res = out.download()
        for h in (out, g, gnn, d, sp):
            h.free()
        return res

    def spelled_out(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, activation="relu")
        gnn.forwardPass()
        out = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.get_output(out)
        res = out.download()
        for h in (out, gnn, d, sp):
            h.free()
        return res

    per_rank, named, want = H.run_spmd(2, rank), H.run_spmd(2, spelled_out), H.run_spmd(2, lambda world: plain_output(world, case))
    assert all(np.isfinite(r).all() for r in per_rank)
    assert all(np.array_equal(a, b) and np.array_equal(c, b) for a, b, c in zip(per_rank, want, named))
