"""The GAT's layer normalisation without a GPU (GAT.set_norm, include/hnh_gat_norm.h; tests/gat_norm_ref.py is the definition).

* The norm's own backward pass (dz, dgamma, dbeta) against central finite differences in np.longdouble, three activations, plain and
  shifted rows; through a two-layer model (norm, bias and a projection on both layers, elu then identity, scores additive and transformer)
  every dW, da, dW_q, dW_k, db, dW_res, dgamma, dbeta and probes of dX against central differences of the fp64 model at the siblings' step
  and bound (1e-6, 1e-6; the model's sparse products are fp64), the LeakyReLU inputs at least 100 steps from 0.
* With the norm off the model computes gat_skip_ref's and gat_qkv_ref's forward and backward bit for bit.
* Declarations: the group is declared in include/hnh_gat_norm.h, bound, exported by the HIP library and absent from hnh_kernels.h and from
  the CPU test double; the host calls are declared in include/hnh_dist.h and bound.
* Every host refusal, on the test double: an unknown mode, a layer out of range, eps <= 0 or not finite, gamma / beta of the wrong length,
  attention none, a schedule other than 15d_fusion2 with c = 1, rows wider than the limit; a normalised layer's forwardPass names the missing
  symbol and launches nothing; a model with norm="none" on every layer is bit-equal to one constructed without the keyword."""
import ctypes as C

import numpy as np
import pytest

import gat_norm_ref as N
import gat_qkv_ref as Q
import gat_skip_ref as S
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared, fd_problem, make_gat, plain_output

LD = np.longdouble
LAYERS = [(12, 8, 2), (16, 5, 3)]
ACTS = ("elu", "identity")
RESIDUAL = ("projection", "projection")
STEP = 1e-6


# ------------------------------------------------------------------------------------------------ the norm against finite differences
@pytest.mark.parametrize("name", ["relu", "elu", "identity"])
@pytest.mark.parametrize("shift", [0.0, 1000.0])
def test_norm_backward_matches_finite_differences_in_longdouble(name, shift):
    """L = <g, out>.  Central differences at h = 1e-5 in np.longdouble (eps64 where longdouble is fp64: the bound below then still holds
    for h = 1e-5, rounding 1e-16 / 1e-5 = 1e-11): truncation h^2 |L'''| ~ 1e-10 of gradients of order one; bound 1e-7, relative to the
    largest entry.  relu: the draw keeps every |y| above 1e-3, a hundred steps from the kink."""
    rows, cols_, eps, h = 7, 10, 1e-5, LD(1e-5)
    for seed in range(200):
        rng = np.random.default_rng(seed)
        z = (shift + rng.uniform(-1, 1, (rows, cols_))).astype(LD)
        gamma, beta = rng.uniform(0.5, 1.5, cols_).astype(LD), rng.uniform(-1, 1, cols_).astype(LD)
        if np.abs(N.ln_forward(z, gamma, beta, eps, name, LD)[3]).min() > 1e-3:
            break
    else:
        raise AssertionError("no draw keeps y away from 0")
    g = rng.uniform(-1, 1, (rows, cols_)).astype(LD)
    dz, dgamma, dbeta, _ = N.ln_backward(g, z, gamma, beta, eps, name, LD)
    assert dz.dtype == LD and dgamma.dtype == LD

    def loss(zz, ga, be):
        return np.sum(g * N.ln_forward(zz, ga, be, eps, name, LD)[0])

    def fd(which, idx):
        args = [z.copy(), gamma.copy(), beta.copy()], [z.copy(), gamma.copy(), beta.copy()]
        args[0][which][idx] += h
        args[1][which][idx] -= h
        return (loss(*args[0]) - loss(*args[1])) / (2 * h)

    errs = {}
    for which, an, label in ((0, dz, "dz"), (1, dgamma, "dgamma"), (2, dbeta, "dbeta")):
        num = np.array([fd(which, idx) for idx in np.ndindex(an.shape)], dtype=LD).reshape(an.shape)
        errs[label] = float(np.max(np.abs(num - an)) / np.max(np.abs(an)))
    print("observed finite-difference errors of the norm (%s, shift %g): %s" % (name, shift, errs))
    # (shifted rows: L is evaluated at |z| ~ 1e3, so where longdouble is no wider than fp64 the difference quotient itself carries
    # 1e3 eps / h; the extended type removes that)
    bound = 1e-7 if np.finfo(LD).eps < 1e-18 or shift == 0.0 else 1e-4
    assert max(errs.values()) <= bound, errs
    # the float64 twin agrees with the extended one
    dz64, dg64, db64, _ = N.ln_backward(np.float64(g), np.float64(z), np.float64(gamma), np.float64(beta), eps, name)
    assert dz64.dtype == np.float64 and np.max(np.abs(dz64 - dz)) <= 1e-9 * (1 + shift) and np.max(np.abs(dg64 - dgamma)) <= 1e-9 * (1 + shift)


def test_a_one_pass_variance_would_be_caught():
    """The shifted rows are what tells the two-pass variance from E[z^2] - mu^2: in fp64 the latter misses the forward bound of the GPU
    test by orders of magnitude, the former stays inside."""
    rng = np.random.default_rng(0)
    z = 1000.0 + rng.uniform(-1, 1, (5, 256))
    gamma, beta, eps = np.ones(256), np.zeros(256), 1e-5
    want, (mu, rstd), _, _ = N.ln_forward(z, gamma, beta, eps, "identity", LD)
    two = N.ln_forward(z, gamma, beta, eps, "identity")[0]
    var1 = np.mean(z * z, axis=1) - np.mean(z, axis=1) ** 2
    one = (z - np.mean(z, axis=1)[:, None]) / np.sqrt(var1 + eps)[:, None]
    bound = 32 * np.finfo(np.float64).eps * (1 + np.abs(z).max(axis=1) * rstd.astype(np.float64))
    assert np.all(np.max(np.abs(two - want), axis=1) <= bound)
    assert np.max(np.max(np.abs(one - want), axis=1) / bound) > 10


def model(score):
    """fd_problem's graph under the two-layer model: the first seed at which every LeakyReLU input is 200 steps from 0"""
    rows, cols, m, _, _, _, _ = fd_problem()
    g = np.random.default_rng(9).uniform(-1, 1, (m, LAYERS[-1][1] * LAYERS[-1][2]))
    for seed in range(400):
        rng = np.random.default_rng(3000 + seed)
        x = rng.uniform(-1, 1, (m, LAYERS[0][0]))
        heads = [(li, h, fin, fph) for li, (fin, fph, nh) in enumerate(LAYERS) for h in range(nh)]
        p = {"w": {(li, h): rng.standard_normal((fin, fph)) / np.sqrt(fin) for li, h, fin, fph in heads}}
        if score == "additive":
            p["av"] = {(li, h): (rng.standard_normal(fph), rng.standard_normal(fph)) for li, h, fin, fph in heads}
        else:
            p["wq"] = {(li, h): rng.standard_normal((fin, fph)) / np.sqrt(fin) for li, h, fin, fph in heads}
            p["wk"] = {(li, h): rng.standard_normal((fin, fph)) / np.sqrt(fin) for li, h, fin, fph in heads}
        p["bias"] = {li: rng.uniform(-1, 1, fph * nh) for li, (fin, fph, nh) in enumerate(LAYERS)}
        p["wr"] = {li: rng.standard_normal((fin, fph * nh)) / np.sqrt(fin) for li, (fin, fph, nh) in enumerate(LAYERS)}
        p["gamma"] = {li: rng.uniform(0.5, 1.5, fph * nh) for li, (fin, fph, nh) in enumerate(LAYERS)}
        p["beta"] = {li: rng.uniform(-1, 1, fph * nh) for li, (fin, fph, nh) in enumerate(LAYERS)}
        mode = dict(score=score, activations=ACTS, residual=RESIDUAL, norm="layer")
        if score != "additive" or kink_margin(rows, cols, m, x, p, mode) >= 200 * STEP:
            return rows, cols, m, x, p, g, mode
    raise AssertionError("no seed keeps every LeakyReLU input 200 steps from 0")


def kink_margin(rows, cols, m, x, p, mode):
    _, trace = N.forward(rows, cols, m, x, LAYERS, T.GAT_ALPHA, p, keep_trace=True, **mode)
    return min(np.abs(ht[1]).min() for t in trace for ht in t[3])


@pytest.mark.parametrize("score", ["additive", "transformer"])
def test_model_backward_matches_finite_differences(score):
    rows, cols, m, x, p, g, mode = model(score)
    alpha = T.GAT_ALPHA
    grads = N.backward(rows, cols, m, x, LAYERS, alpha, g, p, **mode)
    assert set(grads) == set(p) | {"x"} and set(grads["gamma"]) == {0, 1} and set(grads["beta"]) == {0, 1}
    rng = np.random.default_rng(3)

    def loss(pp, xx):
        if score == "additive":
            assert kink_margin(rows, cols, m, xx, pp, mode) >= 99 * STEP
        return float(np.sum(g * N.forward(rows, cols, m, xx, LAYERS, alpha, pp, **mode)))

    def probes_of(shape, n=3):
        if len(shape) == 1:
            return [(i,) for i in range(shape[0])]
        return [tuple(0 for _ in shape), tuple(s - 1 for s in shape)] + [tuple(int(rng.integers(0, s)) for s in shape) for _ in range(n)]

    errs = {}
    for kind, tensors in p.items():
        for key, value in tensors.items():
            for part in (range(len(value)) if isinstance(value, tuple) else (None,)):
                an = grads[kind][key] if part is None else grads[kind][key][part]
                assert np.abs(an).max() > 0, "every gradient has a nonzero entry"
                num = []
                pr = probes_of(an.shape)
                for idx in pr:
                    pair = []
                    for hh in (STEP, -STEP):
                        pp = {k: dict(v) for k, v in p.items()}
                        if part is None:
                            pp[kind][key] = value.copy()
                            pp[kind][key][idx] += hh
                        else:
                            vecs = [v.copy() for v in value]
                            vecs[part][idx] += hh
                            pp[kind][key] = tuple(vecs)
                        pair.append(loss(pp, x))
                    num.append((pair[0] - pair[1]) / (2 * STEP))
                errs[(kind, key, part)] = float(np.max(np.abs(np.array(num) - np.array([an[i] for i in pr]))) / np.abs(an).max())
    pr = probes_of(x.shape, 6)
    num = []
    for idx in pr:
        xp, xm = x.copy(), x.copy()
        xp[idx] += STEP
        xm[idx] -= STEP
        num.append((loss(p, xp) - loss(p, xm)) / (2 * STEP))
    errs["x"] = float(np.max(np.abs(np.array(num) - np.array([grads["x"][i] for i in pr]))) / np.abs(grads["x"]).max())
    print("observed worst finite-difference error of the normalised model (%s) %.2e" % (score, max(errs.values())))
    assert max(errs.values()) <= 1e-6, errs


def test_norm_off_is_the_existing_references_bit_for_bit():
    rows, cols, m, x, p, g, mode = model("additive")
    alpha = T.GAT_ALPHA
    off = dict(mode, norm=None)
    kw = dict(score="additive", activations=ACTS, residual=RESIDUAL, bias=p["bias"], res_weights=p["wr"])
    assert np.array_equal(N.forward(rows, cols, m, x, LAYERS, alpha, p, **off), S.forward(rows, cols, m, x, LAYERS, alpha, p["w"], p["av"], **kw))
    got = N.backward(rows, cols, m, x, LAYERS, alpha, g, p, **off)
    dw, da, db, dwr, dx = S.backward(rows, cols, m, x, LAYERS, alpha, g, p["w"], p["av"], **kw)
    assert "gamma" not in got and np.array_equal(got["x"], dx)
    assert all(np.array_equal(got["w"][k], dw[k]) and all(np.array_equal(a, b) for a, b in zip(got["av"][k], da[k])) for k in dw)
    assert all(np.array_equal(got["bias"][k], db[k]) and np.array_equal(got["wr"][k], dwr[k]) for k in db)
    rows, cols, m, x, p, g, mode = model("transformer")
    kw = dict(activations=ACTS, residual=RESIDUAL, bias=p["bias"], res_weights=p["wr"])
    off = dict(mode, norm="none")
    assert np.array_equal(N.forward(rows, cols, m, x, LAYERS, alpha, p, **off), Q.forward(rows, cols, m, x, LAYERS, p["w"], p["wq"], p["wk"], **kw))
    got = N.backward(rows, cols, m, x, LAYERS, alpha, g, p, **off)
    dw, dq, dk, db, dwr, dx = Q.backward(rows, cols, m, x, LAYERS, g, p["w"], p["wq"], p["wk"], **kw)
    assert np.array_equal(got["x"], dx)
    assert all(np.array_equal(got["w"][k], dw[k]) and np.array_equal(got["wq"][k], dq[k]) and np.array_equal(got["wk"][k], dk[k]) for k in dw)


# ------------------------------------------------------------------------------------------------ declarations and refusals
NORM_SYMBOLS = ("hnh_layernorm_fwd_f64", "hnh_layernorm_bwd_workspace", "hnh_layernorm_bwd_f64")
HOST_CALLS = ("hnh_gat_set_norm", "hnh_gat_set_norm_weights", "hnh_gat_get_norm_weights", "hnh_gat_get_norm_grad")


def test_new_symbols_are_declared_bound_and_exported():
    lib = K.load()  # the HIP library: dlopen needs no GPU
    double = C.CDLL(T.ORACLE_BACKEND)
    for n in NORM_SYMBOLS:
        assert n in declared("hnh_gat_norm.h") and n in K.NORM_SIGNATURES and n not in K.SIGNATURES
        assert getattr(lib, n).argtypes == K.NORM_SIGNATURES[n][1] and getattr(lib, n).restype == K.NORM_SIGNATURES[n][0]
        assert n not in declared("hnh_kernels.h") and not hasattr(double, n), "the group stays out of hnh_kernels.h and of the CPU test double"
    assert set(K.NORM_SIGNATURES) == set(NORM_SYMBOLS)
    for table in (K.SIGNATURES, K.GRAD_SIGNATURES, K.SKIP_SIGNATURES, K.TRAIN_SIGNATURES, K.QKV_SIGNATURES):
        assert not set(NORM_SYMBOLS) & set(table), "disjoint from the existing tables"
    for n in HOST_CALLS:
        assert n in declared("hnh_dist.h") and n in H.SIGNATURES and hasattr(H.lib(), n)
    txt = open(ROOT + "/include/hnh_gat_norm.h").read()
    assert "#define HNH_NORM_MAX_COLS %d" % K.NORM_MAX_COLS in txt and K.NORM_MAX_COLS >= 14 * 256
    dist = open(ROOT + "/include/hnh_dist.h").read()
    for name, code in H.GAT.NORM.items():
        assert "#define HNH_GAT_NORM_%s %d" % (name.upper(), code) in dist
    assert H.GAT.NORM == {"none": 0, "layer": 1}
    # the workspace function needs no device: nothing for an empty or an unsupported problem, 2 cols doubles per row range otherwise
    ws = lib.hnh_layernorm_bwd_workspace
    assert ws(0, 8) == 0 and ws(8, 0) == 0 and ws(8, K.NORM_MAX_COLS + 1) == 0
    for rows, cols in ((1, 1), (257, 7), (5000, 768), (1 << 18, 256), (1 << 16, 3584)):
        got = ws(rows, cols)
        assert got > 0 and got % (2 * cols) == 0 and got // (2 * cols) <= max(1, (rows + 15) // 16)


def test_norm_on_the_test_double():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")
    layers = [(16, 8, 2), (16, 4, 3)]
    nl = len(layers)

    def rank(world):
        for bad in (dict(norm="batch"), dict(norm=("layer",)), dict(norm=("layer", "rms")), dict(norm=1)):
            with pytest.raises((ValueError, TypeError)):
                make_gat(world, case, "15d_fusion2", 1, layers=layers, **bad)
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, layers=layers, attention="softmax", norm=("layer", "none"))
        g = H.Dense.create(world, *gnn.buffer_shape(nl))
        for call in (gnn.forwardPass, lambda: gnn.backwardPass(g)):
            with pytest.raises(H.HnhError, match=r"norm layer of layer 0.*hnh_layernorm_fwd_f64.*include/hnh_gat_norm\.h"):
                call()
        gnn.set_norm(0, "none")
        gnn.set_norm(1, "layer", eps=1e-3)
        with pytest.raises(H.HnhError, match=r"norm layer of layer 1.*hnh_layernorm_fwd_f64"):
            gnn.forwardPass()
        gnn.set_attention("none")
        with pytest.raises(H.HnhError, match=r"norm layer of layer 1.*attention mode softmax only"):
            gnn.forwardPass()
        world.sync()  # nothing was launched
        # an unknown mode, a layer out of range, a bad eps, vectors of the wrong length: Python and the C ABI both refuse, and the object stays
        for bad in ("batch", "", None, 1):
            with pytest.raises(ValueError):
                gnn.set_norm(0, bad)
        assert H.lib().hnh_gat_set_norm(gnn.h, 0, 2, 1e-5) != 0 and H.lib().hnh_gat_set_norm(gnn.h, 0, -1, 1e-5) != 0
        for layer in (-1, 2, 7):
            for call in (lambda: gnn.set_norm(layer, "layer"), lambda: gnn.set_norm_weights(layer, np.ones(16), np.zeros(16)),
                         lambda: gnn.get_norm_weights(layer), lambda: gnn.norm_grad(layer)):
                with pytest.raises(ValueError):
                    call()
            buf = np.zeros(16)
            assert H.lib().hnh_gat_set_norm(gnn.h, layer, 1, 1e-5) != 0
            for name in ("hnh_gat_set_norm_weights", "hnh_gat_get_norm_weights", "hnh_gat_get_norm_grad"):
                assert getattr(H.lib(), name)(gnn.h, layer, buf.ctypes.data, buf.ctypes.data, 16) != 0, "a layer out of range is refused by the C ABI too"
        for eps in (0.0, -1e-5, float("inf"), float("nan")):
            with pytest.raises(ValueError):
                gnn.set_norm(0, "layer", eps=eps)
            assert H.lib().hnh_gat_set_norm(gnn.h, 0, 1, eps) != 0
        with pytest.raises(H.HnhError, match=r"layer 0.*positive finite eps"):
            H._check(H.lib().hnh_gat_set_norm(gnn.h, 0, 1, 0.0), "gat_set_norm")
        for shape in ((15,), (16, 1), (17,)):
            with pytest.raises(ValueError):
                gnn.set_norm_weights(0, np.ones(shape), np.zeros(shape))
        buf = np.ones(17)
        assert H.lib().hnh_gat_set_norm_weights(gnn.h, 0, buf.ctypes.data, buf.ctypes.data, 17) != 0
        assert H.lib().hnh_gat_set_norm_weights(gnn.h, 1, buf.ctypes.data, buf.ctypes.data, 16) != 0, "layer 1 has 12 values per row"
        assert H.lib().hnh_gat_set_norm_weights(gnn.h, 0, None, buf.ctypes.data, 16) != 0
        # gamma = 1 and beta = 0 until set; they can be set and read back without a kernel of the group; a refused call changed nothing
        ga, be = gnn.get_norm_weights(0)
        assert np.all(ga == 1.0) and np.all(be == 0.0)
        ga, be = np.arange(16.0), -np.arange(16.0)
        gnn.set_norm_weights(0, ga, be)
        got = gnn.get_norm_weights(0)
        assert np.array_equal(got[0], ga) and np.array_equal(got[1], be)
        with pytest.raises(H.HnhError, match="no GAT norm gradient of layer 0"):
            gnn.norm_grad(0)
        for h in (g, gnn, d, sp):
            h.free()
        # the wrong schedule names itself, and so does a row wider than the limit
        sp, d, gnn = make_gat(world, case, "15d_fusion1", 1, layers=layers, attention="softmax", norm="layer")
        with pytest.raises(H.HnhError, match=r"norm layer of layer 0.*15d_fusion1.*c = 1"):
            gnn.forwardPass()
        for h in (gnn, d, sp):
            h.free()
        wide = [(16, 257, 16)]  # 4112 values per row
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, layers=wide, attention="softmax", norm="layer")
        with pytest.raises(H.HnhError, match=r"norm layer of layer 0.*at most %d values.*4112" % K.NORM_MAX_COLS):
            gnn.forwardPass()
        world.sync()
        for h in (gnn, d, sp):
            h.free()
        return True

    def everything_off(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, norm="none")
        gnn.set_norm(0, "layer")
        gnn.set_norm_weights(0, 2.0 * np.ones(T.GAT_LAYERS[0][1] * T.GAT_LAYERS[0][2]), np.ones(T.GAT_LAYERS[0][1] * T.GAT_LAYERS[0][2]))
        gnn.set_norm(0, "none")  # switched on and off again: the plain GAT (attention none), on the test double
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
