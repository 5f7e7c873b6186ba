"""numpy reference of the GAT's layer normalisation (include/hnh_gat_norm.h; GAT.set_norm), next to tests/gat_skip_ref.py, tests/gat_v2_ref.py,
tests/gat_qkv_ref.py and tests/gat_edge_learn_ref.py, whose pieces it composes: the norm sits between those models' pre-activation and their
activation, for every score ("dot" | "additive" | "gatv2" | "transformer", the last with an optional, optionally learned, per-edge bias).

The norm of a row z (all heads side by side, C columns), gamma, beta, eps and an activation phi:
    mu = mean_c z    var = mean_c (z - mu)^2 (biased; the deviations are formed before they are squared)    rstd = 1 / sqrt(var + eps)
    xh = (z - mu) rstd    y = gamma xh + beta    out = phi(y)
    dY = G phi'(y)    dgamma = sum_r dY xh    dbeta = sum_r dY    t = gamma dY    dz = rstd (t - mean_c t - xh mean_c (t xh))
ln_forward / ln_backward take a dtype: np.longdouble gives the tests' yardstick.

The model.  Those modules' forward() and backward() apply the activation inside their layer loops and offer no seam between the
pre-activation and it, so this module holds its own layer loop around what they expose per head and per layer: gat_skip_ref._head (the
head's aggregate for the scores dot, additive and gatv2), gat_skip_ref.addend_of / residuals_of (r + b), gat_ref.true_grad with the
identity (dZ and delta of a head from dL/d(pre-activation)), gat_pass_ref's dropout factors, gat_qkv_ref.scale_of; the heads' backward
expressions are those modules', restated on the head's trace.  A layer with the norm off computes those models' own expressions.

All parameters travel in ONE dictionary `p`:
    "w" {(layer, head): W (W_v for score transformer)}    "av" {(layer, head): (a1, a2) | a} (additive | gatv2)    "wq", "wk" {(layer, head): W}
    "bias" {layer: b}    "wr" {layer: W_res}    "edge_bias" {layer: one value per entry of the edge list}    "gamma", "beta" {layer: vector}
and gradients come back in a dictionary of the same shape (plus "x": dL/dX of the input)."""
import numpy as np

import gat_pass_ref as P
import gat_qkv_ref as Q
import gat_skip_ref as S
import gat_v2_ref as V
from gat_ref import _smat, act, activations_of, adam_step, heads_of, leaky, row_softmax, sgd_step, true_grad, xent

SCORES = ("dot", "additive", "gatv2", "transformer")
UNDECAYED = ("gamma", "beta", "edge_bias")


# ------------------------------------------------------------------------------------------------ the norm itself
def _act(y, name, dtype):
    if name == "identity":
        return y
    if name == "relu":
        return np.where(y > 0, y, dtype(0))
    return np.where(y >= 0, y, np.expm1(np.minimum(y, dtype(0))))


def _slope(y, name, dtype):
    if name == "identity":
        return np.ones_like(y)
    if name == "relu":
        return np.where(y > 0, dtype(1), dtype(0))
    return np.where(y >= 0, dtype(1), np.exp(np.minimum(y, dtype(0))))


def ln_stats(z, eps, dtype=np.float64):
    z = np.asarray(z, dtype=dtype)
    mu = np.sum(z, axis=1) / dtype(z.shape[1])
    dev = z - mu[:, None]
    var = np.sum(dev * dev, axis=1) / dtype(z.shape[1])
    return mu, dtype(1) / np.sqrt(var + dtype(eps)), dev


def ln_forward(z, gamma, beta, eps, name, dtype=np.float64):
    """(out, (mu, rstd), xh, y)"""
    mu, rstd, dev = ln_stats(z, eps, dtype)
    xh = dev * rstd[:, None]
    y = np.asarray(gamma, dtype=dtype)[None, :] * xh + np.asarray(beta, dtype=dtype)[None, :]
    return _act(y, name, dtype), (mu, rstd), xh, y


def ln_backward(g, z, gamma, beta, eps, name, dtype=np.float64):
    """(dz, dgamma, dbeta, dY)"""
    _, (mu, rstd), xh, y = ln_forward(z, gamma, beta, eps, name, dtype)
    dy = np.asarray(g, dtype=dtype) * _slope(y, name, dtype)
    t = np.asarray(gamma, dtype=dtype)[None, :] * dy
    c = dtype(z.shape[1])
    m1, m2 = np.sum(t, axis=1) / c, np.sum(t * xh, axis=1) / c
    dz = rstd[:, None] * (t - m1[:, None] - xh * m2[:, None])
    return dz, np.sum(dy * xh, axis=0), np.sum(dy, axis=0), dy


# ------------------------------------------------------------------------------------------------ the model
def norms_of(layers, norm):
    n = [norm or "none"] * len(layers) if norm is None or isinstance(norm, str) else list(norm)
    assert len(n) == len(layers) and all(v in ("none", "layer") for v in n)
    return n


def _eps(eps, li):
    return eps.get(li, 1e-5) if isinstance(eps, dict) else eps


def _gain(p, li, width):
    return p.get("gamma", {}).get(li, np.ones(width)), p.get("beta", {}).get(li, np.zeros(width))


def _head_forward(score, rows, cols, m, xd, p, key, alpha, ck, eb):
    """The head's trace: gat_skip_ref._head's six entries, or gat_qkv_ref's (V, s, p, o, lse, (Q, K)) with the edge bias in s."""
    if score != "transformer":
        return S._head(rows, cols, m, xd @ p["w"][key], p["av"][key] if score != "dot" else None, score, alpha, ck)
    qm, km, vm = xd @ p["wq"][key], xd @ p["wk"][key], xd @ p["w"][key]
    s = Q.scale_of(vm.shape[1]) * np.einsum("ij,ij->i", qm[rows], km[cols])
    if eb is not None:
        s = s + eb
    pr, lse = row_softmax(rows, m, s)
    return (vm, s, pr, Q._smat(rows, cols, pr, (m, m)) @ vm, lse, (qm, km))


def forward(rows, cols, m, x, layers, alpha, p, *, score="additive", rates=(0.0, 0.0), seed=0, activations=None, residual=None, norm=None,
            eps=1e-5, keep_trace=False):
    """The forward pass under attention softmax.  keep_trace=True also returns per layer (Xd, feature factor, out, heads, pre) with pre the
    rows o + r + b BEFORE the norm (or before the activation of a layer without)."""
    pa, q = rates
    assert score in SCORES
    if pa > 0.0 and score != "additive":
        raise ValueError("attention dropout supports score additive only")
    acts, res, nrm = activations_of(layers, activations), S.residuals_of(layers, residual), norms_of(layers, norm)
    trace = []
    for li, (fin, fph, heads) in enumerate(layers):
        assert x.shape[1] == fin
        ff = P.feature_factor(seed, li, x.shape, q) if q > 0.0 else None
        xd = x if ff is None else ff * x
        add = S.addend_of(xd, li, res, p.get("bias"), p.get("wr"))
        pre = np.zeros((m, fph * heads))
        heads_t = []
        for h in range(heads):
            ck = P.attention_factor(seed, li, h, rows, cols, pa) if pa > 0.0 else None
            ht = _head_forward(score, rows, cols, m, xd, p, (li, h), alpha, ck, p.get("edge_bias", {}).get(li))
            sl = slice(h * fph, (h + 1) * fph)
            pre[:, sl] = ht[3] if add is None else ht[3] + add[:, sl]
            heads_t.append(ht)
        if nrm[li] == "layer":
            gamma, beta = _gain(p, li, fph * heads)
            out = ln_forward(pre, gamma, beta, _eps(eps, li), acts[li])[0]
        else:
            out = act(pre, acts[li])
        trace.append((xd, ff, out, heads_t, pre))
        x = out
    return (x, trace) if keep_trace else x


def _head_backward(score, rows, cols, m, ht, dz, delta, p, key, alpha):
    """(dXd's shares in the order they are added, {kind: gradient}, per-entry edge-bias gradient or None) of one head from dZ and delta"""
    if score == "transformer":
        vm, s, pr, o, lse, (qm, km) = ht
        sc = Q.scale_of(vm.shape[1])
        inner = np.einsum("ij,ij->i", dz[rows], vm[cols]) - delta[rows]
        deb = pr * inner
        sg = Q._smat(rows, cols, sc * pr * inner, (m, m))
        dq, dk, dv = sg @ km, sg.T @ qm, Q._smat(rows, cols, pr, (m, m)).T @ dz
        grads = {"w": dv, "wq": dq, "wk": dk}  # (dA of each weight: the caller multiplies by Xd^T)
        return [dv @ p["w"][key].T, dq @ p["wq"][key].T, dk @ p["wk"][key].T], grads, {}, deb
    a_mat, z, a, o, lse, last = ht
    fph = a_mat.shape[1]
    direct = {}
    if score == "gatv2":
        vec, u = p["av"][key], last
        gij = a * (np.einsum("ij,ij->i", dz[rows], a_mat[cols]) - delta[rows])
        du = gij[:, None] * (np.where(u > 0, 1.0, alpha) * vec[None, :])
        da_mat = np.zeros((m, fph))
        np.add.at(da_mat, rows, du)
        np.add.at(da_mat, cols, du)
        da_mat += V._smat(rows, cols, a, (m, m)).T @ dz
        direct["av"] = gij @ leaky(u, alpha)
    elif score == "additive":
        a1, a2 = p["av"][key]
        ck = last
        da = np.einsum("ij,ij->i", dz[rows], a_mat[cols])
        dzz = a * ((da if ck is None else ck * da) - delta[rows]) * np.where(z > 0, 1.0, alpha)
        ds = np.bincount(rows, weights=dzz, minlength=m)
        dt = np.bincount(cols, weights=dzz, minlength=m)
        da_mat = _smat(rows, cols, a if ck is None else ck * a, m).T @ dz + np.outer(ds, a1) + np.outer(dt, a2)
        direct["av"] = (a_mat.T @ ds, a_mat.T @ dt)
    else:
        da = np.einsum("ij,ij->i", dz[rows], a_mat[cols])
        s_dz = _smat(rows, cols, a * (da - delta[rows]) * np.where(z > 0, 1.0, alpha), m)
        da_mat = s_dz @ a_mat + _smat(rows, cols, a, m).T @ dz + s_dz.T @ a_mat
    return [da_mat @ p["w"][key].T], {"w": da_mat}, direct, None


def backward(rows, cols, m, x, layers, alpha, grad_out, p, *, score="additive", rates=(0.0, 0.0), seed=0, activations=None, residual=None,
             norm=None, eps=1e-5):
    """Gradients of L with dL/d(output) = grad_out, the masks held fixed: a dictionary shaped like `p` ("w", "av", "wq", "wk", "bias", "wr",
    "edge_bias", "gamma", "beta": the entries that exist) plus "x"."""
    acts, res, nrm = activations_of(layers, activations), S.residuals_of(layers, residual), norms_of(layers, norm)
    _, trace = forward(rows, cols, m, x, layers, alpha, p, score=score, rates=rates, seed=seed, activations=acts, residual=res, norm=nrm, eps=eps,
                       keep_trace=True)
    out_g = {k: {} for k in ("w", "av", "wq", "wk", "bias", "wr", "edge_bias", "gamma", "beta")}
    g = grad_out
    for li in range(len(layers) - 1, -1, -1):
        fin, fph, heads = layers[li]
        xd, ff, out, heads_t, pre = trace[li]
        if nrm[li] == "layer":
            gamma, beta = _gain(p, li, fph * heads)
            g, out_g["gamma"][li], out_g["beta"][li], _ = ln_backward(g, pre, gamma, beta, _eps(eps, li), acts[li])
            name, stored = "identity", pre  # from here on the layer is an identity layer whose output is pre
        else:
            name, stored = acts[li], out
        dxd = np.zeros_like(xd)
        dz_all = np.zeros_like(out)
        deb_sum = None
        for h in range(heads):
            sl = slice(h * fph, (h + 1) * fph)
            o = heads_t[h][3]
            dz, _ = true_grad(g[:, sl], pre[:, sl], stored[:, sl], name)
            delta = np.sum(dz * o, axis=1)  # (against the aggregate, not the pre-activation)
            dz_all[:, sl] = dz
            shares, via_x, direct, deb = _head_backward(score, rows, cols, m, heads_t[h], dz, delta, p, (li, h), alpha)
            for kind, d_a in via_x.items():
                out_g[kind][(li, h)] = xd.T @ d_a
            for kind, v in direct.items():
                out_g[kind][(li, h)] = v
            if deb is not None:
                deb_sum = deb if deb_sum is None else deb_sum + deb
            for share in shares:
                dxd += share
        if li in p.get("edge_bias", {}):
            out_g["edge_bias"][li] = deb_sum
        if li in p.get("bias", {}):
            out_g["bias"][li] = dz_all.sum(axis=0)
        if res[li] == "projection":
            out_g["wr"][li] = xd.T @ dz_all
            dxd = dxd + dz_all @ p["wr"][li].T
        elif res[li] == "identity":
            dxd = dxd + dz_all
        g = dxd if ff is None else ff * dxd
    out_g["x"] = g
    return {k: v for k, v in out_g.items() if k == "x" or len(v)}


def pre_norm_rows(rows, cols, m, x, layers, alpha, p, **mode):
    """per layer the rows before the norm / the activation (m x H f)"""
    _, trace = forward(rows, cols, m, x, layers, alpha, p, keep_trace=True, **mode)
    return [t[4] for t in trace]


# ------------------------------------------------------------------------------------------------ training
def _flatten(p, learned_edge=()):
    flat = {}
    for kind, d in p.items():
        for key, v in d.items():
            if kind == "edge_bias" and key not in learned_edge:
                continue
            if isinstance(v, tuple):
                for q, part in enumerate(v):
                    flat[(kind, key, q)] = np.array(part, dtype=np.float64)
            else:
                flat[(kind, key, None)] = np.array(v, dtype=np.float64)
    return flat


def _unflatten(flat, p):
    out = {kind: dict(d) for kind, d in p.items()}
    for (kind, key, q), v in flat.items():
        if q is None:
            out[kind][key] = v
        else:
            parts = list(out[kind][key])
            parts[q] = v
            out[kind][key] = tuple(parts)
    return out


def train(rows, cols, m, x, layers, alpha, labels, mask, heads, p, optimizer, steps, *, learned_edge=(), seed0=0, perturb=None, **mode):
    """`steps` training steps over every tensor of `p` (the edge bias of the layers in learned_edge only); gamma, beta and the edge bias are
    NEVER decayed.  perturb = (scale, rng) as in gat_ref.train.  Returns (losses, accuracies, p after the steps)."""
    nh, _ = heads_of(layers, heads)
    opt = dict(optimizer)
    kind_o, lr = opt.pop("kind"), opt.pop("lr")
    undecayed = dict(opt, weight_decay=0.0)
    rates = mode.get("rates", (0.0, 0.0))
    dropout = rates[0] > 0.0 or rates[1] > 0.0
    flat = _flatten(p, learned_edge)
    mom = {k: np.zeros_like(v) for k, v in flat.items()}
    var = {k: np.zeros_like(v) for k, v in flat.items()}
    losses, accs = [], []
    for t in range(1, steps + 1):
        pt = _unflatten(flat, p)
        md = dict(mode, seed=(seed0 + t) & 0xFFFFFFFFFFFFFFFF if dropout else seed0)
        out = forward(rows, cols, m, x, layers, alpha, pt, **md)
        loss, acc, g = xent(out, labels, mask, nh)
        losses.append(float(loss))
        accs.append(float(acc))
        grads = _flatten({k: v for k, v in backward(rows, cols, m, x, layers, alpha, g, pt, **md).items() if k != "x"}, learned_edge)
        for k in flat:
            gk = grads[k]
            if perturb is not None:
                scale, rng = perturb
                gk = gk + scale * np.max(np.abs(gk)) * rng.uniform(-1.0, 1.0, gk.shape)
            hyper = undecayed if k[0] in UNDECAYED else opt
            if kind_o == "adam":
                flat[k], mom[k], var[k] = adam_step(flat[k], gk, mom[k], var[k], t, lr, **hyper)
            else:
                flat[k], var[k] = sgd_step(flat[k], gk, var[k], lr, **hyper)
    return losses, accs, _unflatten(flat, p)


def parameter_divergence(a, b, learned_edge=()):
    """max over the tensors of max|a - b| / max|b| for two parameter dictionaries"""
    fa, fb = _flatten(a, learned_edge), _flatten(b, learned_edge)
    return max(float(np.max(np.abs(fa[k] - fb[k])) / np.max(np.abs(fb[k]))) for k in fb)
