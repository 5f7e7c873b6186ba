"""numpy reference of the GAT's per-layer output activation (GAT.set_activation, csrc/host/gat.hpp, the HNH_ATTN_ACT_* flags of
include/hnh_attention.h and hnh_act_grad_cols_f64 of include/hnh_grad.h) — the definition the tests hold the product to.  A sibling of
gat_dropout_ref.py and gat_additive_ref.py, whose forward and backward it restates with one more argument: `activations`, one of
"relu" | "elu" | "identity" per layer.  With "relu" everywhere the arithmetic is theirs, operation for operation.

With o the head's aggregate (dropout factors included):
    out = phi(o):   relu  max(o, 0)      elu  o for o > 0, expm1(o) otherwise      identity  o
    dZ  = G phi'(o),   delta_i = <dZ_i, o_i>      (relu: [o > 0]; elu: 1 for o > 0, exp(o) otherwise; identity: 1)
The model reference differentiates the true o.  The product keeps no pre-activation: stored_grad() restates its recovery from the STORED
output (u = 1 + out: dZ = G u and o = log1p(out) where out < 0, the term 0 where u == 0), and stored_grad_ld() is the same in
np.longdouble, the kernel tests' reference."""
import numpy as np

import gat_additive_ref as A
import gat_dropout_ref as D
import gat_train_ref as TR
from gat_backward_ref import weights_of
from gat_softmax_ref import leaky, row_softmax

ACTIVATIONS = ("relu", "elu", "identity")
ACT_CODE = {"relu": 0, "elu": 1, "identity": 2}  # HNH_ACT_* / HNH_GAT_ACT_*


def activations_of(layers, activations):
    acts = [activations] * len(layers) if isinstance(activations, str) else list(activations or ["relu"] * len(layers))
    assert len(acts) == len(layers) and all(a in ACTIVATIONS for a in acts)
    return acts


def act(o, name):
    if name == "relu":
        return np.maximum(o, 0.0)
    if name == "identity":
        return np.array(o, copy=True)
    return np.where(o > 0, o, np.expm1(np.minimum(o, 0)))  # (minimum: expm1 of a large positive o must not overflow on the unused side)


def act_ld(o, name):
    """act() of a longdouble aggregate, in longdouble"""
    o = np.asarray(o, dtype=np.longdouble)
    if name == "relu":
        return np.maximum(o, np.longdouble(0))
    if name == "identity":
        return o.copy()
    return np.where(o > 0, o, np.expm1(np.minimum(o, np.longdouble(0))))


def true_grad(g, o, out, name):
    """(dZ, delta) from the TRUE pre-activation o (the definition)"""
    if name == "relu":
        dz = g * (out > 0)
    elif name == "identity":
        dz = g * 1.0
    else:
        dz = g * np.where(o > 0, 1.0, np.exp(np.minimum(o, 0)))
    return dz, np.sum(dz * o, axis=1)


def stored_grad(g, out, name, dtype=np.float64):
    """(dZ, delta) from the STORED output alone, as hnh_act_grad_cols_f64 computes them."""
    g, out = np.asarray(g, dtype=dtype), np.asarray(out, dtype=dtype)
    if name == "relu":
        dz = np.where(out > 0, g, dtype(0))
        return dz, np.sum(dz * out, axis=1)
    if name == "identity":
        return g.copy(), np.sum(g * out, axis=1)
    neg = out < 0
    u = dtype(1) + out
    dz = np.where(neg, g * u, g)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = np.where(neg, np.log1p(np.where(neg, out, dtype(0))), out)
        term = np.where(neg & ~(u > 0), dtype(0), dz * o)  # a unit saturated at -1: dZ = 0, and 0 * -inf is 0 here
    return dz, np.sum(term, axis=1)


def stored_grad_ld(g, out, name):
    return stored_grad(g, out, name, np.longdouble)


# ------------------------------------------------------------------------------------------------ the model
def forward(rows, cols, m, x, layers, alpha: float, weights=None, vectors=None, rates=(0.0, 0.0), seed: int = 0, activations=None,
            score: str = "additive", keep_trace: bool = False):
    """gat_dropout_ref.forward (score "additive") or gat_softmax_ref.forward (score "dot", rates (0, 0)) with the layers' activations.
    keep_trace=True also returns per layer (Xd, feature factor, out, heads) with per head (A, z, a, o, lse, c m)."""
    p, q = rates
    assert score in ("additive", "dot") and (score == "additive" or p == 0.0)
    acts = activations_of(layers, activations)
    w = weights_of(layers, weights)
    av = A.vectors_of(layers, vectors) if score == "additive" else None
    trace = []
    for li, (fin, fph, heads) in enumerate(layers):
        assert x.shape[1] == fin
        ff = D.feature_factor(seed, li, x.shape, q) if q > 0.0 else np.ones(x.shape)
        xd = ff * x
        out = np.zeros((m, fph * heads))
        heads_t = []
        for h in range(heads):
            a_mat = xd @ w[(li, h)]
            if score == "additive":
                a1, a2 = av[(li, h)]
                z = (a_mat @ a1)[rows] + (a_mat @ a2)[cols]
            else:
                z = np.einsum("ij,ij->i", a_mat[rows], a_mat[cols])
            a, lse = row_softmax(rows, m, leaky(z, alpha))
            ck = D.attention_factor(seed, li, h, rows, cols, p) if p > 0.0 else np.ones(len(rows))
            o = A._smat(rows, cols, ck * a, m) @ a_mat
            out[:, h * fph:(h + 1) * fph] = act(o, acts[li])
            heads_t.append((a_mat, z, a, o, lse, ck))
        trace.append((xd, ff, out, heads_t))
        x = out
    return (x, trace) if keep_trace else x


def backward(rows, cols, m, x, layers, alpha: float, grad_out, weights=None, vectors=None, rates=(0.0, 0.0), seed: int = 0, activations=None,
             score: str = "additive"):
    """({(layer, head): dW}, {(layer, head): (da1, da2)}, dX0) for L with dL/d(output) = grad_out, the masks held fixed (score "dot": the
    second dictionary is empty)."""
    p, q = rates
    acts = activations_of(layers, activations)
    w = weights_of(layers, weights)
    av = A.vectors_of(layers, vectors) if score == "additive" else None
    _, trace = forward(rows, cols, m, x, layers, alpha, w, av, rates, seed, acts, score, keep_trace=True)
    g = grad_out
    dws, das = {}, {}
    for li in range(len(layers) - 1, -1, -1):
        fin, fph, heads = layers[li]
        xd, ff, out, heads_t = trace[li]
        dxd = np.zeros_like(xd)
        for h in range(heads):
            a_mat, z, a, o, lse, ck = heads_t[h]
            sl = slice(h * fph, (h + 1) * fph)
            dz, delta = true_grad(g[:, sl], o, out[:, sl], acts[li])
            da = np.einsum("ij,ij->i", dz[rows], a_mat[cols])
            dzz = a * (ck * da - delta[rows]) * np.where(z > 0, 1.0, alpha)
            if score == "additive":
                a1, a2 = av[(li, h)]
                ds = np.bincount(rows, weights=dzz, minlength=m)
                dt = np.bincount(cols, weights=dzz, minlength=m)
                dagg = A._smat(rows, cols, ck * a, m).T @ dz
                da_mat = dagg + np.outer(ds, a1) + np.outer(dt, a2)
                das[(li, h)] = (a_mat.T @ ds, a_mat.T @ dt)
            else:
                s_de = A._smat(rows, cols, dzz, m)
                da_mat = s_de @ a_mat + A._smat(rows, cols, a, m).T @ dz + s_de.T @ a_mat
            dws[(li, h)] = xd.T @ da_mat
            dxd += da_mat @ w[(li, h)].T
        g = ff * dxd
    return dws, das, g


def pre_activations(rows, cols, m, x, layers, alpha: float, weights=None, vectors=None, rates=(0.0, 0.0), seed: int = 0, activations=None,
                    score: str = "additive"):
    """Per layer, the list of the heads' raw aggregates o (m x f each): what the activation is applied to."""
    _, trace = forward(rows, cols, m, x, layers, alpha, weights, vectors, rates, seed, activations, score, keep_trace=True)
    return [[ht[3] for ht in heads_t] for _, _, _, heads_t in trace]


# ------------------------------------------------------------------------------------------------ training
def train(rows, cols, m, x, layers, alpha, labels, mask, heads, w, av, optimizer, steps, activations=None, perturb=None):
    """gat_train_ref.train (rates (0, 0)) with the layers' activations: (losses, accuracies, w, av)."""
    nh, _ = TR.heads_of(layers, heads)
    opt = dict(optimizer)
    kind, lr = opt.pop("kind"), opt.pop("lr")
    params = {("w",) + k: v.copy() for k, v in w.items()}
    params.update({("a1",) + k: av[k][0].copy() for k in av})
    params.update({("a2",) + k: av[k][1].copy() for k in av})
    mom = {k: np.zeros_like(v) for k, v in params.items()}
    var = {k: np.zeros_like(v) for k, v in params.items()}
    losses, accs = [], []
    for t in range(1, steps + 1):
        wt = {k: params[("w",) + k] for k in w}
        at = {k: (params[("a1",) + k], params[("a2",) + k]) for k in av}
        out = forward(rows, cols, m, x, layers, alpha, wt, at, activations=activations)
        loss, acc, g = TR.xent(out, labels, mask, nh)
        losses.append(float(loss))
        accs.append(float(acc))
        dw, da, _ = backward(rows, cols, m, x, layers, alpha, g, wt, at, activations=activations)
        grads = {("w",) + k: dw[k] for k in dw}
        grads.update({("a1",) + k: da[k][0] for k in da})
        grads.update({("a2",) + k: da[k][1] for k in da})
        for k in params:
            gk = grads[k]
            if perturb is not None:
                scale, rng = perturb
                gk = gk + scale * np.max(np.abs(gk)) * rng.uniform(-1.0, 1.0, gk.shape)
            if kind == "adam":
                params[k], mom[k], var[k] = TR.adam_step(params[k], gk, mom[k], var[k], t, lr, **opt)
            else:
                params[k], var[k] = TR.sgd_step(params[k], gk, var[k], lr, **opt)
    return losses, accs, {k: params[("w",) + k] for k in w}, {k: (params[("a1",) + k], params[("a2",) + k]) for k in av}
