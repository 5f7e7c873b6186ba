"""numpy reference of the GAT with a bias and skip (residual) connections per layer (include/hnh_gat_skip.h; GAT.set_bias / set_residual),
next to tests/gat_ref.py and tests/gat_v2_ref.py, whose head-level pieces it reuses: one forward, one backward, one training loop for the
three scores "dot" | "additive" | "gatv2" under attention softmax (the only mode the product supports an addend in).

Layer l with input X, H heads of f features, activation phi_l; Xd = c_q mask o X under feature dropout (X itself at q = 0):
    o_h   = the head's attention aggregate, exactly as in gat_ref / gat_v2_ref (any score, any dropout)
    r     = 0 (residual "none")  |  Xd (residual "identity": input_features == H f)  |  Xd W_res (residual "projection")
    b     = the layer's bias (H f entries; absent = 0)
    out[:, h f:(h+1) f] = phi_l(o_h + r[:, h f:(h+1) f] + b[h f:(h+1) f])
Backward, with G = dL/d(out) and pre = o + r + b:
    dZ = G phi_l'(pre)     delta_i = <dZ_i, o_i> per head  (the softmax's row scalar is taken against the AGGREGATE, not the pre-activation)
    the head's dA, da1, da2 (da) from dZ and delta exactly as in gat_ref / gat_v2_ref;   dW_h = Xd^T dA
    db = colsum(dZ_all)     dW_res = Xd^T dZ_all     dXd = sum_h dA W_h^T + dZ_all W_res^T (projection) | + dZ_all (identity)
    dX = c_q mask o dXd
A layer with residual "none" and no bias runs gat_ref's / gat_v2_ref's own expressions: the same bits.

residual: None | one name | one name per layer.  bias: None | {layer: vector of H f}.  res_weights: {layer: input_features x H f} for
every "projection" layer.  The trace has gat_ref's shape: per layer (Xd, feature factor, out, heads) with per head the six entries of
the score's own reference, o being the aggregate WITHOUT the addend; addend_of() gives r + b of a layer."""
import numpy as np

import gat_pass_ref as P
import gat_ref as R
import gat_v2_ref as V
from gat_ref import _smat, act, activations_of, adam_step, heads_of, leaky, row_softmax, sgd_step, true_grad, weights_of, xent

RESIDUALS = ("none", "identity", "projection")
SCORES = ("dot", "additive", "gatv2")


def residuals_of(layers, residual):
    res = [residual or "none"] * len(layers) if residual is None or isinstance(residual, str) else list(residual)
    assert len(res) == len(layers) and all(r in RESIDUALS for r in res)
    for (fin, fph, heads), r in zip(layers, res):
        if r == "identity" and fin != fph * heads:
            raise ValueError("residual identity needs input_features == heads * features_per_head")
    return res


def vectors_of(layers, vectors, score):
    if score == "additive":
        return R.vectors_of(layers, vectors)
    return V.vectors_of(layers, vectors) if score == "gatv2" else None


def addend_of(xd, li, res, bias, res_weights):
    """r + b of layer li (m x H f), or None for a layer without either"""
    r = None
    if res[li] == "identity":
        r = xd
    elif res[li] == "projection":
        r = xd @ res_weights[li]
    b = None if bias is None else bias.get(li)
    if r is None and b is None:
        return None
    if r is None:
        return np.broadcast_to(b[None, :], (xd.shape[0], len(b))).copy()
    return r if b is None else r + b[None, :]


def _head(rows, cols, m, a_mat, vec, score, alpha, ck):
    """One head's forward: the six trace entries of the score's own reference."""
    if score == "gatv2":
        z, u = V.scores(a_mat, a_mat, rows, cols, vec, alpha)
        p, lse = row_softmax(rows, m, z)
        return (a_mat, z, p, V._smat(rows, cols, p, (m, m)) @ a_mat, lse, u)
    if score == "additive":
        z = (a_mat @ vec[0])[rows] + (a_mat @ vec[1])[cols]
    else:
        z = np.einsum("ij,ij->i", a_mat[rows], a_mat[cols])
    a, lse = row_softmax(rows, m, leaky(z, alpha))
    return (a_mat, z, a, _smat(rows, cols, a if ck is None else ck * a, m) @ a_mat, lse, ck)


def forward(rows, cols, m, x, layers, alpha: float, weights=None, vectors=None, *, score: str = "additive", rates=(0.0, 0.0), seed: int = 0,
            activations=None, residual=None, bias=None, res_weights=None, keep_trace: bool = False):
    p, q = rates
    assert score in SCORES
    if p > 0.0 and score != "additive":
        raise ValueError("attention dropout supports score additive only")
    acts = activations_of(layers, activations)
    res = residuals_of(layers, residual)
    w = weights_of(layers, weights)
    av = vectors_of(layers, vectors, score)
    trace = []
    for li, (fin, fph, heads) in enumerate(layers):
        assert x.shape[1] == fin
        ff = P.feature_factor(seed, li, x.shape, q) if q > 0.0 else None
        xd = x if ff is None else ff * x
        add = addend_of(xd, li, res, bias, res_weights)
        out = np.zeros((m, fph * heads))
        heads_t = []
        for h in range(heads):
            ck = P.attention_factor(seed, li, h, rows, cols, p) if p > 0.0 else None
            ht = _head(rows, cols, m, xd @ w[(li, h)], None if av is None else av[(li, h)], score, alpha, ck)
            sl = slice(h * fph, (h + 1) * fph)
            out[:, sl] = act(ht[3] if add is None else ht[3] + add[:, sl], acts[li])
            heads_t.append(ht)
        trace.append((xd, ff, out, heads_t))
        x = out
    return (x, trace) if keep_trace else x


def backward(rows, cols, m, x, layers, alpha: float, grad_out, weights=None, vectors=None, *, score: str = "additive", rates=(0.0, 0.0),
             seed: int = 0, activations=None, residual=None, bias=None, res_weights=None, forget_addend: bool = False,
             from_stored: bool = False):
    """({(layer, head): dW}, {(layer, head): (da1, da2) | da}, {layer: db}, {layer: dW_res}, dX0) for L with dL/d(output) = grad_out, the masks
    held fixed.  The second dictionary is empty with score dot; the third and fourth hold the layers that have a bias / a projection.
    forget_addend=True is WRONG on purpose: delta_i = <dZ_i, o_i + r_i + b>, what a backward pass gets that recovers the pre-activation
    from the stored output and does not take the addend out again; the tests use it to show that their inputs would notice.
    from_stored=True forms dZ and delta the way the product does, from the stored output and the addend alone (stored_grad below)."""
    acts = activations_of(layers, activations)
    res = residuals_of(layers, residual)
    w = weights_of(layers, weights)
    av = vectors_of(layers, vectors, score)
    kw = dict(score=score, rates=rates, seed=seed, activations=acts, residual=res, bias=bias, res_weights=res_weights)
    _, trace = forward(rows, cols, m, x, layers, alpha, w, av, keep_trace=True, **kw)
    g = grad_out
    dws, das, dbs, dwrs = {}, {}, {}, {}
    for li in range(len(layers) - 1, -1, -1):
        fin, fph, heads = layers[li]
        xd, ff, out, heads_t = trace[li]
        add = addend_of(xd, li, res, bias, res_weights)
        dxd = np.zeros_like(xd)
        dz_all = np.zeros_like(out)
        for h in range(heads):
            a_mat, z, a, o, lse, last = heads_t[h]
            sl = slice(h * fph, (h + 1) * fph)
            if from_stored:
                dz, delta = stored_grad(g[:, sl], out[:, sl], acts[li], np.zeros_like(o) if add is None else add[:, sl])
            elif add is None:
                dz, delta = true_grad(g[:, sl], o, out[:, sl], acts[li])
            else:
                dz, _ = true_grad(g[:, sl], o + add[:, sl], out[:, sl], acts[li])
                delta = np.sum(dz * (o + add[:, sl] if forget_addend else o), axis=1)
            dz_all[:, sl] = dz
            if score == "gatv2":
                vec, u = av[(li, h)], last
                gij = a * (np.einsum("ij,ij->i", dz[rows], a_mat[cols]) - delta[rows])
                du = gij[:, None] * (np.where(u > 0, 1.0, alpha) * vec[None, :])
                da_mat = np.zeros((m, fph))
                np.add.at(da_mat, rows, du)
                np.add.at(da_mat, cols, du)
                da_mat += V._smat(rows, cols, a, (m, m)).T @ dz
                das[(li, h)] = gij @ leaky(u, alpha)
            elif score == "additive":
                a1, a2 = av[(li, h)]
                ck = last
                da = np.einsum("ij,ij->i", dz[rows], a_mat[cols])
                dzz = a * ((da if ck is None else ck * da) - delta[rows]) * np.where(z > 0, 1.0, alpha)
                ds = np.bincount(rows, weights=dzz, minlength=m)
                dt = np.bincount(cols, weights=dzz, minlength=m)
                dagg = _smat(rows, cols, a if ck is None else ck * a, m).T @ dz
                da_mat = dagg + np.outer(ds, a1) + np.outer(dt, a2)
                das[(li, h)] = (a_mat.T @ ds, a_mat.T @ dt)
            else:
                da = np.einsum("ij,ij->i", dz[rows], a_mat[cols])
                dzz = a * (da - delta[rows]) * np.where(z > 0, 1.0, alpha)
                s_dz = _smat(rows, cols, dzz, m)
                da_mat = s_dz @ a_mat + _smat(rows, cols, a, m).T @ dz + s_dz.T @ a_mat
            dws[(li, h)] = xd.T @ da_mat
            dxd += da_mat @ w[(li, h)].T
        if bias is not None and li in bias:
            dbs[li] = dz_all.sum(axis=0)
        if res[li] == "projection":
            dwrs[li] = xd.T @ dz_all
            dxd = dxd + dz_all @ res_weights[li].T
        elif res[li] == "identity":
            dxd = dxd + dz_all
        g = dxd if ff is None else ff * dxd
    return dws, das, dbs, dwrs, g


def pre_activations(rows, cols, m, x, layers, alpha: float, weights=None, vectors=None, **mode):
    """Per layer (LeakyReLU inputs of every head as one vector, aggregates o (m x H f), addend (m x H f, zeros without))."""
    score = mode.get("score", "additive")
    _, trace = forward(rows, cols, m, x, layers, alpha, weights, vectors, keep_trace=True, **mode)
    res = residuals_of(layers, mode.get("residual"))
    outl = []
    for li, (xd, ff, out, heads_t) in enumerate(trace):
        add = addend_of(xd, li, res, mode.get("bias"), mode.get("res_weights"))
        kinks = np.concatenate([(ht[5] if score == "gatv2" else ht[1]).reshape(-1) for ht in heads_t])
        outl.append((kinks, np.hstack([ht[3] for ht in heads_t]), np.zeros_like(out) if add is None else add))
    return outl


def train(rows, cols, m, x, layers, alpha, labels, mask, heads, w, av, optimizer, steps, *, score="additive", rates=(0.0, 0.0), seed0=0,
          activations=None, residual=None, bias=None, res_weights=None, perturb=None):
    """gat_ref.train with the bias and W_res of every layer that has them among the parameters.  Returns (losses, accuracies, w, av, bias,
    res_weights)."""
    nh, _ = heads_of(layers, heads)
    opt = dict(optimizer)
    kind, lr = opt.pop("kind"), opt.pop("lr")
    av = vectors_of(layers, av, score)
    bias, res_weights = dict(bias or {}), dict(res_weights or {})
    params = {("w",) + k: v.copy() for k, v in w.items()}
    if score == "additive":
        params.update({("a1",) + k: av[k][0].copy() for k in av})
        params.update({("a2",) + k: av[k][1].copy() for k in av})
    elif score == "gatv2":
        params.update({("a",) + k: av[k].copy() for k in av})
    params.update({("b", li): v.copy() for li, v in bias.items()})
    params.update({("wr", li): v.copy() for li, v in res_weights.items()})
    mom = {k: np.zeros_like(v) for k, v in params.items()}
    var = {k: np.zeros_like(v) for k, v in params.items()}
    losses, accs = [], []
    dropout = rates[0] > 0.0 or rates[1] > 0.0

    def unpack():
        wt = {k: params[("w",) + k] for k in w}
        if score == "additive":
            at = {k: (params[("a1",) + k], params[("a2",) + k]) for k in av}
        else:
            at = {k: params[("a",) + k] for k in av} if score == "gatv2" else None
        return wt, at, {li: params[("b", li)] for li in bias}, {li: params[("wr", li)] for li in res_weights}

    for t in range(1, steps + 1):
        wt, at, bt, rt = unpack()
        mode = dict(score=score, rates=rates, seed=(seed0 + t) & 0xFFFFFFFFFFFFFFFF if dropout else seed0, activations=activations, residual=residual,
                    bias=bt or None, res_weights=rt or None)
        out = forward(rows, cols, m, x, layers, alpha, wt, at, **mode)
        loss, acc, g = xent(out, labels, mask, nh)
        losses.append(float(loss))
        accs.append(float(acc))
        dw, da, db, dwr, _ = backward(rows, cols, m, x, layers, alpha, g, wt, at, **mode)
        grads = {("w",) + k: dw[k] for k in dw}
        if score == "additive":
            grads.update({("a1",) + k: da[k][0] for k in da})
            grads.update({("a2",) + k: da[k][1] for k in da})
        elif score == "gatv2":
            grads.update({("a",) + k: da[k] for k in da})
        grads.update({("b", li): db[li] for li in db})
        grads.update({("wr", li): dwr[li] for li in dwr})
        for k in params:
            gk = grads[k]
            if perturb is not None:
                scale, rng = perturb
                gk = gk + scale * np.max(np.abs(gk)) * rng.uniform(-1.0, 1.0, gk.shape)
            if kind == "adam":
                params[k], mom[k], var[k] = adam_step(params[k], gk, mom[k], var[k], t, lr, **opt)
            else:
                params[k], var[k] = sgd_step(params[k], gk, var[k], lr, **opt)
    return (losses, accs) + unpack()


def parameter_divergence(a, b):
    """max over the tensors of max|a - b| / max|b| for two results of train() (their last four entries)"""
    worst = 0.0
    for da, db in zip(a[2:], b[2:]):
        for k in (db or {}):
            for va, vb in zip(da[k] if isinstance(db[k], tuple) else (da[k],), db[k] if isinstance(db[k], tuple) else (db[k],)):
                worst = max(worst, float(np.max(np.abs(va - vb)) / np.max(np.abs(vb))))
    return worst


def stored_grad(g, out, name, addend, dtype=np.float64):
    """(dZ, delta) from the STORED output and the addend, as hnh_skip_grad_cols_f64 computes them: gat_ref.stored_grad's dZ, and
    delta_r = sum_c dZ (phi^{-1}(out) - addend), the term 0 where dZ is (relu at out <= 0, elu saturated at -1)."""
    g, out, addend = (np.asarray(v, dtype=dtype) for v in (g, out, addend))
    dz, _ = R.stored_grad(g, out, name, dtype)
    if name == "identity":
        return dz, np.sum(dz * (out - addend), axis=1)
    if name == "relu":
        return dz, np.sum(np.where(out > 0, dz * (out - addend), dtype(0)), axis=1)
    neg = out < 0
    u = dtype(1) + out
    with np.errstate(divide="ignore", invalid="ignore"):
        o = np.where(neg, np.log1p(np.where(neg, out, dtype(0))), out)
        term = np.where(neg & ~(u > 0), dtype(0), dz * (o - addend))
    return dz, np.sum(term, axis=1)
