"""numpy reference of the GAT's score "transformer" (include/hnh_attn_qkv.h; scaled dot-product attention with separate query, key and value
projections: TransformerConv / UniMP), next to tests/gat_ref.py, tests/gat_v2_ref.py and tests/gat_skip_ref.py, whose pieces it is built on:
activations, the bias, both residuals and feature dropout come along.

Per head h of layer l, Xd = c_q mask o X (X itself at q = 0), Q = Xd W_q, K = Xd W_k, V = Xd W_v, scale = 1 / sqrt(f), over the nonzeros
(i, j) of S (values 1; a repeated pair counts as often as it appears; no LeakyReLU anywhere):
    s_ij = scale <Q_i, K_j>     lse_i = log sum_j exp(s_ij)     p_ij = exp(s_ij - lse_i)     o_i = sum_j p_ij V_j
    out[:, h f:(h+1) f] = phi(o_h + r[:, h f:(h+1) f] + b[h f:(h+1) f])        (r, b: gat_skip_ref.addend_of; absent = 0)
Backward, from G = dL/d(out), with dZ = G phi'(o + r + b) and delta_i = <dZ_i, o_i>:
    g_ij = scale p_ij (<dZ_i, V_j> - delta_i)
    dQ_i = sum_j g_ij K_j      dK_j = sum_i g_ij Q_i      dV_j = sum_i p_ij dZ_i
    dW_q = Xd^T dQ,  dW_k = Xd^T dK,  dW_v = Xd^T dV      dXd = sum_h (dV W_v^T + dQ W_q^T + dK W_k^T) (+ the skip connection's share)
    db = colsum(dZ_all)     dW_res = Xd^T dZ_all     dX = c_q mask o dXd
by_passes=True restates each head through the single passes below, on the packed operands of gat_pass_ref.fused_pack, as the product does:
    fwd_pass and row_pass gather [K_j (0) | V_j (0)] (the pack without scalars), col_pass over S^T gathers [Q_i (0) | dZ_i (0) | lse_i delta_i].
Weights are {(layer, head): W}: `weights` is W_v (the head's weight of the other scores), `wq` and `wk` the two new ones."""
import math

import numpy as np
import scipy.sparse as sp

import gat_pass_ref as P
import gat_skip_ref as S
from gat_ref import act, activations_of, adam_step, heads_of, row_softmax, sgd_step, true_grad, weights_of, xent

__all__ = ["forward", "backward", "pre_activations", "train", "fwd_pass", "fwd_pass_ld", "row_pass", "col_pass", "qk_weights_of"]


def qk_weights_of(layers, seed: int = 91, scale: float = 1.0):
    """({(layer, head): W_q}, {(layer, head): W_k}): seeded normal matrices of scale / sqrt(fan-in)"""
    rng = np.random.default_rng(seed)
    wq = {(li, h): rng.standard_normal((fin, fph)) * scale / np.sqrt(fin) for li, (fin, fph, heads) in enumerate(layers) for h in range(heads)}
    wk = {(li, h): rng.standard_normal((fin, fph)) * scale / np.sqrt(fin) for li, (fin, fph, heads) in enumerate(layers) for h in range(heads)}
    return wq, wk


def _smat(rows, cols, vals, shape):
    return sp.csr_matrix((vals, (rows, cols)), shape=shape)  # duplicates are summed, as the passes over the list do


def scale_of(f: int) -> float:
    return 1.0 / math.sqrt(f)


# ------------------------------------------------------------------------------------------------ single passes, as the kernels take them
def _halves(packed, f):
    fp = f + (f & 1)
    return packed[:, :f], packed[:, fp:fp + f]


def fwd_pass(rows, cols, m, q_rows, kv_cols, f, scale):
    """(o, lse, s, p): own rows Q, gathered operand [K | V] (the pack without scalars)"""
    k, v = _halves(kv_cols, f)
    s = scale * np.einsum("ij,ij->i", q_rows[rows, :f], k[cols])
    p, lse = row_softmax(rows, m, s)
    return _smat(rows, cols, p, (m, kv_cols.shape[0])) @ v, lse, s, p


def fwd_pass_ld(rows, cols, m, q_rows, kv_cols, f, scale):
    """fwd_pass in np.longdouble (math.fsum where longdouble is no wider than fp64): (o, lse, s) as longdouble, before the activation."""
    ld = np.longdouble
    wide = np.finfo(ld).eps <= 1e-18
    order = np.argsort(rows, kind="stable")
    r, c = np.asarray(rows)[order], np.asarray(cols)[order]
    k, v = _halves(kv_cols, f)
    q, k, v = np.asarray(q_rows[:, :f], dtype=ld), np.asarray(k, dtype=ld), np.asarray(v, dtype=ld)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))])
    o = np.zeros((m, f), dtype=ld)
    lse = np.zeros(m, dtype=ld)
    s_all = np.zeros(len(r), dtype=ld)
    for i in range(m):
        b, t = rowptr[i], rowptr[i + 1]
        if t == b:
            continue
        terms = q[i][None, :] * k[c[b:t]]
        s = (np.sum(terms, axis=1) if wide else np.array([math.fsum(row) for row in terms], dtype=ld)) * ld(scale)
        s_all[b:t] = s
        mx = s.max()
        ex = np.exp(s - mx)
        tot = np.sum(ex) if wide else ld(math.fsum(ex))
        lse[i] = mx + np.log(tot)
        contrib = (ex[:, None] / tot) * v[c[b:t]]
        o[i] = np.sum(contrib, axis=0) if wide else [math.fsum(contrib[:, kk]) for kk in range(f)]
    back = np.empty_like(s_all)
    back[order] = s_all
    return o, lse, back


def row_pass(rows, cols, m, q_rows, dz_rows, lse, delta, kv_cols, f, scale, out=None):
    """dQ (+ out): dQ_i = sum_j g_ij K_j over a block of S; the own rows' Q, dZ, lse, delta, the gathered [K_j | V_j]."""
    k, v = _halves(kv_cols, f)
    s = scale * np.einsum("ij,ij->i", q_rows[rows, :f], k[cols])
    gij = scale * np.exp(s - lse[rows]) * (np.einsum("ij,ij->i", dz_rows[rows, :f], v[cols]) - delta[rows])
    r = np.zeros((m, f)) if out is None else np.array(out, copy=True)
    np.add.at(r, rows, gij[:, None] * k[cols])
    return r


def col_pass(trows, tcols, m, k_rows, v_rows, packed, f, scale, out=None, out2=None):
    """(dK, dV) (+ out, out2) over a block of S^T: row j = trows is local (K_j, V_j), nonzero (j, i) gathers the packed
    P_i = [Q_i (0) | dZ_i (0) | lse_i delta_i] (gat_pass_ref.fused_pack with softmax)."""
    fp = f + (f & 1)
    yq, yz = _halves(packed, f)
    lse, delta = packed[:, 2 * fp], packed[:, 2 * fp + 1]
    s = scale * np.einsum("ij,ij->i", k_rows[trows, :f], yq[tcols])
    p = np.exp(s - lse[tcols])
    gij = scale * p * (np.einsum("ij,ij->i", v_rows[trows, :f], yz[tcols]) - delta[tcols])
    dk = np.zeros((m, f)) if out is None else np.array(out, copy=True)
    dv = np.zeros((m, f)) if out2 is None else np.array(out2, copy=True)
    np.add.at(dk, trows, gij[:, None] * yq[tcols])
    np.add.at(dv, trows, p[:, None] * yz[tcols])
    return dk, dv


# ------------------------------------------------------------------------------------------------ the model
def forward(rows, cols, m, x, layers, weights=None, wq=None, wk=None, *, rates=(0.0, 0.0), seed: int = 0, activations=None, residual=None,
            bias=None, res_weights=None, by_passes: bool = False, keep_trace: bool = False):
    """The forward pass (attention softmax; rates = (0, q): the product refuses attention dropout with this score).  keep_trace=True also
    returns per layer (Xd, feature factor, out, heads) with per head (V, s, p, o, lse, (Q, K)), o being the aggregate WITHOUT the addend."""
    p_attn, q = rates
    if p_attn > 0.0:
        raise ValueError("score transformer does not support attention dropout")
    acts = activations_of(layers, activations)
    res = S.residuals_of(layers, residual)
    w = weights_of(layers, weights)
    if wq is None or wk is None:
        wq, wk = qk_weights_of(layers)
    trace = []
    for li, (fin, fph, heads) in enumerate(layers):
        assert x.shape[1] == fin
        ff = P.feature_factor(seed, li, x.shape, q) if q > 0.0 else None
        xd = x if ff is None else ff * x
        add = S.addend_of(xd, li, res, bias, res_weights)
        out = np.zeros((m, fph * heads))
        heads_t = []
        for h in range(heads):
            qm, km, vm = xd @ wq[(li, h)], xd @ wk[(li, h)], xd @ w[(li, h)]
            if by_passes:
                o, lse, s, p = fwd_pass(rows, cols, m, qm, np.nan_to_num(P.fused_pack(km, vm)), fph, scale_of(fph))
            else:
                s = scale_of(fph) * np.einsum("ij,ij->i", qm[rows], km[cols])
                p, lse = row_softmax(rows, m, s)
                o = _smat(rows, cols, p, (m, m)) @ vm
            sl = slice(h * fph, (h + 1) * fph)
            out[:, sl] = act(o if add is None else o + add[:, sl], acts[li])
            heads_t.append((vm, s, p, o, lse, (qm, km)))
        trace.append((xd, ff, out, heads_t))
        x = out
    return (x, trace) if keep_trace else x


def backward(rows, cols, m, x, layers, grad_out, weights=None, wq=None, wk=None, *, rates=(0.0, 0.0), seed: int = 0, activations=None,
             residual=None, bias=None, res_weights=None, by_passes: bool = False):
    """({(layer, head): dW_v}, {..: dW_q}, {..: dW_k}, {layer: db}, {layer: dW_res}, dX0) for L with dL/d(output) = grad_out, the feature masks
    held fixed.  The fourth and fifth hold the layers that have a bias / a projection.  by_passes=True computes each head's dQ, dK and dV
    through the packed operands, the row pass and the column pass (over S^T), as the product does."""
    acts = activations_of(layers, activations)
    res = S.residuals_of(layers, residual)
    w = weights_of(layers, weights)
    if wq is None or wk is None:
        wq, wk = qk_weights_of(layers)
    _, trace = forward(rows, cols, m, x, layers, w, wq, wk, rates=rates, seed=seed, activations=acts, residual=res, bias=bias,
                       res_weights=res_weights, by_passes=by_passes, keep_trace=True)
    g = grad_out
    dws, dwqs, dwks, dbs, dwrs = {}, {}, {}, {}, {}
    for li in range(len(layers) - 1, -1, -1):
        fin, fph, heads = layers[li]
        xd, ff, out, heads_t = trace[li]
        add = S.addend_of(xd, li, res, bias, res_weights)
        dxd = np.zeros_like(xd)
        dz_all = np.zeros_like(out)
        sc = scale_of(fph)
        for h in range(heads):
            vm, s, p, o, lse, (qm, km) = heads_t[h]
            sl = slice(h * fph, (h + 1) * fph)
            if add is None:
                dz, delta = true_grad(g[:, sl], o, out[:, sl], acts[li])
            else:
                dz, _ = true_grad(g[:, sl], o + add[:, sl], out[:, sl], acts[li])
                delta = np.sum(dz * o, axis=1)
            dz_all[:, sl] = dz
            if by_passes:
                kv = np.nan_to_num(P.fused_pack(km, vm))
                dq = row_pass(rows, cols, m, qm, dz, lse, delta, kv, fph, sc)
                dk, dv = col_pass(cols, rows, m, km, vm, P.fused_pack(qm, dz, lse, delta), fph, sc)
            else:
                gij = sc * p * (np.einsum("ij,ij->i", dz[rows], vm[cols]) - delta[rows])
                sg = _smat(rows, cols, gij, (m, m))
                dq, dk, dv = sg @ km, sg.T @ qm, _smat(rows, cols, p, (m, m)).T @ dz
            key = (li, h)
            dws[key], dwqs[key], dwks[key] = xd.T @ dv, xd.T @ dq, xd.T @ dk
            dxd += dv @ w[key].T
            dxd += dq @ wq[key].T
            dxd += dk @ wk[key].T
        if bias is not None and li in bias:
            dbs[li] = dz_all.sum(axis=0)
        if res[li] == "projection":
            dwrs[li] = xd.T @ dz_all
            dxd = dxd + dz_all @ res_weights[li].T
        elif res[li] == "identity":
            dxd = dxd + dz_all
        g = dxd if ff is None else ff * dxd
    return dws, dwqs, dwks, dbs, dwrs, g


def pre_activations(rows, cols, m, x, layers, weights=None, wq=None, wk=None, **mode):
    """Everything a finite-difference step must not carry across 0, as one vector: the activation's input o + r + b of every row that has a
    nonzero or an addend.  (The score itself has no kink.)"""
    _, trace = forward(rows, cols, m, x, layers, weights, wq, wk, keep_trace=True, **{k: v for k, v in mode.items() if k != "by_passes"})
    res = S.residuals_of(layers, mode.get("residual"))
    live = np.zeros(m, dtype=bool)
    live[rows] = True
    parts = []
    for li, (xd, ff, out, heads_t) in enumerate(trace):
        add = S.addend_of(xd, li, res, mode.get("bias"), mode.get("res_weights"))
        o = np.hstack([ht[3] for ht in heads_t])
        parts.append((o[live] if add is None else o + add).reshape(-1))
    return np.concatenate(parts)


def train(rows, cols, m, x, layers, labels, mask, heads, w, wq, wk, optimizer, steps, *, rates=(0.0, 0.0), seed0=0, activations=None,
          residual=None, bias=None, res_weights=None, perturb=None):
    """gat_skip_ref.train for this score: K steps over every W_v, W_q, W_k and the bias and W_res of every layer that has them.  Returns
    (losses, accuracies, w, wq, wk, bias, res_weights)."""
    nh, _ = heads_of(layers, heads)
    opt = dict(optimizer)
    kind, lr = opt.pop("kind"), opt.pop("lr")
    bias, res_weights = dict(bias or {}), dict(res_weights or {})
    params = {("w",) + k: v.copy() for k, v in w.items()}
    params.update({("wq",) + k: v.copy() for k, v in wq.items()})
    params.update({("wk",) + k: v.copy() for k, v in wk.items()})
    params.update({("b", li): v.copy() for li, v in bias.items()})
    params.update({("wr", li): v.copy() for li, v in res_weights.items()})
    mom = {k: np.zeros_like(v) for k, v in params.items()}
    var = {k: np.zeros_like(v) for k, v in params.items()}
    losses, accs = [], []
    dropout = rates[1] > 0.0

    def unpack():
        return ({k: params[("w",) + k] for k in w}, {k: params[("wq",) + k] for k in wq}, {k: params[("wk",) + k] for k in wk},
                {li: params[("b", li)] for li in bias}, {li: params[("wr", li)] for li in res_weights})

    for t in range(1, steps + 1):
        wt, qt, kt, bt, rt = unpack()
        mode = dict(rates=rates, seed=(seed0 + t) & 0xFFFFFFFFFFFFFFFF if dropout else seed0, activations=activations, residual=residual,
                    bias=bt or None, res_weights=rt or None)
        out = forward(rows, cols, m, x, layers, wt, qt, kt, **mode)
        loss, acc, g = xent(out, labels, mask, nh)
        losses.append(float(loss))
        accs.append(float(acc))
        dw, dq, dk, db, dwr, _ = backward(rows, cols, m, x, layers, g, wt, qt, kt, **mode)
        grads = {("w",) + k: dw[k] for k in dw}
        grads.update({("wq",) + k: dq[k] for k in dq})
        grads.update({("wk",) + k: dk[k] for k in dk})
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
    """max over the tensors of max|a - b| / max|b| for two results of train() (their last five entries)"""
    worst = 0.0
    for da, db in zip(a[2:], b[2:]):
        for k in (db or {}):
            worst = max(worst, float(np.max(np.abs(da[k] - db[k])) / np.max(np.abs(db[k]))))
    return worst
