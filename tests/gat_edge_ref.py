"""numpy reference of the per-edge bias on the GAT's score "transformer" (include/hnh_attn_edge.h, GAT.set_edge_bias), built on
tests/gat_qkv_ref.py: the same model with one more term in the logit,
    s_e = scale <Q_i, K_j> + b_e     lse_i = log sum_e exp(s_e)     p_e = exp(s_e - lse_i)     o_i = sum_e p_e V_j
and the backward pass of gat_qkv_ref with p_e from the biased s_e.  The bias of a layer is shared by its heads and is not learned.

A bias belongs to a nonzero, not to a pair: `edge_bias` is {layer: vector}, entry e of a layer's vector belonging to entry e of the edge
list (rows, cols) the model is called with, so two copies of a repeated pair may carry different values.  keys(rows, cols) names every
entry by its global (row, col, copy), copy counting the earlier entries of the same pair, and bias_of(fn, rows, cols) evaluates
fn(row, col, copy) on them: the order-free way to write a bias down.  A layer that is absent from the dict has none.

backward() returns, after gat_qkv_ref's six results, {layer: db} with db_e = sum over the layer's heads of g_e / scale, the derivative of
L in the bias itself: the product does not export it, but a finite difference in b_e checks p_e through it.

The single passes take the bias in block order (entry e of the (rows, cols) list they are given): fwd_pass, fwd_pass_ld (np.longdouble),
row_pass, col_pass (over a block of S^T, bias in S^T's order)."""
import math

import numpy as np

import gat_pass_ref as P
import gat_qkv_ref as Q
import gat_skip_ref as S
from gat_ref import act, activations_of, adam_step, heads_of, row_softmax, sgd_step, true_grad, weights_of, xent

__all__ = ["forward", "backward", "train", "fwd_pass", "fwd_pass_ld", "row_pass", "col_pass", "keys", "bias_of", "hash_bias"]

scale_of = Q.scale_of
parameter_divergence = Q.parameter_divergence
_smat = Q._smat
_halves = Q._halves


def keys(rows, cols):
    """(row, col, copy) of every entry: copy = the number of earlier entries of the list with the same (row, col)"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.lexsort((np.arange(len(rows)), cols, rows))
    r, c = rows[order], cols[order]
    new = np.ones(len(r), dtype=bool)
    new[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    start = np.maximum.accumulate(np.where(new, np.arange(len(r)), 0))
    copy = np.empty(len(r), dtype=np.int64)
    copy[order] = np.arange(len(r)) - start
    return rows, cols, copy


def bias_of(fn, rows, cols):
    """fn(row, col, copy) -> float64 on the entries of (rows, cols)"""
    return np.asarray(fn(*keys(rows, cols)), dtype=np.float64)


def hash_bias(rows, cols, lo=-2.0, hi=2.0, salt=0):
    """A bias in [lo, hi) that depends on the global (row, col) alone, exactly computable anywhere: what GAT.edge_bias_from is given."""
    h = (np.asarray(rows, dtype=np.uint64) * np.uint64(2654435761) + np.asarray(cols, dtype=np.uint64) * np.uint64(40503) + np.uint64(salt)) % np.uint64(4093)
    return lo + (hi - lo) * h.astype(np.float64) / 4093.0


# ------------------------------------------------------------------------------------------------ single passes, as the kernels take them
def fwd_pass(rows, cols, m, q_rows, kv_cols, f, scale, bias):
    """(o, lse, s, p) with s the BIASED logit: gat_qkv_ref.fwd_pass with bias[e] on entry e"""
    k, v = _halves(kv_cols, f)
    s = scale * np.einsum("ij,ij->i", q_rows[rows, :f], k[cols]) + bias
    p, lse = row_softmax(rows, m, s)
    return _smat(rows, cols, p, (m, kv_cols.shape[0])) @ v, lse, s, p


def fwd_pass_ld(rows, cols, m, q_rows, kv_cols, f, scale, bias):
    """fwd_pass in np.longdouble (math.fsum where longdouble is no wider than fp64): (o, lse, s) as longdouble, before the activation."""
    ld = np.longdouble
    wide = np.finfo(ld).eps <= 1e-18
    order = np.argsort(rows, kind="stable")
    r, c, b = np.asarray(rows)[order], np.asarray(cols)[order], np.asarray(bias, dtype=ld)[order]
    k, v = _halves(kv_cols, f)
    q, k, v = np.asarray(q_rows[:, :f], dtype=ld), np.asarray(k, dtype=ld), np.asarray(v, dtype=ld)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))])
    o = np.zeros((m, f), dtype=ld)
    lse = np.zeros(m, dtype=ld)
    s_all = np.zeros(len(r), dtype=ld)
    for i in range(m):
        lo, hi = rowptr[i], rowptr[i + 1]
        if hi == lo:
            continue
        terms = q[i][None, :] * k[c[lo:hi]]
        s = (np.sum(terms, axis=1) if wide else np.array([math.fsum(row) for row in terms], dtype=ld)) * ld(scale) + b[lo:hi]
        s_all[lo:hi] = s
        mx = s.max()
        ex = np.exp(s - mx)
        tot = np.sum(ex) if wide else ld(math.fsum(ex))
        lse[i] = mx + np.log(tot)
        contrib = (ex[:, None] / tot) * v[c[lo:hi]]
        o[i] = np.sum(contrib, axis=0) if wide else [math.fsum(contrib[:, kk]) for kk in range(f)]
    back = np.empty_like(s_all)
    back[order] = s_all
    return o, lse, back


def row_pass(rows, cols, m, q_rows, dz_rows, lse, delta, kv_cols, f, scale, bias, out=None):
    """dQ (+ out) over a block of S, bias in the block's order"""
    k, v = _halves(kv_cols, f)
    s = scale * np.einsum("ij,ij->i", q_rows[rows, :f], k[cols]) + bias
    gij = scale * np.exp(s - lse[rows]) * (np.einsum("ij,ij->i", dz_rows[rows, :f], v[cols]) - delta[rows])
    r = np.zeros((m, f)) if out is None else np.array(out, copy=True)
    np.add.at(r, rows, gij[:, None] * k[cols])
    return r


def col_pass(trows, tcols, m, k_rows, v_rows, packed, f, scale, bias, out=None, out2=None):
    """(dK, dV) (+ out, out2) over a block of S^T, bias in S^T's order: entry e = (j, i) carries the bias of S_ij"""
    fp = f + (f & 1)
    yq, yz = _halves(packed, f)
    lse, delta = packed[:, 2 * fp], packed[:, 2 * fp + 1]
    s = scale * np.einsum("ij,ij->i", k_rows[trows, :f], yq[tcols]) + bias
    p = np.exp(s - lse[tcols])
    gij = scale * p * (np.einsum("ij,ij->i", v_rows[trows, :f], yz[tcols]) - delta[tcols])
    dk = np.zeros((m, f)) if out is None else np.array(out, copy=True)
    dv = np.zeros((m, f)) if out2 is None else np.array(out2, copy=True)
    np.add.at(dk, trows, gij[:, None] * yq[tcols])
    np.add.at(dv, trows, p[:, None] * yz[tcols])
    return dk, dv


# ------------------------------------------------------------------------------------------------ the model
def _bias(edge_bias, li, n):
    b = None if edge_bias is None else edge_bias.get(li)
    if b is None:
        return None
    b = np.asarray(b, dtype=np.float64)
    assert b.shape == (n,) and np.all(np.isfinite(b)), "one finite value per entry of the edge list"
    return b


def forward(rows, cols, m, x, layers, weights=None, wq=None, wk=None, *, edge_bias=None, rates=(0.0, 0.0), seed: int = 0, activations=None,
            residual=None, bias=None, res_weights=None, by_passes: bool = False, keep_trace: bool = False):
    """gat_qkv_ref.forward with edge_bias = {layer: one value per entry of (rows, cols)}; the trace's s is the biased logit."""
    p_attn, q = rates
    if p_attn > 0.0:
        raise ValueError("score transformer does not support attention dropout")
    acts = activations_of(layers, activations)
    res = S.residuals_of(layers, residual)
    w = weights_of(layers, weights)
    if wq is None or wk is None:
        wq, wk = Q.qk_weights_of(layers)
    trace = []
    for li, (fin, fph, heads) in enumerate(layers):
        assert x.shape[1] == fin
        ff = P.feature_factor(seed, li, x.shape, q) if q > 0.0 else None
        xd = x if ff is None else ff * x
        add = S.addend_of(xd, li, res, bias, res_weights)
        eb = _bias(edge_bias, li, len(rows))
        out = np.zeros((m, fph * heads))
        heads_t = []
        for h in range(heads):
            qm, km, vm = xd @ wq[(li, h)], xd @ wk[(li, h)], xd @ w[(li, h)]
            if by_passes:
                o, lse, s, p = fwd_pass(rows, cols, m, qm, np.nan_to_num(P.fused_pack(km, vm)), fph, scale_of(fph), 0.0 if eb is None else eb)
            else:
                s = scale_of(fph) * np.einsum("ij,ij->i", qm[rows], km[cols])
                if eb is not None:
                    s = s + eb
                p, lse = row_softmax(rows, m, s)
                o = _smat(rows, cols, p, (m, m)) @ vm
            sl = slice(h * fph, (h + 1) * fph)
            out[:, sl] = act(o if add is None else o + add[:, sl], acts[li])
            heads_t.append((vm, s, p, o, lse, (qm, km)))
        trace.append((xd, ff, out, heads_t))
        x = out
    return (x, trace) if keep_trace else x


def backward(rows, cols, m, x, layers, grad_out, weights=None, wq=None, wk=None, *, edge_bias=None, rates=(0.0, 0.0), seed: int = 0,
             activations=None, residual=None, bias=None, res_weights=None, by_passes: bool = False):
    """gat_qkv_ref.backward's six results, then {layer: dL/db_e per entry} for the layers that have an edge bias.  by_passes=True computes
    each head through the packed operands, the row pass and the column pass (over S^T, its bias in S^T's order: the transposed list)."""
    acts = activations_of(layers, activations)
    res = S.residuals_of(layers, residual)
    w = weights_of(layers, weights)
    if wq is None or wk is None:
        wq, wk = Q.qk_weights_of(layers)
    _, trace = forward(rows, cols, m, x, layers, w, wq, wk, edge_bias=edge_bias, rates=rates, seed=seed, activations=acts, residual=res, bias=bias,
                       res_weights=res_weights, by_passes=by_passes, keep_trace=True)
    g = grad_out
    dws, dwqs, dwks, dbs, dwrs, debs = {}, {}, {}, {}, {}, {}
    for li in range(len(layers) - 1, -1, -1):
        fin, fph, heads = layers[li]
        xd, ff, out, heads_t = trace[li]
        add = S.addend_of(xd, li, res, bias, res_weights)
        eb = _bias(edge_bias, li, len(rows))
        dxd = np.zeros_like(xd)
        dz_all = np.zeros_like(out)
        sc = scale_of(fph)
        if eb is not None:
            debs[li] = np.zeros(len(rows))
        for h in range(heads):
            vm, s, p, o, lse, (qm, km) = heads_t[h]
            sl = slice(h * fph, (h + 1) * fph)
            if add is None:
                dz, delta = true_grad(g[:, sl], o, out[:, sl], acts[li])
            else:
                dz, _ = true_grad(g[:, sl], o + add[:, sl], out[:, sl], acts[li])
                delta = np.sum(dz * o, axis=1)
            dz_all[:, sl] = dz
            gij = sc * p * (np.einsum("ij,ij->i", dz[rows], vm[cols]) - delta[rows])
            if by_passes:
                kv = np.nan_to_num(P.fused_pack(km, vm))
                b0 = 0.0 if eb is None else eb
                dq = row_pass(rows, cols, m, qm, dz, lse, delta, kv, fph, sc, b0)
                dk, dv = col_pass(cols, rows, m, km, vm, P.fused_pack(qm, dz, lse, delta), fph, sc, b0)  # (the same list read as S^T: the same order)
            else:
                sg = _smat(rows, cols, gij, (m, m))
                dq, dk, dv = sg @ km, sg.T @ qm, _smat(rows, cols, p, (m, m)).T @ dz
            if eb is not None:
                debs[li] += gij / sc
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
    return dws, dwqs, dwks, dbs, dwrs, g, debs


def pre_activations(rows, cols, m, x, layers, weights=None, wq=None, wk=None, **mode):
    """gat_qkv_ref.pre_activations for this model"""
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


def train(rows, cols, m, x, layers, labels, mask, heads, w, wq, wk, optimizer, steps, *, edge_bias=None, rates=(0.0, 0.0), seed0=0, activations=None,
          residual=None, bias=None, res_weights=None, perturb=None):
    """gat_qkv_ref.train with a fixed edge bias (no parameter: no optimizer touches it).  Returns (losses, accuracies, w, wq, wk, bias,
    res_weights)."""
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
        mode = dict(edge_bias=edge_bias, rates=rates, seed=(seed0 + t) & 0xFFFFFFFFFFFFFFFF if dropout else seed0, activations=activations,
                    residual=residual, bias=bt or None, res_weights=rt or None)
        out = forward(rows, cols, m, x, layers, wt, qt, kt, **mode)
        loss, acc, g = xent(out, labels, mask, nh)
        losses.append(float(loss))
        accs.append(float(acc))
        dw, dq, dk, db, dwr, _, _ = backward(rows, cols, m, x, layers, g, wt, qt, kt, **mode)
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
