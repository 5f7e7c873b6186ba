"""numpy reference of the GAT's score "gatv2" (include/hnh_attn_v2.h; Brody, Alon and Yahav's dynamic attention with shared weights), next
to tests/gat_ref.py, whose small pieces it reuses and which raises on the score it does not know.

Per head h of layer l, A = Xd W_h, a = the head's ONE vector (f entries), over the nonzeros (i, j) of S (values 1; a repeated pair counts as
often as it appears):
    u_ijc = A_ic + A_jc      sg_ijc = u_ijc > 0 ? 1 : alpha      z_ij = sum_c a_c sg_ijc u_ijc      (no outer LeakyReLU)
    lse_i = log sum_j exp(z_ij)     p_ij = exp(z_ij - lse_i)     o_i = sum_j p_ij A_j     out[:, h f:(h+1) f] = phi(o)
Backward, from G = dL/d(out), with dZ = G phi'(o) and delta_i = <dZ_i, o_i>:
    g_ij = p_ij (<dZ_i, A_j> - delta_i)
    definition:  dA_i += sum_j g_ij (a o sg_ij),  dA_j += sum_i g_ij (a o sg_ij) + p_ij dZ_i,  da = sum_ij g_ij LReLU(u_ij)
    by passes:   R_ic = sum_j g_ij sg_ijc (row pass over S),  C_jc = sum_i g_ij sg_ijc and dAgg_j = sum_i p_ij dZ_i (column pass over S^T,
                 gathering the packed P_i = [A_i | dZ_i | lse_i delta_i] of gat_pass_ref.fused_pack),  T = R + C,  dA = dAgg + T o a,
                 da_c = sum_r A_rc T_rc   (LReLU(u) = sg (A_ic + A_jc): the sum over the nonzeros splits into the two sides)
    dW_h = Xd^T dA,   dX = c_q mask o sum_h dA W_h^T
Vectors are {(layer, head): a}; a pair (a1, a2), the shape gat_ref and the product's set_attention_vectors use, is read as a = a1."""
import math

import numpy as np
import scipy.sparse as sp

import gat_pass_ref as P
from gat_ref import act, activations_of, adam_step, heads_of, leaky, row_softmax, sgd_step, true_grad, weights_of, xent

__all__ = ["forward", "backward", "train", "fwd_pass", "fwd_pass_ld", "row_pass", "col_pass", "finish", "stored_grad"]
from gat_ref import stored_grad  # noqa: E402,F401  (the product's dZ and delta from the stored output: the same for every score)


def vec(v):
    return v[0] if isinstance(v, tuple) else v


def vectors_of(layers, vectors=None, seed: int = 78, scale: float = 1.0):
    """{(layer, head): a} — the given ones, else seeded normal vectors of scale / sqrt(f)."""
    if vectors is not None:
        return {k: vec(v) for k, v in vectors.items()}
    rng = np.random.default_rng(seed)
    return {(li, h): rng.standard_normal(fph) * scale / np.sqrt(fph) for li, (fin, fph, heads) in enumerate(layers) for h in range(heads)}


def _smat(rows, cols, vals, shape):
    return sp.csr_matrix((vals, (rows, cols)), shape=shape)  # duplicates are summed, as the passes over the list do


def edge_sums(x_rows, y_cols, rows, cols):
    """u = A_i + A_j per nonzero (nnz x f)"""
    return x_rows[rows] + y_cols[cols]


def scores(x_rows, y_cols, rows, cols, a, alpha):
    """(z, u) per nonzero"""
    u = edge_sums(x_rows, y_cols, rows, cols)
    return leaky(u, alpha) @ a, u


# ------------------------------------------------------------------------------------------------ the model
def forward(rows, cols, m, x, layers, alpha: float, weights=None, vectors=None, *, rates=(0.0, 0.0), seed: int = 0, activations=None,
            keep_trace: bool = False):
    """The forward pass (attention softmax; rates = (0, q): the product refuses attention dropout with this score).  keep_trace=True also
    returns per layer (Xd, feature factor, out, heads) with per head (A, z, p, o, lse, u)."""
    p_attn, q = rates
    if p_attn > 0.0:
        raise ValueError("score gatv2 does not support attention dropout")
    acts = activations_of(layers, activations)
    w = weights_of(layers, weights)
    av = vectors_of(layers, vectors)
    trace = []
    for li, (fin, fph, heads) in enumerate(layers):
        assert x.shape[1] == fin
        ff = P.feature_factor(seed, li, x.shape, q) if q > 0.0 else None
        xd = x if ff is None else ff * x
        out = np.zeros((m, fph * heads))
        heads_t = []
        for h in range(heads):
            a_mat = xd @ w[(li, h)]
            z, u = scores(a_mat, a_mat, rows, cols, av[(li, h)], alpha)
            p, lse = row_softmax(rows, m, z)
            o = _smat(rows, cols, p, (m, m)) @ a_mat
            out[:, h * fph:(h + 1) * fph] = act(o, acts[li])
            heads_t.append((a_mat, z, p, o, lse, u))
        trace.append((xd, ff, out, heads_t))
        x = out
    return (x, trace) if keep_trace else x


def backward(rows, cols, m, x, layers, alpha: float, grad_out, weights=None, vectors=None, *, rates=(0.0, 0.0), seed: int = 0, activations=None,
             by_passes: bool = False):
    """({(layer, head): dW}, {(layer, head): da}, dX0) for L with dL/d(output) = grad_out, the feature masks held fixed.  by_passes=True
    computes each head's dA and da through the packed operand, the row pass, the column pass (over S^T) and the finish, as the product does."""
    acts = activations_of(layers, activations)
    w = weights_of(layers, weights)
    av = vectors_of(layers, vectors)
    _, trace = forward(rows, cols, m, x, layers, alpha, w, av, rates=rates, seed=seed, activations=acts, keep_trace=True)
    g = grad_out
    dws, das = {}, {}
    for li in range(len(layers) - 1, -1, -1):
        fin, fph, heads = layers[li]
        xd, ff, out, heads_t = trace[li]
        dxd = np.zeros_like(xd)
        for h in range(heads):
            a_mat, z, p, o, lse, u = heads_t[h]
            a = av[(li, h)]
            sl = slice(h * fph, (h + 1) * fph)
            dz, delta = true_grad(g[:, sl], o, out[:, sl], acts[li])
            if by_passes:
                packed = P.fused_pack(a_mat, dz, lse, delta)
                rm = row_pass(rows, cols, m, a_mat, dz, lse, delta, a_mat, a, fph, alpha)
                cm, dagg = col_pass(cols, rows, m, a_mat, a, packed, fph, alpha)
                da_mat, da_vec = finish(dagg, rm, cm, a_mat, a)
            else:
                gij = p * (np.einsum("ij,ij->i", dz[rows], a_mat[cols]) - delta[rows])
                du = gij[:, None] * (np.where(u > 0, 1.0, alpha) * a[None, :])  # dL/du_ij
                da_mat = np.zeros((m, fph))
                np.add.at(da_mat, rows, du)
                np.add.at(da_mat, cols, du)
                da_mat += _smat(rows, cols, p, (m, m)).T @ dz
                da_vec = gij @ leaky(u, alpha)
            das[(li, h)] = da_vec
            dws[(li, h)] = xd.T @ da_mat
            dxd += da_mat @ w[(li, h)].T
        g = dxd if ff is None else ff * dxd
    return dws, das, g


def pre_activations(rows, cols, m, x, layers, alpha: float, weights=None, vectors=None, **mode):
    """Everything a finite-difference step must not carry across 0, as one vector: every u_ijc = A_ic + A_jc of every head (the kinks sit
    per edge and per feature) and every aggregate of a row that has a nonzero."""
    _, trace = forward(rows, cols, m, x, layers, alpha, weights, vectors, keep_trace=True, **mode)
    live = np.zeros(m, dtype=bool)
    live[rows] = True
    return np.concatenate([v for _, _, _, heads_t in trace for ht in heads_t for v in (ht[5].reshape(-1), ht[3][live].reshape(-1))])


def train(rows, cols, m, x, layers, alpha, labels, mask, heads, w, av, optimizer, steps, rates=(0.0, 0.0), seed0=0, activations=None, perturb=None):
    """gat_ref.train for this score: K steps over every W and every a.  Returns (losses, accuracies, w, av)."""
    nh, _ = heads_of(layers, heads)
    opt = dict(optimizer)
    kind, lr = opt.pop("kind"), opt.pop("lr")
    av = vectors_of(layers, av)
    params = {("w",) + k: v.copy() for k, v in w.items()}
    params.update({("a",) + k: av[k].copy() for k in av})
    mom = {k: np.zeros_like(v) for k, v in params.items()}
    var = {k: np.zeros_like(v) for k, v in params.items()}
    losses, accs = [], []
    dropout = rates[1] > 0.0
    for t in range(1, steps + 1):
        mode = dict(rates=rates, seed=(seed0 + t) & 0xFFFFFFFFFFFFFFFF if dropout else seed0, activations=activations)
        wt = {k: params[("w",) + k] for k in w}
        at = {k: params[("a",) + k] for k in av}
        out = forward(rows, cols, m, x, layers, alpha, wt, at, **mode)
        loss, acc, g = xent(out, labels, mask, nh)
        losses.append(float(loss))
        accs.append(float(acc))
        dw, da, _ = backward(rows, cols, m, x, layers, alpha, g, wt, at, **mode)
        grads = {("w",) + k: dw[k] for k in dw}
        grads.update({("a",) + k: da[k] for k in da})
        for k in params:
            gk = grads[k]
            if perturb is not None:
                scale, rng = perturb
                gk = gk + scale * np.max(np.abs(gk)) * rng.uniform(-1.0, 1.0, gk.shape)
            if kind == "adam":
                params[k], mom[k], var[k] = adam_step(params[k], gk, mom[k], var[k], t, lr, **opt)
            else:
                params[k], var[k] = sgd_step(params[k], gk, var[k], lr, **opt)
    return losses, accs, {k: params[("w",) + k] for k in w}, {k: params[("a",) + k] for k in av}


def parameter_divergence(w_a, av_a, w_b, av_b):
    """max over the tensors of max|a - b| / max|b|"""
    worst = 0.0
    for k in w_b:
        worst = max(worst, float(np.max(np.abs(w_a[k] - w_b[k])) / np.max(np.abs(w_b[k]))))
        worst = max(worst, float(np.max(np.abs(vec(av_a[k]) - vec(av_b[k]))) / np.max(np.abs(vec(av_b[k])))))
    return worst


# ------------------------------------------------------------------------------------------------ single passes, as the kernels take them
def fwd_pass(rows, cols, m, x_rows, y_cols, a, f, alpha):
    """(o, lse, z, p): row operand x_rows (A of the block's rows), gathered operand y_cols (A of the block's columns, f columns read)"""
    z, _ = scores(x_rows[:, :f], y_cols[:, :f], rows, cols, a, alpha)
    p, lse = row_softmax(rows, m, z)
    return _smat(rows, cols, p, (m, y_cols.shape[0])) @ y_cols[:, :f], lse, z, p


def fwd_pass_ld(rows, cols, m, x_rows, y_cols, a, f, alpha):
    """fwd_pass in np.longdouble (math.fsum where longdouble is no wider than fp64): (o, lse) as longdouble, before the activation."""
    ld = np.longdouble
    wide = np.finfo(ld).eps <= 1e-18
    order = np.argsort(rows, kind="stable")
    r, c = np.asarray(rows)[order], np.asarray(cols)[order]
    xr, yc, al = np.asarray(x_rows[:, :f], dtype=ld), np.asarray(y_cols[:, :f], dtype=ld), np.asarray(a, dtype=ld)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))])
    o = np.zeros((m, f), dtype=ld)
    lse = np.zeros(m, dtype=ld)
    for i in range(m):
        b, t = rowptr[i], rowptr[i + 1]
        if t == b:
            continue
        u = xr[i][None, :] + yc[c[b:t]]
        terms = (np.maximum(u, ld(0)) + np.minimum(u, ld(0)) * ld(alpha)) * al[None, :]
        z = np.sum(terms, axis=1) if wide else np.array([math.fsum(row) for row in terms], dtype=ld)
        mx = z.max()
        ex = np.exp(z - mx)
        tot = np.sum(ex) if wide else ld(math.fsum(ex))
        lse[i] = mx + np.log(tot)
        contrib = (ex[:, None] / tot) * yc[c[b:t]]
        o[i] = np.sum(contrib, axis=0) if wide else [math.fsum(contrib[:, k]) for k in range(f)]
    return o, lse


def row_pass(rows, cols, m, x_rows, dz_rows, lse, delta, y_cols, a, f, alpha, out=None):
    """R (+ out): R_i = sum_j g_ij sg_ij over a block of S; the own rows' A, dZ, lse, delta, the gathered A_j."""
    z, u = scores(x_rows[:, :f], y_cols[:, :f], rows, cols, a, alpha)
    gij = np.exp(z - lse[rows]) * (np.einsum("ij,ij->i", dz_rows[rows, :f], y_cols[cols, :f]) - delta[rows])
    r = np.zeros((m, f)) if out is None else np.array(out, copy=True)
    np.add.at(r, rows, gij[:, None] * np.where(u > 0, 1.0, alpha))
    return r


def col_pass(trows, tcols, m, x_rows, a, packed, f, alpha, out=None, out2=None):
    """(C, dAgg) (+ out, out2) over a block of S^T: row j = trows is local (A_j = x_rows), nonzero (j, i) gathers the packed
    P_i = [A_i (0) | dZ_i (0) | lse_i delta_i] (gat_pass_ref.fused_pack with softmax)."""
    fp = f + (f & 1)
    ya, yz, lse, delta = packed[:, :f], packed[:, fp:fp + f], packed[:, 2 * fp], packed[:, 2 * fp + 1]
    z, u = scores(x_rows[:, :f], ya, trows, tcols, a, alpha)
    p = np.exp(z - lse[tcols])
    gij = p * (np.einsum("ij,ij->i", x_rows[trows, :f], yz[tcols]) - delta[tcols])
    cm = np.zeros((m, f)) if out is None else np.array(out, copy=True)
    dagg = np.zeros((m, f)) if out2 is None else np.array(out2, copy=True)
    np.add.at(cm, trows, gij[:, None] * np.where(u > 0, 1.0, alpha))
    np.add.at(dagg, trows, p[:, None] * yz[tcols])
    return cm, dagg


def finish(dagg, rm, cm, a_mat, a):
    """(dA, da): dA = dAgg + (R + C) o a, da = colsum(A o (R + C))"""
    t = rm + cm
    return dagg + t * a[None, :], np.sum(a_mat * t, axis=0)
