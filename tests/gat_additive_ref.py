"""numpy reference of the GAT's additive (a1, a2) attention score (GAT score "additive", csrc/host/gat.hpp,
include/hnh_attn_additive.h) — the definition the tests hold the product to.  A sibling of gat_softmax_ref.py.

Per head h of a layer (A = X W_h, rows x f; a1, a2 = the head's vectors), over the nonzeros (i, j) of S (a repeated pair counts as often
as it appears):
    s_i = <A_i, a1>   t_j = <A_j, a2>   z_ij = s_i + t_j   e_ij = LeakyReLU_alpha(z_ij)
    lse_i = log sum_j exp(e_ij)   a_ij = exp(e_ij - lse_i)   o_i = sum_j a_ij A_j   out[:, h f ..] = ReLU(o)   (o_i = 0, lse_i = 0: empty row)
Backward, from dZ = G[:, h f ..] * [out > 0], delta_i = <dZ_i, o_i>:
    da_ij = <dZ_i, A_j>   dz_ij = a_ij (da_ij - delta_i) (z_ij > 0 ? 1 : alpha)
    ds_i = sum_j dz_ij    dt_j = sum_i dz_ij    dAgg_j = sum_i a_ij dZ_i
    dA = dAgg + ds a1^T + dt a2^T    da1 = A^T ds   da2 = A^T dt   dW_h = X^T dA   dX += dA W_h^T
The packed layouts (scored, pack) and the passes as the kernels take them (fwd_pass, row_pass, col_pass; fwd_pass_ld in extended
precision) are restated here too."""
import math

import numpy as np
import scipy.sparse as sp

from gat_backward_ref import weights_of
from gat_softmax_ref import leaky, row_softmax


def _smat(rows, cols, vals, m):
    return sp.csr_matrix((vals, (rows, cols)), shape=(m, m))  # duplicates are summed, as the passes over the list do


def vectors_of(layers, vectors=None, seed: int = 77, scale: float = 1.0):
    """{(layer, head): (a1, a2)} — the given ones, else seeded normal vectors of scale / sqrt(f)."""
    if vectors is not None:
        return vectors
    rng = np.random.default_rng(seed)
    return {(li, h): (rng.standard_normal(fph) * scale / np.sqrt(fph), rng.standard_normal(fph) * scale / np.sqrt(fph))
            for li, (fin, fph, heads) in enumerate(layers) for h in range(heads)}


# ------------------------------------------------------------------------------------------------ the packed layouts
def scored_width(f: int) -> int:
    return f + (f & 1) + 2


def packed_width(f: int) -> int:
    return f + (f & 1) + 4


def scored(a_mat, a1, a2, ld=None):
    """M = [A (0) | s t]; columns beyond the scored width (a wider pitch) hold NaN: nothing may read them."""
    n, f = a_mat.shape
    fp = f + (f & 1)
    m = np.full((n, ld or fp + 2), np.nan)
    m[:, :fp] = 0.0
    m[:, :f] = a_mat
    m[:, fp] = a_mat @ a1
    m[:, fp + 1] = a_mat @ a2
    return m


def pack(dz, s, lse, delta, ld=None):
    """Q = [dZ (0) | s lse delta 0]"""
    n, f = dz.shape
    fp = f + (f & 1)
    q = np.full((n, ld or fp + 4), np.nan)
    q[:, :fp + 4] = 0.0
    q[:, :f] = dz
    q[:, fp], q[:, fp + 1], q[:, fp + 2] = s, lse, delta
    return q


# ------------------------------------------------------------------------------------------------ the three passes, as the kernels take them
def fwd_pass(rows, cols, m, m_rows, m_cols, f, alpha):
    """(o, lse, z): row operand m_rows (scored rows of the block's rows), gathered operand m_cols."""
    fp = f + (f & 1)
    z = m_rows[rows, fp] + m_cols[cols, fp + 1]
    a, lse = row_softmax(rows, m, leaky(z, alpha))
    return _rect(rows, cols, a, m, m_cols[:, :f]), lse, z


def _rect(rows, cols, vals, m, y):
    return sp.csr_matrix((vals, (rows, cols)), shape=(m, y.shape[0])) @ y


def fwd_pass_ld(rows, cols, m, m_rows, m_cols, f, alpha, chunk: int = 8192):
    """fwd_pass in np.longdouble (math.fsum per row where longdouble is no wider than fp64): (o, lse) as longdouble."""
    ld = np.longdouble
    wide = np.finfo(ld).eps <= 1e-18
    fp = f + (f & 1)
    order = np.argsort(rows, kind="stable")
    r, c = np.asarray(rows)[order], np.asarray(cols)[order]
    z = np.asarray(m_rows[:, fp], dtype=ld)[r] + np.asarray(m_cols[:, fp + 1], dtype=ld)[c]
    e = np.maximum(z, ld(0)) + np.minimum(z, ld(0)) * ld(alpha)
    yc = np.asarray(m_cols[:, :f], dtype=ld)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))])
    mx = np.full(m, -np.inf, dtype=ld)
    np.maximum.at(mx, r, e)
    ex = np.exp(e - mx[r])
    o = np.zeros((m, f), dtype=ld)
    lse = np.zeros(m, dtype=ld)
    for i in range(m):
        b, t = rowptr[i], rowptr[i + 1]
        if t == b:
            continue
        tot = np.sum(ex[b:t]) if wide else ld(math.fsum(ex[b:t]))
        lse[i] = mx[i] + np.log(tot)
        contrib = (ex[b:t, None] / tot) * yc[c[b:t]]
        o[i] = np.sum(contrib, axis=0) if wide else [math.fsum(contrib[:, k]) for k in range(f)]
    return o, lse


def gate(z, lse_nz, da, delta_nz, alpha):
    """(a, dz) per nonzero"""
    a = np.exp(leaky(z, alpha) - lse_nz)
    return a, a * (da - delta_nz) * np.where(z > 0, 1.0, alpha)


def row_pass(rows, cols, m, dz_rows, m_rows, lse, delta, m_cols, f, alpha):
    """ds over a block of S: the rows' dZ, s, lse, delta; gathered M."""
    fp = f + (f & 1)
    z = m_rows[rows, fp] + m_cols[cols, fp + 1]
    da = np.einsum("ij,ij->i", dz_rows[rows], m_cols[cols, :f])
    _, dzz = gate(z, lse[rows], da, delta[rows], alpha)
    return np.bincount(rows, weights=dzz, minlength=m)


def col_pass(trows, tcols, m, m_rows, q_cols, f, alpha):
    """(dAgg, dt) over a block of S^T: row j = trows (A_j, t_j from the scored rows), nonzero (j, i) gathers Q_i."""
    fp = f + (f & 1)
    z = q_cols[tcols, fp] + m_rows[trows, fp + 1]
    da = np.einsum("ij,ij->i", m_rows[trows, :f], q_cols[tcols, :f])
    a, dzz = gate(z, q_cols[tcols, fp + 1], da, q_cols[tcols, fp + 2], alpha)
    return _rect(trows, tcols, a, m, q_cols[:, :f]), np.bincount(trows, weights=dzz, minlength=m)


# ------------------------------------------------------------------------------------------------ the model
def forward(rows, cols, m, x, layers, alpha: float, weights=None, vectors=None, keep: bool = False):
    """The forward pass with explicit weights and vectors; keep=True also returns per layer the inputs and per head (A, z, a, o, lse)."""
    w = weights_of(layers, weights)
    av = vectors_of(layers, vectors)
    trace = []
    for li, (fin, fph, heads) in enumerate(layers):
        assert x.shape[1] == fin
        out = np.zeros((m, fph * heads))
        heads_t = []
        for h in range(heads):
            a_mat = x @ w[(li, h)]
            a1, a2 = av[(li, h)]
            z = (a_mat @ a1)[rows] + (a_mat @ a2)[cols]
            a, lse = row_softmax(rows, m, leaky(z, alpha))
            o = _smat(rows, cols, a, m) @ a_mat
            out[:, h * fph:(h + 1) * fph] = np.maximum(o, 0.0)
            heads_t.append((a_mat, z, a, o, lse))
        trace.append((x, out, heads_t))
        x = out
    return (x, trace) if keep else x


def backward(rows, cols, m, x, layers, alpha: float, grad_out, weights=None, vectors=None, by_passes: bool = False):
    """Returns ({(layer, head): dW}, {(layer, head): (da1, da2)}, dX0) for L with dL/d(output) = grad_out.  by_passes=True computes each
    head through the packed operands and the two passes (row_pass over S, col_pass over S^T), as the product does."""
    w = weights_of(layers, weights)
    av = vectors_of(layers, vectors)
    _, trace = forward(rows, cols, m, x, layers, alpha, w, av, keep=True)
    g = grad_out
    dws, das = {}, {}
    for li in range(len(layers) - 1, -1, -1):
        fin, fph, heads = layers[li]
        xin, out, heads_t = trace[li]
        dx = np.zeros_like(xin)
        for h in range(heads):
            a_mat, z, a, o, lse = heads_t[h]
            a1, a2 = av[(li, h)]
            sl = slice(h * fph, (h + 1) * fph)
            dz = g[:, sl] * (out[:, sl] > 0)
            delta = np.sum(dz * o, axis=1)
            if by_passes:
                mm = scored(a_mat, a1, a2)
                q = pack(dz, mm[:, fph + (fph & 1)], lse, delta)
                ds = row_pass(rows, cols, m, dz, mm, lse, delta, mm, fph, alpha)
                dagg, dt = col_pass(cols, rows, m, mm, q, fph, alpha)
            else:
                da = np.einsum("ij,ij->i", dz[rows], a_mat[cols])
                dzz = a * (da - delta[rows]) * np.where(z > 0, 1.0, alpha)
                ds = np.bincount(rows, weights=dzz, minlength=m)
                dt = np.bincount(cols, weights=dzz, minlength=m)
                dagg = _smat(rows, cols, a, m).T @ dz
            da_mat = dagg + np.outer(ds, a1) + np.outer(dt, a2)
            das[(li, h)] = (a_mat.T @ ds, a_mat.T @ dt)
            dws[(li, h)] = xin.T @ da_mat
            dx += da_mat @ w[(li, h)].T
        g = dx
    return dws, das, g


def pre_activations(rows, cols, m, x, layers, alpha: float, weights=None, vectors=None):
    """Every LeakyReLU input z and every ReLU input o of rows that have a nonzero (other rows are identically zero)."""
    _, trace = forward(rows, cols, m, x, layers, alpha, weights, vectors, keep=True)
    live = np.zeros(m, dtype=bool)
    live[rows] = True
    out = []
    for _, _, heads_t in trace:
        for _, z, _, o, _ in heads_t:
            out.append(z)
            out.append(o[live].reshape(-1))
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------ training
SGD_STEPS, SGD_LR_SCALE, SGD_TARGET_SCALE = 5, 0.02, 0.05  # the quadratic loss of test_sgd_lowers_the_loss (softmax), on W, a1 and a2


def sgd_step_size(lr_scale, w, av, dw, da):
    """lr_scale * |parameters| / |gradient| over W, a1 and a2 of every (layer, head), fixed at the first step."""
    num = sum(np.sum(v * v) for v in w.values()) + sum(np.sum(a * a) + np.sum(b * b) for a, b in av.values())
    den = sum(np.sum(v * v) for v in dw.values()) + sum(np.sum(a * a) + np.sum(b * b) for a, b in da.values())
    return lr_scale * np.sqrt(num / den)


def sgd(rows, cols, m, x, layers, alpha, target, w, av, steps=SGD_STEPS, lr_scale=SGD_LR_SCALE):
    """Plain gradient descent on 0.5 |out - target|^2: returns (losses of steps + 1 forward passes, final vectors)."""
    w = dict(w)
    av = {k: (a.copy(), b.copy()) for k, (a, b) in av.items()}
    losses, lr = [], None
    for step in range(steps + 1):
        diff = forward(rows, cols, m, x, layers, alpha, w, av) - target
        losses.append(0.5 * float(np.sum(diff * diff)))
        if step == steps:
            break
        dw, da, _ = backward(rows, cols, m, x, layers, alpha, diff, w, av)
        if lr is None:
            lr = sgd_step_size(lr_scale, w, av, dw, da)
        w = {k: w[k] - lr * dw[k] for k in w}
        av = {k: (av[k][0] - lr * da[k][0], av[k][1] - lr * da[k][1]) for k in av}
    return losses, av
