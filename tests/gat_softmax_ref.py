"""numpy reference of the GAT's softmax attention (GAT attention mode "softmax", csrc/host/gat.hpp, include/hnh_attention.h) — the
definition the tests hold the product to.  A sibling of gat_backward_ref.py.

Forward, per head h of layer i: X = input of the layer, A = X W_h, on the nonzeros (i, j) of S (a repeated pair counts as often as
it appears):
    s_ij = LeakyReLU_alpha(<A_i, A_j>)
    m_i = max_j s_ij,   l_i = sum_j exp(s_ij - m_i),   lse_i = m_i + log l_i,   a_ij = exp(s_ij - lse_i)
    o_i = sum_j a_ij A_j   (0 for a row without nonzeros),   out[:, h f:(h+1) f] = ReLU(o)
Backward, from G = dL/d(out):
    dZ    = G[:, cols] * [out[:, cols] > 0],   delta_i = <dZ_i, o_i>
    ds_ij = a_ij (<dZ_i, A_j> - delta_i),      de_ij = ds_ij * LeakyReLU'_alpha(e_ij)
    dA    = S_de A  +  S_a^T dZ  +  S_de^T A,  dW_h = X^T dA,  dX += dA W_h^T
attention_ld is attention() in extended precision (the kernel tests' reference); max_rises finds where a row's running max rises."""
import math

import numpy as np
import scipy.sparse as sp

from gat_backward_ref import weights_of


def _smat(rows, cols, vals, m):
    return sp.csr_matrix((vals, (rows, cols)), shape=(m, m))  # duplicates are summed, as SpMM over the list does


def leaky(e, alpha: float):
    return np.maximum(e, 0.0) + np.minimum(e, 0.0) * alpha


def row_softmax(rows, m, s):
    """(a, lse): the softmax weights of the scores s over each row's nonzeros, and lse per row (0 for a row without nonzeros)."""
    mx = np.full(m, -np.inf)
    np.maximum.at(mx, rows, s)
    ex = np.exp(s - mx[rows])
    tot = np.bincount(rows, weights=ex, minlength=m)
    live = tot > 0
    lse = np.zeros(m)
    lse[live] = mx[live] + np.log(tot[live])
    return np.exp(s - lse[rows]), lse


def attention(rows, cols, m, y_rows, y_cols, alpha: float):
    """One softmax pass with row operand y_rows and gathered operand y_cols (the kernel's X and Y): returns (o, lse, s)."""
    s = leaky(np.einsum("ij,ij->i", y_rows[rows], y_cols[cols]), alpha)
    a, lse = row_softmax(rows, m, s)
    return _smat(rows, cols, a, m) @ y_cols, lse, s


def attention_ld(rows, cols, m, y_rows, y_cols, alpha: float, chunk: int = 8192, fsum=None):
    """attention() with the scores, max, sum, lse and o in np.longdouble: (o, lse, s) as longdouble arrays.  Where longdouble is no
    wider than fp64 (or fsum=True) the sums of a row (l and every column of o) are taken with math.fsum instead."""
    ld = np.longdouble
    wide = not fsum if fsum is not None else np.finfo(ld).eps <= 1e-18
    order = np.argsort(rows, kind="stable")
    r, c = np.asarray(rows)[order], np.asarray(cols)[order]
    xr, yc = np.asarray(y_rows, dtype=ld), np.asarray(y_cols, dtype=ld)
    n = len(r)
    s = np.empty(n, dtype=ld)
    for e0 in range(0, n, chunk):
        e1 = min(n, e0 + chunk)
        s[e0:e1] = np.sum(xr[r[e0:e1]] * yc[c[e0:e1]], axis=1)
    s = np.maximum(s, ld(0)) + np.minimum(s, ld(0)) * ld(alpha)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))])
    mx = np.full(m, -np.inf, dtype=ld)
    np.maximum.at(mx, r, s)
    ex = np.exp(s - mx[r])
    tot = np.zeros(m, dtype=ld)
    live = rowptr[1:] > rowptr[:-1]
    if wide:
        np.add.at(tot, r, ex)
    else:
        for i in np.nonzero(live)[0]:
            tot[i] = math.fsum(ex[rowptr[i]:rowptr[i + 1]])
    lse = np.zeros(m, dtype=ld)
    lse[live] = mx[live] + np.log(tot[live])
    a = np.exp(s - lse[r])
    o = np.zeros((m, yc.shape[1]), dtype=ld)
    r0 = 0
    while r0 < m:  # whole rows, about `chunk` nonzeros at a time
        r1 = max(r0 + 1, int(np.searchsorted(rowptr, rowptr[r0] + chunk, side="right")) - 1)
        r1 = min(r1, m)
        e0, e1 = rowptr[r0], rowptr[r1]
        if e1 > e0:
            contrib = a[e0:e1, None] * yc[c[e0:e1]]
            nz = np.nonzero(live[r0:r1])[0]
            if wide:
                o[r0 + nz] = np.add.reduceat(contrib, rowptr[r0 + nz] - e0, axis=0)
            else:
                for i in nz:
                    seg = contrib[rowptr[r0 + i] - e0:rowptr[r0 + i + 1] - e0]
                    o[r0 + i] = [math.fsum(seg[:, k]) for k in range(seg.shape[1])]
        r0 = r1
    s_out = np.empty(n, dtype=ld)
    s_out[order] = s
    return o, lse, s_out


def max_rises(rowptr, s):
    """Per row, the positions (0-based within the row, in row order) where the prefix max of the scores s rises strictly: the
    nonzeros at which the online softmax rescales its state.  Position 0 of a non-empty row always counts (it leaves the empty state)."""
    s = np.asarray(s)
    out = []
    for i in range(len(rowptr) - 1):
        seg = s[rowptr[i]:rowptr[i + 1]]
        if len(seg) == 0:
            out.append(np.zeros(0, dtype=np.int64))
            continue
        before = np.concatenate([[-np.inf], np.maximum.accumulate(seg)[:-1]])
        out.append(np.nonzero(seg > before)[0])
    return out


def forward(rows, cols, m, x, layers, alpha: float, weights=None, keep: bool = False):
    """The forward pass with explicit weights; keep=True also returns per layer the inputs and per head (A, e, a, o, lse)."""
    w = weights_of(layers, weights)
    trace = []
    for li, (fin, fph, heads) in enumerate(layers):
        assert x.shape[1] == fin
        out = np.zeros((m, fph * heads))
        heads_t = []
        for h in range(heads):
            a_mat = x @ w[(li, h)]
            e = np.einsum("ij,ij->i", a_mat[rows], a_mat[cols])
            a, lse = row_softmax(rows, m, leaky(e, alpha))
            o = _smat(rows, cols, a, m) @ a_mat
            out[:, h * fph:(h + 1) * fph] = np.maximum(o, 0.0)
            heads_t.append((a_mat, e, a, o, lse))
        trace.append((x, out, heads_t))
        x = out
    return (x, trace) if keep else x


def backward(rows, cols, m, x, layers, alpha: float, grad_out, weights=None):
    """Returns ({(layer, head): dW}, dX0) for L with dL/d(output) = grad_out."""
    w = weights_of(layers, weights)
    _, trace = forward(rows, cols, m, x, layers, alpha, w, keep=True)
    g = grad_out
    dws = {}
    for li in range(len(layers) - 1, -1, -1):
        fin, fph, heads = layers[li]
        xin, out, heads_t = trace[li]
        dx = np.zeros_like(xin)
        for h in range(heads):
            a_mat, e, a, o, _ = heads_t[h]
            sl = slice(h * fph, (h + 1) * fph)
            dz = g[:, sl] * (out[:, sl] > 0)
            delta = np.sum(dz * o, axis=1)
            da = np.einsum("ij,ij->i", dz[rows], a_mat[cols])
            de = a * (da - delta[rows]) * np.where(e > 0, 1.0, alpha)
            s_de = _smat(rows, cols, de, m)
            da_mat = s_de @ a_mat + _smat(rows, cols, a, m).T @ dz + s_de.T @ a_mat
            dws[(li, h)] = xin.T @ da_mat
            dx += da_mat @ w[(li, h)].T
        g = dx
    return dws, g


def pre_activations(rows, cols, m, x, layers, alpha: float, weights=None):
    """Every LeakyReLU input e and every ReLU input o of rows that have a nonzero (other rows are identically zero)."""
    _, trace = forward(rows, cols, m, x, layers, alpha, weights, keep=True)
    live = np.zeros(m, dtype=bool)
    live[rows] = True
    out = []
    for _, _, heads_t in trace:
        for _, e, _, o, _ in heads_t:
            out.append(e)
            out.append(o[live].reshape(-1))
    return np.concatenate(out)
