"""numpy restatement of the GAT's FUSED backward mode (include/hnh_attn_grad.h, csrc/host/gat.hpp) — the two passes as the kernels
see them, over the nonzero lists of S and S^T and the packed operand.  The definitions the product is held to stay
gat_backward_ref.backward and gat_softmax_ref.backward; this file only has to agree with them (tests/test_gat_fused_backward_cpu.py),
and serves the kernel tests as the per-pass reference.

    row pass over S      (i, j):  e = <A_i, Y_j>, da = <dZ_i, Y_j>, gate with lse_i / delta_i,  Out_i += de Y_j
    column pass over S^T (j, i):  e = <X_j, P_i[0:f]>, da = <X_j, P_i[fp:fp+f]>, gate with P_i[2fp], P_i[2fp+1],
                                  Out_j += a P_i[fp:fp+f] + de P_i[0:f]
with g(e) = e > 0 ? 1 : alpha and
    attention none:     a = LeakyReLU(e),            de = da g(e)
    attention softmax:  a = exp(LeakyReLU(e) - lse), de = a (da - delta) g(e)
A repeated (row, column) pair counts as often as it appears."""
import numpy as np

import gat_backward_ref as RN
import gat_softmax_ref as RS


def packed_width(f: int, softmax: bool) -> int:
    return 2 * (f + (f & 1)) + (2 if softmax else 0)


def pack(a_mat, dz, lse=None, delta=None, ld=None):
    """P = [A (0) | dZ (0) | lse delta] with the pad column present when f is odd; columns beyond the packed width keep NaN."""
    rows, f = a_mat.shape
    fp = f + (f & 1)
    pw = packed_width(f, lse is not None)
    p = np.full((rows, ld if ld is not None else pw), np.nan)
    p[:, :pw] = 0.0
    p[:, :f] = a_mat
    p[:, fp:fp + f] = dz
    if lse is not None:
        p[:, 2 * fp] = lse
        p[:, 2 * fp + 1] = delta
    return p


def gate(e, da, alpha, lse=None, delta=None):
    """(a, de) per nonzero; lse / delta already gathered onto the nonzeros."""
    slope = np.where(e > 0, 1.0, alpha)
    s = e * slope
    if lse is None:
        return s, da * slope
    a = np.exp(s - lse)
    return a, a * (da - delta) * slope


def row_pass(rows, cols, m, a_mat, dz, y, alpha, lse=None, delta=None, out=None):
    """Out (m x f, or `out` accumulated in place) after the row pass over the nonzeros (rows[k], cols[k])."""
    f = a_mat.shape[1]
    out = np.zeros((m, f)) if out is None else out
    yj = y[cols, :f]
    e = np.einsum("ij,ij->i", a_mat[rows, :f], yj)
    da = np.einsum("ij,ij->i", dz[rows, :f], yj)
    _, de = gate(e, da, alpha, None if lse is None else lse[rows], None if delta is None else delta[rows])
    np.add.at(out, rows, de[:, None] * yj)
    return out


def col_pass(rows_t, cols_t, m, x, p, f, softmax, alpha, out=None):
    """Out after the column pass over the nonzeros (rows_t[k], cols_t[k]) of S^T with the packed operand p."""
    fp = f + (f & 1)
    out = np.zeros((m, f)) if out is None else out
    pa, pz = p[cols_t, :f], p[cols_t, fp:fp + f]
    e = np.einsum("ij,ij->i", x[rows_t, :f], pa)
    da = np.einsum("ij,ij->i", x[rows_t, :f], pz)
    a, de = gate(e, da, alpha, p[cols_t, 2 * fp] if softmax else None, p[cols_t, 2 * fp + 1] if softmax else None)
    np.add.at(out, rows_t, a[:, None] * pz + de[:, None] * pa)
    return out


def head_grad(rows, cols, m, a_mat, dz, alpha, lse=None, delta=None):
    """dA of one head: the row pass over S, then the column pass over S^T onto the same rows."""
    f = a_mat.shape[1]
    out = row_pass(rows, cols, m, a_mat, dz, a_mat, alpha, lse, delta)
    p = pack(a_mat, dz, lse, delta)
    return col_pass(cols, rows, m, a_mat, p, f, lse is not None, alpha, out)


def backward(rows, cols, m, x, layers, alpha: float, grad_out, weights=None, attention: str = "none"):
    """({(layer, head): dW}, dX0) computed the fused way; the forward trace comes from the references."""
    softmax = attention == "softmax"
    ref = RS if softmax else RN
    w = RN.weights_of(layers, weights)
    _, trace = ref.forward(rows, cols, m, x, layers, alpha, w, keep=True)
    g = grad_out
    dws = {}
    for li in range(len(layers) - 1, -1, -1):
        fin, fph, heads = layers[li]
        xin, out, heads_t = trace[li]
        dx = np.zeros_like(xin)
        for h in range(heads):
            a_mat = heads_t[h][0]
            sl = slice(h * fph, (h + 1) * fph)
            dz = g[:, sl] * (out[:, sl] > 0)
            lse = delta = None
            if softmax:
                lse = heads_t[h][4]
                delta = np.sum(dz * out[:, sl], axis=1)  # (= <dZ_i, o_i>: dZ is 0 where ReLU cleared o)
            da_mat = head_grad(rows, cols, m, a_mat, dz, alpha, lse, delta)
            dws[(li, h)] = xin.T @ da_mat
            dx += da_mat @ w[(li, h)].T
        g = dx
    return dws, g
