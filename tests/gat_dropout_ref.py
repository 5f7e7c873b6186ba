"""numpy reference of the GAT's dropout (GAT.set_dropout, csrc/host/gat.hpp, include/hnh_attn_dropout.h) — the definition the tests hold
the product to.  A sibling of gat_additive_ref.py, which it calls through to at rates (0, 0).

The mask: Philox-4x32 with 10 rounds, restated here in numpy integer arithmetic.  key = (seed & 0xffffffff, seed >> 32), counter =
(gi, gj, w2, stream); attention mask of edge (i, j), head h of layer l: gi = i, gj = j, w2 = l * 65536 + h, stream 0; feature mask of entry
(r, k) of layer l's input: gi = r, gj = k, w2 = l, stream 1.  Kept iff word 0 >= T = floor(p 2^32); kept values are scaled by c = 1 / (1 - p).
A repeated pair (i, j) has the same key: every copy gets the same mask.

With m_ij in {0, 1}, everything else as in gat_additive_ref.py:
    lse_i, a_ij unchanged (normalised over ALL edges)    o_i = sum_j c m_ij a_ij A_j    (all edges dropped: o_i = 0, lse_i kept)
    delta_i = <dZ_i, o_i>   dz_ij = a_ij (c m_ij <dZ_i, A_j> - delta_i) g(z_ij)   dAgg_j = sum_i c m_ij a_ij dZ_i
    Xd = c_q mask o X replaces X in the head products and in dW = Xd^T dA;  dX = c_q mask o (dA_all Wt)
The operands with the ids (scored: M' = [A (0) | s t | id 0], pack: Q' = [dZ (0) | s lse delta id]) and the three passes as the kernels
take them are restated too: the passes read the gathered row's id from the operand and add row_id0 to the own row."""
import math

import numpy as np
import scipy.sparse as sp

import gat_additive_ref as A
from gat_backward_ref import weights_of
from gat_softmax_ref import leaky, row_softmax

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
STREAM_ATTENTION, STREAM_FEATURE = 0, 1


# ------------------------------------------------------------------------------------------------ the generator
def philox4x32_10(counter, key):
    """The four output words (uint32 arrays) of Philox-4x32-10; counter = 4 and key = 2 broadcastable arrays of 32-bit values."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK32 for v in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return [v.astype(np.uint32) for v in c]


def word(seed, stream, w2, gi, gj):
    """Word 0 for the 64-bit seed: the number the keep test compares (hnh_dropout_word, hnh_dropout_words_u32)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10((gi, gj, w2, stream), (seed & 0xFFFFFFFF, seed >> 32))[0]


def threshold(p: float) -> int:
    return int(math.floor(p * 4294967296.0))


def keep(seed, stream, w2, gi, gj, p):
    """bool: kept iff word 0 >= floor(p 2^32)"""
    return word(seed, stream, w2, gi, gj) >= np.uint32(threshold(p))


def attention_factor(seed, layer, head, gi, gj, p):
    """c m_ij per edge"""
    return keep(seed, STREAM_ATTENTION, layer * 65536 + head, gi, gj, p) / (1.0 - p)


def feature_factor(seed, layer, shape, p, row_id0=0):
    """c_q mask of a rows x cols input whose first row has the global id row_id0"""
    r, k = np.meshgrid(np.arange(shape[0], dtype=np.uint64) + np.uint64(row_id0), np.arange(shape[1], dtype=np.uint64), indexing="ij")
    return keep(seed, STREAM_FEATURE, layer, r, k, p) / (1.0 - p)


# ------------------------------------------------------------------------------------------------ the operands with the ids
def scored_width(f: int) -> int:
    return f + (f & 1) + 4


def scored(a_mat, a1, a2, ids, ld=None):
    """M' = [A (0) | s t | id 0]; columns beyond the width hold NaN: nothing may read them."""
    n, f = a_mat.shape
    fp = f + (f & 1)
    m = np.full((n, ld or fp + 4), np.nan)
    m[:, :fp + 2] = A.scored(a_mat, a1, a2)
    m[:, fp + 2] = np.asarray(ids, dtype=np.float64)
    m[:, fp + 3] = 0.0
    return m


def pack(dz, s, lse, delta, ids, ld=None):
    """Q' = [dZ (0) | s lse delta id]"""
    f = dz.shape[1]
    q = A.pack(dz, s, lse, delta, ld)
    q[:, f + (f & 1) + 3] = np.asarray(ids, dtype=np.float64)
    return q


def _ids(col):
    ids = np.asarray(col)
    assert np.all(ids == np.floor(ids)) and np.all(ids >= 0) and np.all(ids < 2.0 ** 32)
    return ids.astype(np.uint64)


# ------------------------------------------------------------------------------------------------ the three passes, as the kernels take them
def _rect(rows, cols, vals, m, y):
    return sp.csr_matrix((vals, (rows, cols)), shape=(m, y.shape[0])) @ y


def fwd_factor(rows, cols, m_cols, f, drop):
    """c m per nonzero of a block of S: own row = row_id0 + local row, column id from the gathered operand"""
    seed, w2, p, row_id0 = drop
    fp = f + (f & 1)
    return keep(seed, STREAM_ATTENTION, w2, np.asarray(rows, dtype=np.uint64) + np.uint64(row_id0), _ids(m_cols[:, fp + 2])[cols], p) / (1.0 - p)


def fwd_pass(rows, cols, m, m_rows, m_cols, f, alpha, drop):
    """(o, lse, z, ck); drop = (seed, w2, p, row_id0)"""
    fp = f + (f & 1)
    z = m_rows[rows, fp] + m_cols[cols, fp + 1]
    a, lse = row_softmax(rows, m, leaky(z, alpha))
    ck = fwd_factor(rows, cols, m_cols, f, drop)
    return _rect(rows, cols, ck * a, m, m_cols[:, :f]), lse, z, ck


def fwd_pass_ld(rows, cols, m, m_rows, m_cols, f, alpha, drop):
    """fwd_pass in np.longdouble (math.fsum per row where longdouble is no wider than fp64): (o, lse) as longdouble."""
    ld = np.longdouble
    wide = np.finfo(ld).eps <= 1e-18
    fp = f + (f & 1)
    order = np.argsort(rows, kind="stable")
    r, c = np.asarray(rows)[order], np.asarray(cols)[order]
    ck = np.asarray(fwd_factor(r, c, m_cols, f, drop), dtype=ld)
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
        contrib = (ck[b:t, None] * ex[b:t, None] / tot) * yc[c[b:t]]
        o[i] = np.sum(contrib, axis=0) if wide else [math.fsum(contrib[:, k]) for k in range(f)]
    return o, lse


def gate(z, lse_nz, da, delta_nz, alpha, ck):
    """(c m a, dz) per nonzero"""
    a = np.exp(leaky(z, alpha) - lse_nz)
    return ck * a, a * (ck * da - delta_nz) * np.where(z > 0, 1.0, alpha)


def row_pass(rows, cols, m, dz_rows, m_rows, lse, delta, m_cols, f, alpha, drop):
    """ds over a block of S"""
    fp = f + (f & 1)
    z = m_rows[rows, fp] + m_cols[cols, fp + 1]
    da = np.einsum("ij,ij->i", dz_rows[rows], m_cols[cols, :f])
    _, dzz = gate(z, lse[rows], da, delta[rows], alpha, fwd_factor(rows, cols, m_cols, f, drop))
    return np.bincount(rows, weights=dzz, minlength=m)


def col_pass(trows, tcols, m, m_rows, q_cols, f, alpha, drop):
    """(dAgg, dt) over a block of S^T: row j = trows is a COLUMN of S (gj = row_id0 + j), nonzero (j, i) gathers Q'_i, whose id is gi."""
    seed, w2, p, row_id0 = drop
    fp = f + (f & 1)
    z = q_cols[tcols, fp] + m_rows[trows, fp + 1]
    da = np.einsum("ij,ij->i", m_rows[trows, :f], q_cols[tcols, :f])
    ck = keep(seed, STREAM_ATTENTION, w2, _ids(q_cols[:, fp + 3])[tcols], np.asarray(trows, dtype=np.uint64) + np.uint64(row_id0), p) / (1.0 - p)
    a, dzz = gate(z, q_cols[tcols, fp + 1], da, q_cols[tcols, fp + 2], alpha, ck)
    return _rect(trows, tcols, a, m, q_cols[:, :f]), np.bincount(trows, weights=dzz, minlength=m)


# ------------------------------------------------------------------------------------------------ the model
def forward(rows, cols, m, x, layers, alpha: float, weights=None, vectors=None, rates=(0.0, 0.0), seed: int = 0, keep_trace: bool = False):
    """The forward pass; rates = (attention p, feature q).  keep_trace=True also returns per layer (Xd, feature factor, out, heads) with
    per head (A, z, a, o, lse, c m)."""
    p, q = rates
    if p == 0.0 and q == 0.0 and not keep_trace:
        return A.forward(rows, cols, m, x, layers, alpha, weights, vectors)
    w = weights_of(layers, weights)
    av = A.vectors_of(layers, vectors)
    trace = []
    for li, (fin, fph, heads) in enumerate(layers):
        assert x.shape[1] == fin
        ff = feature_factor(seed, li, x.shape, q) if q > 0.0 else np.ones(x.shape)
        xd = ff * x
        out = np.zeros((m, fph * heads))
        heads_t = []
        for h in range(heads):
            a_mat = xd @ w[(li, h)]
            a1, a2 = av[(li, h)]
            z = (a_mat @ a1)[rows] + (a_mat @ a2)[cols]
            a, lse = row_softmax(rows, m, leaky(z, alpha))
            ck = attention_factor(seed, li, h, rows, cols, p) if p > 0.0 else np.ones(len(rows))
            o = A._smat(rows, cols, ck * a, m) @ a_mat
            out[:, h * fph:(h + 1) * fph] = np.maximum(o, 0.0)
            heads_t.append((a_mat, z, a, o, lse, ck))
        trace.append((xd, ff, out, heads_t))
        x = out
    return (x, trace) if keep_trace else x


def backward(rows, cols, m, x, layers, alpha: float, grad_out, weights=None, vectors=None, rates=(0.0, 0.0), seed: int = 0, by_passes: bool = False):
    """({(layer, head): dW}, {(layer, head): (da1, da2)}, dX0) for L with dL/d(output) = grad_out, the masks held fixed."""
    p, q = rates
    if p == 0.0 and q == 0.0:
        return A.backward(rows, cols, m, x, layers, alpha, grad_out, weights, vectors, by_passes)
    w = weights_of(layers, weights)
    av = A.vectors_of(layers, vectors)
    _, trace = forward(rows, cols, m, x, layers, alpha, w, av, rates, seed, keep_trace=True)
    g = grad_out
    dws, das = {}, {}
    ids = np.arange(m)
    for li in range(len(layers) - 1, -1, -1):
        fin, fph, heads = layers[li]
        xd, ff, out, heads_t = trace[li]
        dxd = np.zeros_like(xd)
        for h in range(heads):
            a_mat, z, a, o, lse, ck = heads_t[h]
            a1, a2 = av[(li, h)]
            sl = slice(h * fph, (h + 1) * fph)
            dz = g[:, sl] * (out[:, sl] > 0)
            delta = np.sum(dz * o, axis=1)
            if by_passes:
                drop = (seed, li * 65536 + h, p, 0)
                mm = scored(a_mat, a1, a2, ids)
                qq = pack(dz, mm[:, fph + (fph & 1)], lse, delta, ids)
                ds = row_pass(rows, cols, m, dz, mm, lse, delta, mm, fph, alpha, drop)
                dagg, dt = col_pass(cols, rows, m, mm, qq, fph, alpha, drop)
            else:
                da = np.einsum("ij,ij->i", dz[rows], a_mat[cols])
                dzz = a * (ck * da - delta[rows]) * np.where(z > 0, 1.0, alpha)
                ds = np.bincount(rows, weights=dzz, minlength=m)
                dt = np.bincount(cols, weights=dzz, minlength=m)
                dagg = A._smat(rows, cols, ck * a, m).T @ dz
            da_mat = dagg + np.outer(ds, a1) + np.outer(dt, a2)
            das[(li, h)] = (a_mat.T @ ds, a_mat.T @ dt)
            dws[(li, h)] = xd.T @ da_mat
            dxd += da_mat @ w[(li, h)].T
        g = ff * dxd
    return dws, das, g


def pre_activations(rows, cols, m, x, layers, alpha: float, weights=None, vectors=None, rates=(0.0, 0.0), seed: int = 0):
    """Every LeakyReLU input z and every ReLU input o of rows that have a nonzero.  A row whose edges are all dropped has o = 0 exactly,
    whatever the perturbation, like a row without nonzeros."""
    _, trace = forward(rows, cols, m, x, layers, alpha, weights, vectors, rates, seed, keep_trace=True)
    live = np.zeros(m, dtype=bool)
    live[rows] = True
    out = []
    for _, _, _, heads_t in trace:
        for _, z, _, o, _, _ in heads_t:
            out.append(z)
            out.append(o[live].reshape(-1))
    return np.concatenate(out)
