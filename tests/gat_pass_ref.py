"""numpy restatements of the GAT's single passes as the kernels take them — what the ctypes tests compare one launch against.  The
definition of the model is gat_ref.py; this file only has to agree with it (gat_ref.backward(by_passes=True) and the CPU tests).

The softmax pass (include/hnh_attention.h), row operand X and gathered operand Y over the nonzeros (i, j):
    s_ij = LeakyReLU_alpha(<X_i, Y_j>)    lse_i = log sum_j exp(s_ij)    o_i = sum_j exp(s_ij - lse_i) Y_j    (empty row: o = 0, lse = 0)
attention_ld is attention() in extended precision; max_rises finds where a row's running max rises.

The fused backward passes for score dot (include/hnh_attn_grad.h), packed operand P = [A (0) | dZ (0) | lse delta]:
    row pass over S      (i, j):  e = <A_i, Y_j>, da = <dZ_i, Y_j>, gate with lse_i / delta_i,  Out_i += de Y_j
    column pass over S^T (j, i):  e = <X_j, P_i[0:f]>, da = <X_j, P_i[fp:fp+f]>, gate with P_i[2fp], P_i[2fp+1],
                                  Out_j += a P_i[fp:fp+f] + de P_i[0:f]
with g(e) = e > 0 ? 1 : alpha;  attention none: a = LeakyReLU(e), de = da g(e);  softmax: a = exp(LeakyReLU(e) - lse), de = a (da - delta) g(e).

The additive passes (include/hnh_attn_additive.h), operands M = [A (0) | s t] and Q = [dZ (0) | s lse delta 0]: the forward pass
(fwd_pass, fwd_pass_ld in extended precision), the row pass (ds) and the column pass (dAgg, dt).  With drop = (seed, w2, p, row_id0)
they are the masked passes of include/hnh_attn_dropout.h: the operands carry the ids (M' = [A (0) | s t | id 0], Q' = [dZ (0) | s lse
delta id]), the passes read the gathered row's id from the operand and add row_id0 to the own row.

The mask: Philox-4x32 with 10 rounds in numpy integer arithmetic.  key = (seed & 0xffffffff, seed >> 32), counter = (gi, gj, w2, stream);
attention mask of edge (i, j), head h of layer l: gi = i, gj = j, w2 = l * 65536 + h, stream 0; feature mask of entry (r, k) of layer l's
input: gi = r, gj = k, w2 = l, stream 1.  Kept iff word 0 >= T = floor(p 2^32); kept values are scaled by c = 1 / (1 - p).  A repeated
pair (i, j) has the same key: every copy gets the same mask.

A repeated (row, column) pair counts as often as it appears."""
import math

import numpy as np
import scipy.sparse as sp

from gat_ref import _smat, leaky, row_softmax


def _rect(rows, cols, vals, m, y):
    return sp.csr_matrix((vals, (rows, cols)), shape=(m, y.shape[0])) @ y


# ------------------------------------------------------------------------------------------------ the softmax pass
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


# ------------------------------------------------------------------------------------------------ the fused backward passes, score dot
def fused_packed_width(f: int, softmax: bool) -> int:
    return 2 * (f + (f & 1)) + (2 if softmax else 0)


def fused_pack(a_mat, dz, lse=None, delta=None, ld=None):
    """P = [A (0) | dZ (0) | lse delta] with the pad column present when f is odd; columns beyond the packed width keep NaN."""
    rows, f = a_mat.shape
    fp = f + (f & 1)
    pw = fused_packed_width(f, lse is not None)
    p = np.full((rows, ld if ld is not None else pw), np.nan)
    p[:, :pw] = 0.0
    p[:, :f] = a_mat
    p[:, fp:fp + f] = dz
    if lse is not None:
        p[:, 2 * fp] = lse
        p[:, 2 * fp + 1] = delta
    return p


def fused_gate(e, da, alpha, lse=None, delta=None):
    """(a, de) per nonzero; lse / delta already gathered onto the nonzeros."""
    slope = np.where(e > 0, 1.0, alpha)
    s = e * slope
    if lse is None:
        return s, da * slope
    a = np.exp(s - lse)
    return a, a * (da - delta) * slope


def fused_row_pass(rows, cols, m, a_mat, dz, y, alpha, lse=None, delta=None, out=None):
    """Out (m x f, or `out` accumulated in place) after the row pass over the nonzeros (rows[k], cols[k])."""
    f = a_mat.shape[1]
    out = np.zeros((m, f)) if out is None else out
    yj = y[cols, :f]
    e = np.einsum("ij,ij->i", a_mat[rows, :f], yj)
    da = np.einsum("ij,ij->i", dz[rows, :f], yj)
    _, de = fused_gate(e, da, alpha, None if lse is None else lse[rows], None if delta is None else delta[rows])
    np.add.at(out, rows, de[:, None] * yj)
    return out


def fused_col_pass(rows_t, cols_t, m, x, p, f, softmax, alpha, out=None):
    """Out after the column pass over the nonzeros (rows_t[k], cols_t[k]) of S^T with the packed operand p."""
    fp = f + (f & 1)
    out = np.zeros((m, f)) if out is None else out
    pa, pz = p[cols_t, :f], p[cols_t, fp:fp + f]
    e = np.einsum("ij,ij->i", x[rows_t, :f], pa)
    da = np.einsum("ij,ij->i", x[rows_t, :f], pz)
    a, de = fused_gate(e, da, alpha, p[cols_t, 2 * fp] if softmax else None, p[cols_t, 2 * fp + 1] if softmax else None)
    np.add.at(out, rows_t, a[:, None] * pz + de[:, None] * pa)
    return out


def head_grad(rows, cols, m, a_mat, dz, alpha, lse=None, delta=None):
    """dA of one head: the row pass over S, then the column pass over S^T onto the same rows."""
    f = a_mat.shape[1]
    out = fused_row_pass(rows, cols, m, a_mat, dz, a_mat, alpha, lse, delta)
    p = fused_pack(a_mat, dz, lse, delta)
    return fused_col_pass(cols, rows, m, a_mat, p, f, lse is not None, alpha, out)


# ------------------------------------------------------------------------------------------------ the mask generator
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
STREAM_ATTENTION, STREAM_FEATURE = 0, 1


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


# ------------------------------------------------------------------------------------------------ the additive operands
def scored_width(f: int, ids: bool = False) -> int:
    return f + (f & 1) + (4 if ids else 2)


def packed_width(f: int) -> int:
    return f + (f & 1) + 4


def scored(a_mat, a1, a2, ids=None, ld=None):
    """M = [A (0) | s t], or with ids M' = [A (0) | s t | id 0]; columns beyond the width (a wider pitch) hold NaN: nothing may read them."""
    n, f = a_mat.shape
    fp = f + (f & 1)
    m = np.full((n, ld or scored_width(f, ids is not None)), np.nan)
    m[:, :fp] = 0.0
    m[:, :f] = a_mat
    m[:, fp] = a_mat @ a1
    m[:, fp + 1] = a_mat @ a2
    if ids is not None:
        m[:, fp + 2] = np.asarray(ids, dtype=np.float64)
        m[:, fp + 3] = 0.0
    return m


def pack(dz, s, lse, delta, ids=None, ld=None):
    """Q = [dZ (0) | s lse delta 0], or with ids Q' = [dZ (0) | s lse delta id]"""
    n, f = dz.shape
    fp = f + (f & 1)
    q = np.full((n, ld or fp + 4), np.nan)
    q[:, :fp + 4] = 0.0
    q[:, :f] = dz
    q[:, fp], q[:, fp + 1], q[:, fp + 2] = s, lse, delta
    if ids is not None:
        q[:, fp + 3] = np.asarray(ids, dtype=np.float64)
    return q


def _ids(col):
    ids = np.asarray(col)
    assert np.all(ids == np.floor(ids)) and np.all(ids >= 0) and np.all(ids < 2.0 ** 32)
    return ids.astype(np.uint64)


# ------------------------------------------------------------------------------------------------ the three additive passes
def fwd_factor(rows, cols, m_cols, f, drop):
    """c m per nonzero of a block of S: own row = row_id0 + local row, column id from the gathered operand"""
    seed, w2, p, row_id0 = drop
    fp = f + (f & 1)
    return keep(seed, STREAM_ATTENTION, w2, np.asarray(rows, dtype=np.uint64) + np.uint64(row_id0), _ids(m_cols[:, fp + 2])[cols], p) / (1.0 - p)


def fwd_pass(rows, cols, m, m_rows, m_cols, f, alpha, drop=None):
    """(o, lse, z, c m): row operand m_rows (scored rows of the block's rows), gathered operand m_cols; c m is None without drop."""
    fp = f + (f & 1)
    z = m_rows[rows, fp] + m_cols[cols, fp + 1]
    a, lse = row_softmax(rows, m, leaky(z, alpha))
    ck = None if drop is None else fwd_factor(rows, cols, m_cols, f, drop)
    return _rect(rows, cols, a if ck is None else ck * a, m, m_cols[:, :f]), lse, z, ck


def fwd_pass_ld(rows, cols, m, m_rows, m_cols, f, alpha, drop=None):
    """fwd_pass in np.longdouble (math.fsum per row where longdouble is no wider than fp64): (o, lse) as longdouble."""
    ld = np.longdouble
    wide = np.finfo(ld).eps <= 1e-18
    fp = f + (f & 1)
    order = np.argsort(rows, kind="stable")
    r, c = np.asarray(rows)[order], np.asarray(cols)[order]
    ck = None if drop is None else np.asarray(fwd_factor(r, c, m_cols, f, drop), dtype=ld)
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
        kept = ex[b:t, None] if ck is None else ck[b:t, None] * ex[b:t, None]
        contrib = (kept / tot) * yc[c[b:t]]
        o[i] = np.sum(contrib, axis=0) if wide else [math.fsum(contrib[:, k]) for k in range(f)]
    return o, lse


def gate(z, lse_nz, da, delta_nz, alpha, ck=None):
    """(c m a, dz) per nonzero"""
    a = np.exp(leaky(z, alpha) - lse_nz)
    if ck is None:
        return a, a * (da - delta_nz) * np.where(z > 0, 1.0, alpha)
    return ck * a, a * (ck * da - delta_nz) * np.where(z > 0, 1.0, alpha)


def row_pass(rows, cols, m, dz_rows, m_rows, lse, delta, m_cols, f, alpha, drop=None):
    """ds over a block of S: the rows' dZ, s, lse, delta; gathered M."""
    fp = f + (f & 1)
    z = m_rows[rows, fp] + m_cols[cols, fp + 1]
    da = np.einsum("ij,ij->i", dz_rows[rows], m_cols[cols, :f])
    _, dzz = gate(z, lse[rows], da, delta[rows], alpha, None if drop is None else fwd_factor(rows, cols, m_cols, f, drop))
    return np.bincount(rows, weights=dzz, minlength=m)


def col_pass(trows, tcols, m, m_rows, q_cols, f, alpha, drop=None):
    """(dAgg, dt) over a block of S^T: row j = trows (A_j, t_j from the scored rows) is a COLUMN of S (gj = row_id0 + j), nonzero (j, i)
    gathers Q_i, whose id is gi."""
    fp = f + (f & 1)
    z = q_cols[tcols, fp] + m_rows[trows, fp + 1]
    da = np.einsum("ij,ij->i", m_rows[trows, :f], q_cols[tcols, :f])
    ck = None
    if drop is not None:
        seed, w2, p, row_id0 = drop
        ck = keep(seed, STREAM_ATTENTION, w2, _ids(q_cols[:, fp + 3])[tcols], np.asarray(trows, dtype=np.uint64) + np.uint64(row_id0), p) / (1.0 - p)
    a, dzz = gate(z, q_cols[tcols, fp + 1], da, q_cols[tcols, fp + 2], alpha, ck)
    return _rect(trows, tcols, a, m, q_cols[:, :f]), np.bincount(trows, weights=dzz, minlength=m)
