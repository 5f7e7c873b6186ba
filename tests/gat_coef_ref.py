"""numpy reference of the attention-coefficient export (include/hnh_attn_coef.h): one pass over the nonzeros of a block,
    values[e] = exp(z_e - lse_i)            dot       z = LeakyReLU(<X_i, Y_j>)
                                            gatv2     z = sum_c a_c LeakyReLU(X_ic + Y_jc)
                                            additive  z = LeakyReLU(s_i + t_j)
and, with drop, c m_e exp(z_e - lse_i) with the mask of include/hnh_attn_dropout.h.  coef_pass is the float64 statement, coef_pass_ld its
np.longdouble twin (math.fsum where longdouble is no wider than fp64).  operands() are the inputs the kernel tests use on the GPU, and the
CPU test shows that the float64 reference alone stays far inside the bound the kernel is held to on exactly these inputs.  The definition the
tests hold both to is the model's trace: gat_ref.forward / gat_v2_ref.forward(keep_trace=True)."""
import math

import numpy as np

import gat_pass_ref as P
import gat_ref as R

SCORES = ("dot", "additive", "gatv2")
SCORE_CODE = {"dot": 0, "additive": 1, "gatv2": 2}  # HNH_ATTN_COEF_*


def drop_factor(rows, cols, drop):
    """c m per nonzero; drop = (seed, w2, p, ids of the rows, ids of the columns)"""
    seed, w2, p, row_ids, col_ids = drop
    gi, gj = np.asarray(row_ids, dtype=np.uint64)[rows], np.asarray(col_ids, dtype=np.uint64)[cols]
    return P.keep(seed, P.STREAM_ATTENTION, w2, gi, gj, p) / (1.0 - p)


def scores(rows, cols, x, y, score, alpha, a=None, dtype=np.float64):
    """z per nonzero.  dot, gatv2: x = the rows' A, y = the columns' A (every column given is read); additive: x = s per row, y = t per column."""
    wide = dtype != np.longdouble or np.finfo(np.longdouble).eps <= 1e-18
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    al = dtype(alpha)
    if score == "additive":
        z = x[rows] + y[cols]
        return np.maximum(z, 0) + np.minimum(z, 0) * al
    if score == "dot":
        terms = x[rows] * y[cols]
    elif score == "gatv2":
        u = x[rows] + y[cols]
        terms = (np.maximum(u, 0) + np.minimum(u, 0) * al) * np.asarray(a, dtype=dtype)[None, :]
    else:
        raise ValueError(score)
    z = np.sum(terms, axis=1) if wide else np.array([math.fsum(t) for t in terms], dtype=dtype)
    return z if score == "gatv2" else np.maximum(z, 0) + np.minimum(z, 0) * al


def coef_pass(rows, cols, x, y, lse, score, alpha, a=None, drop=None, dtype=np.float64):
    z = scores(rows, cols, x, y, score, alpha, a, dtype)
    v = np.exp(z - np.asarray(lse, dtype=dtype)[rows])
    return v if drop is None else v * drop_factor(rows, cols, drop).astype(dtype)


def coef_pass_ld(rows, cols, x, y, lse, score, alpha, a=None, drop=None):
    return coef_pass(rows, cols, x, y, lse, score, alpha, a, drop, dtype=np.longdouble)


def lse_of(rows, m, z):
    """log-sum-exp per row of the scores z (any dtype), 0 for a row without nonzeros"""
    dt = z.dtype.type
    mx = np.full(m, -np.inf, dtype=z.dtype)
    np.maximum.at(mx, rows, z)
    tot = np.zeros(m, dtype=z.dtype)
    np.add.at(tot, rows, np.exp(z - mx[rows]))
    live = tot > 0
    lse = np.zeros(m, dtype=z.dtype)
    lse[live] = mx[live] + np.log(tot[live])
    return lse


def operands(score, f, rows, cols, m, ncols, seed=0, big=0.0):
    """The kernel tests' inputs: dict(x, y, a, lse) for coef_pass (x, y: A of the rows and of the columns, uniform in (-1, 1); additive:
    s and t from vectors of scale 1 / sqrt(f); gatv2: a of scale 1 / sqrt(f)), lse = the float64 rounding of the longdouble log-sum-exp.
    big > 0 scales the vectors (additive, gatv2) or x (dot) so that |z| reaches about `big`."""
    rng = np.random.default_rng(7000 + 31 * f + seed + 1000 * SCORE_CODE[score])
    xa, ya = rng.uniform(-1, 1, (m, f)), rng.uniform(-1, 1, (ncols, f))
    a1, a2 = rng.standard_normal(f) / np.sqrt(f), rng.standard_normal(f) / np.sqrt(f)
    o = dict(A_rows=xa, A_cols=ya, a1=a1, a2=a2, a=None)
    if score == "additive":
        if big:
            sc = big / np.abs((xa @ a1)[rows] + (ya @ a2)[cols]).max()
            a1, a2 = a1 * sc, a2 * sc
            o.update(a1=a1, a2=a2)
        o.update(x=xa @ a1, y=ya @ a2)
    elif score == "gatv2":
        if big:
            z0 = scores(rows, cols, xa, ya, "gatv2", 0.2, a1)
            a1 = a1 * (big / np.abs(z0).max())
        o.update(x=xa, y=ya, a=a1)
    else:
        if big:
            xa = xa * (big / np.abs(np.einsum("ij,ij->i", xa[rows], ya[cols])).max())
            o.update(A_rows=xa)
        o.update(x=xa, y=ya)
    return o


def with_lse(o, rows, cols, m, score, alpha):
    z = scores(rows, cols, o["x"], o["y"], score, alpha, o["a"], np.longdouble)
    o["lse"] = np.float64(lse_of(rows, m, z))
    return o


def row_sums(rows, m, v):
    return np.bincount(rows, weights=np.float64(v), minlength=m)


def model_trace(score, rows, cols, m, x, layers, alpha, w, av, **mode):
    """Per (layer, head): dict(A, a, lse, ck, vec) from the model's trace (the definition): gat_ref for dot and additive, gat_v2_ref for
    gatv2 (whose trace holds u in ck's place: no attention dropout there)."""
    import gat_v2_ref as V
    if score == "gatv2":
        _, trace = V.forward(rows, cols, m, x, layers, alpha, w, av, keep_trace=True, **mode)
    else:
        _, trace = R.forward(rows, cols, m, x, layers, alpha, w, av if score == "additive" else None, attention="softmax", score=score, keep_trace=True,
                             **mode)
    out = {}
    for li, (_, _, layer_out, heads) in enumerate(trace):
        for h, (a_mat, z, a, o, lse, last) in enumerate(heads):
            out[(li, h)] = dict(A=a_mat, a=a, lse=lse, o=o, ck=None if score == "gatv2" else last, out=layer_out)
    return out
