"""The numpy definition of implicit-feedback ALS with confidence weights (api.ImplicitALS, csrc/host/als_implicit.hpp), in any dtype.

S has nnz stored pairs (rows[e], cols[e]) with a weight w_e >= 0: confidence c_e = 1 + w_e, preference 1 on the stored pairs and 0 on
every other of the M N pairs (confidence 1 there); lambda > 0.

    L(A, B) = sum over ALL i, j of c_ij (p_ij - <a_i, b_j>)^2 + lambda (|A|^2 + |B|^2)                                    loss_grid
            = sum_{e in S} [(1 + w_e)(1 - s_e)^2 - s_e^2] + <A^T A, B^T B>_F + lambda (|A|_F^2 + |B|_F^2),  s_e = <a_i, b_j>   loss

Half-step for X with Y fixed and G = Y^T Y:  rhs_i = sum_{e in row i} (1 + w_e) y_j,  M(x)_i = sum_e w_e <x_i, y_j> y_j + lambda x_i + x_i G,
start r = rhs - M(x), p = r, rs_i = <r_i, r_i>, then `iters` times per row

    Mp = M(p)_i;  bdot = <p_i, Mp>;  live = rs_i > 0 and bdot > 0;  alpha = live ? rs_i / bdot : 0;  x_i += alpha p_i;  r_i -= alpha Mp
    rsnew = <r_i, r_i>;  beta = live ? rsnew / rs_i : 0;  p_i = r_i + beta p_i;  rs_i = rsnew

without an epsilon: a row that is not live keeps x_i and r_i bit for bit.  Empty rows are ordinary rows (M = G + lambda I, rhs = 0).
dense_solve is the independent check: (G + Y_i^T diag(w) Y_i + lambda I) x = rhs_i by numpy.linalg.solve, row by row."""
import functools

import numpy as np

import als_common
from oracle import oracle as O

LAMBDA = 0.1


def rowdot(x, y):
    return np.einsum("ij,ij->i", x, y)


@functools.lru_cache(maxsize=None)
def inputs(name, R):
    """The shared inputs of the model and operator tests: graph, weights in [2, 42], factors of order one per row."""
    m, n, rows, cols = als_common.graph(name)
    w = 40.0 * (0.05 + np.abs(O.sparse_values(rows, cols, n, 5)) % 1.0)
    assert w.min() >= 2.0 and w.max() <= 42.0
    case = dict(name="%s_r%d" % (name, R), M=m, N=n, R=R, rows=rows, cols=cols, w=w, A=O.dense_fill(m, R, 3) * np.sqrt(R),
                B=O.dense_fill(n, R, 4) * np.sqrt(R), vals=np.ones(len(rows)))
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def scatter_rows(rows, contrib, nrows):
    out = np.zeros((nrows, contrib.shape[1]), dtype=contrib.dtype)
    np.add.at(out, rows, contrib)
    return out


def apply_m(rows, cols, w, x, y, gram, lam):
    s = rowdot(x[rows], y[cols])
    return scatter_rows(rows, (w * s)[:, None] * y[cols], x.shape[0]) + lam * x + x @ gram


def half_step(rows, cols, w, x, y, lam, iters, dtype=np.float64):
    """One half-step for x (its rows indexed by `rows`, y's by `cols`); returns the new x."""
    w, x, y, lam = w.astype(dtype), x.astype(dtype), y.astype(dtype), dtype(lam)
    gram = y.T @ y
    rhs = scatter_rows(rows, (1 + w)[:, None] * y[cols], x.shape[0])
    r = rhs - apply_m(rows, cols, w, x, y, gram, lam)
    p = r.copy()
    rs = rowdot(r, r)
    for _ in range(iters):
        mp = apply_m(rows, cols, w, p, y, gram, lam)
        bdot = rowdot(p, mp)
        live = (rs > 0) & (bdot > 0)
        alpha = np.where(live, rs / np.where(live, bdot, 1), 0).astype(dtype)
        x = np.where(live[:, None], x + alpha[:, None] * p, x)
        r = np.where(live[:, None], r - alpha[:, None] * mp, r)
        rsnew = rowdot(r, r)
        beta = np.where(live, rsnew / np.where(live, rs, 1), 0).astype(dtype)
        p = np.where(live[:, None], r + beta[:, None] * p, r)
        rs = rsnew
    return x


def loss(rows, cols, w, a, b, lam, dtype=np.float64):
    w, a, b, lam = w.astype(dtype), a.astype(dtype), b.astype(dtype), dtype(lam)
    s = rowdot(a[rows], b[cols])
    return np.sum((1 + w) * (1 - s) ** 2 - s ** 2) + np.sum((a.T @ a) * (b.T @ b)) + lam * (np.sum(a * a) + np.sum(b * b))


def loss_grid(rows, cols, w, a, b, lam, m, n):
    """The objective as it is written: every one of the M N pairs."""
    conf, pref = np.ones((m, n)), np.zeros((m, n))
    conf[rows, cols] += w
    pref[rows, cols] = 1.0
    return np.sum(conf * (pref - a @ b.T) ** 2) + lam * (np.sum(a * a) + np.sum(b * b))


def run(rows, cols, w, a, b, lam, steps, iters, dtype=np.float64):
    """`steps` alternating steps; returns (A, B, the loss at the start and after every half-step)."""
    a, b = a.astype(dtype), b.astype(dtype)
    losses = [loss(rows, cols, w, a, b, lam, dtype)]
    for _ in range(steps):
        a = half_step(rows, cols, w, a, b, lam, iters, dtype)
        losses.append(loss(rows, cols, w, a, b, lam, dtype))
        b = half_step(cols, rows, w, b, a, lam, iters, dtype)
        losses.append(loss(rows, cols, w, a, b, lam, dtype))
    return a, b, np.array(losses, dtype=dtype)


def dense_solve(rows, cols, w, y, lam, nrows):
    """(G + Y_i^T diag(w) Y_i + lambda I) x_i = rhs_i for every row i, by numpy.linalg.solve."""
    R = y.shape[1]
    base = y.T @ y + lam * np.eye(R)
    out = np.zeros((nrows, R))
    order = np.argsort(rows, kind="stable")
    starts = np.searchsorted(rows[order], np.arange(nrows + 1))
    for i in range(nrows):
        e = order[starts[i]:starts[i + 1]]
        yi = y[cols[e]]
        out[i] = np.linalg.solve(base + yi.T @ (w[e][:, None] * yi), yi.T @ (1 + w[e]))
    return out


@functools.lru_cache(maxsize=None)
def expected(name, R, steps=2, iters=2):
    """The float64 model's answer for the operator tests: two alternating steps of two iterations from the case's factors."""
    c = inputs(name, R)
    a, b, losses = run(c["rows"], c["cols"], c["w"], c["A"], c["B"], LAMBDA, steps, iters)
    out = dict(A=a, B=b, losses=losses, gramA=a.T @ a, gramB=b.T @ b)
    for v in out.values():
        v.setflags(write=False)
    return out
