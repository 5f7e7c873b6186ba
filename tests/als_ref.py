"""The ALS-CG application in plain numpy: the definition the operator tests compare against.

Every function restates, statement by statement, what the reference's ALS code computes (als_conjugate_gradients.cpp:38-301: batched
conjugate gradients on the normal equations, one independent system per row), in global coordinates and with S == 1 in the queries.
All of them take their precision from the arrays they are given, so the same statements run in np.float64 (what the operator is compared
with) and in np.longdouble (which tells how far float64 itself can be trusted, tests/test_als_model_cpu.py).

`ridx`, `cidx` name the nonzeros from the side of the factor being optimised: (rows, cols) of S for A, (cols, rows) for B.
"""
import numpy as np

from oracle import oracle as O

LAMBDA = 1e-13           # .cpp:271
NAN_AVOIDANCE = 1e-8     # .cpp:40


def rowdot(x, y):
    """batch_dot_product: one dot product per row."""
    return np.einsum("ij,ij->i", x, y)


def queries(ridx, cidx, X, Y, lam=LAMBDA):
    """computeQueries (.cpp:265-301): (S .* (X Y^T)|_S) Y + lam X with S == 1."""
    Yc = Y[cidx]
    vals = rowdot(X[ridx], Yc)                                        # SDDMM with all-ones S values
    out = np.zeros_like(X)
    np.add.at(out, ridx, vals[:, None] * Yc)                          # SpMM
    return out + X.dtype.type(lam) * X                                # :288 / :299


def rhs(ridx, cidx, gt, Y, nrows):
    """computeRHS (.cpp:192-205): SpMM of the ground-truth values with the fixed factor, into `nrows` zeroed rows."""
    out = np.zeros((nrows, Y.shape[1]), dtype=Y.dtype)
    np.add.at(out, ridx, gt.astype(Y.dtype)[:, None] * Y[cidx])
    return out


def cg_iteration(ridx, cidx, Y, x, r, p, rsold, lam=LAMBDA, eps=NAN_AVOIDANCE):
    """One pass of the loop of cg_optimizer (.cpp:80-140).  Returns the new (x, r, p, rsold)."""
    eps = x.dtype.type(eps)
    Mp = queries(ridx, cidx, p, Y, lam)                               # :82-87
    bdot = rowdot(p, Mp)                                              # :91
    bdot = bdot + eps                                                 # :99
    rsold = rsold + eps                                               # :100, in place: the constant stays in rsold
    alpha = rsold / bdot                                              # :102
    x = x + alpha[:, None] * p                                        # :112-117
    r = r - alpha[:, None] * Mp                                       # :118
    rsnew = rowdot(r, r)                                              # :120
    coeffs = rsnew / rsold                                            # :136
    p = r + coeffs[:, None] * p                                       # :137
    return x, r, p, rsnew                                             # :138


def half_step(ridx, cidx, gt, X, Y, iters, lam=LAMBDA, eps=NAN_AVOIDANCE, trace=False, iteration=cg_iteration):
    """cg_optimizer (.cpp:38-141) for the factor X with Y fixed.  Returns the new X; with trace=True also the list of
    (x, r, p, rsold) after every iteration."""
    b = rhs(ridx, cidx, gt, Y, len(X))                                # :63-65
    Mx = queries(ridx, cidx, X, Y, lam)                               # :66
    r = b - Mx                                                        # :68
    p = r.copy()                                                      # :69
    rsold = rowdot(r, r)                                              # :70
    steps = []
    for _ in range(iters):
        X, r, p, rsold = iteration(ridx, cidx, Y, X, r, p, rsold, lam, eps)
        if trace:
            steps.append((X, r, p, rsold))
    return (X, steps) if trace else X


def residual(rows, cols, vals, A, B):
    """computeResidual (.cpp:207-219): || (A B^T)|_S - ground truth ||_2 over the nonzeros."""
    return np.sqrt(np.sum((rowdot(A[rows], B[cols]) - vals.astype(A.dtype)) ** 2))


def run(rows, cols, vals, A, B, steps, iters, dtype=np.float64, half=half_step):
    """`steps` alternating steps from (A, B): the A half-step over (rows, cols), then the B half-step over (cols, rows) with the new A.
    Returns A, B and the steps + 1 residuals (before the first step, after each)."""
    A, B = A.astype(dtype), B.astype(dtype)
    res = [residual(rows, cols, vals, A, B)]
    for _ in range(steps):
        A = half(rows, cols, vals, A, B, iters)
        B = half(cols, rows, vals, B, A, iters)
        res.append(residual(rows, cols, vals, A, B))
    return A, B, np.array(res)


def forced(rows, cols, vals, A, B, steps, iters, dtype=np.float64, half=half_step):
    """The same alternating steps, every half-step reported on its own: a list of (which, A_in, B_in, updated), `which` 0 for A and
    1 for B, where (A_in, B_in) is the state the half-step starts from and `updated` the factor it returns.  The state is carried
    in `dtype` and handed on rounded to float64, so a float64 solver can be started from exactly the same numbers."""
    A, B = A.astype(np.float64), B.astype(np.float64)
    out = []
    for _ in range(steps):
        new = half(rows, cols, vals, A.astype(dtype), B.astype(dtype), iters)
        out.append((0, A, B, new))
        A = new.astype(np.float64)
        new = half(cols, rows, vals, B.astype(dtype), A.astype(dtype), iters)
        out.append((1, A, B, new))
        B = new.astype(np.float64)
    return out


def hashed_fill(nrows, R, seed, scale):
    """Distributed_ALS::hashed_fill in global coordinates: uniform(-1, 1) keyed by row * R + column, times `scale`."""
    return (O.hashed_uniform(np.arange(nrows * R, dtype=np.uint64), seed) * scale).reshape(nrows, R)


def hashed_init(m, n, R, seed):
    """The built-in initialisation (Distributed_ALS(d, true) and initializeEmbeddings): the two factors whose SDDMM is the artificial
    ground truth, and the initial embeddings.  Returns (Agt, Bgt, A0, B0).  The scales are written as the host code computes them,
    so the fills are the same doubles."""
    r = float(R)
    return (hashed_fill(m, R, seed + 1, 1.0 / (r * float(m) * r)), hashed_fill(n, R, seed + 2, 1.0 / (r * float(n) * r)),
            hashed_fill(m, R, seed + 3, 1.4 / r), hashed_fill(n, R, seed + 4, 1.0 / (1.3 * r)))
