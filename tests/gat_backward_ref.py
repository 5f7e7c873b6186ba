"""numpy reference of the GAT backward pass (GAT::backwardPass, csrc/host/gat.hpp) — the definition the tests hold the product to.

Forward, per head h of layer i (oracle.gat_forward): X = input of the layer, A = X W_h, e_ij = <A_i, A_j> on the nonzeros of S
(values 1), a = LeakyReLU_alpha(e), Z_i = sum_j a_ij A_j, out[:, h f:(h+1) f] = ReLU(Z).
Backward, from G = dL/d(out):
    dZ    = G[:, cols] * [out[:, cols] > 0]
    da_ij = <dZ_i, A_j>,  de_ij = da_ij * (e_ij > 0 ? 1 : alpha)
    dA    = S_de A  +  S_a^T dZ  +  S_de^T A
    dW_h  = X^T dA,  dX += dA W_h^T
Nonzeros are kept as a list (a repeated (i, j) pair counts as often as it appears, like the kernels)."""
import numpy as np
import scipy.sparse as sp

from oracle import oracle as O


def weights_of(layers, weights=None, seed: int = 31):
    """{(layer, head): W} — the given ones, else the hashed weights of oracle.gat_weight."""
    if weights is not None:
        return weights
    return {(li, h): O.gat_weight(li, h, fin, fph, seed) for li, (fin, fph, heads) in enumerate(layers) for h in range(heads)}


def _smat(rows, cols, vals, m):
    return sp.csr_matrix((vals, (rows, cols)), shape=(m, m))  # duplicates are summed, as SpMM over the list does


def forward(rows, cols, m, x, layers, alpha: float, weights=None, keep: bool = False):
    """The forward pass with explicit weights; keep=True also returns per layer the inputs and per head (A, e, Z)."""
    w = weights_of(layers, weights)
    trace = []
    for li, (fin, fph, heads) in enumerate(layers):
        assert x.shape[1] == fin
        out = np.zeros((m, fph * heads))
        heads_t = []
        for h in range(heads):
            a_mat = x @ w[(li, h)]
            e = np.einsum("ij,ij->i", a_mat[rows], a_mat[cols])
            act = np.maximum(e, 0.0) + np.minimum(e, 0.0) * alpha
            z = _smat(rows, cols, act, m) @ a_mat
            out[:, h * fph:(h + 1) * fph] = np.maximum(z, 0.0)
            heads_t.append((a_mat, e, z))
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
            a_mat, e, _ = heads_t[h]
            sl = slice(h * fph, (h + 1) * fph)
            dz = g[:, sl] * (out[:, sl] > 0)
            act = np.maximum(e, 0.0) + np.minimum(e, 0.0) * alpha
            da = np.einsum("ij,ij->i", dz[rows], a_mat[cols])
            de = da * np.where(e > 0, 1.0, alpha)
            s_de = _smat(rows, cols, de, m)
            da_mat = s_de @ a_mat + _smat(rows, cols, act, m).T @ dz + s_de.T @ a_mat
            dws[(li, h)] = xin.T @ da_mat
            dx += da_mat @ w[(li, h)].T
        g = dx
    return dws, g


def pre_activations(rows, cols, m, x, layers, alpha: float, weights=None):
    """Every LeakyReLU input e and every ReLU input Z of rows that have a nonzero (other rows are identically zero)."""
    _, trace = forward(rows, cols, m, x, layers, alpha, weights, keep=True)
    live = np.zeros(m, dtype=bool)
    live[rows] = True
    out = []
    for _, _, heads_t in trace:
        for _, e, z in heads_t:
            out.append(e)
            out.append(z[live].reshape(-1))
    return np.concatenate(out)
