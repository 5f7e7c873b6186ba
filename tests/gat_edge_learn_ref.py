"""numpy reference of the LEARNED per-edge bias of the GAT's score "transformer" (include/hnh_attn_edge_grad.h, GAT.set_edge_bias_learned),
built on tests/gat_edge_ref.py, whose backward() already returns
    dL/db_e = sum over the layer's heads of p_e (<dZ_i, V_j> - delta_i)        (= sum_h g_e / scale, heads added in the order 0 .. H-1)
per entry of the edge list.

row_pass / col_pass: gat_edge_ref's passes as the grad entry points take them: the same dQ / (dK, dV), and the per-entry gradient of ONE
head in the block's order, overwriting (dbias=None) or added to an earlier head's vector (accumulate: dbias + this head's value).

train(): gat_edge_ref.train with the bias of the layers in `learned` as a parameter: updated by the same optimizer, step count and
hyper-parameters as every other tensor but NEVER decayed (weight_decay = 0 for these tensors alone), so an entry at -1e300, whose gradient
and moments are exactly 0, stays -1e300.  The other layers' bias stays fixed.  backward(by_passes=True) sums the heads through the pass
twins: the convention of the passes against the definition."""
import numpy as np

import gat_edge_ref as E
import gat_pass_ref as P
from gat_ref import adam_step, heads_of, sgd_step, xent

__all__ = ["row_pass", "col_pass", "bias_grad_by_passes", "train"]


def row_pass(rows, cols, m, q_rows, dz_rows, lse, delta, kv_cols, f, scale, bias, out=None, dbias=None):
    """(dQ (+ out), db): db_e = p_e (<dZ_i, V_j> - delta_i) of entry e of the block of S, or dbias + that"""
    k, v = E._halves(kv_cols, f)
    s = scale * np.einsum("ij,ij->i", q_rows[rows, :f], k[cols]) + bias
    gb = np.exp(s - lse[rows]) * (np.einsum("ij,ij->i", dz_rows[rows, :f], v[cols]) - delta[rows])
    return E.row_pass(rows, cols, m, q_rows, dz_rows, lse, delta, kv_cols, f, scale, bias, out=out), (gb if dbias is None else dbias + gb)


def col_pass(trows, tcols, m, k_rows, v_rows, packed, f, scale, bias, out=None, out2=None, dbias=None):
    """(dK, dV, db) over a block of S^T: entry e = (j, i) gets the gradient of the bias of S_ij, in S^T's order"""
    fp = f + (f & 1)
    yq, yz = E._halves(packed, f)
    lse, delta = packed[:, 2 * fp], packed[:, 2 * fp + 1]
    s = scale * np.einsum("ij,ij->i", k_rows[trows, :f], yq[tcols]) + bias
    gb = np.exp(s - lse[tcols]) * (np.einsum("ij,ij->i", v_rows[trows, :f], yz[tcols]) - delta[tcols])
    dk, dv = E.col_pass(trows, tcols, m, k_rows, v_rows, packed, f, scale, bias, out=out, out2=out2)
    return dk, dv, (gb if dbias is None else dbias + gb)


def bias_grad_by_passes(rows, cols, m, x, layers, grad_out, weights, wq, wk, *, edge_bias, **mode):
    """{layer: (db from the row passes, db from the column passes)} with the heads accumulated as the device does (accumulate = h > 0), the
    column pass over the transposed list (the same entries in the same order).  Plain layers only (no dropout, bias or residual)."""
    from gat_ref import activations_of, true_grad
    acts = activations_of(layers, mode.get("activations"))
    _, trace = E.forward(rows, cols, m, x, layers, weights, wq, wk, edge_bias=edge_bias, activations=acts, keep_trace=True)
    g = grad_out
    res = {}
    for li in range(len(layers) - 1, -1, -1):
        fin, fph, heads = layers[li]
        xd, ff, out, heads_t = trace[li]
        assert ff is None
        sc = E.scale_of(fph)
        eb = edge_bias.get(li)
        dxd = np.zeros_like(xd)
        db_row = db_col = None
        for h in range(heads):
            vm, s, p, o, lse, (qm, km) = heads_t[h]
            sl = slice(h * fph, (h + 1) * fph)
            dz, delta = true_grad(g[:, sl], o, out[:, sl], acts[li])
            kv = np.nan_to_num(P.fused_pack(km, vm))
            b0 = np.zeros(len(rows)) if eb is None else eb
            dq, db_row = row_pass(rows, cols, m, qm, dz, lse, delta, kv, fph, sc, b0, dbias=db_row)
            dk, dv, db_col = col_pass(cols, rows, m, km, vm, P.fused_pack(qm, dz, lse, delta), fph, sc, b0, dbias=db_col)
            dxd += dv @ weights[(li, h)].T
            dxd += dq @ wq[(li, h)].T
            dxd += dk @ wk[(li, h)].T
        if eb is not None:
            res[li] = (db_row, db_col)
        g = dxd
    return res


def train(rows, cols, m, x, layers, labels, mask, heads, w, wq, wk, optimizer, steps, *, edge_bias, learned, train_others=True, activations=None,
          perturb=None):
    """`steps` training steps with the bias of the layers in `learned` as a parameter (not decayed); train_others=False freezes every other
    tensor (the bias alone is trained).  perturb = (scale, rng) as in gat_ref.train.  Returns (losses, accuracies, w, wq, wk, edge_bias) with
    edge_bias = {layer: vector} of every layer that has one."""
    nh, _ = heads_of(layers, heads)
    opt = dict(optimizer)
    kind, lr = opt.pop("kind"), opt.pop("lr")
    undecayed = dict(opt, weight_decay=0.0)
    assert all(li in edge_bias for li in learned), "only a layer with a bias can learn it"
    params = {}
    if train_others:
        params.update({("w",) + k: v.copy() for k, v in w.items()})
        params.update({("wq",) + k: v.copy() for k, v in wq.items()})
        params.update({("wk",) + k: v.copy() for k, v in wk.items()})
    params.update({("eb", li): np.array(edge_bias[li], dtype=np.float64) for li in learned})
    mom = {k: np.zeros_like(v) for k, v in params.items()}
    var = {k: np.zeros_like(v) for k, v in params.items()}
    losses, accs = [], []

    def unpack():
        pick = lambda name, first: {k: params.get((name,) + k, first[k]) for k in first}  # noqa: E731
        eb = {li: params.get(("eb", li), np.asarray(edge_bias[li], dtype=np.float64)) for li in edge_bias}
        return pick("w", w), pick("wq", wq), pick("wk", wk), eb

    for t in range(1, steps + 1):
        wt, qt, kt, ebt = unpack()
        out = E.forward(rows, cols, m, x, layers, wt, qt, kt, edge_bias=ebt, activations=activations)
        loss, acc, g = xent(out, labels, mask, nh)
        losses.append(float(loss))
        accs.append(float(acc))
        dw, dq, dk, _, _, _, deb = E.backward(rows, cols, m, x, layers, g, wt, qt, kt, edge_bias=ebt, activations=activations)
        grads = {("w",) + k: dw[k] for k in dw}
        grads.update({("wq",) + k: dq[k] for k in dq})
        grads.update({("wk",) + k: dk[k] for k in dk})
        grads.update({("eb", li): deb[li] for li in deb})
        for k in params:
            gk = grads[k]
            if perturb is not None:
                scale, rng = perturb
                gk = gk + scale * np.max(np.abs(gk)) * rng.uniform(-1.0, 1.0, gk.shape)
            hyper = undecayed if k[0] == "eb" else opt
            if kind == "adam":
                params[k], mom[k], var[k] = adam_step(params[k], gk, mom[k], var[k], t, lr, **hyper)
            else:
                params[k], var[k] = sgd_step(params[k], gk, var[k], lr, **hyper)
    return (losses, accs) + unpack()
