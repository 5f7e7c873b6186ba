"""numpy reference of the GAT's training step (GAT.loss / optimizer_step / train_step, csrc/host/gat.hpp, include/hnh_train.h) — the
definition the tests hold the product to.  Built on gat_dropout_ref.py's forward and backward (score "additive"; rates (0, 0) call through
to gat_additive_ref.py).

The loss over the rows r with mask[r] and labels[r] >= 0 (n of them), for an output row of `heads` blocks of `classes` values:
    z_c = (1 / heads) sum_h out[r, h classes + c]      lp = z - max(z) - log(sum(exp(z - max(z))))
    loss = (1 / n) sum_r -lp[label_r]    accuracy = (1 / n) #{r: argmax z = label_r}  (ties: the lowest index)
    G[r, h classes + c] = (1 / n) (exp(lp_c) - [c == label_r]) / heads,  0 on the other rows
The optimizers, per element with g' = g + weight_decay p:
    Adam   m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  p -= lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)
    SGD    v = momentum v + g';  p -= lr v
train(): step t = 1 .. K uses the masks of seed0 + t when a dropout rate is nonzero, and reports the loss and accuracy of the parameters
BEFORE the update."""
import numpy as np

import gat_dropout_ref as RD


def heads_of(layers, heads):
    """(heads to average, classes) of the last layer for heads = "mean" | "concat\""""
    fin, fph, nh = layers[-1]
    return (nh, fph) if heads == "mean" else (1, nh * fph)


def xent_rows(out, labels, heads: int, inv_n, dtype=np.float64):
    """(loss_sum, correct, G) as the kernel defines them; labels < 0 are not in the loss.  dtype=np.longdouble: the extended twin."""
    out = np.asarray(out, dtype=dtype)
    labels = np.asarray(labels)
    rows, n = out.shape
    classes = n // heads
    assert classes * heads == n and np.all(labels < classes)
    z = out.reshape(rows, heads, classes).sum(axis=1) * (dtype(1) / dtype(heads))
    mx = z.max(axis=1, keepdims=True)
    lp = z - mx - np.log(np.sum(np.exp(z - mx), axis=1, keepdims=True))
    live = labels >= 0
    idx = np.flatnonzero(live)
    loss_sum = -np.sum(lp[idx, labels[idx]], dtype=dtype)
    correct = int(np.count_nonzero(np.argmax(z[idx], axis=1) == labels[idx]))  # (argmax returns the first maximum)
    onehot = np.zeros((rows, classes), dtype=dtype)
    onehot[idx, labels[idx]] = 1
    gz = np.where(live[:, None], dtype(inv_n) * (np.exp(lp) - onehot) / dtype(heads), dtype(0))
    return loss_sum, correct, np.tile(gz, (1, heads))


def xent(out, labels, mask, heads: int, dtype=np.float64):
    """(loss, accuracy, G = dL/d(out)) over the rows of mask (None: every row) with a label >= 0."""
    labels = np.asarray(labels)
    lab = labels if mask is None else np.where(np.asarray(mask, dtype=bool), labels, -1)
    n = int(np.count_nonzero(lab >= 0))
    assert n > 0
    loss_sum, correct, g = xent_rows(out, lab, heads, dtype(1) / dtype(n), dtype)
    return loss_sum / dtype(n), correct / n, g


def xent_ld(out, labels, mask, heads: int):
    return xent(out, labels, mask, heads, np.longdouble)


def adam_step(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """(p, m, v) after step t (1-based)"""
    gd = g + weight_decay * p
    m = beta1 * m + (1.0 - beta1) * gd
    v = beta2 * v + (1.0 - beta2) * gd * gd
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    return p - lr * (m / bc1) / (np.sqrt(v / bc2) + eps), m, v


def sgd_step(p, g, v, lr, momentum=0.0, weight_decay=0.0):
    """(p, v)"""
    v = momentum * v + (g + weight_decay * p)
    return p - lr * v, v


def train(rows, cols, m, x, layers, alpha, labels, mask, heads, w, av, optimizer, steps, rates=(0.0, 0.0), seed0=0, perturb=None):
    """K training steps.  optimizer = dict(kind="adam" | "sgd", lr=.., [beta1, beta2, eps, momentum, weight_decay]).  perturb = (scale, rng):
    every gradient gets scale * max|g| * u, u uniform in [-1, 1], added before the update.  Returns (losses, accuracies, w, av)."""
    nh, _ = heads_of(layers, heads)
    opt = dict(optimizer)
    kind, lr = opt.pop("kind"), opt.pop("lr")
    w = {k: v.copy() for k, v in w.items()}
    av = {k: (a.copy(), b.copy()) for k, (a, b) in av.items()}
    params = {("w",) + k: w[k] for k in w}
    params.update({("a1",) + k: av[k][0] for k in av})
    params.update({("a2",) + k: av[k][1] for k in av})
    mom = {k: np.zeros_like(p) for k, p in params.items()}
    var = {k: np.zeros_like(p) for k, p in params.items()}
    losses, accs = [], []
    dropout = rates[0] > 0.0 or rates[1] > 0.0
    for t in range(1, steps + 1):
        seed = (seed0 + t) & 0xFFFFFFFFFFFFFFFF if dropout else seed0
        wt = {k: params[("w",) + k] for k in w}
        at = {k: (params[("a1",) + k], params[("a2",) + k]) for k in av}
        out = RD.forward(rows, cols, m, x, layers, alpha, wt, at, rates, seed)
        loss, acc, g = xent(out, labels, mask, nh)
        losses.append(float(loss))
        accs.append(float(acc))
        dw, da, _ = RD.backward(rows, cols, m, x, layers, alpha, g, wt, at, rates, seed)
        grads = {("w",) + k: dw[k] for k in dw}
        grads.update({("a1",) + k: da[k][0] for k in da})
        grads.update({("a2",) + k: da[k][1] for k in da})
        for k in params:
            gk = grads[k]
            if perturb is not None:
                scale, rng = perturb
                gk = gk + scale * np.max(np.abs(gk)) * rng.uniform(-1.0, 1.0, gk.shape)
            if kind == "adam":
                params[k], mom[k], var[k] = adam_step(params[k], gk, mom[k], var[k], t, lr, **opt)
            else:
                params[k], var[k] = sgd_step(params[k], gk, var[k], lr, **opt)
    return losses, accs, {k: params[("w",) + k] for k in w}, {k: (params[("a1",) + k], params[("a2",) + k]) for k in av}


def evaluate(rows, cols, m, x, layers, alpha, labels, mask, heads, w, av):
    """(loss, accuracy) over mask from a forward pass without dropout"""
    out = RD.forward(rows, cols, m, x, layers, alpha, w, av)
    loss, acc, _ = xent(out, labels, mask, heads_of(layers, heads)[0])
    return float(loss), float(acc)


def parameter_divergence(w_a, av_a, w_b, av_b):
    """max over the tensors of max|a - b| / max|b|"""
    worst = 0.0
    for k in w_b:
        worst = max(worst, float(np.max(np.abs(w_a[k] - w_b[k])) / np.max(np.abs(w_b[k]))))
        for i in (0, 1):
            worst = max(worst, float(np.max(np.abs(av_a[k][i] - av_b[k][i])) / np.max(np.abs(av_b[k][i]))))
    return worst


# ------------------------------------------------------------------------------------------------ the learning problem
LEARN_STEPS = 40
LEARN_OPTIMIZER = dict(kind="adam", lr=0.01, weight_decay=5e-4)


def planted_partition(layers, n=256, classes=4, degree=12, inside=0.8, train_share=0.3, seed=1):
    """A planted partition: `degree` edges per row, each inside the row's class with probability `inside` and uniform otherwise, and one
    self loop per row; x = 0.5 prototype[class] + standard normal noise; a training mask of train_share; parameters of scale
    1 / sqrt(fan-in).  Drawn in this order from default_rng(seed): labels, prototypes, noise, edges, mask, W, (a1, a2).  With the defaults
    and T.GAT_LAYERS the reference trains from loss 1.378 to 0.089 in 40 steps, monotonically, with a held-out accuracy of 0.964.
    Returns dict(rows, cols, m, x, labels, mask, w, av)."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, classes, n).astype(np.int32)
    fin = layers[0][0]
    proto = rng.standard_normal((classes, fin))
    x = 0.5 * proto[labels] + rng.standard_normal((n, fin))
    members = [np.flatnonzero(labels == c) for c in range(classes)]
    own = rng.random((n, degree)) < inside
    uniform = rng.integers(0, n, (n, degree))
    pick = rng.random((n, degree))
    within = np.array([[members[labels[i]][int(pick[i, k] * len(members[labels[i]]))] for k in range(degree)] for i in range(n)])
    rows = np.concatenate([np.repeat(np.arange(n), degree), np.arange(n)]).astype(np.int64)
    cols = np.concatenate([np.where(own, within, uniform).reshape(-1), np.arange(n)]).astype(np.int64)
    mask = rng.random(n) < train_share
    w = {(li, h): rng.standard_normal((f_in, fph)) / np.sqrt(f_in) for li, (f_in, fph, heads) in enumerate(layers) for h in range(heads)}
    av = {(li, h): (rng.standard_normal(fph) / np.sqrt(fph), rng.standard_normal(fph) / np.sqrt(fph))
          for li, (f_in, fph, heads) in enumerate(layers) for h in range(heads)}
    return dict(rows=rows, cols=cols, m=n, x=x, labels=labels, mask=mask, w=w, av=av)
