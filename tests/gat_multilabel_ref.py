"""numpy reference of the GAT's multi-label head (include/hnh_train_multilabel.h; GAT.set_multilabel_targets), next to tests/gat_ref.py, which
stays the model: the weighted sigmoid cross-entropy over rows x classes with the counts of micro-averaged F1 as the kernel defines them
(bce_rows, usable with np.longdouble), the mean loss of the operator (bce), the bit packing of the targets, micro-F1, a training loop
built from gat_ref.forward / backward / adam_step / sgd_step, and planted_tags, an overlapping-community graph with several tags per
vertex."""
import numpy as np

import gat_ref as R

PUBLISHED = ("elu", "identity")  # the published activations of a two-layer network: the logits take both signs


def pack_bits(targets, ld_t=None, garbage=None):
    """(rows, classes) of 0/1 -> uint32 (rows, ld_t): bit (c % 32) of word c / 32.  garbage = a numpy Generator: the bits beyond `classes`
    in a row's last word and every word beyond it are random."""
    t = np.asarray(targets).astype(bool)
    rows, classes = t.shape
    words = (classes + 31) // 32
    ld_t = words if ld_t is None else ld_t
    assert ld_t >= words
    out = np.zeros((rows, ld_t), dtype=np.uint32) if garbage is None else garbage.integers(0, 1 << 32, (rows, ld_t), dtype=np.uint64).astype(np.uint32)
    padded = np.zeros((rows, words * 32), dtype=np.uint64)
    padded[:, :classes] = t
    packed = (padded.reshape(rows, words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    keep = np.zeros(words * 32, dtype=np.uint64)
    keep[:classes] = 1
    keep = (keep.reshape(words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)  # the class bits of every word
    out[:, :words] = (out[:, :words] & ~keep) | packed
    return out


def unpack_bits(words, classes):
    """uint32 (rows, ld_t) -> bool (rows, classes)"""
    w = np.asarray(words, dtype=np.uint32)
    c = np.arange(classes)
    return ((w[:, c // 32] >> (c % 32).astype(np.uint32)) & np.uint32(1)).astype(bool)


def micro_f1(tp, fp, fn):
    """2 tp / (2 tp + fp + fn); 0.0 when nothing is predicted and nothing is present"""
    denom = 2 * tp + fp + fn
    return 2.0 * tp / denom if denom > 0 else 0.0


def bce_rows(out, targets, mask, heads: int, inv_n, pos_weight=None, dtype=np.float64):
    """(loss_sum, tp, fp, fn, G) as the kernel defines them.  targets: (rows, classes) of 0/1; mask: one bool per row (None: every row
    is in the loss), a masked-out row gets G = 0.  dtype=np.longdouble: the extended twin."""
    out = np.asarray(out, dtype=dtype)
    rows, n = out.shape
    classes = n // heads
    y = np.asarray(targets).astype(bool)
    assert classes * heads == n and y.shape == (rows, classes)
    live = np.ones(rows, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    w = np.ones(classes, dtype=dtype) if pos_weight is None else np.asarray(pos_weight, dtype=dtype)
    yd = y.astype(dtype)
    z = out.reshape(rows, heads, classes).sum(axis=1) * (dtype(1) / dtype(heads))
    e = np.exp(-np.abs(z))
    sp = np.log1p(e)
    loss = w * yd * (np.maximum(-z, 0) + sp) + (1 - yd) * (np.maximum(z, 0) + sp)
    s = np.where(z >= 0, 1 / (1 + e), e / (1 + e))
    gz = np.where(live[:, None], (dtype(inv_n) / dtype(heads)) * (s * (1 - yd + w * yd) - w * yd), dtype(0))
    pred = z > 0
    sel = live[:, None]
    tp, fp, fn = (int(np.count_nonzero(sel & a & b)) for a, b in ((y, pred), (~y, pred), (y, ~pred)))
    return np.sum(loss[live], dtype=dtype), tp, fp, fn, np.tile(gz, (1, heads))


def bce(out, targets, mask, heads: int, pos_weight=None, dtype=np.float64):
    """(loss, micro-F1, G = dL/d(out), (tp, fp, fn)): the mean over selected rows x classes"""
    rows = np.asarray(out).shape[0]
    count = rows if mask is None else int(np.count_nonzero(mask))
    classes = np.asarray(out).shape[1] // heads
    assert count > 0
    inv_n = dtype(1) / dtype(count * classes)
    loss_sum, tp, fp, fn, g = bce_rows(out, targets, mask, heads, inv_n, pos_weight, dtype)
    return loss_sum * inv_n, micro_f1(tp, fp, fn), g, (tp, fp, fn)


def train(rows, cols, m, x, layers, alpha, targets, mask, heads, w, av, optimizer, steps, pos_weight=None, activations=PUBLISHED, perturb=None):
    """gat_ref.train with the sigmoid head (no dropout): returns (losses, micro-F1s, w, av)."""
    nh, _ = R.heads_of(layers, heads)
    opt = dict(optimizer)
    kind, lr = opt.pop("kind"), opt.pop("lr")
    params = {("w",) + k: v.copy() for k, v in w.items()}
    params.update({("a1",) + k: av[k][0].copy() for k in av})
    params.update({("a2",) + k: av[k][1].copy() for k in av})
    mom = {k: np.zeros_like(v) for k, v in params.items()}
    var = {k: np.zeros_like(v) for k, v in params.items()}
    losses, f1s = [], []
    mode = dict(R.TRAINED, activations=activations)
    for t in range(1, steps + 1):
        wt = {k: params[("w",) + k] for k in w}
        at = {k: (params[("a1",) + k], params[("a2",) + k]) for k in av}
        out = R.forward(rows, cols, m, x, layers, alpha, wt, at, **mode)
        loss, f1, g, _ = bce(out, targets, mask, nh, pos_weight)
        losses.append(float(loss))
        f1s.append(float(f1))
        dw, da, _ = R.backward(rows, cols, m, x, layers, alpha, g, wt, at, **mode)
        grads = {("w",) + k: dw[k] for k in dw}
        grads.update({("a1",) + k: da[k][0] for k in da})
        grads.update({("a2",) + k: da[k][1] for k in da})
        for k in params:
            gk = grads[k]
            if perturb is not None:
                scale, rng = perturb
                gk = gk + scale * np.max(np.abs(gk)) * rng.uniform(-1.0, 1.0, gk.shape)
            if kind == "adam":
                params[k], mom[k], var[k] = R.adam_step(params[k], gk, mom[k], var[k], t, lr, **opt)
            else:
                params[k], var[k] = R.sgd_step(params[k], gk, var[k], lr, **opt)
    return losses, f1s, {k: params[("w",) + k] for k in w}, {k: (params[("a1",) + k], params[("a2",) + k]) for k in av}


def evaluate(rows, cols, m, x, layers, alpha, targets, mask, heads, w, av, pos_weight=None, activations=PUBLISHED):
    """(loss, micro-F1) over mask"""
    out = R.forward(rows, cols, m, x, layers, alpha, w, av, activations=activations, **R.TRAINED)
    loss, f1, _, _ = bce(out, targets, mask, R.heads_of(layers, heads)[0], pos_weight)
    return float(loss), float(f1)


LEARN_STEPS = 60
LEARN_OPTIMIZER = dict(kind="adam", lr=0.02, weight_decay=5e-4)
# what the learning tests ask of the held-out micro-F1: the reference's own value on planted_tags() (0.751; tests/test_gat_multilabel_cpu.py
# prints it) minus 0.05, rounded down to a multiple of 0.05
HELD_OUT_F1 = 0.70


def planted_tags(layers, n=256, tags=None, share=0.35, degree=12, inside=0.9, train_share=0.5, signal=1.5, seed=2):
    """Overlapping communities: every vertex carries each of `tags` tags (default: the last layer's features_per_head) with probability
    `share`, independently, so most carry several and some none; `degree` edges per row, each to a member of one of the row's own tags
    (picked at random) with probability `inside` and uniform otherwise, and one self loop per row; x = signal * the sum of its tags' prototypes
    + standard normal noise; a training mask of train_share; parameters of scale 1 / sqrt(fan-in).  Drawn in this order from
    default_rng(seed): targets, prototypes, noise, edges, mask, W, (a1, a2).  With the defaults, T.GAT_LAYERS and the PUBLISHED activations the
    reference trains (LEARN_OPTIMIZER, LEARN_STEPS) from loss 0.746 to 0.247 with a held-out micro-F1 of 0.751.  Returns dict(rows, cols, m, x, targets, mask, w, av)."""
    rng = np.random.default_rng(seed)
    tags = layers[-1][1] if tags is None else tags
    targets = rng.random((n, tags)) < share
    fin = layers[0][0]
    proto = rng.standard_normal((tags, fin))
    x = signal * (targets.astype(np.float64) @ proto) + rng.standard_normal((n, fin))
    members = [np.flatnonzero(targets[:, c]) for c in range(tags)]
    assert all(len(mb) > 0 for mb in members)
    own = rng.random((n, degree)) < inside
    uniform = rng.integers(0, n, (n, degree))
    pick_tag, pick = rng.random((n, degree)), rng.random((n, degree))
    cols = uniform.copy()
    for i in range(n):
        mine = np.flatnonzero(targets[i])
        if len(mine) == 0:
            continue  # (a vertex without a tag has uniform neighbours)
        for k in range(degree):
            if own[i, k]:
                mb = members[mine[int(pick_tag[i, k] * len(mine))]]
                cols[i, k] = mb[int(pick[i, k] * len(mb))]
    rows = np.concatenate([np.repeat(np.arange(n), degree), np.arange(n)]).astype(np.int64)
    cols = np.concatenate([cols.reshape(-1), np.arange(n)]).astype(np.int64)
    mask = rng.random(n) < train_share
    w = {(li, h): rng.standard_normal((f_in, fph)) / np.sqrt(f_in) for li, (f_in, fph, heads) in enumerate(layers) for h in range(heads)}
    av = {(li, h): (rng.standard_normal(fph) / np.sqrt(fph), rng.standard_normal(fph) / np.sqrt(fph))
          for li, (f_in, fph, heads) in enumerate(layers) for h in range(heads)}
    return dict(rows=rows, cols=cols, m=n, x=x, targets=targets, mask=mask, w=w, av=av)
