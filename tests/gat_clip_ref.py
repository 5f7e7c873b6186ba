"""numpy reference of gradient clipping by global norm, AdamW and the learning-rate schedules of the GAT's training step
(include/hnh_train_clip.h; GAT.set_grad_clip / set_optimizer("adamw") / set_learning_rate / set_lr_schedule), built on tests/gat_ref.py.

    norm = sqrt(sum over every learned tensor of sum g^2)      coef = min(1, max_norm / (norm + 1e-6))      g <- coef g
(torch.nn.utils.clip_grad_norm_), before the optimizer sees the gradient, so L2 weight decay is added to the clipped gradient.
    AdamW:  p <- p (1 - lr weight_decay),  then Adam's step with g' = g                                      (torch.optim.AdamW)
    lr_t = lr factor(t), t the 1-based step:  t / W for t <= W;  then constant 1 | linear 1 - (1 - f)(t - W)/(T - W) |
           cosine f + (1 - f)(1 + cos(pi (t - W)/(T - W)))/2;  f for t > T (linear and cosine)
train() is gat_ref.train with these three and the same perturb hook; it also returns the norms before clipping."""
import numpy as np

import gat_ref as R

SCHEDULES = ("constant", "linear", "cosine")


def grad_norm(grads):
    """The global 2-norm of a list (or dict) of arrays"""
    arrays = grads.values() if isinstance(grads, dict) else grads
    return float(np.sqrt(sum(float(np.sum(np.square(np.asarray(g, dtype=np.float64)))) for g in arrays)))


def clip_coef(grads, max_norm):
    """min(1, max_norm / (norm + 1e-6)); 1.0 with max_norm None or 0 (clipping off)"""
    if not max_norm:
        return 1.0
    return min(1.0, max_norm / (grad_norm(grads) + 1e-6))


def adamw_step(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """(p, m, v) after step t (1-based): decoupled decay, then gat_ref.adam_step without the L2 term"""
    return R.adam_step(p * (1.0 - lr * weight_decay), g, m, v, t, lr, beta1, beta2, eps, 0.0)


def lr_factor(kind, t, W=0, T=0, min_factor=0.0):
    assert kind in SCHEDULES and t >= 1
    if t <= W:
        return t / W
    if kind == "constant":
        return 1.0
    if t > T:
        return min_factor
    s = (t - W) / (T - W)
    if kind == "linear":
        return 1.0 - (1.0 - min_factor) * s
    return min_factor + (1.0 - min_factor) * 0.5 * (1.0 + np.cos(np.pi * s))


def train(rows, cols, m, x, layers, alpha, labels, mask, heads, w, av, optimizer, steps, rates=(0.0, 0.0), seed0=0, activations=None, perturb=None,
          max_norm=None, schedule=None, lr_at=None):
    """gat_ref.train with optimizer kind "adam" | "sgd" | "adamw", clipping at max_norm (None: off), schedule = dict(kind=.., W=.., T=..,
    min_factor=..) (None: none) and lr_at = {step: new base rate}, set before that step is taken (set_learning_rate; moments and step
    count stay).  perturb = (scale, rng) as in gat_ref.train: the perturbed gradient is what is clipped.  Returns (losses, accuracies, w,
    av, norms), norms[t - 1] = the global norm of step t before clipping."""
    nh, _ = R.heads_of(layers, heads)
    opt = dict(optimizer)
    kind, lr = opt.pop("kind"), opt.pop("lr")
    params = {("w",) + k: v.copy() for k, v in w.items()}
    params.update({("a1",) + k: av[k][0].copy() for k in av})
    params.update({("a2",) + k: av[k][1].copy() for k in av})
    mom = {k: np.zeros_like(v) for k, v in params.items()}
    var = {k: np.zeros_like(v) for k, v in params.items()}
    losses, accs, norms = [], [], []
    dropout = rates[0] > 0.0 or rates[1] > 0.0
    for t in range(1, steps + 1):
        if lr_at and t in lr_at:
            lr = lr_at[t]
        lr_t = lr * (lr_factor(schedule["kind"], t, schedule.get("W", 0), schedule.get("T", 0), schedule.get("min_factor", 0.0)) if schedule else 1.0)
        mode = dict(R.TRAINED, rates=rates, seed=(seed0 + t) & 0xFFFFFFFFFFFFFFFF if dropout else seed0, activations=activations)
        wt = {k: params[("w",) + k] for k in w}
        at = {k: (params[("a1",) + k], params[("a2",) + k]) for k in av}
        out = R.forward(rows, cols, m, x, layers, alpha, wt, at, **mode)
        loss, acc, g = R.xent(out, labels, mask, nh)
        losses.append(float(loss))
        accs.append(float(acc))
        dw, da, _ = R.backward(rows, cols, m, x, layers, alpha, g, wt, at, **mode)
        grads = {("w",) + k: dw[k] for k in dw}
        grads.update({("a1",) + k: da[k][0] for k in da})
        grads.update({("a2",) + k: da[k][1] for k in da})
        if perturb is not None:
            scale, rng = perturb
            grads = {k: grads[k] + scale * np.max(np.abs(grads[k])) * rng.uniform(-1.0, 1.0, grads[k].shape) for k in params}
        norms.append(grad_norm(grads))
        coef = clip_coef(grads, max_norm)
        for k in params:
            gk = grads[k] if coef == 1.0 else coef * grads[k]
            if kind == "adam":
                params[k], mom[k], var[k] = R.adam_step(params[k], gk, mom[k], var[k], t, lr_t, **opt)
            elif kind == "adamw":
                params[k], mom[k], var[k] = adamw_step(params[k], gk, mom[k], var[k], t, lr_t, **opt)
            else:
                params[k], var[k] = R.sgd_step(params[k], gk, var[k], lr_t, **opt)
    return losses, accs, {k: params[("w",) + k] for k in w}, {k: (params[("a1",) + k], params[("a2",) + k]) for k in av}, norms
