"""An independent LAMB reference for the tests: a plain per-tensor loop, in the dtype it is given.

    m <- m + (1 - b1) (g - m)          v <- b2 v + (1 - b2) g g
    u  = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd_i w
    r_i = |w_i| / |u_i| if tensor i is adapted and both norms are > 0, else 1
    w <- w - lr r_i u

An excluded tensor has wd_i = 0 and is not adapted (a plain Adam step). Nothing here is shared
with ml_trainer_amd/ops/optim.py.
"""
import math

import torch


def lamb_loop(weights, grads_per_step, hp, excluded=(), dtype=torch.float64, grad_scale=1.0, maximize=False):
    """weights: list of tensors; grads_per_step: one list of tensors per step. Returns a dict of
    lists, one entry per tensor: p, m, v after the last step, and of that step w_sq, u_sq (the sums
    of squares the trust ratio was formed from, of the weights before the step) and trust."""
    b1, b2 = hp.get("betas", (0.9, 0.999))
    lr, eps, wd = hp["lr"], hp.get("eps", 1e-6), hp.get("weight_decay", 0.01)
    p = [w.detach().to(dtype).clone() for w in weights]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    out = dict(p=p, m=m, v=v, w_sq=[0.0] * len(p), u_sq=[0.0] * len(p), trust=[1.0] * len(p))
    for t, grads in enumerate(grads_per_step, 1):
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        for i, g in enumerate(grads):
            g = g.to(dtype) * grad_scale
            if maximize:
                g = -g
            m[i] += (1.0 - b1) * (g - m[i])
            v[i] *= b2
            v[i] += (1.0 - b2) * g * g
            wd_i = 0.0 if i in excluded else wd
            u = (m[i] / bc1) / (v[i].sqrt() / math.sqrt(bc2) + eps) + wd_i * p[i]
            w_sq, u_sq = float((p[i] * p[i]).sum()), float((u * u).sum())
            r = 1.0
            if i not in excluded and w_sq > 0.0 and u_sq > 0.0:
                r = float(p[i].norm() / u.norm())
            out["w_sq"][i], out["u_sq"][i], out["trust"][i] = w_sq, u_sq, r
            p[i] -= lr * r * u
    return out
