"""float64 restatement of the Adam step csrc/adam.hip evaluates in fp32 (torch's non-amsgrad Adam with L2 weight decay):

    g' = g + wd p
    m  = m + (g' - m)(1 - beta1)
    v  = beta2 v + (1 - beta2) g'^2
    p  = p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)          bc_i = 1 - beta_i^t, t = 1, 2, ...

tests/test_adam_cpu.py pins it to torch.optim.Adam on float64 parameters; tests/test_adam_gpu.py compares the kernel with it."""
import math

import torch


def adam_step(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """one step, t = the step count AFTER this step (1 for the first); all tensors float64; returns new (p, m, v)"""
    b1, b2 = betas
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    if weight_decay != 0:
        g = g + weight_decay * p
    m = m + (g - m) * (1 - b1)
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def adam_run(p0, grads, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, lrs=None):
    """p0: list of tensors, grads: one list of tensors per step (``None`` entries skip that parameter, as torch does: p, m, v and its step count
    stay), lrs: a learning rate per step (default: lr throughout).  Returns (p, m, v, t) lists after the last step, float64."""
    p = [x.double().clone() for x in p0]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    t = [0] * len(p)
    for k, gs in enumerate(grads):
        for i, g in enumerate(gs):
            if g is None:
                continue
            t[i] += 1
            p[i], m[i], v[i] = adam_step(p[i], g, m[i], v[i], t[i], lr if lrs is None else lrs[k], betas, eps, weight_decay)
    return p, m, v, t
