"""float64 restatement of FusedAdam's gradient guard (csrc/adam.hip: whmr_adam_grad_sumsq, whmr_adam_guard_advance, whmr_adam_step_guarded), i.e. of
``torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2.0, error_if_nonfinite=False)`` followed by torch's Adam, plus the skip:

    norm = sqrt(sum g^2)                      over every parameter that has a gradient at this step, float64
    coef = min(1, max_norm / (norm + 1e-6))   1 when max_norm is None; NaN stays NaN (torch.clamp keeps it)
    g    = g * coef                           in the GRADIENT's dtype, as torch's in-place mul_ leaves it: fp32 gradients are rounded to fp32 once
    skip_nonfinite and norm not finite:       nothing changes, not even the step counts

and then tests/adam_reference.adam_step.  tests/test_adam_guard_cpu.py pins it to torch on the CPU; tests/test_adam_guard_gpu.py compares the kernels
with it.  (The kernel also skips when a thread's fp32 share of the sum overflows although the float64 sum would not; no test goes there.)"""
import math

import torch

import adam_reference as AR


def global_norm(grads):
    """float64 L2 norm over the tensors of ``grads`` that are not None, as a Python float (NaN / Inf possible)"""
    return math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads if g is not None))


def clip_coef(norm, max_norm):
    if max_norm is None:
        return 1.0
    c = max_norm / (norm + 1e-6)
    return c if (c < 1.0 or c != c) else 1.0


def guarded_run(p0, grads, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, skip_nonfinite=False):
    """adam_reference.adam_run behind the guard.  Returns (p, m, v, t, log): the float64 state after the last step and one
    dict(norm, coef, applied) per step."""
    p = [x.double().clone() for x in p0]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    t = [0] * len(p)
    log = []
    for gs in grads:
        norm = global_norm(gs)
        applied = not (skip_nonfinite and not math.isfinite(norm))
        coef = clip_coef(norm, max_grad_norm)
        log.append(dict(norm=norm, coef=coef if applied else 0.0, applied=applied))
        if not applied:
            continue
        for i, g in enumerate(gs):
            if g is None:
                continue
            t[i] += 1
            scaled = g * torch.tensor(coef, dtype=g.dtype)          # the one rounding to the gradient's dtype
            p[i], m[i], v[i] = AR.adam_step(p[i], scaled, m[i], v[i], t[i], lr, betas, eps, weight_decay)
    return p, m, v, t, log
