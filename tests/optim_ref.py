"""f64 restatement of the optimizer formulas of include/pero_hip.h (pero_adam_step_ex, pero_sumsq_partials + pero_grad_norm_finish),
written from the header.  tests/test_optim_ref_cpu.py pins it to torch.optim.Adam / AdamW + torch.nn.utils.clip_grad_norm_ in f64;
tests/test_gpu_optim.py holds the HIP kernels to it."""
import math

import torch


def global_norm(buffers, scale=1.0):
    """scale * sqrt(sum over every buffer of x^2), in f64."""
    total = 0.0
    for b in buffers:
        total += float((b.detach().double() ** 2).sum())
    return scale * math.sqrt(total)


def clip_coefficient(grad_norm, max_norm):
    """min(1, max_norm / (grad_norm + 1e-6)): torch.nn.utils.clip_grad_norm_."""
    return min(1.0, max_norm / (grad_norm + 1e-6))


def adam_step_ex(p, grad, m, v, vmax, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, weight_decay=0.0, decoupled=False,
                 maximize=False, grad_norm=None, max_norm=None):
    """One step in place on f64 tensors p, m, v (and vmax: a tensor switches amsgrad on, None leaves it off); `step` is 1-based,
    `grad_norm` the global gradient norm already multiplied by grad_scale (None: no clip)."""
    assert p.dtype == m.dtype == v.dtype == torch.float64
    g = grad.double() * grad_scale
    if grad_norm is not None:
        g = g * clip_coefficient(grad_norm, max_norm)
    if maximize:
        g = -g
    if weight_decay != 0:
        if decoupled:
            p.mul_(1.0 - lr * weight_decay)
        else:
            g = g + weight_decay * p
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    m.copy_(beta1 * m + (1.0 - beta1) * g)
    v.copy_(beta2 * v + (1.0 - beta2) * g * g)
    if vmax is not None:
        vmax.copy_(torch.maximum(vmax, v))
        denom = vmax.sqrt() / math.sqrt(bc2) + eps
    else:
        denom = v.sqrt() / math.sqrt(bc2) + eps
    p.sub_((lr / bc1) * m / denom)
