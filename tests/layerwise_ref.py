"""f64 restatement of the layer-wise optimizer formulas of include/pero_hip.h (pero_lamb_stage1 / pero_lars_stage1,
pero_layer_ratio_finish, pero_lamb_stage2 / pero_lars_stage2), written from the header: one function per optimizer and step over a list
of separate tensors, unfused, with a plain tensor.norm() per tensor.  tests/test_layerwise_ref_cpu.py pins it to torch.optim.AdamW /
torch.optim.SGD in f64 (adaptation off) and to ratios worked out by hand; tests/test_gpu_layerwise_optim.py holds the HIP kernels to it."""
import torch

from optim_ref import clip_coefficient


def prepared_grad(grad, grad_scale, maximize, grad_norm, max_norm):
    """g' = grad * grad_scale, clipped by the global norm (already multiplied by grad_scale; None: no clip), negated under maximize."""
    g = grad.double() * grad_scale
    if grad_norm is not None:
        g = g * clip_coefficient(grad_norm, max_norm)
    return -g if maximize else g


def trust_ratio(p_norm, u_norm, coefficient, adapt):
    """coefficient * |p| / |u| if the group adapts and both norms are > 0, otherwise exactly 1 (a NaN norm fails the comparison)."""
    if adapt and p_norm > 0 and u_norm > 0:
        return coefficient * p_norm / u_norm
    return 1.0


def lamb_step(params, grads, ms, vs, step, lr, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.01, grad_scale=1.0, maximize=False,
              layer_adaptation=True, grad_norm=None, max_norm=None, terms=None):
    """One LAMB step in place on lists of f64 tensors; `step` is 1-based.  Returns [(|p|, |u|, r)] per tensor (|p| before the step).
    terms (a list, optional) receives per tensor the norm of |mhat / denom| + |weight_decay p|: what |u| would be without cancellation
    between its two terms (the tests' error bounds scale with it)."""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    stats = []
    for p, grad, m, v in zip(params, grads, ms, vs):
        assert p.dtype == m.dtype == v.dtype == torch.float64
        g = prepared_grad(grad, grad_scale, maximize, grad_norm, max_norm)
        m.copy_(beta1 * m + (1.0 - beta1) * g)
        v.copy_(beta2 * v + (1.0 - beta2) * g * g)
        quotient, decay = (m / bc1) / ((v / bc2).sqrt() + eps), weight_decay * p
        u = quotient + decay
        if terms is not None:
            terms.append(float((quotient.abs() + decay.abs()).norm()))
        pn, un = float(p.norm()), float(u.norm())
        r = trust_ratio(pn, un, 1.0, layer_adaptation)
        p.sub_((lr * r) * u)
        stats.append((pn, un, r))
    return stats


def lars_step(params, grads, bufs, lr, momentum=0.9, weight_decay=0.0, trust_coefficient=1e-3, grad_scale=1.0, maximize=False,
              layer_adaptation=True, grad_norm=None, max_norm=None, terms=None):
    """One LARS step in place on lists of f64 tensors (bufs: the momentum buffers, zero before the first step).  Returns the stats;
    terms as in lamb_step: the norm of |g'| + |weight_decay p|."""
    stats = []
    for p, grad, buf in zip(params, grads, bufs):
        assert p.dtype == buf.dtype == torch.float64
        g, decay = prepared_grad(grad, grad_scale, maximize, grad_norm, max_norm), weight_decay * p
        u = g + decay
        if terms is not None:
            terms.append(float((g.abs() + decay.abs()).norm()))
        pn, un = float(p.norm()), float(u.norm())
        r = trust_ratio(pn, un, trust_coefficient, layer_adaptation)
        buf.copy_(momentum * buf + r * u)
        p.sub_(lr * buf)
        stats.append((pn, un, r))
    return stats
