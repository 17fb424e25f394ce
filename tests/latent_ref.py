"""f64 restatement of the latent-target step (include/pero_hip.h "latent-target self-distillation", pero_pretraining_amd/optim.py
WeightEMA, latent_pretraining/): the EMA with its decay schedule, the targets, the loss and its gradient, the span mask, the collapse
monitor, and the whole step on the oracle's backbone.  Not a test module; it never imports the library.  test_latent_ref_cpu.py pins it to
torch; the GPU tests compare the kernels and the model with it.

Like tests/parity_ref.py, the kernel-level functions return `mag` beside the result: the sum of the absolute values the formula adds."""
import numpy as np
import torch

from oracle import pero_oracle as O


# ------------------------------------------------------------------------------------------------ EMA
def ema_decay(k, decay, decay_start=None, ramp_updates=0):
    """tau of update k (0-based), f64."""
    if decay_start is None or ramp_updates == 0:
        return float(decay)
    return float(decay_start) + (float(decay) - float(decay_start)) * min(int(k), int(ramp_updates)) / int(ramp_updates)


def ema_update(avg, params, tau):
    """avg <- avg + (1 - tau) * (p - avg), in the dtype of avg (f64 tensors: the restatement; the GPU test evaluates the same formula in
    numpy float32 for the bit comparison)."""
    return [a + (1.0 - tau) * (p - a) for a, p in zip(avg, params)]


def ema_update_f32(a, p, w):
    """The kernel's chain in numpy float32: every operation rounds once, nothing is contracted."""
    a, p, w = np.asarray(a, np.float32), np.asarray(p, np.float32), np.float32(w)
    return (a + w * (p - a)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ targets
def latent_targets(mats, index, n_pad, eps):
    """(y (n_pad, d) f64, mag (n_pad, d)): mag = mean over k of (|x - mu| + mean|x|) * rs, what an error of mu and of the deviation
    scale with."""
    mats = [torch.as_tensor(m).detach().cpu().double() for m in mats]
    index = torch.as_tensor(index).cpu().long()
    n, d = index.numel(), mats[0].shape[1]
    y = torch.zeros(n_pad, d, dtype=torch.float64)
    mag = torch.zeros(n_pad, d, dtype=torch.float64)
    for m in mats:
        x = m[index]
        mu = x.mean(1, keepdim=True)
        var = ((x - mu) ** 2).mean(1, keepdim=True)
        rs = 1.0 / torch.sqrt(var + eps)
        y[:n] += (x - mu) * rs
        mag[:n] += ((x - mu).abs() + x.abs().mean(1, keepdim=True)) * rs
    return y / len(mats), mag / len(mats)


# ------------------------------------------------------------------------------------------------ loss
def _l(e, beta):
    if beta == 0:
        return e * e
    a = e.abs()
    return torch.where(a < beta, 0.5 * e * e / beta, a - 0.5 * beta)


def _dl(e, beta):
    if beta == 0:
        return 2.0 * e
    return torch.where(e.abs() < beta, e / beta, torch.sign(e))


def latent_loss(pred, y, n, beta):
    """(loss, mag): every term is positive, so mag is the loss itself."""
    e = (torch.as_tensor(pred).detach().cpu().double() - torch.as_tensor(y).detach().cpu().double())[:n]
    loss = _l(e, float(beta)).sum() / (n * e.shape[1])
    return loss, loss.clone()


def latent_loss_grad(pred, y, n, beta, dloss=1.0):
    """dpred (n_pad, d) f64, zero rows behind n."""
    p, t = torch.as_tensor(pred).detach().cpu().double(), torch.as_tensor(y).detach().cpu().double()
    g = torch.zeros_like(p)
    g[:n] = float(dloss) * _dl((p - t)[:n], float(beta)) / (n * p.shape[1])
    return g


def branch_offenders(pred, y, beta, margin=1e-3):
    """Elements whose |e| lies within margin * beta of beta: a rounding could flip the branch of l'."""
    if beta == 0:
        return torch.zeros_like(torch.as_tensor(pred), dtype=torch.bool)
    e = torch.as_tensor(pred).double() - torch.as_tensor(y).double()
    return (e.abs() - beta).abs() < margin * beta


def move_off_branch(pred, y, beta, margin=1e-3):
    """pred with the offenders moved away from the branch point (by 4 margins, outwards)."""
    pred = torch.as_tensor(pred).clone()
    bad = branch_offenders(pred, y, beta, margin)
    e = pred.double() - torch.as_tensor(y).double()
    moved = pred.double() + torch.sign(e) * 4 * margin * beta
    return torch.where(bad, moved.to(pred.dtype), pred)


# ------------------------------------------------------------------------------------------------ masks, monitor
def span_mask(rand, p, mask_span, valid):
    """rand: the (N, S) uniform draws.  mask_span 1: (rand < p) * valid; else starts = rand < p / mask_span, a start masks itself and the
    next mask_span - 1 positions of its line; times valid."""
    rand, valid = np.asarray(rand), np.asarray(valid).astype(int)
    if mask_span == 1:
        return (rand < p).astype(int) * valid
    starts = rand < p / mask_span
    out = np.zeros(rand.shape, dtype=int)
    for i, j in zip(*np.nonzero(starts)):
        out[i, j:j + mask_span] = 1
    return out * valid


def target_std(targets):
    """Mean over d of the (biased) standard deviation over the rows."""
    t = torch.as_tensor(targets).detach().cpu().double()
    return float(t.std(0, unbiased=False).mean())


# ------------------------------------------------------------------------------------------------ the step on the oracle's backbone
def backbone_layers(sd, x_nchw, num_heads, mask=None, offsets=None, max_len=4096, prefix="backbone."):
    """oracle.backbone_tokens, keeping every layer's output rows (N*S, d); in the dtype of x / sd."""
    n, c, h, w = x_nchw.shape
    conv_w = sd[prefix + "conv_layer.weight"]
    pw = conv_w.shape[-1]
    s = w // pw
    if mask is not None:
        x_nchw = O.apply_mask(x_nchw, mask, O.mask_tile(c, conv_w.shape[-2], pw).to(x_nchw.dtype), pw)
    t = O.patch_embed(x_nchw, conv_w, sd[prefix + "conv_layer.bias"], pw)
    t = O.layer_norm(t, sd[prefix + "intermediate_norm.weight"], sd[prefix + "intermediate_norm.bias"])
    t = O.add_positional(t, n, s, O.positional_table(t.shape[-1], max_len), offsets)
    outs, i = [], 0
    while f"{prefix}encoder_layers.layers.{i}.linear1.weight" in sd:
        t = O.encoder_layer(t, O.layer_params(sd, i, prefix + "encoder_layers.layers."), n, s, num_heads)
        outs.append(t)
        i += 1
    return outs


def latent_step(student_sd, teacher_sd, images_u8_nhwc, mask, num_heads, top_k, beta, eps, offsets=None, key="backbone."):
    """One forward of LatentTargetTransformerEncoder in f64.  student_sd: backbone.* / head.* tensors (those that require grad get a
    gradient through the returned loss); teacher_sd: the teacher backbone's tensors under the same `backbone.` prefix.
    Returns (loss, targets (n, d), predictions (n, d), index)."""
    x = O.prepare_images(torch.as_tensor(images_u8_nhwc)).double()
    mask = np.asarray(mask)
    index = torch.from_numpy(np.flatnonzero(mask.reshape(-1) == 1))
    with torch.no_grad():
        touts = backbone_layers({k: v.detach() for k, v in teacher_sd.items()}, x, num_heads, None, offsets, prefix=key)
        k = min(top_k, len(touts))
        targets, _ = latent_targets(touts[len(touts) - k:], index, index.numel(), eps)
    tokens = backbone_layers(student_sd, x, num_heads, mask, offsets, prefix=key)[-1]
    pred = tokens[index] @ student_sd["head.linear.weight"].t() + student_sd["head.linear.bias"]
    loss = _l(pred - targets, float(beta)).sum() / pred.numel()
    return loss, targets, pred, index
