"""Tokenizer-free masked pre-training: self-distillation with latent targets, in the style of data2vec (Baevski et al., 2022).

A teacher whose weights are an exponential moving average of the student's backbone (optim.WeightEMA) encodes the UNMASKED line; at the
masked positions the student regresses, through a linear head, the mean over the teacher's top layers of their outputs normalised over
the feature dimension (ops.latent_targets), under a smooth-L1 / MSE loss (ops.latent_loss_fwd / _bwd).  Nothing is fitted beforehand: the
step starts from a folder of unlabelled line images.

The reference has no counterpart.  What the tests pin is this arithmetic (tests/latent_ref.py restates it in f64); whether it learns good
representations has not been evaluated."""
import numpy as np
import torch

from .. import ops
from ..masked_pretraining.model import LinearHead, _GatherTokensFn, init_backbone, init_head, masked_row_list
from ..optim import WeightEMA

__all__ = ["LatentTargetTransformerEncoder", "LinearHead", "init_backbone", "init_head", "init_model"]


class _LatentLossFn(torch.autograd.Function):
    """mean over the first n rows of l(pred - targets) as one node; the backward reads dloss on the device."""

    @staticmethod
    def forward(ctx, pred, targets, n, beta):
        p = pred.detach()
        if not p.is_contiguous():
            p = p.contiguous()
        ctx.save_for_backward(p, targets)
        ctx.n, ctx.beta = n, beta
        return ops.latent_loss_fwd(p, targets, n, beta)[0]

    @staticmethod
    def backward(ctx, dloss):
        p, targets = ctx.saved_tensors
        dl = dloss.detach().reshape(1).to(torch.float32)   # stays on the device: no host sync
        return ops.latent_loss_bwd(p, targets, ctx.n, ctx.beta, dloss=dl), None, None, None


class LatentTargetTransformerEncoder(torch.nn.Module):
    """backbone: the student (a models.transformers backbone); head: LinearHead(d, d); `.ema`: the teacher, WeightEMA(backbone, decay,
    decay_start, ramp_updates).  top_k: the teacher's top min(top_k, num_blocks) layers are averaged into the targets; beta: the smooth-L1
    threshold (0: MSE); eps: of the targets' normalisation."""

    # True: the encoder layers of teacher AND student attend to each line's valid positions only - the hull of `valid` - instead of all S
    # positions, padding included.  Explicit `key_ranges` of forward() win.  (masked_pretraining.model.MaskedTransformerEncoder's switch.)
    attend_valid_only = False

    def __init__(self, backbone, head, top_k=8, beta=2.0, eps=1e-5, decay=0.999, decay_start=None, ramp_updates=0):
        super().__init__()
        if top_k < 1 or beta < 0 or eps < 0:
            raise ValueError(f"LatentTargetTransformerEncoder: invalid top_k / beta / eps: {top_k}, {beta}, {eps}")
        self.backbone = backbone
        self.head = head
        self.top_k, self.beta, self.eps = int(top_k), float(beta), float(eps)
        self.ema = WeightEMA(backbone, decay=decay, decay_start=decay_start, ramp_updates=ramp_updates)   # no Module: not in state_dict()

    def _apply(self, fn, *args, **kwargs):
        """to() / cuda(): the teacher moves with the student and its flat buffers are laid out again on the new device."""
        super()._apply(fn, *args, **kwargs)
        self.ema.module._apply(fn, *args, **kwargs)
        self.ema.flatten()
        return self

    @property
    def teacher(self):
        return self.ema.module

    def tap_layers(self):
        k = min(self.top_k, self.backbone.num_blocks)
        return list(range(self.backbone.num_blocks - k, self.backbone.num_blocks))

    def _ranges(self, x, valid, key_ranges):
        if key_ranges is not None or not self.attend_valid_only or valid is None:
            return key_ranges
        if isinstance(valid, torch.Tensor) and valid.is_cuda:
            return ops.key_ranges_from_masks((valid != 0).to(torch.uint8))
        v = valid.numpy() if isinstance(valid, torch.Tensor) else np.asarray(valid)
        return ops.key_ranges_from_masks((v != 0).astype(np.uint8), device=x.device)

    def forward(self, x, valid=None, mask=None, rows=None, key_ranges=None):
        """x: uint8 (N,H,W,C) or float32 (N,C,H,W) line images; valid (N, S): the positions that belong to a line (only read for
        attend_valid_only); mask (N, S): 1 where the student's input is masked and the loss is taken; rows: the flat positions with
        mask == 1, when the caller has them on the device already.
        The row list comes from masked_row_list(mask, rows): no device sync when the mask is known on the host (a numpy array, a CPU tensor,
        or an uploaded tensor that carries its host original); a mask that exists on the device only falls back to torch.nonzero, which
        synchronises once per step.
        Returns {"loss", "output_rows", "rows", "targets"}; without `mask`, {"output": head(tokens)} (N, S, d)."""
        key_ranges = self._ranges(x, valid, key_ranges)
        kr = ops.key_ranges_kw(key_ranges)
        if mask is None:
            tokens = self.backbone.encode_tokens(x, None, **kr)
            return {"output": self.head(tokens.view(x.shape[0], -1, tokens.shape[-1]))}
        index = masked_row_list(mask, rows)
        if index is None:   # a device-only mask: one synchronising round trip
            index = torch.nonzero(torch.as_tensor(mask).reshape(-1) == 1, as_tuple=False).reshape(-1)
        n = index.numel()
        if n == 0:   # nothing masked: the NaN of a mean over an empty selection, as the masked model gives (differentiable, like its loss)
            d = self.backbone.model_dim
            empty = torch.empty((0, d), device=x.device, dtype=torch.float32)
            return {"loss": self.head.linear.bias.sum() * float("nan"), "output_rows": empty, "rows": index.to(x.device), "targets": empty}
        n_pad = ((n + 255) // 256) * 256                              # whole 256-row GEMM tiles; pad rows are zero
        # one draw of the positional offsets (the torch.randint call a masked step makes), injected into teacher and student
        w = x.shape[2] if x.dtype == torch.uint8 else x.shape[3]
        offsets = self.backbone.position_model.draw_offsets(x.shape[0], w // self.backbone.patch_size[1], x.device)
        self.teacher.set_offsets(offsets)
        self.backbone.set_offsets(offsets)
        # the teacher first: encode_tokens(x, mask) overwrites a float32 x in place, and the teacher sees the unmasked line
        taps = self.teacher.encode_layers(x, self.tap_layers(), **kr)
        index = index.to(x.device, non_blocking=True)
        targets = ops.latent_targets(taps, index, n_pad, self.eps)
        del taps
        tokens = self.backbone.encode_tokens(x, mask, **kr)           # (N*S, d)
        picked = _GatherTokensFn.apply(tokens, index, n_pad)
        pred = self.head(picked)                                      # (n_pad, d)
        loss = _LatentLossFn.apply(pred, targets, n, self.beta)       # n == 0: NaN, the mean over an empty selection
        return {"loss": loss, "output_rows": pred[:n], "rows": index, "targets": targets[:n]}

    def after_step(self):
        """Behind optimizer.step(): the teacher follows the student."""
        self.ema.update()

    # ---- checkpoint: a plain state_dict; the student under backbone.* / head.* (recognition's load_pretrained_backbone reads the file
    # unchanged), the EMA state under teacher.*
    def save(self, path):
        state = dict(self.state_dict())
        ema = self.ema.state_dict()
        state.update({"teacher." + k: v for k, v in ema["module"].items()})
        state["teacher.n_updates"] = torch.tensor(ema["n_updates"], dtype=torch.int64)
        state["teacher.decay"] = torch.tensor(ema["decay"], dtype=torch.float64)
        state["teacher.decay_start"] = torch.tensor(float("nan") if ema["decay_start"] is None else ema["decay_start"], dtype=torch.float64)
        state["teacher.ramp_updates"] = torch.tensor(ema["ramp_updates"], dtype=torch.int64)
        torch.save(state, path)

    _EMA_KEYS = ("n_updates", "decay", "decay_start", "ramp_updates")

    def load(self, path):
        """Reads what save() wrote, with the loader that executes nothing from the file.  A file without teacher.* entries (a checkpoint of
        another pre-training model with this backbone and head) loads the student and resets the teacher to it."""
        device = next(self.parameters()).device
        sd = torch.load(path, map_location=device, weights_only=True)
        teacher = {k[len("teacher."):]: v for k, v in sd.items() if k.startswith("teacher.")}
        self.load_state_dict({k: v for k, v in sd.items() if not k.startswith("teacher.")})
        if not teacher:
            self.ema.copy_from()
            return
        start = float(teacher["decay_start"])
        self.ema.load_state_dict({"module": {k: v for k, v in teacher.items() if k not in self._EMA_KEYS},
                                  "n_updates": int(teacher["n_updates"]), "decay": float(teacher["decay"]),
                                  "decay_start": None if start != start else start, "ramp_updates": int(teacher["ramp_updates"])})


def init_model(device, backbone_definition, head_definition, path=None, **kw):
    """The masked init_model's wiring; kw: top_k, beta, eps, decay, decay_start, ramp_updates."""
    backbone = init_backbone(backbone_definition)
    head = init_head(head_definition)
    model = LatentTargetTransformerEncoder(backbone, head, **kw)
    model.to(device)
    if path is not None:
        model.load(path)
    return model
