"""CTC fine-tuning of a pre-trained backbone: CTCLoss over the HIP kernels of csrc/ctc.hip and TransformerRecognizer,
the backbone + a character head.  (The reference has no recogniser: an extension, like FusedAdamW.)"""
import collections

import torch

from .. import ops
from ..masked_pretraining.model import LinearHead, init_backbone, init_head


class _CTCFn(torch.autograd.Function):
    """nll (N) f32 of (N, S, C) logits; the backward hands the kernels the upstream (N) gradient as the per-line scale."""

    @staticmethod
    def forward(ctx, output, targets, input_lengths, target_lengths, blank, zero_infinity):
        lg = output.detach().reshape(-1, output.shape[-1])
        if not lg.is_contiguous():
            lg = lg.contiguous()
        tg, il, tl = (torch.as_tensor(t).to(device=lg.device, dtype=torch.int64).contiguous() for t in (targets, input_lengths, target_lengths))
        nll, row_lse, alpha = ops.ctc_fwd(lg, tg, il, tl, blank)
        ctx.save_for_backward(lg, tg, il, tl, row_lse, alpha, nll)
        ctx.shape, ctx.blank, ctx.zero_infinity = output.shape, blank, zero_infinity
        return nll.clone()   # the saved vector stays what the kernels wrote

    @staticmethod
    def backward(ctx, dnll):
        lg, tg, il, tl, row_lse, alpha, nll = ctx.saved_tensors
        g = dnll.detach().to(torch.float32).contiguous()   # stays on the device: no host sync
        dlogits = ops.ctc_bwd(lg, tg, il, tl, row_lse, alpha, nll, g, ctx.blank, ctx.zero_infinity)
        return dlogits.view(ctx.shape), None, None, None, None, None


class CTCLoss(torch.nn.Module):
    """torch.nn.CTCLoss's reductions on (N, S, C) LOGITS (the log-softmax is inside the kernels): "none" -> (N); "sum"; "mean" -> the batch
    mean of nll / clamp(target_length, 1).  zero_infinity: an infeasible line counts 0 and its gradient rows are zeros."""

    def __init__(self, blank=0, reduction="mean", zero_infinity=False):
        super().__init__()
        if reduction not in ("none", "sum", "mean"):
            raise ValueError(f"Unknown reduction: {reduction}")
        self.blank = blank
        self.reduction = reduction
        self.zero_infinity = zero_infinity

    def forward(self, output, targets, input_lengths, target_lengths):
        if output.dim() != 3:
            raise ValueError("CTCLoss: output must be (N, S, C)")
        if not 0 <= self.blank < output.shape[-1]:
            raise ValueError(f"CTCLoss: blank {self.blank} outside [0, {output.shape[-1]})")
        nll = _CTCFn.apply(output, targets, input_lengths, target_lengths, self.blank, self.zero_infinity)
        if self.zero_infinity:
            nll = torch.where(torch.isinf(nll), torch.zeros_like(nll), nll)
        if self.reduction == "none":
            return nll
        if self.reduction == "sum":
            return nll.sum()
        tl = torch.as_tensor(target_lengths).to(device=nll.device).clamp_min(1).to(nll.dtype)
        return (nll / tl).mean()


class TransformerRecognizer(torch.nn.Module):
    # True: with input_lengths the encoder layers attend to the keys [0, input_length) of each line only (the padding of a batch of
    # lines of different widths stays out of every valid token); explicit key_ranges of forward() / decode() win.
    attend_valid_only = False

    def __init__(self, backbone, head, loss=None):
        super().__init__()
        self.backbone = backbone
        self.head = head
        self.loss = CTCLoss() if loss is None else loss

    def _ranges(self, input_lengths, key_ranges):
        if key_ranges is not None or not self.attend_valid_only or input_lengths is None:
            return key_ranges
        il = torch.as_tensor(input_lengths).to(torch.int64)
        return torch.stack((torch.zeros_like(il), il.clamp_min(1)), dim=1)   # an empty line attends to its first position (the kernels' clamp)

    def encode(self, images, key_ranges=None):
        n = images.shape[0]
        tokens = self.backbone.encode_tokens(images, None, **ops.key_ranges_kw(key_ranges))   # (N*S, d) row-major
        return self.head(tokens.view(n, -1, tokens.shape[-1]))

    def forward(self, images, targets=None, target_lengths=None, input_lengths=None, key_ranges=None):
        output = self.encode(images, **ops.key_ranges_kw(self._ranges(input_lengths, key_ranges)))
        loss = None
        if targets is not None and target_lengths is not None:
            if input_lengths is None:
                input_lengths = torch.full((output.shape[0],), output.shape[1], dtype=torch.int64, device=output.device)
            loss = self.loss(output, targets, input_lengths, target_lengths)
        return {"output": output, "loss": loss}

    def decode(self, images, input_lengths=None, key_ranges=None, beam_width=None, nbest=1, lm=None, lm_weight=1.0, length_bonus=0.0,
               class_top=None, return_lm_scores=False):
        """Greedy labels (N, S) int64 padded with -1 and their lengths (N), on the device.  With beam_width: beam_decode's results (lm and the
        keywords behind it: beam_decode's)."""
        with torch.no_grad():
            output = self.encode(images, **ops.key_ranges_kw(self._ranges(input_lengths, key_ranges)))
        return _decode_output(output, input_lengths, getattr(self.loss, "blank", 0), beam_width, nbest=nbest, lm=lm, lm_weight=lm_weight,
                              length_bonus=length_bonus, class_top=class_top, return_lm_scores=return_lm_scores)

    def align(self, images, targets, target_lengths, input_lengths=None, key_ranges=None):
        """forced_align of the lines' own logits to the given strings: where every character sits and how sure the model is of it."""
        with torch.no_grad():
            output = self.encode(images, **ops.key_ranges_kw(self._ranges(input_lengths, key_ranges)))
        return forced_align(output, targets, target_lengths, input_lengths, getattr(self.loss, "blank", 0))

    def transcribe(self, images, input_lengths=None, key_ranges=None, beam_width=None, lm=None, lm_weight=1.0, length_bonus=0.0, class_top=None):
        """Decode (greedy, or with beam_width the best beam hypothesis, with lm under that language model) and align the decoded strings to the
        same logits, in one encoder pass: (labels (N, S) int64 padded with -1, lengths (N), Alignment), all on the device."""
        blank = getattr(self.loss, "blank", 0)
        with torch.no_grad():
            output = self.encode(images, **ops.key_ranges_kw(self._ranges(input_lengths, key_ranges)))
            beam_kw = dict(lm=lm, lm_weight=lm_weight, length_bonus=length_bonus, class_top=class_top)
            labels, lengths = (t.contiguous() for t in _decode_output(output, input_lengths, blank, beam_width, **beam_kw)[:2])
            return labels, lengths, forced_align(output, labels, lengths, input_lengths, blank)

    def save(self, path):
        torch.save(self.state_dict(), path)

    def load(self, path):
        device = next(self.parameters()).device
        self.load_state_dict(torch.load(path, map_location=device, weights_only=True))

    def load_pretrained_backbone(self, path):
        """The `backbone.*` entries of a plain state_dict written by MaskedTransformerEncoder.save or the joint model's save, strictly
        (every backbone tensor must be there, with its shape); the pre-training head's entries are ignored, this model's head is untouched."""
        device = next(self.parameters()).device
        sd = torch.load(path, map_location=device, weights_only=True)
        self.backbone.load_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, strict=True)


def _decoder_args(output, input_lengths):
    n, S, C = output.shape
    lg = output.detach().reshape(-1, C)
    if not lg.is_contiguous():
        lg = lg.contiguous()
    if input_lengths is None:
        il = torch.full((n,), S, dtype=torch.int64, device=lg.device)
    else:
        il = torch.as_tensor(input_lengths).to(device=lg.device, dtype=torch.int64).contiguous()
    return lg, il


def greedy_decode(output, input_lengths=None, blank=0):
    return ops.ctc_greedy(*_decoder_args(output, input_lengths), blank)


def _decode_output(output, input_lengths, blank, beam_width, **beam_kw):
    """The package's one choice of decoder.  Both results begin with (labels, lengths); beam_kw: beam_decode's keywords, unused by greedy."""
    if beam_width is None:
        return greedy_decode(output, input_lengths, blank)
    return beam_decode(output, input_lengths, blank, beam_width, **beam_kw)


def beam_decode(output, input_lengths=None, blank=0, beam_width=16, nbest=1, lm=None, lm_weight=1.0, length_bonus=0.0, class_top=None,
                return_lm_scores=False):
    """CTC prefix beam search of (N, S, C) logits on the device: the nbest <= beam_width best label strings of every line,
    (labels (N, nbest, S) int64 padded with -1, lengths (N, nbest) int64, scores (N, nbest) f32 log-probabilities, best first); a line with
    fewer hypotheses has length 0 and score -inf in the rest.  nbest = 1 drops the hypothesis axis: (N, S), (N), (N).
    lm (an NGramLM over the same classes and blank): shallow fusion, scores = log-probability + lm_weight * LM(string) + length_bonus * |string|
    with the model's end term (ops.ctc_beam_lm; class_top: the classes of a frame that may start a new string).  return_lm_scores: a fourth
    result, the language-model part of every score (needs lm)."""
    if not 1 <= nbest <= beam_width:
        raise ValueError(f"beam_decode: nbest {nbest} outside [1, beam_width = {beam_width}]")
    if lm is None:
        if return_lm_scores:
            raise ValueError("beam_decode: return_lm_scores needs lm")
        labels, lengths, scores, _ = ops.ctc_beam(*_decoder_args(output, input_lengths), beam_width, blank)
        results = (labels, lengths, scores)
    else:
        if lm.blank != blank or lm.num_classes != output.shape[-1]:
            raise ValueError(f"beam_decode: the language model is over {lm.num_classes} classes with blank {lm.blank}, the logits have "
                             f"{output.shape[-1]} classes and the call blank {blank}")
        labels, lengths, scores, _, lm_scores = ops.ctc_beam_lm(*_decoder_args(output, input_lengths), beam_width, lm, lm_weight, length_bonus,
                                                                class_top, True, blank)
        results = (labels, lengths, scores, lm_scores) if return_lm_scores else (labels, lengths, scores)
    if nbest == 1:
        return tuple(r[:, 0] for r in results)
    return tuple(r[:, :nbest] for r in results)


Alignment = collections.namedtuple("Alignment", ["states", "spans", "label_logp", "score", "path_logit", "confidences", "nll", "path_share"])
Alignment.__doc__ = """forced_align's results, on the device.  states (N, S) int32, spans (N, Lmax, 2) int32 [first frame, last frame + 1),
label_logp (N, Lmax), score (N), path_logit (N): pero_ctc_align's outputs (include/pero_hip.h).  confidences (N, Lmax) f32: per label the
geometric mean of its frames' probabilities, 0 where there is no label.  nll (N) and path_share (N) = exp(score + nll), the best path's share
of the string's total probability (a line-level confidence): only with with_nll, else None."""


def forced_align(output, targets, target_lengths, input_lengths=None, blank=0, with_nll=False):
    """CTC forced alignment of (N, S, C) logits to targets (N, Lmax) (padding behind target_lengths is never read) on the device; nothing
    is read back to the host.  An infeasible line (too few frames for its string) has states and spans -1, score -inf, confidences 0."""
    if output.dim() != 3:
        raise ValueError("forced_align: output must be (N, S, C)")
    if not 0 <= blank < output.shape[-1]:
        raise ValueError(f"forced_align: blank {blank} outside [0, {output.shape[-1]})")
    lg, il = _decoder_args(output, input_lengths)
    if lg.dtype not in (torch.float32, torch.bfloat16):
        lg = lg.float()
    tg, tl = (torch.as_tensor(t).to(device=lg.device, dtype=torch.int64).contiguous() for t in (targets, target_lengths))
    states, spans, path_logit, score, label_logp = ops.ctc_align(lg, tg, il, tl, blank)
    frames = spans[..., 1] - spans[..., 0]
    confidences = torch.where(frames > 0, torch.exp(label_logp / frames.clamp_min(1)), torch.zeros_like(label_logp))
    nll = path_share = None
    if with_nll:
        nll = ops.ctc_fwd(lg, tg, il, tl, blank)[0]
        path_share = torch.exp(score + nll)   # an infeasible line: exp(-inf + inf) = NaN
        path_share = torch.where(torch.isfinite(nll), path_share, torch.zeros_like(path_share))
    return Alignment(states, spans, label_logp, score, path_logit, confidences, nll, path_share)


def init_model(device, backbone_definition, head_definition, path=None, pretrained_path=None, blank=0, reduction="mean", zero_infinity=False):
    """The masked train.py helper for a recogniser.  path: a recogniser checkpoint; pretrained_path: a pre-training checkpoint whose backbone is taken."""
    model = TransformerRecognizer(init_backbone(backbone_definition), init_head(head_definition),
                                  loss=CTCLoss(blank=blank, reduction=reduction, zero_infinity=zero_infinity))
    model.to(device)
    if pretrained_path is not None:
        model.load_pretrained_backbone(pretrained_path)
    if path is not None:
        model.load(path)
    return model


__all__ = ["Alignment", "CTCLoss", "TransformerRecognizer", "LinearHead", "beam_decode", "forced_align", "greedy_decode", "init_backbone", "init_head",
           "init_model"]
