"""Retrieval evaluation of the joint-embedding model: does a position of view 1 find its twin in view 2?

The reference looks at this by eye (joint_embedding_pretraining/visualizer.py:63-97: normalise both outputs, multiply one random query per
line with every key of the batch, torch.topk, a collage of crops).  Here the same question is answered with numbers, for every position
that has a twin: `retrieve` is the fused cosine top-k (ops.sim_topk: the similarity matrix is never stored), `alignment_targets` says
which key is the twin, and `RetrievalMeter` accumulates the rank histogram on the device (ops.retrieval_hist) for `Tester(retrieval_ks=)`.
"""
from collections import namedtuple

import torch

from .. import ops

Retrieved = namedtuple("Retrieved", ["indices", "scores"])


def retrieve(queries, keys, k=10, key_mask=None, skip=None, normalize=True):
    """The k most similar keys of every query.  queries (..., D) and keys (..., D): f32 or bf16 device tensors of one dtype (D % 8 == 0);
    key_mask: the keys' leading shape, a key takes part where it is non-zero; skip: the queries' leading shape, the flat key index a query
    must not retrieve (self-retrieval), -1 for none.  normalize: cosine scores (each dot is scaled by the two inverse row norms inside the
    kernel; no normalised copy is made), else plain dot products.

    Returns Retrieved(indices (queries' leading shape, k) int32: flat key indices, best first, -1 behind the last qualifying key;
    scores (same shape) f32, -inf there).  Equal scores come back lower key index first; NaN scores never enter.

    The reference's visualizer passes `largest=False` to torch.topk and so shows the k LEAST similar crops of the batch.  That is not
    reproduced: the collage is meant to show what the model confuses a position with, recall@k and MRR are defined on the most similar
    keys, and a list of least similar keys says nothing about whether the twin was found."""
    d = queries.shape[-1]
    q2, k2 = queries.reshape(-1, d), keys.reshape(-1, d)
    if q2.stride(1) != 1:
        q2 = q2.contiguous()
    if k2.stride(1) != 1:
        k2 = k2.contiguous()
    valid = None
    if key_mask is not None:
        valid = (torch.as_tensor(key_mask, device=k2.device).reshape(-1) != 0).to(torch.uint8)
    sk = None if skip is None else torch.as_tensor(skip, device=q2.device).reshape(-1).to(torch.int32)
    qs = ops.inv_rownorm(q2) if normalize else None
    ks = ops.inv_rownorm(k2) if normalize else None
    idx, val = ops.sim_topk(q2, k2, k, q_scale=qs, key_scale=ks, key_valid=valid, skip=sk)
    lead = tuple(queries.shape[:-1])
    return Retrieved(idx.view(*lead, k), val.view(*lead, k))


def alignment_targets(image_masks1, image_masks2, shift_masks1, shift_masks2, device=None):
    """For every (line, position) of view 1 the flat index line * S + position of its twin in view 2, int32 (lines, S) on the device; -1
    where the position is not selected or where the line's two views select different numbers of positions.  The pairing is that of
    ops.ntxent_slots (pero_ntxent_slots): a position is selected in a view when its shift mask and its image mask are both 1, and the
    k-th selected position of view 1 pairs with the k-th of view 2."""
    slot, count = ops.ntxent_slots(image_masks1, image_masks2, shift_masks1, shift_masks2, device=device)
    lines, S = count.numel(), slot.shape[1]
    slot1, slot2 = slot[:lines].long(), slot[lines:].long()
    pos = torch.arange(S, device=slot.device).expand(lines, S)
    # position of view 2 by rank: unselected positions scatter into a spare column S
    by_rank = torch.full((lines, S + 1), -1, device=slot.device, dtype=torch.long)
    by_rank.scatter_(1, torch.where(slot2 >= 0, slot2, torch.full_like(slot2, S)), torch.where(slot2 >= 0, pos, torch.full_like(pos, -1)))
    twin = by_rank.gather(1, torch.where(slot1 >= 0, slot1, torch.full_like(slot1, S)))
    ok = (slot1 >= 0) & (twin >= 0) & (count >= 0)[:, None]
    base = (torch.arange(lines, device=slot.device) * S)[:, None]
    return torch.where(ok, base + twin, torch.full_like(twin, -1)).to(torch.int32)


def metrics_from_hist(hist, ks):
    """hist: the k + 2 integers of pero_retrieval_hist on the host -> {'recall@j' for j in ks, 'mrr@K', 'retrieval_queries'}."""
    hist = [int(v) for v in hist]
    K = len(hist) - 2
    n = hist[0]
    out = {f"recall@{j}": (sum(hist[1:1 + j]) / n if n else float("nan")) for j in ks}
    out[f"mrr@{K}"] = sum(hist[1 + r] / (r + 1) for r in range(K)) / n if n else float("nan")
    out["retrieval_queries"] = n
    return out


class RetrievalMeter:
    """Rank histogram of the twins over the batches of one test(): queries are the view-1 positions that have a twin (compacted, so that
    the others cost nothing), keys are all view-2 positions of the batch with image_masks2 == 1 - the same line's other positions are the
    hard negatives and stay in.  The histogram stays on the device until result(); per batch the host reads one number, the count of
    queries, to size the compacted query matrix."""

    def __init__(self, ks):
        self.ks = tuple(sorted({int(j) for j in ks}))
        if not self.ks or self.ks[0] < 1:
            raise ValueError("retrieval_ks must be positive integers")
        if self.ks[-1] > ops.SIM_TOPK_MAX:
            raise ValueError(f"retrieval_ks: max {self.ks[-1]} exceeds {ops.SIM_TOPK_MAX} (PERO_SIM_TOPK_MAX)")
        self.k = self.ks[-1]
        self.hist = None

    def lists(self, output1, output2, image_masks1, image_masks2, shift_masks1, shift_masks2):
        """(idx (Q, k), val (Q, k), target (Q)) of one batch's Q queries, or None when no position has a twin."""
        d = output1.shape[-1]
        targets = alignment_targets(image_masks1, image_masks2, shift_masks1, shift_masks2, device=output1.device).reshape(-1)
        rows = torch.nonzero(targets >= 0).reshape(-1)
        if rows.numel() == 0:
            return None
        x = output1.reshape(-1, d)
        y = output2.reshape(-1, d)
        q = ops.gather_rows(x if x.is_contiguous() else x.contiguous(), rows)
        y = y if y.is_contiguous() else y.contiguous()
        valid = (torch.as_tensor(image_masks2, device=y.device).reshape(-1) == 1).to(torch.uint8)
        idx, val = ops.sim_topk(q, y, self.k, q_scale=ops.inv_rownorm(q), key_scale=ops.inv_rownorm(y), key_valid=valid)
        return idx, val, targets[rows].contiguous()

    def update(self, output1, output2, image_masks1, image_masks2, shift_masks1, shift_masks2):
        if self.hist is None:
            self.hist = torch.zeros(self.k + 2, device=output1.device, dtype=torch.int64)
        got = self.lists(output1, output2, image_masks1, image_masks2, shift_masks1, shift_masks2)
        if got is not None:
            ops.retrieval_hist(got[0], got[2], self.hist)

    def result(self):
        """One read of the histogram."""
        hist = [0] * (self.k + 2) if self.hist is None else self.hist.cpu().tolist()
        return metrics_from_hist(hist, self.ks)
