"""Batch operator of the latent-target step: `prepare_batch(batch) -> (images, valid, mask)`.

`valid` (N, S) marks the positions that belong to a line: `labels >= 0` when the batch carries labels (the collator labels the padding
-1), else `batch["image_masks"]`.  The mask is drawn on the HOST from numpy's global stream and stays a host array, so the model's row
list costs no device sync.  mask_span == 1 is the masked operator's draw - `np.random.rand(*shape) < p`, times valid - so a seeded run
masks the positions the masked step would.  mask_span > 1 masks runs: starts are drawn with `np.random.rand(*shape) < p / mask_span`, a
start masks itself and the next mask_span - 1 positions of its line (cut at the line's end), and the result is multiplied by valid."""
import numpy as np

from ..masked_pretraining.batch_operator import BatchOperator as _Base
from ..masked_pretraining.batch_operator import _to_device


def span_mask(starts, mask_span):
    """(N, S) bool starts -> (N, S) int mask: position j is masked if any of j - mask_span + 1 .. j is a start."""
    starts = np.asarray(starts).astype(bool)
    out = starts.copy()
    for k in range(1, int(mask_span)):
        out[:, k:] |= starts[:, :-k] if k < starts.shape[1] else False
    return out.astype(int)


class BatchOperator(_Base):
    def __init__(self, device, masking_prob, mask_span=1, float_images=False):
        super().__init__(device, masking_prob, float_images=float_images)
        if mask_span < 1:
            raise ValueError(f"BatchOperator: mask_span must be at least 1, got {mask_span}")
        self.mask_span = int(mask_span)

    def prepare_batch(self, batch):
        valid = self._valid(batch)
        return self._prepare_batch_images(batch), _to_device(valid, self.device), self._create_mask(batch, valid)

    @staticmethod
    def _valid(batch):
        """(N, S) int host array: 1 on a line's own positions."""
        if batch.get("labels") is not None:
            labels = batch["labels"]
            labels = labels.cpu().numpy() if hasattr(labels, "cpu") else np.asarray(labels)
            return (labels >= 0).astype(int)
        masks = batch["image_masks"]
        masks = masks.cpu().numpy() if hasattr(masks, "cpu") else np.asarray(masks)
        return (masks != 0).astype(int)

    def _create_mask(self, batch, valid=None):
        valid = self._valid(batch) if valid is None else valid
        if self.mask_span == 1:
            drawn = np.random.rand(*valid.shape) < self.masking_prob
            return drawn.astype(int) * valid
        starts = np.random.rand(*valid.shape) < self.masking_prob / self.mask_span
        return span_mask(starts, self.mask_span) * valid
