"""Batch operator of the CTC fine-tuning step: `prepare_batch(batch) -> (images, targets, target_lengths, input_lengths)`.
The uint8 NHWC batch goes to the device as it is (the fused front end converts it, like the masked operator's);
input_lengths = ceil(width / patch width): the positions that see at least one pixel column of the line."""
import numpy as np
import torch


def _to_device(value, device):
    return torch.as_tensor(value).to(device, non_blocking=True)


class BatchOperator:
    def __init__(self, device, patch_width=8):
        self.device = device
        self.patch_width = patch_width

    def prepare_batch(self, batch):
        """batch: {"images" u8 (N, H, W, C), "targets" (N, Lmax), "target_lengths" (N), "widths" (N) in pixels}."""
        images = _to_device(batch["images"], self.device)
        targets = _to_device(batch["targets"], self.device).long()
        target_lengths = _to_device(batch["target_lengths"], self.device).long()
        widths = _to_device(batch["widths"], self.device).long()
        input_lengths = torch.div(widths + (self.patch_width - 1), self.patch_width, rounding_mode="floor")
        return images, targets, target_lengths, input_lengths

    @staticmethod
    def batch_size(batch):
        return len(batch["images"])


def host_targets(batch):
    """The transcriptions of a batch as Python lists, from the host copy the dataloader made."""
    t, l = np.asarray(batch["targets"]), np.asarray(batch["target_lengths"])
    return [t[i, :int(l[i])].tolist() for i in range(len(l))]
