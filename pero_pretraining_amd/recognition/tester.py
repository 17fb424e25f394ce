"""Tester of a recogniser: average loss and character error rate.  The logits never leave the device: pero_ctc_greedy decodes
there, and the decoded labels and their lengths (N * (S + 1) integers) are read back once per batch; the edit distances are
computed on the host."""
import torch

from ..precision import autocast
from .batch_operator import host_targets
from .model import greedy_decode


def levenshtein(a, b):
    """Edit distance (insertions, deletions, substitutions, each 1) of two sequences."""
    if len(a) < len(b):
        a, b = b, a
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        diag, row[0] = row[0], i
        for j, y in enumerate(b, 1):
            diag, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, diag + (x != y))
    return row[len(b)]


class Tester:
    def __init__(self, batch_operator, model, dataloader, max_lines=None, bfloat16=False):
        self.batch_operator = batch_operator
        self.model = model
        self.dataloader = dataloader
        self.max_lines = max_lines
        self.bfloat16 = bfloat16

    def test(self):
        """{'loss': mean of the batch losses, 'cer': sum of edit distances / sum of target lengths}."""
        total_loss, num_lines, num_batches, distance, characters = 0, 0, 0, 0, 0
        self.model.eval()
        with torch.no_grad():
            for batch in self.dataloader:
                images, targets, target_lengths, input_lengths = self.batch_operator.prepare_batch(batch)
                with autocast(self.bfloat16):
                    result = self.model(images, targets, target_lengths, input_lengths)
                total_loss = total_loss + result["loss"]
                labels, lengths = greedy_decode(result["output"], input_lengths, getattr(self.model.loss, "blank", 0))
                decoded = torch.cat((lengths[:, None], labels), dim=1).cpu().tolist()   # the batch's one device -> host transfer
                for line, truth in zip(decoded, host_targets(batch)):
                    distance += levenshtein(line[1:1 + line[0]], truth)
                    characters += len(truth)
                num_lines += self.batch_operator.batch_size(batch)
                num_batches += 1
                if self.max_lines is not None and num_lines > self.max_lines:
                    break
        self.model.train()
        return {"loss": float(total_loss) / num_batches, "cer": distance / max(characters, 1)}
