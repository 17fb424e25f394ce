"""Tester of a recogniser: average loss and character error rate.  Nothing leaves the device inside the loop: pero_ctc_greedy
(or, with beam_width, pero_ctc_beam; with lm as well, pero_ctc_beam_lm) decodes there, pero_edit_distance compares the decoded labels with the targets there and adds
into one pair of integer totals, which is read once behind the last batch."""
import torch

from .. import ops
from ..precision import autocast
from .model import beam_decode, greedy_decode


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
    def __init__(self, batch_operator, model, dataloader, max_lines=None, bfloat16=False, beam_width=None, lm=None, lm_weight=1.0, length_bonus=0.0,
                 class_top=None):
        self.batch_operator = batch_operator
        self.model = model
        self.dataloader = dataloader
        self.max_lines = max_lines
        self.bfloat16 = bfloat16
        self.beam_width = beam_width   # None: greedy decoding
        self.lm_kw = dict(lm=lm, lm_weight=lm_weight, length_bonus=length_bonus, class_top=class_top)   # beam_decode's; lm None: no language model

    def test(self):
        """{'loss': mean of the batch losses, 'cer': sum of edit distances / sum of target lengths}."""
        total_loss, num_lines, num_batches, totals = 0, 0, 0, None
        self.model.eval()
        with torch.no_grad():
            for batch in self.dataloader:
                images, targets, target_lengths, input_lengths = self.batch_operator.prepare_batch(batch)
                with autocast(self.bfloat16):
                    result = self.model(images, targets, target_lengths, input_lengths)
                total_loss = total_loss + result["loss"]
                blank = getattr(self.model.loss, "blank", 0)
                if self.beam_width is None:
                    labels, lengths = greedy_decode(result["output"], input_lengths, blank)
                else:
                    labels, lengths, _ = beam_decode(result["output"], input_lengths, blank, self.beam_width, **self.lm_kw)
                if totals is None:
                    totals = torch.zeros(2, dtype=torch.int64, device=labels.device)   # sum of distances, sum of target lengths
                ops.edit_distance(labels.contiguous(), lengths.contiguous(), targets.contiguous(), target_lengths.contiguous(), totals)
                num_lines += self.batch_operator.batch_size(batch)
                num_batches += 1
                if self.max_lines is not None and num_lines > self.max_lines:
                    break
        self.model.train()
        distance, characters = totals.tolist()   # the run's one read of the counts
        return {"loss": float(total_loss) / num_batches, "cer": distance / max(characters, 1)}
