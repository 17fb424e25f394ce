"""Tester of a recogniser: average loss and character error rate.  Nothing leaves the device inside the loop: pero_ctc_greedy
(or, with beam_width, pero_ctc_beam; with lm as well, pero_ctc_beam_lm) decodes there, pero_edit_distance compares the decoded labels with the targets there and adds
into one pair of integer totals, which is read once behind the last batch.  With word_separators or details, pero_edit_ops takes its place: the
same table with its backtrace, so the totals also hold substitutions, insertions, deletions and hits, over characters and over words, and a
confusion matrix grows on the device; all of it is still read once."""
import torch

from .. import ops
from ..precision import autocast
from .model import _decode_output


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
                 class_top=None, word_separators=None, details=False):
        self.batch_operator = batch_operator
        self.model = model
        self.dataloader = dataloader
        self.max_lines = max_lines
        self.bfloat16 = bfloat16
        self.beam_width = beam_width   # None: greedy decoding
        self.lm_kw = dict(lm=lm, lm_weight=lm_weight, length_bonus=length_bonus, class_top=class_top)   # beam_decode's; lm None: no language model
        self.word_separators = None if word_separators is None else tuple(word_separators)   # class ids that separate words: adds 'wer'
        self.details = details   # adds the operation counts, the line error rate and the confusion matrix

    def test(self):
        """{'loss': mean of the batch losses, 'cer': sum of edit distances / sum of target lengths}.
        word_separators adds 'wer', the same ratio over words.  details adds 'substitutions', 'insertions', 'deletions', 'hits', 'lines',
        'line_error_rate' (lines with any error / lines), 'confusion' ((C + 1, C + 1) int64 on the host, C = the logits' classes:
        [reference][hypothesis], index C = the gap; see top_confusions) and, with word_separators, the counts again as 'word_...'."""
        scorer = self._distance_scorer if self.word_separators is None and not self.details else self._operations_scorer
        total_loss, num_lines, num_batches, add, report = 0, 0, 0, None, None
        self.model.eval()
        with torch.no_grad():
            for batch in self.dataloader:
                images, targets, target_lengths, input_lengths = self.batch_operator.prepare_batch(batch)
                with autocast(self.bfloat16):
                    result = self.model(images, targets, target_lengths, input_lengths)
                total_loss = total_loss + result["loss"]
                blank = getattr(self.model.loss, "blank", 0)
                labels, lengths = (t.contiguous() for t in _decode_output(result["output"], input_lengths, blank, self.beam_width, **self.lm_kw)[:2])
                if add is None:
                    add, report = scorer(result["output"].shape[-1], labels.device)
                add(labels, lengths, targets.contiguous(), target_lengths.contiguous())
                num_lines += self.batch_operator.batch_size(batch)
                num_batches += 1
                if self.max_lines is not None and num_lines > self.max_lines:
                    break
        self.model.train()
        return {"loss": float(total_loss) / num_batches, **report()}

    # A scorer: (add(labels, lengths, targets, target_lengths), report()) over counters on the device; report is the run's one read of them.
    def _distance_scorer(self, C, device):
        totals = torch.zeros(2, dtype=torch.int64, device=device)   # sum of distances, sum of target lengths

        def report():
            distance, characters = totals.tolist()
            return {"cer": distance / max(characters, 1)}
        return lambda *pair: ops.edit_distance(*pair, totals), report

    def _operations_scorer(self, C, device):
        totals = torch.zeros((2, 6), dtype=torch.int64, device=device)   # pero_edit_ops' totals: row 0 characters, row 1 words
        confusion = torch.zeros((C + 1, C + 1), dtype=torch.int64, device=device) if self.details else None
        is_sep = None if self.word_separators is None else ops.edit_separator_table(self.word_separators, C, device)   # built once

        def add(*pair):
            ops.edit_ops(*pair, num_classes=C, totals=totals[0], confusion=confusion, want_script=False)
            if is_sep is not None:
                ops.edit_ops(*pair, num_classes=C, separators=is_sep, totals=totals[1], want_script=False)

        def report():
            (sub, ins, dele, hit, lines, wrong), word = totals.tolist()
            out = {"cer": (sub + ins + dele) / max(hit + sub + dele, 1)}
            if self.word_separators is not None:
                out["wer"] = (word[0] + word[1] + word[2]) / max(word[3] + word[0] + word[2], 1)
            if self.details:
                out.update(substitutions=sub, insertions=ins, deletions=dele, hits=hit, lines=lines, line_error_rate=wrong / max(lines, 1),
                           confusion=confusion.cpu())
                if self.word_separators is not None:
                    out.update(word_substitutions=word[0], word_insertions=word[1], word_deletions=word[2], word_hits=word[3])
            return out
        return add, report
