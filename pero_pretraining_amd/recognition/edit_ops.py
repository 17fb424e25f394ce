"""What a recogniser got wrong, not only how much: the edit operations between hypotheses and references (pero_edit_ops: substitutions,
insertions, deletions and hits per line, the script that aligns the two strings, a confusion matrix; with separators the same over words)
and a host helper that lists the largest confusions."""
import torch

from .. import ops


class EditOperations:
    """edit_operations' results, on the device.  counts (N, 4) int64: substitutions, insertions, deletions, hits of every pair; script
    (N, La + Lb) int8: 0 hit, 1 substitution, 2 insertion (of a hypothesis element), 3 deletion (of a reference element) in forward order, -1
    behind script_lengths (N) int32 (include/pero_hip.h states the tie rule).  hyp_spans (N, (La + 1) / 2, 2), ref_spans (N, (Lb + 1) / 2, 2)
    int32: at word level [begin, end) of every word in its row, -1 behind the last; None at symbol level."""

    def __init__(self, counts, script, script_lengths, hyp_spans=None, ref_spans=None):
        self.counts, self.script, self.script_lengths, self.hyp_spans, self.ref_spans = counts, script, script_lengths, hyp_spans, ref_spans

    @property
    def distance(self):
        """(N) int64: the edit distance of every pair."""
        return self.counts[:, :3].sum(1)

    def pairs(self):
        """(N, La + Lb, 2) int32: the (hypothesis, reference) element indices of every step of the script (word indices at word level), -1 for
        the gap of an insertion or deletion and behind script_lengths.  Computed on the device: a step's index is the count of the steps in
        front of it that took an element of that side."""
        code = self.script
        takes_hyp = (code >= 0) & (code != 3)
        takes_ref = (code >= 0) & (code != 2)
        i = torch.where(takes_hyp, takes_hyp.cumsum(1) - 1, -1)
        j = torch.where(takes_ref, takes_ref.cumsum(1) - 1, -1)
        return torch.stack((i, j), dim=2).to(torch.int32)


def edit_operations(hyp, hyp_lengths, ref, ref_lengths, separators=None, num_classes=None, confusion=None):
    """The edit operations that turn every reference ref[n][:ref_lengths[n]] into the hypothesis hyp[n][:hyp_lengths[n]] (padded label matrices
    (N, La), (N, Lb); the padding is never read), on the device: an EditOperations.  separators (class ids; needs num_classes): the operations
    are over words, the runs of labels between separators.  confusion ((num_classes + 1, num_classes + 1) int64 on the device, symbol level
    only): confusion[r][h] += 1 for every reference label r read as h, row / column num_classes being the gap (a deletion / an insertion);
    accumulated, so one matrix can collect a whole test set."""
    dev = hyp.device
    a, a_len, b, b_len = (torch.as_tensor(t).to(device=dev, dtype=torch.int64).contiguous() for t in (hyp, hyp_lengths, ref, ref_lengths))
    counts, script, script_len, a_spans, b_spans = ops.edit_ops(a, a_len, b, b_len, num_classes=num_classes, separators=separators, confusion=confusion,
                                                                want_spans=separators is not None)
    return EditOperations(counts, script, script_len, a_spans, b_spans)


def top_confusions(confusion, k=20, symbols=None):
    """The k largest off-diagonal entries of a confusion matrix ((C + 1, C + 1), row = reference, column = hypothesis, index C = the gap) as
    [(reference, hypothesis, count)], zero entries left out: count descending, then reference, then hypothesis (the gap last).  symbols: a
    sequence or mapping from class id to a name; the gap is None either way.  Reads the matrix to the host."""
    m = torch.as_tensor(confusion).detach().cpu()
    C = m.shape[0] - 1
    r, h = torch.nonzero(m, as_tuple=True)
    entries = sorted((-int(m[i, j]), int(i), int(j)) for i, j in zip(r.tolist(), h.tolist()) if i != j)

    def name(c):
        return None if c == C else (c if symbols is None else symbols[c])
    return [(name(i), name(j), -neg) for neg, i, j in entries[:k]]
