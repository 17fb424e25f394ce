"""Evaluation loop of the joint-embedding model (surface of the reference's joint_embedding_pretraining/tester.py:
`Tester(batch_operator, model, dataloader, max_lines=None).test() -> {'loss': mean batch loss}`, `test_step(batch)`).

The reference's class reads `self.bfloat16` without ever setting it (tester.py:4-10 vs :47) although its train.py:125
passes `bfloat16=`; the keyword is accepted here (decision recorded in DESIGN.md section 7).  The loss stays a device tensor
through the loop: no per-batch synchronisation.

`retrieval_ks=(1, 5, 10)` adds what a loss value cannot say: whether a position of view 1 finds its twin among all view-2 positions of the
batch (retrieval.RetrievalMeter: fused cosine top-k, rank histogram on the device, read once per test()).  The result gains `recall@j`
for each j, `mrr@K` (K = the largest j) and `retrieval_queries`.  The default, None, makes no new call and returns `{'loss'}` alone."""
import torch

from ..precision import autocast
from .retrieval import RetrievalMeter


class Tester:
    def __init__(self, batch_operator, model, dataloader, max_lines=None, bfloat16=False, retrieval_ks=None):
        self.batch_operator = batch_operator
        self.model = model
        self.dataloader = dataloader
        self.max_lines = max_lines
        self.bfloat16 = bfloat16
        self.retrieval_ks = None if retrieval_ks is None else tuple(retrieval_ks)
        self._meter = None
        if self.retrieval_ks is not None:
            RetrievalMeter(self.retrieval_ks)   # a bad k raises here, not after the first batch

    def test(self):
        losses, lines_seen = [], 0
        self._meter = None if self.retrieval_ks is None else RetrievalMeter(self.retrieval_ks)
        self.model.eval()
        try:
            with torch.no_grad():
                for batch in self.dataloader:
                    losses.append(self.test_step(batch)["loss"])
                    lines_seen += self.batch_operator.batch_size(batch)
                    if self.max_lines is not None and lines_seen > self.max_lines:  # stops after the batch that exceeds it
                        break
        finally:
            self.model.train()
        result = {"loss": sum(losses) / len(losses)}
        if self._meter is not None:
            result.update(self._meter.result())
        return result

    def test_step(self, batch):
        prepared = self.batch_operator.prepare_batch(batch)
        with autocast(self.bfloat16):
            result = self.model.forward(*prepared)
        if self.retrieval_ks is not None:
            if self._meter is None:   # test_step outside test(): the meter lives until the next test()
                self._meter = RetrievalMeter(self.retrieval_ks)
            self._meter.update(result["output1"], result["output2"], *prepared[2:])
        return result
