"""Tester of the latent-target model: {"loss": mean of the batch losses, "target_std": the collapse monitor}.

target_std is the mean over the feature dimension of the standard deviation (biased) over ALL masked rows of the test of the targets: a
teacher that collapses to one vector for every position drives it to 0 while the loss looks excellent.  The sums (rows, column sums,
column sums of squares, in f64) and the loss are accumulated on the device and read once per test()."""
import torch

from ..precision import autocast


class Tester:
    def __init__(self, batch_operator, model, dataloader, max_lines=None, bfloat16=False):
        self.batch_operator = batch_operator
        self.model = model
        self.dataloader = dataloader
        self.max_lines = max_lines
        self.bfloat16 = bfloat16

    def test(self):
        total_loss, s1, s2 = None, None, None
        rows = num_lines = num_batches = 0
        self.model.eval()
        with torch.no_grad():
            for batch in self.dataloader:
                result = self.test_step(batch)
                t = result["targets"].double()
                if total_loss is None:
                    total_loss = torch.zeros((), device=t.device, dtype=torch.float64)
                    s1 = torch.zeros(t.shape[1], device=t.device, dtype=torch.float64)
                    s2 = torch.zeros(t.shape[1], device=t.device, dtype=torch.float64)
                total_loss += result["loss"].double()
                s1 += t.sum(0)
                s2 += (t * t).sum(0)
                rows += t.shape[0]                      # a host number: the row list's length
                num_lines += self.batch_operator.batch_size(batch)
                num_batches += 1
                if self.max_lines is not None and num_lines > self.max_lines:
                    break
        self.model.train()
        mean = s1 / rows
        std = (s2 / rows - mean * mean).clamp_min(0).sqrt().mean()
        loss, std = torch.stack([total_loss / num_batches, std]).cpu().tolist()   # the only device -> host transfer of the loop
        return {"loss": loss, "target_std": std}

    def test_step(self, batch):
        images, valid, mask = self.batch_operator.prepare_batch(batch)
        with autocast(self.bfloat16):
            return self.model.forward(images, valid, mask)
