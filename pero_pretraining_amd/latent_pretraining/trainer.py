"""Trainer of the latent-target step, with the masked Trainer's surface.  The step is zero_grad -> forward -> backward -> optimizer.step()
-> model.after_step() (the teacher's EMA update: one launch).  Capturing the step as a hipGraph and data-parallel training are not
offered here."""
from ..masked_pretraining.trainer import Trainer as _Base
from ..precision import autocast


class Trainer(_Base):
    def __init__(self, batch_operator, model, dataloader, optimizer, scheduler, bfloat16=False, data_parallel=None, hip_graph=False):
        if data_parallel is not None or hip_graph:
            raise ValueError("latent_pretraining.Trainer: data_parallel and hip_graph are not supported for the latent-target step")
        super().__init__(batch_operator, model, dataloader, optimizer, scheduler, bfloat16=bfloat16)

    def train_step(self, batch):
        return self.train_step_prepared(*self.batch_operator.prepare_batch(batch))

    def train_step_prepared(self, images, valid, mask, rows=None):
        self.optimizer.zero_grad()
        with autocast(self.bfloat16):
            output = self.model.forward(images, valid, mask, rows=rows)
        loss = output["loss"]
        loss.backward()
        self.optimizer.step()
        self.model.after_step()
        return loss.detach()

    step = train_step
