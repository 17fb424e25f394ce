"""Trainer of the CTC fine-tuning step, with the masked Trainer's surface: train(end, start, view_step), train_step(batch) -> loss,
train_step_prepared, on_view_step.  (Capturing the step as a hipGraph is not offered here.)"""
import time

from ..precision import autocast


class Trainer:
    def __init__(self, batch_operator, model, dataloader, optimizer, scheduler, bfloat16=False, data_parallel=None, hip_graph=False):
        if data_parallel is not None or hip_graph:
            raise ValueError("recognition.Trainer: data_parallel and hip_graph are not supported for the recogniser step")
        self.batch_operator = batch_operator
        self.model = model
        self.dataloader = dataloader
        self.optimizer = optimizer
        self.scheduler = scheduler
        self.bfloat16 = bfloat16
        self.on_view_step = None

    def train(self, end_iteration, start_iteration=0, view_step=1000):
        dataloader_iterator = iter(self.dataloader)
        start_time = time.time()
        iteration_count = 0
        for iteration in range(start_iteration, end_iteration + 1):
            try:
                batch = next(dataloader_iterator)
            except StopIteration:
                dataloader_iterator = iter(self.dataloader)
                batch = next(dataloader_iterator)
            self.scheduler.update_learning_rate(iteration)
            self.train_step(batch)
            iteration_count += 1
            if self.on_view_step is not None and iteration > 0 and iteration % view_step == 0:
                elapsed_time = time.time() - start_time
                self.on_view_step(iteration, self.model, elapsed_time, iteration_count)
                iteration_count = 0
                start_time = time.time()

    def train_step(self, batch):
        return self.train_step_prepared(*self.batch_operator.prepare_batch(batch))

    def train_step_prepared(self, images, targets, target_lengths, input_lengths=None):
        self.optimizer.zero_grad()
        with autocast(self.bfloat16):
            output = self.model(images, targets, target_lengths, input_lengths)
        loss = output["loss"]
        loss.backward()
        self.optimizer.step()
        return loss.detach()

    step = train_step
