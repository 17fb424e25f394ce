"""The object wiring of masked_pretraining/train.py for the latent-target step, under the same names and without a command line:
init_model, init_batch_operator, init_testers, init_training (with its `optimizer=` choices), view_step_handler and resume, which also
restores the teacher (the `teacher.*` entries of the checkpoint)."""
import os
from functools import partial

from ..common.helpers import get_checkpoint_path, get_training_state_path, load_training_state, save_training_state
from ..common.lr_scheduler import WarmupSchleduler
from ..masked_pretraining.train import save_model  # noqa: F401  (same semantics)
from ..optim import FusedAdam, FusedAdamW, FusedLAMB, FusedLARS, decay_groups, layerwise_groups
from .batch_operator import BatchOperator
from .model import init_model  # noqa: F401
from .tester import Tester
from .trainer import Trainer


def init_batch_operator(device, masking_prob, mask_span=1):
    return BatchOperator(device=device, masking_prob=masking_prob, mask_span=mask_span)


def init_testers(batch_operator, model, trn_dataloader, tst_dataloader, bfloat16=False):
    return (Tester(batch_operator, model, trn_dataloader, max_lines=1000, bfloat16=bfloat16),
            Tester(batch_operator, model, tst_dataloader, bfloat16=bfloat16))


def report(iteration, dataset, result, scheduler, clearml_logger=None):
    name = dataset.name() if callable(getattr(dataset, "name", None)) else str(getattr(dataset, "name", "dataset"))
    print(f"TEST {name} iteration:{iteration} loss:{float(result['loss']):.6f} target_std:{float(result['target_std']):.6f} "
          f"lr:{scheduler.current_lr:.6e}")
    if clearml_logger is not None:
        clearml_logger.report_scalar(title="loss", series=name, value=result["loss"], iteration=iteration)
        clearml_logger.report_scalar(title="target_std", series=name, value=result["target_std"], iteration=iteration)


def test_model(iteration, tester, scheduler, clearml_logger=None):
    result = tester.test()
    report(iteration, tester.dataloader, result, scheduler, clearml_logger=clearml_logger)
    return result


def view_step_handler(iteration, model, elapsed_time, iteration_count, trn_tester, tst_tester, checkpoints_directory, scheduler,
                      optimizer=None, clearml_logger=None):
    print(f"Iteration: {iteration}, time: {elapsed_time:.2f} s, speed: {iteration_count / elapsed_time:.2f} it/s.")
    save_model(model, get_checkpoint_path(checkpoints_directory, iteration))
    if trn_tester is not None:
        test_model(iteration, trn_tester, scheduler, clearml_logger=clearml_logger)
    if tst_tester is not None:
        test_model(iteration, tst_tester, scheduler, clearml_logger=clearml_logger)
    if optimizer is not None:  # last: the testers draw masks from the same host RNG stream the trainer continues with
        save_training_state(get_training_state_path(checkpoints_directory, iteration), optimizer, iteration)


def init_training(batch_operator, model, dataset, trn_tester, tst_tester, learning_rate, warmup_iterations, checkpoints_directory,
                  bfloat16=False, clearml_logger=None, weight_decay=0.0, max_grad_norm=None, optimizer="adam", momentum=0.9):
    """masked_pretraining/train.py's init_training over the STUDENT's parameters (model.parameters(): backbone and head; the teacher is
    not a sub-module and has no gradient): "adam" (FusedAdam, or FusedAdamW over decay_groups with weight_decay > 0), "lamb", "lars"."""
    if optimizer == "lamb":
        optimizer = FusedLAMB(layerwise_groups(model, weight_decay), lr=learning_rate, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    elif optimizer == "lars":
        optimizer = FusedLARS(layerwise_groups(model, weight_decay), lr=learning_rate, momentum=momentum, weight_decay=weight_decay,
                              max_grad_norm=max_grad_norm)
    elif optimizer != "adam":
        raise ValueError(f"Unknown optimizer: {optimizer!r} (adam, lamb, lars)")
    elif weight_decay > 0:
        optimizer = FusedAdamW(decay_groups(model, weight_decay), lr=learning_rate, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    else:
        optimizer = FusedAdam(model.parameters(), lr=learning_rate, max_grad_norm=max_grad_norm)
    scheduler = WarmupSchleduler(optimizer, learning_rate, warmup_iterations, 1)
    trainer = Trainer(batch_operator, model, dataset, optimizer, scheduler, bfloat16=bfloat16)
    trainer.on_view_step = partial(view_step_handler, trn_tester=trn_tester, tst_tester=tst_tester, checkpoints_directory=checkpoints_directory,
                                   scheduler=scheduler, optimizer=optimizer, clearml_logger=clearml_logger)
    return trainer


def resume(trainer, checkpoints_directory, start_iteration):
    """Restore what view_step_handler wrote at `start_iteration`: student AND teacher with its update count (model.load reads the
    teacher.* entries), then the optimizer and the RNG streams when the training state file is there.  Returns the iteration to pass to
    Trainer.train(start_iteration=...), as masked_pretraining.train.resume does."""
    trainer.model.load(get_checkpoint_path(checkpoints_directory, start_iteration))
    state_path = get_training_state_path(checkpoints_directory, start_iteration)
    if os.path.exists(state_path):
        load_training_state(state_path, trainer.optimizer)
        return start_iteration + 1
    return start_iteration
