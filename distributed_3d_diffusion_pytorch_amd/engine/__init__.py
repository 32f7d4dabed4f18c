from .optim import FusedAdam, ema_decay_for, warmup_lr
from .trainer import Trainer
from .sampler import DiffusionSampler, RecordEntry, SolverState, shard_range
from .evaluate import (EvalObject, evaluate_objects, gt_ceiling, heldout_loss, knn_block, load_objects,
                       nearest_train, summarize, summarize_consistency, summarize_ensemble)
from .field import field_consistency, field_rows, fit_field, fit_fields, summarize_field

__all__ = ["FusedAdam", "ema_decay_for", "warmup_lr", "Trainer", "DiffusionSampler", "RecordEntry", "SolverState",
           "shard_range", "EvalObject", "evaluate_objects", "heldout_loss", "load_objects", "summarize",
           "summarize_consistency", "summarize_ensemble", "gt_ceiling", "fit_field", "fit_fields", "field_consistency",
           "field_rows", "summarize_field", "knn_block", "nearest_train"]
