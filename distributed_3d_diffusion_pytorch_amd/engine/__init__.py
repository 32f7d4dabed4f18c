from .optim import FusedAdam, ema_decay_for, warmup_lr
from .trainer import Trainer
from .sampler import DiffusionSampler, RecordEntry, SolverState, shard_range
from .evaluate import (EvalObject, evaluate_objects, gt_ceiling, heldout_loss, load_objects, summarize,
                       summarize_consistency, summarize_ensemble)

__all__ = ["FusedAdam", "ema_decay_for", "warmup_lr", "Trainer", "DiffusionSampler", "RecordEntry", "SolverState",
           "shard_range", "EvalObject", "evaluate_objects", "heldout_loss", "load_objects", "summarize",
           "summarize_consistency", "summarize_ensemble", "gt_ceiling"]
