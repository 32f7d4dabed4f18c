from .schedule import (logsnr_schedule_cosine, alpha_sigma, q_sample, diffusion_loss, v_target, min_snr_weight,
                       check_prediction, check_loss_weight, PREDICTIONS, LOSS_WEIGHTS,
                       loss_bins_report,
                       sampler_logsnrs, cfg_posterior, solver_row, solver_step, SOLVERS, SPACINGS)

__all__ = ["logsnr_schedule_cosine", "alpha_sigma", "q_sample", "diffusion_loss", "v_target", "min_snr_weight",
           "check_prediction", "check_loss_weight", "PREDICTIONS", "LOSS_WEIGHTS",
           "loss_bins_report",
           "sampler_logsnrs", "cfg_posterior", "solver_row", "solver_step", "SOLVERS", "SPACINGS"]
