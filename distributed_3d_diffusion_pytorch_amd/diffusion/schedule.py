"""Continuous-time DDPM math (cosine logSNR schedule, forward noising,
ancestral CFG posterior, the few-step DDIM / DPM-Solver++(2M) updates).

Parity targets (all device-agnostic here; the reference runs parts of this on
the CPU, D11):
  * logsnr_schedule_cosine  -> `train.py:30-34` (dupes `sampling.py:59-63`)
  * q_sample                -> `train.py:50-60`
  * cfg posterior           -> `train.py:131-166`, `sampling.py:78-112`
  * ancestral step          -> `train.py:118-128`, `sampling.py:115-127`
The on-device fused forms are ``ops.diffusion_inputs`` (t, lambda, eps, q_sample and CFG drop in
one launch) and the sampler kernels driven by ``engine.sampler`` (CFG combine, x0 clamp,
posterior and noise in one launch per step).
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch


def _ab(logsnr_min: float, logsnr_max: float) -> Tuple[float, float]:
    b = math.atan(math.exp(-0.5 * logsnr_max))
    a = math.atan(math.exp(-0.5 * logsnr_min)) - b
    return a, b


def logsnr_schedule_cosine(t: torch.Tensor, *, logsnr_min: float = -20.0,
                           logsnr_max: float = 20.0) -> torch.Tensor:
    """lambda(t) = -2 log tan(a t + b);  lambda(0)=+20, lambda(1)~-20."""
    a, b = _ab(logsnr_min, logsnr_max)
    return -2.0 * torch.log(torch.tan(a * t + b))


def alpha_sigma(logsnr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """alpha = sqrt(sigmoid(l)), sigma = sqrt(sigmoid(-l))."""
    return torch.sigmoid(logsnr).sqrt(), torch.sigmoid(-logsnr).sqrt()


def q_sample(z: torch.Tensor, logsnr: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    """z_t = alpha(l) z + sigma(l) eps with per-example logsnr [B]."""
    alpha, sigma = alpha_sigma(logsnr)
    shape = (-1,) + (1,) * (z.dim() - 1)
    return alpha.view(shape) * z + sigma.view(shape) * noise


PREDICTIONS = ("eps", "v")
LOSS_WEIGHTS = ("none", "min_snr")


def check_prediction(prediction: str) -> str:
    if prediction not in PREDICTIONS:
        raise ValueError(f"prediction {prediction!r}: expected one of {PREDICTIONS}")
    return prediction


def check_loss_weight(loss_weight: str) -> str:
    if loss_weight not in LOSS_WEIGHTS:
        raise ValueError(f"loss_weight {loss_weight!r}: expected one of {LOSS_WEIGHTS}")
    return loss_weight


def v_target(z: torch.Tensor, logsnr: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    """v = alpha(l) eps - sigma(l) z for clean ``z`` and per-example logsnr [B]
    (Salimans & Ho 2022); with z_t = q_sample: eps = sigma z_t + alpha v and
    z = alpha z_t - sigma v."""
    alpha, sigma = alpha_sigma(logsnr)
    shape = (-1,) + (1,) * (z.dim() - 1)
    return alpha.view(shape) * noise - sigma.view(shape) * z


def min_snr_weight(logsnr: torch.Tensor, prediction: str = "eps", gamma: float = 5.0) -> torch.Tensor:
    """min-SNR-gamma loss weight (Hang et al. 2023) per example: min(SNR, gamma)
    divided by the factor that turns the x0 loss into the eps or v loss, in
    forms that neither overflow nor cancel:
        eps:  min(1, gamma e^-lambda)          v:  min(sigmoid(lambda), gamma sigmoid(-lambda))"""
    check_prediction(prediction)
    if prediction == "eps":
        return torch.clamp(gamma * torch.exp(-logsnr), max=1.0)
    return torch.minimum(torch.sigmoid(logsnr), gamma * torch.sigmoid(-logsnr))


def diffusion_loss(eps: torch.Tensor, eps_hat: torch.Tensor, loss_type: str = "l2", *,
                   logsnr: Optional[torch.Tensor] = None, prediction: str = "eps", loss_weight: str = "none",
                   gamma: float = 5.0) -> torch.Tensor:
    """mean_b[ w(lambda_b) mean_{c,p} l(eps_hat - eps) ] with ``eps`` the
    target the model was asked for (eps or v) and ``logsnr`` [B] the examples'
    lambda; ``loss_weight="none"`` is w = 1 (the plain mean).  The weights are
    not normalised by their sum: micro-batches reproduce the full batch."""
    check_prediction(prediction)
    check_loss_weight(loss_weight)
    eps_hat = eps_hat.float()
    eps = eps.float()
    if loss_weight == "none":
        if loss_type == "l2":
            return torch.mean((eps - eps_hat) ** 2)
        if loss_type == "l1":
            return torch.mean((eps - eps_hat).abs())
        if loss_type == "huber":
            return torch.nn.functional.smooth_l1_loss(eps_hat, eps)
        raise NotImplementedError(loss_type)
    if logsnr is None:
        raise ValueError(f"loss_weight={loss_weight!r} needs the batch's logsnr")
    if loss_type == "l2":
        el = (eps - eps_hat) ** 2
    elif loss_type == "l1":
        el = (eps - eps_hat).abs()
    elif loss_type == "huber":
        el = torch.nn.functional.smooth_l1_loss(eps_hat, eps, reduction="none")
    else:
        raise NotImplementedError(loss_type)
    wgt = min_snr_weight(logsnr.reshape(-1).float(), prediction, gamma)
    return torch.mean(wgt.view((-1,) + (1,) * (el.dim() - 1)) * el)


def loss_bins_report(table, logsnr_min: float = -20.0, logsnr_max: float = 20.0) -> dict:
    """The noise-level table of ``ops.loss_bins_add`` ([NB,5]: count, sum of
    the loss, of the weighted loss, of the squared error in eps units and in
    x0 units; bins uniform in t) as a JSON-ready dict: ``t_edges`` and
    ``logsnr_edges`` (NB + 1 values), ``count`` and the per-bin means ``loss``,
    ``weighted``, ``mse_eps``, ``mse_x0`` (None for an empty bin).  Only
    ``mse_eps`` and ``mse_x0`` compare across objectives."""
    rows = table.detach().double().cpu().tolist() if isinstance(table, torch.Tensor) else [list(r) for r in table]
    nb = len(rows)
    a, b = _ab(logsnr_min, logsnr_max)
    t_edges = [j / nb for j in range(nb + 1)]
    out = {"t_edges": t_edges, "logsnr_edges": [-2.0 * math.log(math.tan(a * t + b)) for t in t_edges],
           "count": [int(round(r[0])) for r in rows]}
    for col, name in enumerate(("loss", "weighted", "mse_eps", "mse_x0"), start=1):
        out[name] = [r[col] / r[0] if r[0] > 0 else None for r in rows]
    return out


SPACINGS = ("t", "logsnr")
SOLVERS = ("ancestral", "ddim", "dpmpp2m")


def sampler_logsnrs(timesteps: int, logsnr_min: float = -20.0, logsnr_max: float = 20.0,
                    dtype=torch.float32, spacing: str = "t") -> Tuple[torch.Tensor, torch.Tensor]:
    """(lambda_k, lambda_{k+1}), k=0..T-1.  ``spacing="t"``: t_k = 1 - k/T on
    the cosine schedule (`sampling.py:134-135`); ``"logsnr"``: lambda uniform
    from logsnr_min to logsnr_max (equal solver step sizes h)."""
    if spacing == "t":
        ts = torch.linspace(1.0, 0.0, timesteps + 1, dtype=dtype)
        lam = logsnr_schedule_cosine(ts, logsnr_min=logsnr_min, logsnr_max=logsnr_max)
    elif spacing == "logsnr":
        lam = torch.linspace(logsnr_min, logsnr_max, timesteps + 1, dtype=dtype)
    else:
        raise ValueError(f"spacing {spacing!r}: expected one of {SPACINGS}")
    return lam[:-1], lam[1:]


def _x0(z, out, alpha, sigma, prediction: str):
    """Clamped data prediction from the guided model output."""
    if prediction == "eps":
        return ((z - sigma * out) / alpha).clamp(-1.0, 1.0)
    return (alpha * z - sigma * out).clamp(-1.0, 1.0)


def cfg_posterior(z: torch.Tensor, eps_cond: torch.Tensor, eps_uncond: torch.Tensor,
                  w: torch.Tensor, logsnr: torch.Tensor, logsnr_next: torch.Tensor, prediction: str = "eps"
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Classifier-free-guided DDPM posterior mean / variance (reference math,
    `train.py:140-166`).  ``w`` is per-example [b]; logsnr scalars.  With
    ``prediction="v"`` the two model outputs are v and the guided one gives
    x0 = clamp(alpha z - sigma v, -1, 1); everything after x0 is the same."""
    check_prediction(prediction)
    shape = (-1,) + (1,) * (z.dim() - 1)
    w = w.to(z.dtype).view(shape)
    logsnr = torch.as_tensor(logsnr, dtype=z.dtype, device=z.device)
    logsnr_next = torch.as_tensor(logsnr_next, dtype=z.dtype, device=z.device)
    c = -torch.expm1(logsnr - logsnr_next)
    alpha, sigma = alpha_sigma(logsnr)
    alpha_next = torch.sigmoid(logsnr_next).sqrt()
    eps = (1.0 + w) * eps_cond - w * eps_uncond
    x0 = _x0(z, eps, alpha, sigma, prediction)
    mean = alpha_next * (z * (1.0 - c) / alpha + c * x0)
    var = torch.sigmoid(-logsnr_next) * c
    return mean, var


# ------------------------------------------------------- few-step solvers
# One step lambda -> lambda' of every solver is the linear update
#     z' = kz z + k0 x0 + k1 x0_prev + kn N(0,1),
# x0 = clamp((z - sigma eps)/alpha, -1, 1) the guided data prediction (v-prediction:
# clamp(alpha z - sigma v, -1, 1)) and x0_prev the previous step's.  With h = (lambda' - lambda)/2 and
# c = -expm1(lambda - lambda'):
#   ddim (eta in [0,1]):  s = eta sigma' sqrt(c) (0 on the last step),
#       g = sqrt(sigma'^2 - s^2)/sigma;  kz = g, k0 = alpha' - g alpha, kn = s
#       (eta = 1 is the ancestral posterior, eta = 0 the probability-flow step)
#   dpmpp2m (DPM-Solver++ 2M, data prediction):  q = -alpha' expm1(-h),
#       kz = sigma'/sigma;  first and LAST step first order (k0 = q), else with
#       r = h_prev/h:  k0 = q (1 + 1/(2r)), k1 = -q/(2r)
# The last step of the cosine schedule is a big logSNR jump: extrapolating x0
# over it costs more than the second order gains, hence the first-order final
# step (the "lower_order_final" rule of the DPM-Solver authors).
def _sig(x: float) -> float:
    return 1.0 / (1.0 + math.exp(-x)) if x >= 0 else math.exp(x) / (1.0 + math.exp(x))


def solver_row(lam: Sequence[float], lam_next: Sequence[float], k: int, solver: str = "ddim", eta: float = 0.0,
               lam0: float = 20.0, first_order: bool = False) -> List[float]:
    """The 8 per-step scalars ``[lambda, alpha, sigma, kz, k0, k1, kn,
    lambda0]`` of step ``k`` of the schedule ``(lam, lam_next)`` (lists of
    ``sampler_logsnrs``), computed in fp64; slots 0 and 7 are what the CFG
    input assembly reads.  ``first_order``: the dpmpp2m step without history
    (what a step takes when no previous x0 is at hand)."""
    if solver not in ("ddim", "dpmpp2m"):
        raise ValueError(f"solver {solver!r}: expected 'ddim' or 'dpmpp2m'")
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"eta {eta}: expected a value in [0, 1]")
    if solver == "dpmpp2m" and eta != 0.0:
        raise ValueError("dpmpp2m is deterministic: eta must be 0")
    T = len(lam)
    l, ln = float(lam[k]), float(lam_next[k])
    alpha, sigma = math.sqrt(_sig(l)), math.sqrt(_sig(-l))
    alpha_n, sigma_n = math.sqrt(_sig(ln)), math.sqrt(_sig(-ln))
    h = 0.5 * (ln - l)
    k1 = kn = 0.0
    if solver == "ddim":
        e = eta if k < T - 1 else 0.0
        c = -math.expm1(l - ln)
        # sigma'^2 - s^2 = sigma'^2 m with m = 1 - eta^2 c = (1 - eta^2) + eta^2 exp(lambda - lambda'):
        # no cancellation; alpha' - g alpha = -alpha' expm1(-h + log(m)/2) likewise
        m = (1.0 - e * e) + e * e * math.exp(l - ln)
        kn = e * sigma_n * math.sqrt(c)
        kz = sigma_n * math.sqrt(m) / sigma
        k0 = -alpha_n * math.expm1(-h + 0.5 * math.log(m)) if m > 0.0 else alpha_n
    else:
        q = -alpha_n * math.expm1(-h)
        kz = sigma_n / sigma
        k0 = q
        if not first_order and 0 < k < T - 1:
            r = 0.5 * (l - float(lam[k - 1])) / h
            k0, k1 = q * (1.0 + 0.5 / r), -0.5 * q / r
    return [l, alpha, sigma, kz, k0, k1, kn, float(lam0)]


def solver_step(z: torch.Tensor, eps_cond: torch.Tensor, eps_uncond: torch.Tensor, w: torch.Tensor,
                x0_prev: Optional[torch.Tensor], row, noise: Optional[torch.Tensor], prediction: str = "eps"
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One solver step in the dtype of ``z``: ``(z', x0)`` from a
    ``solver_row`` (8 floats or a tensor of them).  ``x0_prev`` is read only
    when the row's k1 != 0, ``noise`` only when kn != 0 (either may be None
    otherwise); the returned clamped x0 is the next step's ``x0_prev``.
    ``prediction="v"``: the model outputs are v (see :func:`cfg_posterior`)."""
    check_prediction(prediction)
    _, alpha, sigma, kz, k0, k1, kn = (float(v) for v in row[:7])
    shape = (-1,) + (1,) * (z.dim() - 1)
    w = w.to(z.dtype).view(shape)
    eps = (1.0 + w) * eps_cond - w * eps_uncond
    x0 = _x0(z, eps, alpha, sigma, prediction)
    out = kz * z + k0 * x0
    if k1 != 0.0:
        out = out + k1 * x0_prev.to(z.dtype)
    if kn != 0.0:
        out = out + kn * noise.to(z.dtype)
    return out, x0
