"""Test-local float64 oracle of ``ops.image_metrics`` (shared by the CPU and
GPU metric / evaluation tests).  Written from the definition -- Wang et al.
2004 SSIM with a dense 11 x 11 Gaussian window (sigma 1.5) over the valid
region, L = 1 -- and independent of ``ops.torch_impl``."""
import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def map01(x: torch.Tensor, quantize: bool) -> torch.Tensor:
    """fp32 [-1, 1] -> float64 [0, 1]; quantize: the numpy expression of
    ``sampling.py:save_png`` (float32 arithmetic, ``astype(uint8)``)."""
    a = x.detach().cpu().float().numpy()
    if quantize:
        q = ((np.clip(a, -1, 1) + 1) * 127.5).astype(np.uint8)
        return torch.from_numpy(q.astype(np.float64) / 255.0)
    return torch.from_numpy((np.clip(a, -1, 1).astype(np.float64) + 1.0) / 2.0)


def metrics01(x: torch.Tensor, y: torch.Tensor):
    """(mse [N], ssim [N]) float64 of two float64 [N,C,H,W] batches in [0, 1]."""
    N, C, H, W = x.shape
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-k * k / (2 * 1.5 ** 2))
    g = g / g.sum()
    win = torch.outer(g, g).view(1, 1, 11, 11)

    def mean(v):
        return F.conv2d(v.reshape(N * C, 1, H, W), win)

    mx, my = mean(x), mean(y)
    vx, vy, cxy = mean(x * x) - mx * mx, mean(y * y) - my * my, mean(x * y) - mx * my
    s = (2 * mx * my + C1) * (2 * cxy + C2) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return (x - y).square().reshape(N, -1).mean(1), s.reshape(N, -1).mean(1)


def oracle(pred: torch.Tensor, target: torch.Tensor, quantize: bool):
    return metrics01(map01(pred, quantize), map01(target, quantize))


def cases(N: int, H: int, W: int, seed: int = 0):
    """name -> (pred, target) fp32 [N,3,H,W] CPU pairs: the image kinds the
    metric has to get right (textured, nearly equal, smooth, flat, SRN-like)."""
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    rnd = lambda: torch.rand(N, 3, H, W, generator=g) * 2 - 1  # noqa: E731
    nz = lambda s: torch.randn(N, 3, H, W, generator=g) * s  # noqa: E731
    out = {}
    out["noise"] = (rnd(), rnd())
    a = rnd()
    out["noisy_copy"] = (a, a + nz(0.05))
    ramp = (torch.linspace(-0.9, 0.9, W).view(1, 1, 1, W) * torch.linspace(0.5, 1.0, H).view(1, 1, H, 1)) \
        .expand(N, 3, H, W).contiguous()
    out["noisy_ramp"] = (ramp, ramp + nz(0.01))
    out["flat"] = (torch.ones(N, 3, H, W), torch.full((N, 3, H, W), 2 * 254 / 255 - 1))
    # SRN-like: a shaded blob on a 1.0 (white) background, and its noisy copy (noise exceeds 1.0 on the
    # background, where the clamp removes it again)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    blob = ((xx / 0.6) ** 2 + (yy / 0.35) ** 2 < 1).float().view(1, 1, H, W)
    shade = torch.stack([0.2 + 0.3 * xx, -0.4 + 0.2 * yy, 0.1 * xx * yy], 0).view(1, 3, H, W)
    srn = (blob * shade + (1 - blob)).expand(N, 3, H, W).contiguous()
    out["srn_like"] = (srn, srn + nz(0.03))
    return out
