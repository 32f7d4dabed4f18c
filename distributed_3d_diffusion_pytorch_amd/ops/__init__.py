"""NHWC op set of the X-UNet, dispatched to hand-written HIP kernels (gfx950)
or to the PyTorch reference composition.

Every function here has identical semantics in both backends; the torch
versions (``torch_impl``) are the numerics oracle used by the tests.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import torch_impl as _t
from ._backend import use_hip, set_backend, load_library, library_error, lib_path

_hip = None


def _h():
    global _hip
    if _hip is None:
        from . import hip_impl
        _hip = hip_impl
    return _hip


def group_norm(x, weight, bias, groups: int = 32, eps: float = 1e-5, silu: bool = False, res_slot=None):
    if use_hip(x):
        return _h().group_norm(x, weight, bias, groups, eps, silu, res_slot)
    return _t.group_norm(x, weight, bias, groups, eps, silu)


def gn_film(x, weight, bias, ss, groups: int = 32, eps: float = 1e-5, dropout_p: float = 0.0,
            training: bool = False, seed: int = 0, ss_map: Optional[torch.Tensor] = None):
    """ss_map (int32 [N], inference): image n is modulated by ss[ss_map[n]]
    (shared conditioning, XUNet.forward(shared_cond=))."""
    if use_hip(x):
        return _h().gn_film(x, weight, bias, ss, groups, eps, dropout_p, training, seed, ss_map)
    return _t.gn_film(x, weight, bias, ss, groups, eps, dropout_p, training, seed, ss_map)


def conv3x3(x, weight, bias, stride: int = 1, residual: Optional[torch.Tensor] = None,
            out_scale: float = 1.0, row_bias: Optional[torch.Tensor] = None, res_period: int = 0,
            gn_groups: int = 0, res_slot=None, keep_pad: bool = False):
    """gn_groups: the output feeds a GroupNorm with that many groups (the HIP
    path then fuses that GroupNorm's statistics into the conv epilogue).
    res_slot / in_slot (HIP path; :class:`ResGradSlot`): hand the residual's /
    the input's gradient to the GroupNorm that reads the same tensor.
    keep_pad: (IC or OC not a multiple of 8, i.e. stem / head) the HIP path
    returns the channel-padded output (the fused loss reads it in place).
    Inputs may carry zero channels beyond the weight's IC (pre-padded stem
    input)."""
    if use_hip(x):
        return _h().conv3x3(x, weight, bias, stride, residual, out_scale, row_bias, res_period, gn_groups, res_slot,
                            keep_pad)
    if x.shape[-1] > weight.shape[1]:
        x = x[..., :weight.shape[1]]
    return _t.conv3x3(x, weight, bias, stride, residual, out_scale, row_bias, res_period)


def linear(x, weight, bias, residual: Optional[torch.Tensor] = None, out_scale: float = 1.0, res_slot=None,
           in_slot=None, gn_groups: int = 0):
    """gn_groups: the output feeds a GroupNorm with that many groups (the HIP
    epilogue then also emits its partial statistics)."""
    if use_hip(x):
        return _h().linear(x, weight, bias, residual, out_scale, res_slot, in_slot, gn_groups)
    return _t.linear(x, weight, bias, residual, out_scale)


def attn_out(a, W_out, b_out, W_lin, b_lin, residual: Optional[torch.Tensor] = None, out_scale: float = 1.0,
             res_slot=None, gn_groups: int = 0):
    """The attention block's output map ``linear(out_proj(a))`` + residual,
    x out_scale (`xunet.py:175,217-220`).  HIP: one merged GEMM forward and
    backward (hip_impl.attn_out); torch: the two layers as written."""
    if use_hip(a):
        return _h().attn_out(a, W_out, b_out, W_lin, b_lin, residual, out_scale, res_slot, gn_groups)
    return _t.linear(_t.linear(a, W_out, b_out), W_lin, b_lin, residual, out_scale)


def carry_gn_stats(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """A reshaped view keeps the fused GroupNorm statistics of its source."""
    part = getattr(src, "_d3d_gnpart", None)
    if part is not None:
        dst._d3d_gnpart = part
    return dst


def cond_conv(rays_dir, orig_pe, weight, bias, stride: int, row_bias=None, residual=None, res_period: int = 0,
              silu_out: bool = False):
    """``silu_out``: (HIP) the output also carries silu(output) for the FiLM
    projections (film_batch then skips its SiLU pass); ignored by the torch
    composition, which film_batch handles itself."""
    if use_hip(rays_dir):
        return _h().cond_conv(rays_dir, orig_pe, weight, bias, stride, row_bias, residual, res_period,
                              silu_out=silu_out)
    return _t.cond_conv(rays_dir, orig_pe, weight, bias, stride, row_bias, residual, res_period)


def ray_posenc_dir(R, t, K, H: int, W: int, cond_mask, rescale_from: int = 0, out_dtype=None):
    if out_dtype == torch.bfloat16 and R.is_cuda and use_hip(R, any_dtype=True):
        return _h().ray_posenc_dir(R, t, K, H, W, cond_mask, rescale_from)
    y = _t.ray_posenc_dir(R, t, K, H, W, cond_mask, rescale_from)
    return y.to(out_dtype) if out_dtype is not None else y


def ray_conditioning(R, t, K, H: int, W: int, cond_mask, rescale_from: int = 0, out_dtype=None):
    """(masked ray-direction image [2B,H,W,>=51], masked origin posenc [2B,93]
    fp32) -- :func:`ray_posenc_dir` and :func:`ray_origin_pe` together; two
    HIP launches for bf16 GPU runs."""
    if out_dtype == torch.bfloat16 and R.is_cuda and use_hip(R, any_dtype=True):
        return _h().ray_conditioning(R, t, K, H, W, cond_mask, rescale_from)
    return ray_posenc_dir(R, t, K, H, W, cond_mask, rescale_from, out_dtype), ray_origin_pe(t, cond_mask)


def ray_origin_pe(t, cond_mask):
    return _t.ray_origin_pe(t, cond_mask)


def cat_gn_silu_dense(a, b, gw, gb, dw, db, groups: int = 32, eps: float = 1e-5):
    if use_hip(a):
        return _h().cat_gn_silu_dense(a, b, gw, gb, dw, db, groups, eps)
    return _t.cat_gn_silu_dense(a, b, gw, gb, dw, db, groups, eps)


def film_batch(emb, weights, biases, block_events: bool = False, split: int = 0):
    """``dense_i(silu(emb))`` for every FiLM projection of one level
    (``block_events``, HIP path: one GEMM and ready event per block;
    ``split``: blocks ``[split:]`` get their own, earlier weight-gradient job)."""
    if use_hip(emb):
        return _h().film_batch(emb, weights, biases, block_events, split)
    return _t.film_batch(emb, weights, biases)


def attention(qkv, heads: int, cross: bool):
    if use_hip(qkv):
        return _h().attention(qkv, heads, cross)
    return _t.attention(qkv, heads, cross)


def diffusion_inputs(img, seed: int, e0: int = 0, cond_prob: float = 0.1, logsnr_min: float = -20.0,
                     logsnr_max: float = 20.0, dtype=torch.float32, prediction: str = "eps"):
    """Counter-based training-input draw (see torch_impl.diffusion_inputs);
    one HIP launch for bf16 GPU runs.  Slot 1 of the result is the loss target
    of ``prediction`` (eps, or v = alpha eps - sigma z_clean)."""
    if dtype == torch.bfloat16 and img.is_cuda and use_hip(img, any_dtype=True):
        return _h().diffusion_inputs(img, seed, e0, cond_prob, logsnr_min, logsnr_max, dtype, prediction=prediction)
    return _t.diffusion_inputs(img, seed, e0, cond_prob, logsnr_min, logsnr_max, dtype, prediction=prediction)


def diff_loss_nhwc(y, target, loss_type: str = "l2", *, logsnr=None, prediction: str = "eps",
                   loss_weight: str = "none", gamma: float = 5.0):
    """mean_b[ w(lambda_b) mean_{c,p} l(y - target) ] on the NHWC head output;
    ``logsnr`` is the [B,2] tensor of :func:`diffusion_inputs` (column 1 is
    read), required unless ``loss_weight="none"`` (see torch_impl.diff_loss_nhwc)."""
    kw = dict(logsnr=logsnr, prediction=prediction, loss_weight=loss_weight, gamma=gamma)
    if use_hip(y):
        return _h().diff_loss_nhwc(y, target, loss_type, **kw)
    return _t.diff_loss_nhwc(y, target, loss_type, **kw)


def diff_loss_rows(y, target, loss_type: str = "l2"):
    """Per-example loss rows [B,2] fp32 (no autograd): column 0 the example's
    mean of l(y - target), column 1 its mean of (y - target)^2, over the 3 H W
    valid elements of the NHWC head output."""
    if use_hip(y):
        return _h().diff_loss_rows(y, target, loss_type)
    return _t.diff_loss_rows(y, target, loss_type)


def loss_bins_add(table, rows, logsnr, *, prediction: str = "eps", loss_weight: str = "none", gamma: float = 5.0,
                  logsnr_min: float = -20.0, logsnr_max: float = 20.0):
    """Adds a batch to the noise-level table, in place: ``table`` fp64 [NB,5],
    bins uniform in t, columns (count, sum row0, sum w row0, sum f_eps row1,
    sum f_x row1) with ``rows`` of :func:`diff_loss_rows` and ``logsnr`` the
    [B,2] tensor of :func:`diffusion_inputs` (see torch_impl.loss_bins_add)."""
    kw = dict(prediction=prediction, loss_weight=loss_weight, gamma=gamma, logsnr_min=logsnr_min,
              logsnr_max=logsnr_max)
    if table.is_cuda and use_hip(table, any_dtype=True):
        return _h().loss_bins_add(table, rows.float().contiguous(), logsnr.float().contiguous(), **kw)
    return _t.loss_bins_add(table, rows, logsnr, **kw)


def avgpool2(x):
    if use_hip(x):
        return _h().avgpool2(x)
    return _t.avgpool2(x)


def upsample2(x):
    if use_hip(x):
        return _h().upsample2(x)
    return _t.upsample2(x)


def logsnr_mlp(logsnr, w1, b1, w2, b2, max_time: float = 1.0, dtype=None):
    """posenc_ddpm(clamp(logsnr)) -> Linear -> SiLU -> Linear, [B, 2] -> [2B, E]
    fp32.  HIP (``csrc/mlp.hip``) for bf16 GPU runs (``dtype``: the model's
    activation dtype)."""
    if dtype == torch.bfloat16 and logsnr.is_cuda and use_hip(logsnr, any_dtype=True):
        return _h().logsnr_mlp(logsnr, w1, b1, w2, b2, max_time)
    return _t.logsnr_mlp(logsnr, w1, b1, w2, b2, max_time)


def silu(x):
    if use_hip(x):
        return _h().silu(x)
    return _t.silu(x)


def ray_posenc(R, t, K, H: int, W: int, cond_mask, pos_emb, first_emb, other_emb,
               rescale_from: int = 0, out_dtype: torch.dtype = torch.float32):
    if out_dtype == torch.bfloat16 and use_hip(R, any_dtype=True):
        return _h().ray_posenc(R, t, K, H, W, cond_mask, pos_emb, first_emb, other_emb,
                               rescale_from, out_dtype)
    return _t.ray_posenc(R, t, K, H, W, cond_mask, pos_emb, first_emb, other_emb,
                         rescale_from).to(out_dtype)


def image_metrics(pred, target, quantize: bool = True):
    """Per-image ``(mse [N], ssim [N])`` (fp32) of two ``[N, C, H, W]`` batches
    in [-1, 1], scored on the [0, 1] scale.  ``quantize``: both images first
    go through the uint8 value ``sampling.py:save_png`` writes, so the result
    equals the metrics of the written PNGs.  SSIM is Wang et al. 2004 (11-tap
    Gaussian, sigma 1.5, valid region, L = 1, per channel).  HIP
    (``csrc/metrics.hip``) on the GPU, the float64 torch composition on the CPU."""
    if pred.dim() != 4 or pred.shape != target.shape:
        raise ValueError(f"image_metrics takes two [N,C,H,W] batches of one shape, got {tuple(pred.shape)} and "
                         f"{tuple(target.shape)}")
    if pred.shape[-2] < 11 or pred.shape[-1] < 11:
        raise ValueError(f"image_metrics needs H, W >= 11 (one SSIM window), got {tuple(pred.shape[-2:])}")
    if pred.is_cuda and pred.shape[0] > 0 and use_hip(pred, any_dtype=True):
        return _h().image_metrics(pred, target, quantize)
    return _t.image_metrics(pred, target, quantize)


def scene_render(table, R, t, K, H: int, W: int, *, aa: int = 3, return_aux: bool = False):
    """Ray-cast images ``[N,3,H,W]`` fp32 in [-1, 1] of procedural scenes
    (``data.procedural``): ``table`` fp64 [N,6,16] (per primitive slot the
    world-to-unit map A [9], centre [3], albedo [3], kind 0 empty / 1 ellipsoid
    / 2 box), cameras ``R`` [N,3,3] cam-to-world, ``t`` [N,3] and ``K`` [N,3,3]
    fp64, ``K`` the intrinsics of the 128 x 128 image (the op rescales it to
    ``H`` x ``W`` as ``camera_rays(..., rescale_from=128)`` does).  A pixel is
    the mean of ``aa`` x ``aa`` sub-pixel rays (1..4); the background is white.
    ``return_aux``: also ``depth`` [N,H,W] fp32 (+inf on a miss) and ``prim``
    [N,H,W] int32 (-1 on a miss) of the pixel-centre ray.  HIP
    (``csrc/scene.hip``) on the GPU, the float64 torch form on the CPU."""
    _t.scene_render_check(table, R, t, K, H, W, aa)
    if table.is_cuda and table.shape[0] > 0 and use_hip(table, any_dtype=True):
        return _h().scene_render(table, R, t, K, H, W, aa=aa, return_aux=return_aux)
    return _t.scene_render(table, R, t, K, H, W, aa=aa, return_aux=return_aux)


def view_consistency(table, K, R_src, t_src, img_src, R_tgt, t_tgt, img_tgt, ref=None, *,
                     return_class: bool = False):
    """Geometry-aware scores of N (source view, target view) pairs of
    procedural scenes: ``table`` [N,6,16], ``K`` [N,3,3] (the 128 x 128
    intrinsics, rescaled to the image size as in ``scene_render``), cameras
    ``R_*`` [N,3,3] cam-to-world and ``t_*`` [N,3], all fp64; ``img_src``,
    ``img_tgt`` and optionally ``ref`` (the target view's ground truth)
    ``[N,3,H,W]`` fp32 in [-1, 1], contiguous.  Every target pixel is
    classified with the scene's true geometry as background (0), disoccluded
    (1: a surface the source camera does not see), co-visible (2) or clean (3:
    co-visible with the pixel and its bilinear footprint in the source image
    on one smooth piece of surface).  Returns ``stats`` [N,8] fp64: the pixel
    counts of classes 0, 1, 2 (3 counted in 2), the count of clean pixels, the
    sums of ``((img_tgt - ref) / 2)^2`` over each class's pixels and channels
    (0 without ``ref``) and the sum of ``((img_tgt - warp) / 2)^2`` over the
    clean pixels, ``warp`` the source image interpolated at the pixel's
    reprojection; ``mse = sum / (3 count)``.  ``return_class``: also the class
    plane ``[N,H,W]`` int32.  HIP (``csrc/consistency.hip``, which states the
    rule) on the GPU, the float64 torch form on the CPU."""
    N, H, W = _t.view_consistency_check(table, K, R_src, t_src, img_src, R_tgt, t_tgt, img_tgt, ref)
    if N == 0:
        stats = torch.zeros(0, _t.VC_STATS, dtype=torch.float64, device=table.device)
        return (stats, torch.zeros(0, H, W, dtype=torch.int32, device=table.device)) if return_class else stats
    impl = _h() if table.is_cuda and use_hip(table, any_dtype=True) else _t
    return impl.view_consistency(table, K, R_src, t_src, img_src, R_tgt, t_tgt, img_tgt, ref, return_class=return_class)


def ensemble_stats(samples, target, klass=None, *, quantize: bool = True, return_maps: bool = False):
    """Bias, spread and per-sample error of ``samples`` fp32 ``[G,C,3,H,W]`` --
    C samples of each of G target views -- against ``target`` fp32
    ``[G,3,H,W]``, both in [-1, 1] and contiguous, per visibility class
    ``klass`` int32 ``[G,H,W]`` (the class plane of ``view_consistency``: 0
    background, 1 disoccluded, 2 co-visible, 3 clean; ``None``: every pixel is
    class 0; a pixel whose class is outside 0..3 enters no row).  Both images
    are scored on the [0, 1] scale (``quantize``: through the uint8 value
    ``save_png`` writes, as in ``image_metrics``).  Per pixel, with ``m`` the
    mean of the C samples: ``B`` = sum over the channels of ``(m - y)^2``,
    ``V`` = of the population variance of the samples around ``m``, ``E`` = of
    the mean of ``(x_c - y)^2``; ``E = B + V`` up to rounding.  Returns
    ``stats`` [G,4,4] fp64, row k = ``[n_k, sum B, sum V, sum E]`` over the
    pixels of class k (``mse = sum / (3 n)``).  ``return_maps``: also ``mean``
    [G,3,H,W] fp32 in [-1, 1] (``2 m - 1``) and ``std`` [G,H,W] fp32 on the
    [0, 1] scale (``sqrt(V / 3)``).  HIP (``csrc/ensemble.hip``, which states
    the rule) on the GPU, the float64 torch form on the CPU."""
    G, C, H, W = _t.ensemble_stats_check(samples, target, klass)
    if G == 0:
        dev = samples.device
        stats = torch.zeros(0, _t.ES_CLASSES, _t.ES_COLS, dtype=torch.float64, device=dev)
        return (stats, torch.zeros(0, 3, H, W, dtype=torch.float32, device=dev),
                torch.zeros(0, H, W, dtype=torch.float32, device=dev)) if return_maps else stats
    impl = _h() if samples.is_cuda and use_hip(samples, any_dtype=True) else _t
    return impl.ensemble_stats(samples, target, klass, quantize=quantize, return_maps=return_maps)


def psnr(mse):
    """``10 log10(1 / mse)`` on the [0, 1] scale; ``+inf`` where ``mse == 0``."""
    return -10.0 * torch.log10(torch.as_tensor(mse, dtype=torch.float32))


posenc_ddpm = _t.posenc_ddpm
camera_rays = _t.camera_rays
posenc_nerf = _t.posenc_nerf

__all__ = ["diffusion_inputs", "diff_loss_nhwc", "diff_loss_rows", "loss_bins_add", "group_norm", "gn_film", "conv3x3", "linear", "film_batch", "cat_gn_silu_dense", "cond_conv", "ray_posenc_dir",
           "ray_origin_pe", "ray_conditioning", "attention", "avgpool2", "upsample2",
           "silu", "logsnr_mlp", "ray_posenc", "image_metrics", "scene_render", "view_consistency", "ensemble_stats", "psnr", "posenc_ddpm", "camera_rays", "posenc_nerf", "set_backend",
           "use_hip", "load_library", "library_error", "lib_path"]


def gn_silu_conv3x3(x, gw, gb, cw, cb, groups: int = 32, eps: float = 1e-5, gn1_groups: int = 0, res_slot=None):
    """``conv3x3(silu(group_norm(x)))``: HIP path with the GroupNorm + SiLU in
    the conv's input staging when the shape allows it (``None`` otherwise:
    the caller runs the two ops)."""
    if use_hip(x) and _h().gn_silu_conv_ok(x, cw.shape[0], groups):
        return _h().gn_silu_conv3x3(x, gw, gb, cw, cb, groups, eps, gn1_groups, res_slot)
    return None


def res_slot(x: torch.Tensor):
    """A residual-gradient hand-off slot for x (HIP path), else None."""
    if use_hip(x):
        return _h().ResGradSlot()
    return None
