"""Pure-PyTorch implementations of the NHWC op set.

These are the numerics oracle for the HIP kernels (fp32 composition of the
same op) and the CPU execution path.  Layout convention everywhere in the
framework: activations are ``[N, H, W, C]`` with ``N = 2*B`` and the two views
of an example adjacent (``n = 2*b + frame``), i.e. the reference's
``[B, F=2, C, H, W]`` (`xunet.py:61-71`) folded frame-into-batch, channels-last.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

INV_SQRT2 = 1.0 / math.sqrt(2.0)


def _cast(t: Optional[torch.Tensor], dtype: torch.dtype) -> Optional[torch.Tensor]:
    if t is None:
        return None
    return t if t.dtype == dtype else t.to(dtype)


def group_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, groups: int = 32,
               eps: float = 1e-5, silu: bool = False) -> torch.Tensor:
    """GroupNorm over each (example, frame) image; optional fused SiLU.
    Matches ``nn.GroupNorm(32, C)`` on the frame-folded batch (`xunet.py:61-71`)."""
    N, H, W, C = x.shape
    xf = x.float().reshape(N, H * W, groups, C // groups)
    mean = xf.mean(dim=(1, 3), keepdim=True)
    var = xf.var(dim=(1, 3), unbiased=False, keepdim=True)
    y = (xf - mean) * torch.rsqrt(var + eps)
    y = y.reshape(N, H, W, C) * weight.float() + bias.float()
    if silu:
        y = F.silu(y)
    return y.to(x.dtype)


def dropout_mask(shape, p: float, seed: int, device) -> torch.Tensor:
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
    keep = (torch.rand(shape, generator=g) >= p).to(device)
    return keep


def gn_film(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, ss: torch.Tensor,
            groups: int = 32, eps: float = 1e-5, dropout_p: float = 0.0,
            training: bool = False, seed: int = 0, ss_map: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dropout(GN(x) * (1 + scale) + shift); ``ss = [scale | shift]`` on the
    channel axis (FiLM, `xunet.py:74-87`; ResBlock ordering `xunet.py:140-146`).
    ``ss_map``: image n takes the modulation ss[ss_map[n]]."""
    C = x.shape[-1]
    h = group_norm(x, weight, bias, groups, eps).float()
    if ss_map is not None:
        ss = ss.index_select(0, ss_map.long())
    ssf = ss.float()
    y = h * (1.0 + ssf[..., :C]) + ssf[..., C:]
    if training and dropout_p > 0.0:
        y = F.dropout(y, dropout_p, training=True)
    return y.to(x.dtype)


def conv3x3(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], stride: int = 1,
            residual: Optional[torch.Tensor] = None, out_scale: float = 1.0,
            row_bias: Optional[torch.Tensor] = None, res_period: int = 0) -> torch.Tensor:
    """3x3 conv, padding 1, on NHWC.  Epilogue: + row_bias[n] (per image),
    + residual (broadcast as residual[n % res_period] when res_period > 0),
    * out_scale."""
    dt = x.dtype
    y = F.conv2d(x.permute(0, 3, 1, 2), _cast(weight, dt), _cast(bias, dt), stride=stride, padding=1)
    y = y.permute(0, 2, 3, 1)
    if row_bias is not None:
        y = y + row_bias.to(dt)[:, None, None, :]
    if residual is not None:
        if res_period:
            residual = residual.repeat(y.shape[0] // res_period, 1, 1, 1)
        y = y + residual
    if out_scale != 1.0:
        y = y * out_scale
    return y.contiguous()


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
           residual: Optional[torch.Tensor] = None, out_scale: float = 1.0) -> torch.Tensor:
    """Per-pixel dense layer (1x1 conv / nn.Linear) with fused residual epilogue."""
    dt = x.dtype
    w = weight.reshape(weight.shape[0], -1)
    y = F.linear(x, _cast(w, dt), _cast(bias, dt))
    if residual is not None:
        y = y + residual
    if out_scale != 1.0:
        y = y * out_scale
    return y


def attention(qkv: torch.Tensor, heads: int, cross: bool) -> torch.Tensor:
    """Multi-head attention within an example: queries of frame f attend to
    keys/values of frame f (self) or frame 1-f (cross) (`xunet.py:202-211`).
    ``qkv``: [N, L, 3C] (packed in_proj output).  Returns [N, L, C]."""
    N, L, C3 = qkv.shape
    C = C3 // 3
    d = C // heads
    q, k, v = qkv.split(C, dim=-1)
    if cross:
        perm = torch.arange(N, device=qkv.device) ^ 1
        k = k[perm]
        v = v[perm]
    q = q.reshape(N, L, heads, d).transpose(1, 2)
    k = k.reshape(N, L, heads, d).transpose(1, 2)
    v = v.reshape(N, L, heads, d).transpose(1, 2)
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * (1.0 / math.sqrt(d))
    p = torch.softmax(s, dim=-1)
    o = torch.matmul(p, v.float()).to(qkv.dtype)
    return o.transpose(1, 2).reshape(N, L, C)


def avgpool2(x: torch.Tensor) -> torch.Tensor:
    N, H, W, C = x.shape
    return x.reshape(N, H // 2, 2, W // 2, 2, C).float().mean(dim=(2, 4)).to(x.dtype)


def upsample2(x: torch.Tensor) -> torch.Tensor:
    N, H, W, C = x.shape
    return x[:, :, None, :, None, :].expand(N, H, 2, W, 2, C).reshape(N, 2 * H, 2 * W, C)


def silu(x: torch.Tensor) -> torch.Tensor:
    return F.silu(x)


def camera_rays(R: torch.Tensor, t: torch.Tensor, K: torch.Tensor, H: int, W: int,
                rescale_from: int = 0):
    """Per-pixel world rays of a pinhole camera (OpenCV convention, pixel
    centres at +0.5), following visu3d's ``Camera.rays()`` as used in
    `xunet.py:311-314`: ``pos = t``, ``dir = R @ normalize(K^-1 [u+.5, v+.5, 1])``.

    R: [B,F,3,3] cam-to-world rotation, t: [B,F,3], K: [B,3,3].
    Returns pos, dir: [B,F,H,W,3] in fp32 (computed in fp64).
    """
    dt = torch.float64
    Rd, td, Kd = R.to(dt), t.to(dt), K.to(dt)
    if rescale_from:
        s = torch.tensor([W / rescale_from, H / rescale_from, 1.0], dtype=dt, device=K.device)
        Kd = Kd * s[None, :, None]
    dev = R.device
    u = torch.arange(W, dtype=dt, device=dev) + 0.5
    v = torch.arange(H, dtype=dt, device=dev) + 0.5
    vv, uu = torch.meshgrid(v, u, indexing="ij")
    pix = torch.stack([uu, vv, torch.ones_like(uu)], dim=-1)          # [H,W,3]
    Kinv = torch.linalg.inv(Kd)                                        # [B,3,3]
    d_cam = torch.einsum("bij,hwj->bhwi", Kinv, pix)                   # [B,H,W,3]
    d_cam = d_cam / d_cam.norm(dim=-1, keepdim=True)
    d_world = torch.einsum("bfij,bhwj->bfhwi", Rd, d_cam)              # [B,F,H,W,3]
    B, Fr = R.shape[:2]
    pos = td[:, :, None, None, :].expand(B, Fr, H, W, 3)
    return pos.float(), d_world.float()


def posenc_nerf(x: torch.Tensor, min_deg: int, max_deg: int) -> torch.Tensor:
    """[x, sin(x*2^k), sin(x*2^k + pi/2)] with scale-major / xyz-minor packing
    (`xunet.py:49-59`)."""
    if min_deg == max_deg:
        return x
    # exact powers of two built on the device (no host->device copy: graph-capturable)
    scales = torch.pow(2.0, torch.arange(min_deg, max_deg, device=x.device, dtype=torch.float32)).to(x.dtype)
    xb = (x[..., None, :] * scales[:, None]).flatten(-2)
    emb = torch.sin(torch.cat([xb, xb + math.pi / 2.0], dim=-1))
    return torch.cat([x, emb], dim=-1)


def posenc_ddpm(t: torch.Tensor, emb_ch: int, max_time: float = 1.0) -> torch.Tensor:
    """DDPM sinusoidal embedding of (clipped) logSNR, t*1000/max_time
    (`xunet.py:32-46`)."""
    t = t.float() * (1000.0 / max_time)
    half = emb_ch // 2
    k = torch.arange(half, dtype=torch.float32, device=t.device)
    freqs = torch.exp(k * (-math.log(10000.0) / (half - 1)))
    arg = t[..., None] * freqs
    return torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1)


def logsnr_mlp(logsnr: torch.Tensor, w1, b1, w2, b2, max_time: float = 1.0) -> torch.Tensor:
    """[B, 2] logSNR -> [2B, E] fp32: clip +-20, DDPM posenc, Linear-SiLU-Linear
    (`xunet.py:273-277,305-308`)."""
    E = w1.shape[0]
    l = torch.clamp(logsnr.float(), -20.0, 20.0)
    e = posenc_ddpm(l, E, max_time=max_time).reshape(-1, E)
    return torch.nn.functional.linear(torch.nn.functional.silu(torch.nn.functional.linear(e, w1, b1)), w2, b2)


def ray_posenc(R: torch.Tensor, t: torch.Tensor, K: torch.Tensor, H: int, W: int,
               cond_mask: torch.Tensor, pos_emb: Optional[torch.Tensor],
               first_emb: Optional[torch.Tensor], other_emb: Optional[torch.Tensor],
               rescale_from: int = 0) -> torch.Tensor:
    """144-channel camera conditioning input, NHWC frame-interleaved
    [2B, H, W, 144] in fp32 (`xunet.py:311-336`): rays -> NeRF posenc (origins
    deg 0..15, directions deg 0..8) -> zeroed for unconditional examples ->
    + learned pos_emb[144,H,W] -> + per-frame embedding."""
    pos, dirs = camera_rays(R, t, K, H, W, rescale_from)
    emb = torch.cat([posenc_nerf(pos, 0, 15), posenc_nerf(dirs, 0, 8)], dim=-1)  # [B,2,H,W,144]
    emb = torch.where(cond_mask.view(-1, 1, 1, 1, 1), emb, torch.zeros_like(emb))
    if pos_emb is not None:
        emb = emb + pos_emb.permute(1, 2, 0)[None, None]
    if first_emb is not None:
        fe = torch.cat([first_emb, other_emb], dim=1).reshape(1, 2, 1, 1, -1)
        emb = emb + fe
    B = emb.shape[0]
    return emb.reshape(B * 2, H, W, emb.shape[-1])


def film_batch(emb, weights, biases):
    """Level-batched FiLM projections (oracle): ``silu(emb)`` through one linear
    over the concatenated weights, split into per-block ``[.., 2C_i]``
    modulations (`xunet.py:84-87`)."""
    semb = F.silu(emb)
    y = F.linear(semb, torch.cat([w.to(semb.dtype) for w in weights], 0),
                 torch.cat([b.to(semb.dtype) for b in biases], 0))
    return tuple(torch.split(y, [w.shape[0] for w in weights], dim=-1))


def ray_posenc_dir(R, t, K, H, W, cond_mask, rescale_from: int = 0, ld: int = 64):
    """Direction half of the ray conditioning (channels 93..143 of
    :func:`ray_posenc`, masked, no learned embeddings), zero-padded to ``ld``
    channels: [2B, H, W, ld] fp32."""
    _, dirs = camera_rays(R, t, K, H, W, rescale_from)
    emb = posenc_nerf(dirs, 0, 8)
    emb = torch.where(cond_mask.view(-1, 1, 1, 1, 1), emb, torch.zeros_like(emb))
    B = emb.shape[0]
    emb = emb.reshape(B * 2, H, W, emb.shape[-1])
    return F.pad(emb, (0, ld - emb.shape[-1]))


def ray_origin_pe(t, cond_mask):
    """Origin half (channels 0..92): NeRF posenc of the camera position, which
    is the same for every pixel of an image: [2B, 93] fp32."""
    B = t.shape[0]
    pe = posenc_nerf(t.float().reshape(B * 2, 3), 0, 15)
    m = cond_mask.to(pe.dtype).repeat_interleave(2)
    return pe * m[:, None]


def cond_conv(rays_dir, orig_pe, weight, bias, stride, row_bias=None, residual=None, res_period=0):
    """Conditioning conv on the split ray input (oracle): rebuild the 144
    channels (origin broadcast over pixels + direction) and convolve."""
    N, H, W, _ = rays_dir.shape
    nd = weight.shape[1] - orig_pe.shape[1]
    full = torch.cat([orig_pe[:, None, None, :].to(rays_dir.dtype).expand(N, H, W, orig_pe.shape[1]),
                      rays_dir[..., :nd]], dim=-1)
    return conv3x3(full, weight, bias, stride, residual, 1.0, row_bias, res_period)


def cat_gn_silu_dense(a, b, gw, gb, dw, db, groups: int = 32, eps: float = 1e-5):
    """silu(GN(cat[a, b])) and dense(cat[a, b]) (decoder block entry, oracle)."""
    x = torch.cat([a, b], -1)
    return group_norm(x, gw, gb, groups, eps, True), linear(x, dw, db)


# ------------------------------------------------ training-input draw ----
# Counter-based RNG shared bit-for-bit with the HIP kernels (common.h
# hash_u32 / normal01; elementwise.hip diffusion_fwd2_k): splitmix64 of
# (seed, index) in wrapping int64 arithmetic with logical shifts.
_M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
K_EPS = 0x5851F42D4C957F2D
K_XN = 0x14057B7EF767814F
K_XU = 0xA0761D6478BD642F       # sampler: unconditional-pass input noise
K_NZ = 0xE7037ED1A0B428DB       # sampler: ancestral-step noise
K_Z0 = 0x8EBC6AF09C88C6E3       # sampler: initial z


def _s64(v: int) -> int:
    v &= _M64
    return v - (1 << 64) if v >= (1 << 63) else v


def _lsr(z: torch.Tensor, k: int) -> torch.Tensor:
    return (z >> k) & ((1 << (64 - k)) - 1)


def hash_u32(seed: int, idx: torch.Tensor) -> torch.Tensor:
    """common.h ``hash_u32`` on an int64 index tensor -> values in [0, 2^32)."""
    z = idx.to(torch.int64) + _s64(seed * GOLDEN + 0x632BE59BD9B4E019)
    z = (z ^ _lsr(z, 30)) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _s64(0x94D049BB133111EB)
    z = z ^ _lsr(z, 31)
    return _lsr(z, 32)


def u01(seed: int, idx: torch.Tensor) -> torch.Tensor:
    return (hash_u32(seed, idx) >> 8).to(torch.float32) * (1.0 / 16777216.0)


def normal01(seed: int, idx: torch.Tensor) -> torch.Tensor:
    idx = idx.to(torch.int64)
    u1 = ((hash_u32(seed, 2 * idx) >> 8) + 1).to(torch.float32) * torch.tensor(1.0 / 16777217.0)
    u2 = (hash_u32(seed, 2 * idx + 1) >> 8).to(torch.float32) * (1.0 / 16777216.0)
    return torch.sqrt(-2.0 * torch.log(u1)) * torch.cos(6.283185307179586 * u2)


def schedule_ab(logsnr_min: float, logsnr_max: float):
    b = math.atan(math.exp(-0.5 * logsnr_max))
    a = math.atan(math.exp(-0.5 * logsnr_min)) - b
    return a, b


def diffusion_inputs(img: torch.Tensor, seed: int, e0: int = 0, cond_prob: float = 0.1,
                     logsnr_min: float = -20.0, logsnr_max: float = 20.0, dtype=torch.float32,
                     prediction: str = "eps"):
    """The training-input draw of `train.py:80-100` for examples
    ``e0 .. e0+B-1`` of a step whose RNG seed is ``seed`` (same numbers as
    ``diffusion_fwd2_k``).  img [B,2,3,H,W] -> (xz [2B,H,W,8] NHWC stem input
    (frame 0 = CFG-dropped x, frame 1 = z_t; channels 3..7 zero), the loss
    target [B,3,H,W] fp32 (``prediction="eps"``: eps; ``"v"``: alpha eps -
    sigma z_clean), logsnr [B,2], keep [B] bool)."""
    if prediction not in ("eps", "v"):
        raise ValueError(f"prediction {prediction!r}: expected 'eps' or 'v'")
    B, _, C, H, W = img.shape
    HW = H * W
    dev = img.device
    s = seed & _M64
    g = torch.arange(B, device=dev, dtype=torch.int64) + e0
    a, b = schedule_ab(logsnr_min, logsnr_max)
    af, bf = torch.tensor(a, dtype=torch.float32), torch.tensor(b, dtype=torch.float32)
    t = u01(s, 4 * g)
    lam = -2.0 * torch.log(torch.tan(af.to(dev) * t + bf.to(dev)))
    keep = u01(s, 4 * g + 1) > cond_prob
    lam0 = (-2.0 * torch.log(torch.tan(bf))).to(dev).expand(B)
    idx = g[:, None, None] * (3 * HW) + torch.arange(3, device=dev)[None, :, None] * HW + \
        torch.arange(HW, device=dev)[None, None, :]
    eps = normal01(s ^ K_EPS, idx).reshape(B, 3, H, W)
    xn = normal01(s ^ K_XN, idx).reshape(B, 3, H, W)
    # alpha / sigma in float64, rounded once: the CPU sigmoid rounds differently in its vector body and its
    # scalar tail, so in float32 an example's value could move by an ulp with its position in the batch
    # (seen with 24 vs 64 examples on an AVX-512 host), and the draw must not depend on the split
    lam64 = lam.double()
    alpha = torch.sqrt(torch.sigmoid(lam64)).float().view(B, 1, 1, 1)
    sigma = torch.sqrt(torch.sigmoid(-lam64)).float().view(B, 1, 1, 1)
    x, z = img[:, 0].float(), img[:, 1].float()
    xc = torch.where(keep.view(B, 1, 1, 1), x, xn)
    zt = alpha * z + sigma * eps
    xz = torch.zeros(B, 2, H, W, 8, dtype=dtype, device=dev)
    xz[:, 0, ..., :3] = xc.permute(0, 2, 3, 1).to(dtype)
    xz[:, 1, ..., :3] = zt.permute(0, 2, 3, 1).to(dtype)
    target = eps if prediction == "eps" else alpha * eps - sigma * z
    return xz.reshape(2 * B, H, W, 8), target, torch.stack([lam0, lam], 1), keep


def loss_weight_mode(prediction: str, loss_weight: str, logsnr) -> int:
    """The loss kernels' weight switch: 0 none, 1 min-SNR for an eps target, 2
    min-SNR for a v target (validates the three arguments)."""
    if prediction not in ("eps", "v"):
        raise ValueError(f"prediction {prediction!r}: expected 'eps' or 'v'")
    if loss_weight not in ("none", "min_snr"):
        raise ValueError(f"loss_weight {loss_weight!r}: expected 'none' or 'min_snr'")
    if loss_weight == "none":
        return 0
    if logsnr is None:
        raise ValueError(f"loss_weight={loss_weight!r} needs the batch's logsnr [B,2]")
    return 1 if prediction == "eps" else 2


def diff_loss_nhwc(y: torch.Tensor, eps: torch.Tensor, loss_type: str = "l2", *, logsnr=None,
                   prediction: str = "eps", loss_weight: str = "none", gamma: float = 5.0) -> torch.Tensor:
    """Diffusion loss (`train.py:102-112`) on the NHWC head output y [B,H,W,>=3]
    (only the first 3 channels are the prediction) against the target ``eps``
    [B,3,H,W] (eps or v).  ``loss_weight="min_snr"``: each example's mean is
    weighted by min-SNR-gamma of ``logsnr[:, 1]`` (``diffusion.min_snr_weight``;
    ``logsnr`` the [B,2] tensor of :func:`diffusion_inputs`), not normalised."""
    wm = loss_weight_mode(prediction, loss_weight, logsnr)
    yh = y[..., :3].permute(0, 3, 1, 2).float()
    if wm == 0:
        if loss_type == "l2":
            return torch.mean((eps.float() - yh) ** 2)
        if loss_type == "l1":
            return torch.mean((eps.float() - yh).abs())
        if loss_type == "huber":
            return F.smooth_l1_loss(yh, eps.float())
        raise NotImplementedError(loss_type)
    from ..diffusion import diffusion_loss
    return diffusion_loss(eps, yh, loss_type, logsnr=logsnr[:, 1], prediction=prediction, loss_weight=loss_weight,
                          gamma=gamma)


# ------------------------------------------------- loss by noise level ---
def _element_loss(d: torch.Tensor, loss_type: str) -> torch.Tensor:
    if loss_type == "l2":
        return d * d
    if loss_type == "l1":
        return d.abs()
    if loss_type == "huber":
        ad = d.abs()
        return torch.where(ad < 1.0, 0.5 * d * d, ad - 0.5)
    raise ValueError(f"loss_type {loss_type!r}: expected 'l2', 'l1' or 'huber'")


def diff_loss_rows(y: torch.Tensor, target: torch.Tensor, loss_type: str = "l2") -> torch.Tensor:
    """Per-example loss rows [B,2] fp32 of the NHWC head output y [B,H,W,>=3]
    against ``target`` [B,3,H,W]: column 0 the example's mean of l(y - target)
    (l the ``loss_type``), column 1 its mean of (y - target)^2, both over the
    3 H W valid elements.  No autograd."""
    d = y.detach()[..., :3].permute(0, 3, 1, 2).float() - target.detach().float()
    el = _element_loss(d, loss_type)
    return torch.stack([el.flatten(1).mean(1), (d * d).flatten(1).mean(1)], 1)


def loss_bin_terms(lam: torch.Tensor, prediction: str, loss_weight: str, gamma: float, nbins: int,
                   logsnr_min: float, logsnr_max: float):
    """(bin [B] int64, w, f_eps, f_x [B] fp64) of the examples' fp32 ``lam``:
    bins uniform in t through the schedule's inverse tau(lambda) = (atan(exp(
    -lambda / 2)) - b) / a; w the configured loss weight; f_eps / f_x the
    factors that turn the target's squared error into eps / x0 units."""
    wm = loss_weight_mode(prediction, loss_weight, lam)
    a, b = schedule_ab(logsnr_min, logsnr_max)
    lam = lam.detach().double()
    tau = (torch.atan(torch.exp(-0.5 * lam)) - b) / a
    bins = torch.floor(tau * nbins).clamp(0, nbins - 1).to(torch.int64)
    sp, sn = torch.sigmoid(lam), torch.sigmoid(-lam)
    if wm == 0:
        w = torch.ones_like(lam)
    elif wm == 1:
        w = torch.clamp(gamma * torch.exp(-lam), max=1.0)
    else:
        w = torch.minimum(sp, gamma * sn)
    if prediction == "eps":
        return bins, w, torch.ones_like(lam), torch.exp(-lam)
    return bins, w, sp, sn


def loss_bins_add(table: torch.Tensor, rows: torch.Tensor, logsnr: torch.Tensor, *, prediction: str = "eps",
                  loss_weight: str = "none", gamma: float = 5.0, logsnr_min: float = -20.0,
                  logsnr_max: float = 20.0) -> torch.Tensor:
    """table [NB,5] fp64 += per bin of logsnr[:, 1]: (count, sum row0, sum w
    row0, sum f_eps row1, sum f_x row1) over the batch's ``rows`` [B,2]
    (:func:`diff_loss_rows`); see :func:`loss_bin_terms`.  In place."""
    if table.dtype != torch.float64 or table.dim() != 2 or table.shape[1] != 5:
        raise ValueError(f"table: expected fp64 [NB,5], got {table.dtype} {tuple(table.shape)}")
    bins, w, fe, fx = loss_bin_terms(logsnr[:, 1], prediction, loss_weight, gamma, table.shape[0], logsnr_min,
                                     logsnr_max)
    r0, r1 = rows[:, 0].detach().double(), rows[:, 1].detach().double()
    vals = torch.stack([torch.ones_like(r0), r0, w * r0, fe * r1, fx * r1], 1)
    table.index_add_(0, bins, vals)          # (CPU: example order)
    return table


# ----------------------------------------------------------- image metrics ---
SSIM_TAPS, SSIM_SIGMA = 11, 1.5
SSIM_C1, SSIM_C2 = 0.01 ** 2, 0.03 ** 2


def ssim_window() -> list:
    """The normalised 11-tap Gaussian (sigma 1.5) of SSIM, in float64."""
    g = [math.exp(-((k - SSIM_TAPS // 2) ** 2) / (2.0 * SSIM_SIGMA ** 2)) for k in range(SSIM_TAPS)]
    s = math.fsum(g)
    return [v / s for v in g]


def image_map01(x: torch.Tensor, quantize: bool) -> torch.Tensor:
    """[-1, 1] fp32 -> [0, 1] float64; ``quantize``: through the uint8 value
    ``sampling.py:save_png`` writes (fp32 add, fp32 multiply, truncation)."""
    if quantize:
        return image_map_u8(x).double() / 255.0
    return (x.float().clamp(-1.0, 1.0).double() + 1.0) * 0.5


def image_metrics(pred: torch.Tensor, target: torch.Tensor, quantize: bool = True):
    """Per-image (mse [N], ssim [N]) fp32 of two [N,C,H,W] batches in [-1, 1]
    on the [0, 1] scale: the float64 composition (CPU path and oracle of
    ``image_metrics_tile_k``).  SSIM: Wang et al. 2004, per channel, separable
    11-tap Gaussian window over the valid region, L = 1."""
    N, C, H, W = pred.shape
    x, y = image_map01(pred, quantize), image_map01(target, quantize)
    mse = (x - y).square().flatten(1).mean(1)
    g = torch.tensor(ssim_window(), dtype=torch.float64, device=x.device)

    def blur(v):
        v = v.reshape(N * C, 1, H, W)
        return F.conv2d(F.conv2d(v, g.view(1, 1, 1, -1)), g.view(1, 1, -1, 1))

    mx, my = blur(x), blur(y)
    vx, vy, cxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    s = ((2 * mx * my + SSIM_C1) * (2 * cxy + SSIM_C2)) / ((mx * mx + my * my + SSIM_C1) * (vx + vy + SSIM_C2))
    return mse.float(), s.reshape(N, -1).mean(1).float()


# ---------------------------------------------------- procedural scenes ---
# The analytic ray caster of data/procedural.py (csrc/scene.hip holds the rule
# in full).  fp64 throughout, written operation by operation in the order the
# kernel uses, so the two agree to rounding.
SCENE_SLOTS, SCENE_WORDS = 6, 16
SCENE_REF = 128                      # K is the intrinsics of the 128 x 128 SRN image
SCENE_LIGHT = (0.3, 0.2, 1.0)
SCENE_AMBIENT, SCENE_DIFFUSE = 0.35, 0.65


def scene_render_check(table, R, t, K, H, W, aa) -> int:
    """Argument check shared by both backends (ValueError); returns N."""
    if table.dim() != 3 or tuple(table.shape[1:]) != (SCENE_SLOTS, SCENE_WORDS):
        raise ValueError(f"scene_render: table must be [N,{SCENE_SLOTS},{SCENE_WORDS}], got {tuple(table.shape)}")
    N = table.shape[0]
    for name, x, shape in (("R", R, (N, 3, 3)), ("t", t, (N, 3)), ("K", K, (N, 3, 3))):
        if tuple(x.shape) != shape:
            raise ValueError(f"scene_render: {name} must be {list(shape)} for {N} images, got {tuple(x.shape)}")
    for name, x in (("table", table), ("R", R), ("t", t), ("K", K)):
        if x.dtype != torch.float64:
            raise ValueError(f"scene_render: {name} must be float64, got {x.dtype}")
        if x.device != table.device:
            raise ValueError(f"scene_render: {name} is on {x.device}, the table on {table.device}")
    for name, v in (("H", H), ("W", W), ("aa", aa)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"scene_render: {name} must be an int, got {v!r}")
    if H < 1 or W < 1:
        raise ValueError(f"scene_render: H, W must be positive, got {H} x {W}")
    if not 1 <= aa <= 4:
        raise ValueError(f"scene_render: aa must be in 1..4, got {aa}")
    return N


def _inv3(M: torch.Tensor) -> torch.Tensor:
    """Inverse of [N,3,3] by the adjugate (scene_render_k's expression)."""
    a, b, c, d, e, f, g, h, i = (M[:, r, s] for r in range(3) for s in range(3))
    A, B, C = e * i - f * h, f * g - d * i, d * h - e * g
    det = a * A + b * B + c * C
    adj = [A, c * h - b * i, b * f - c * e, B, a * i - c * g, c * d - a * f, C, b * g - a * h, a * e - b * d]
    return torch.stack([x / det for x in adj], -1).reshape(-1, 3, 3)


def _scene_prims(table, t):
    """Per slot (A [N,3,3], the origin in the primitive's frame A (t - c) as 3
    x [N], albedo [N,3], kind [N] int64)."""
    N = table.shape[0]
    prims = []
    for p in range(SCENE_SLOTS):
        A = table[:, p, :9].reshape(N, 3, 3)
        x = [t[:, k] - table[:, p, 9 + k] for k in range(3)]
        o = [A[:, k, 0] * x[0] + A[:, k, 1] * x[1] + A[:, k, 2] * x[2] for k in range(3)]
        prims.append((A, o, table[:, p, 12:15], table[:, p, 15].to(torch.int64)))
    return prims


def _scene_dirs(Kinv, R, u, v):
    """World directions (3 x [N,H,W]) through pixel coordinates ``u``, ``v`` [H,W]."""
    e = lambda x: x[:, None, None]  # noqa: E731
    c = [e(Kinv[:, k, 0]) * u + e(Kinv[:, k, 1]) * v + e(Kinv[:, k, 2]) for k in range(3)]
    nrm = torch.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    c = [x / nrm for x in c]
    return [e(R[:, k, 0]) * c[0] + e(R[:, k, 1]) * c[1] + e(R[:, k, 2]) * c[2] for k in range(3)]


def scene_trace(table: torch.Tensor, origin: torch.Tensor, dirs: torch.Tensor):
    """Nearest hits of arbitrary rays, in float64: ``table`` [N,6,16],
    ``origin`` [N,3], unit ``dirs`` [N,H,W,3] -> (t [N,H,W], +inf on a miss;
    prim [N,H,W] int64, -1 on a miss; colour [N,3,H,W] in [0, 1])."""
    return _scene_hit(_scene_prims(table, origin), list(dirs.unbind(-1)))


def _scene_nearest(prims, d):
    """The nearest hit of unit directions ``d`` (3 x [N,H,W]): (t, +inf on a
    miss; prim int64, -1 on a miss; the normal in the primitive's frame, 3 x
    [N,H,W]; face int64: 0 on an ellipsoid, 1 + 2 ax + (sg > 0) on a box)."""
    e = lambda x: x[:, None, None]  # noqa: E731
    inf = torch.full_like(d[0], float("inf"))
    best_t, best_p = inf, torch.full(d[0].shape, -1, dtype=torch.int64, device=d[0].device)
    best_f = torch.zeros_like(best_p)
    n = [torch.zeros_like(d[0]) for _ in range(3)]
    zero, one = torch.zeros_like(d[0]), torch.ones_like(d[0])
    for p, (A, o, _, kind) in enumerate(prims):
        q = [e(A[:, k, 0]) * d[0] + e(A[:, k, 1]) * d[1] + e(A[:, k, 2]) * d[2] for k in range(3)]
        ob = [e(x) + zero for x in o]
        # ellipsoid: the near root of |o + t q|^2 = 1
        qa = q[0] * q[0] + q[1] * q[1] + q[2] * q[2]
        qb = ob[0] * q[0] + ob[1] * q[1] + ob[2] * q[2]
        qc = ob[0] * ob[0] + ob[1] * ob[1] + ob[2] * ob[2] - 1.0
        disc = qb * qb - qa * qc
        t_e = (-qb - torch.sqrt(disc.clamp_min(0.0))) / qa
        m_e = [ob[k] + t_e * q[k] for k in range(3)]
        # box: slabs of [-1, 1]^3, the entry face's normal
        t1 = torch.stack([(-1.0 - ob[k]) * (1.0 / q[k]) for k in range(3)], -1)
        t2 = torch.stack([(1.0 - ob[k]) * (1.0 / q[k]) for k in range(3)], -1)
        tmin, ax = torch.minimum(t1, t2).max(-1)
        tmax = torch.maximum(t1, t2).min(-1).values
        qs = torch.stack(q, -1).gather(-1, ax[..., None])[..., 0]
        sg = torch.where(qs > 0.0, -one, one)
        m_b = [torch.where(ax == k, sg, zero) for k in range(3)]
        is_e, is_b = e(kind == 1), e(kind == 2)
        tt = torch.where(is_e, t_e, tmin)
        hit = ((is_e & (disc > 0.0)) | (is_b & (tmin < tmax))) & (tt > 0.0) & (tt < best_t)
        best_t = torch.where(hit, tt, best_t)
        best_p = torch.where(hit, torch.full_like(best_p, p), best_p)
        n = [torch.where(hit, torch.where(is_e, m_e[k], m_b[k]), n[k]) for k in range(3)]
        face = torch.where(is_e, torch.zeros_like(ax), 1 + 2 * ax + (sg > 0.0).to(ax.dtype))
        best_f = torch.where(hit, face, best_f)
    return best_t, best_p, n, best_f


def _scene_hit(prims, d):
    e = lambda x: x[:, None, None]  # noqa: E731
    best_t, best_p, n, _ = _scene_nearest(prims, d)
    one = torch.ones_like(d[0])
    ln = math.sqrt(sum(x * x for x in SCENE_LIGHT))
    col = [one, one, one]
    for p, (A, _, alb, _) in enumerate(prims):
        w = [e(A[:, 0, k]) * n[0] + e(A[:, 1, k]) * n[1] + e(A[:, 2, k]) * n[2] for k in range(3)]
        wn = torch.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
        w = [x / wn for x in w]
        ndl = w[0] * (SCENE_LIGHT[0] / ln) + w[1] * (SCENE_LIGHT[1] / ln) + w[2] * (SCENE_LIGHT[2] / ln)
        shade = SCENE_AMBIENT + SCENE_DIFFUSE * ndl.clamp_min(0.0)
        col = [torch.where(best_p == p, e(alb[:, k]) * shade, col[k]) for k in range(3)]
    return best_t, best_p, torch.stack(col, 1)


def scene_render(table: torch.Tensor, R: torch.Tensor, t: torch.Tensor, K: torch.Tensor, H: int, W: int, *,
                 aa: int = 3, return_aux: bool = False):
    """Images [N,3,H,W] fp32 in [-1, 1] of the scene tables [N,6,16] (fp64; per
    slot A [9], centre [3], albedo [3], kind) under the cameras ``R`` [N,3,3]
    cam-to-world, ``t`` [N,3] and ``K`` [N,3,3], the intrinsics of the 128 x
    128 image (``camera_rays(..., rescale_from=128)`` gives the pixel-centre
    rays).  A pixel is the mean of ``aa`` x ``aa`` sub-pixel rays.
    ``return_aux``: also depth [N,H,W] fp32 (+inf on a miss) and prim [N,H,W]
    int32 (-1 on a miss) of the pixel-centre ray.  The rule is stated in
    csrc/scene.hip; this float64 form is the CPU path and the kernel's oracle."""
    N = scene_render_check(table, R, t, K, H, W, aa)
    dt, dev = torch.float64, table.device
    s = torch.tensor([W / SCENE_REF, H / SCENE_REF, 1.0], dtype=dt, device=dev)
    Kinv = _inv3(K * s[None, :, None])
    prims = _scene_prims(table, t)
    py, px = torch.meshgrid(torch.arange(H, dtype=dt, device=dev), torch.arange(W, dtype=dt, device=dev),
                            indexing="ij")
    acc = torch.zeros(N, 3, H, W, dtype=dt, device=dev)
    for i in range(aa):
        for j in range(aa):
            acc = acc + _scene_hit(prims, _scene_dirs(Kinv, R, px + (j + 0.5) / aa, py + (i + 0.5) / aa))[2]
    img = (2.0 * (acc / float(aa * aa)) - 1.0).float()
    if not return_aux:
        return img
    depth, prim, _ = _scene_hit(prims, _scene_dirs(Kinv, R, px + 0.5, py + 0.5))
    return img, depth.float(), prim.to(torch.int32)


# The rule that turns (seed, object id, view id) into a scene table and a pose
# (data/procedural.py states it; csrc/procedural.hip is its fused HIP form).
# These float64 functions are the CPU path of ops.procedural_render /
# ops.procedural_batch and the kernel's oracle.
PROC_MAX_VIEWS = 4096                # views of one object (the pose counter's stride)
PROC_MAX_OBJECTS = 1 << 31
PROC_K_COUNT = 0x5BD1E995
PROC_K_POSE = 0x7F4A7C15
PROC_K_BATCH = 0x70726F6365647572    # "procedur": keeps the batch draw apart from the scene and pose draws
PROC_CENTRE = (0.7, 0.5, 0.4)
SRN_FOCAL_128 = 131.25               # SRN cars 128^2 pinhole (fx = fy), principal point at 64
SRN_RADIUS = 1.3
SRN_K = (SRN_FOCAL_128, 0.0, 64.0, 0.0, SRN_FOCAL_128, 64.0, 0.0, 0.0, 1.0)


def srn_intrinsics(device="cpu") -> torch.Tensor:
    """The SRN 128 x 128 pinhole K [3,3] (float64)."""
    return torch.tensor(SRN_K, dtype=torch.float64, device=device).reshape(3, 3)


def orbit_look_at(az: torch.Tensor, el: torch.Tensor, radius: float = SRN_RADIUS):
    """The look-at pose (OpenCV cam-to-world, z up) on the orbit at azimuth
    ``az`` and elevation ``el`` (float64 [n]): R [n,3,3], t [n,3]."""
    pos = radius * torch.stack([torch.cos(el) * torch.cos(az), torch.cos(el) * torch.sin(az), torch.sin(el)], -1)
    fwd = -pos / pos.norm(dim=-1, keepdim=True)
    up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=pos.device).expand_as(fwd)
    right = torch.linalg.cross(fwd, up)
    right = right / right.norm(dim=-1, keepdim=True)
    down = torch.linalg.cross(fwd, right)
    R = torch.stack([right, down, fwd], dim=-1)
    return R, pos


def proc_ids(x, device) -> torch.Tensor:
    return torch.as_tensor(x, dtype=torch.int64, device=device).reshape(-1)


def procedural_scene(seed: int, object_ids, device="cpu") -> torch.Tensor:
    """Scene tables [N,6,16] (float64) of the objects: per slot the 3 x 3 map
    ``A = diag(1 / axes) R^T`` (world to the unit primitive, row-major), the
    centre, the albedo and the kind (0 empty, 1 ellipsoid, 2 box)."""
    dt = torch.float64
    o = proc_ids(object_ids, device)
    N = o.numel()
    count = 3 + hash_u32(seed ^ PROC_K_COUNT, o) % 4                              # [N]
    p = torch.arange(SCENE_SLOTS, device=o.device)
    k = torch.arange(14, device=o.device)
    u = u01(seed, ((o[:, None, None] * SCENE_SLOTS + p[None, :, None]) * 64 + k[None, None, :])).to(dt)   # [N,6,14]
    centre = (u[..., 0:3] - 0.5) * torch.tensor(PROC_CENTRE, dtype=dt, device=o.device)
    axes = 0.08 + 0.22 * u[..., 3:6]
    q = 2.0 * u[..., 6:10] - 1.0 + 1e-3
    q = q / torch.sqrt((q * q).sum(-1, keepdim=True))
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(N, SCENE_SLOTS, 3, 3)
    A = R.transpose(-1, -2) / axes[..., :, None]                                  # diag(1 / axes) R^T
    albedo = 0.1 + 0.8 * u[..., 10:13]
    kind = torch.where(u[..., 13] < 0.5, 1.0, 2.0).to(dt)
    table = torch.cat([A.reshape(N, SCENE_SLOTS, 9), centre, albedo, kind[..., None]], -1)
    live = p[None, :] < count[:, None]
    return torch.where(live[..., None], table, torch.zeros_like(table))


def procedural_pose(seed: int, object_ids, view_ids, device="cpu"):
    """Cam-to-world poses of views ``view_ids`` [n] of objects ``object_ids``
    [n]: R [n,3,3], t [n,3] (float64; OpenCV axes, z up, looking at the origin)."""
    o, v = proc_ids(object_ids, device), proc_ids(view_ids, device)
    if o.shape != v.shape:
        raise ValueError(f"procedural_pose: {o.numel()} object ids and {v.numel()} view ids")
    c = 2 * (o * PROC_MAX_VIEWS + v)
    az = 2.0 * math.pi * u01(seed ^ PROC_K_POSE, c).to(torch.float64)
    el = 0.05 + 0.95 * u01(seed ^ PROC_K_POSE, c + 1).to(torch.float64)
    return orbit_look_at(az, el, SRN_RADIUS)


def split_object(rank, split: str):
    """The id of the split's ``rank``-th object (int or int64 tensor): ids with
    ``o % 10 == 9`` are the held-out split, the rest the training split."""
    return 10 * rank + 9 if split == "val" else rank + rank // 9


def procedural_batch_key(seed: int, batch_index: int) -> int:
    """(seed, batch index) folded into the 64-bit key of the batch draw."""
    return ((seed * 0x2545F4914F6CDD1D + PROC_K_BATCH) + (batch_index + 1) * GOLDEN) & _M64


def procedural_draw(seed: int, batch_index: int, B: int, *, n_objects: int, views: int, split: str,
                    example_offset: int = 0, device="cpu"):
    """(object ids [B], view ids [B,2]) of the batch (int64): example ``g =
    example_offset + j`` draws the ``hash_u32(s, 4 g) % n_objects``-th object
    of the split and two distinct views of ``views``."""
    s = procedural_batch_key(seed, batch_index)
    g = torch.arange(B, dtype=torch.int64, device=device) + example_offset
    obj = split_object(hash_u32(s, 4 * g) % n_objects, split)
    v0 = hash_u32(s, 4 * g + 1) % views
    v1 = (v0 + 1 + hash_u32(s, 4 * g + 2) % (views - 1)) % views
    return obj, torch.stack([v0, v1], 1)


def _proc_int(name, op, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"{op}: {name} must be an int, got {v!r}")
    if v < lo or (hi is not None and v > hi):
        raise ValueError(f"{op}: {name} must be in {lo}..{'' if hi is None else hi}, got {v}")


def procedural_render_check(seed, object_ids, view_ids, H, W, aa) -> int:
    """Argument check shared by both backends (ValueError); returns n.  The
    range check of the ids reads them back (one host synchronise on the GPU)."""
    op = "procedural_render"
    _proc_int("seed", op, seed, -(1 << 63), _M64)
    for name, x in (("object_ids", object_ids), ("view_ids", view_ids)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.int64 or x.dim() != 1:
            raise ValueError(f"{op}: {name} must be a 1-D int64 tensor")
    if object_ids.shape != view_ids.shape or object_ids.device != view_ids.device:
        raise ValueError(f"{op}: {object_ids.numel()} object ids on {object_ids.device} and {view_ids.numel()} view "
                         f"ids on {view_ids.device}")
    _proc_int("H", op, H, 1)
    _proc_int("W", op, W, 1)
    _proc_int("aa", op, aa, 1, 4)
    if object_ids.numel():
        lo, hi, vlo, vhi = torch.stack([object_ids.min(), object_ids.max(), view_ids.min(), view_ids.max()]).tolist()
        if lo < 0 or hi >= PROC_MAX_OBJECTS:
            raise ValueError(f"{op}: object ids must be in [0, 2^31), got {lo}..{hi}")
        if vlo < 0 or vhi >= PROC_MAX_VIEWS:
            raise ValueError(f"{op}: view ids must be in [0, {PROC_MAX_VIEWS}), got {vlo}..{vhi}")
    return object_ids.numel()


def procedural_batch_check(seed, batch_index, B, H, W, n_objects, views, split, example_offset, aa) -> None:
    """Argument check shared by both backends (ValueError)."""
    op = "procedural_batch"
    _proc_int("seed", op, seed, -(1 << 63), _M64)
    _proc_int("batch_index", op, batch_index, 0, 1 << 62)
    _proc_int("B", op, B, 0, 1 << 30)
    _proc_int("H", op, H, 1)
    _proc_int("W", op, W, 1)
    _proc_int("aa", op, aa, 1, 4)
    _proc_int("views", op, views, 2, PROC_MAX_VIEWS)
    _proc_int("n_objects", op, n_objects, 1, PROC_MAX_OBJECTS)
    _proc_int("example_offset", op, example_offset, 0, 1 << 60)
    if split not in ("train", "val"):
        raise ValueError(f"{op}: split {split!r}: expected 'train' or 'val'")
    if split_object(n_objects - 1, split) >= PROC_MAX_OBJECTS:
        raise ValueError(f"{op}: {n_objects} {split} objects reach past id 2^31")


def procedural_render(seed: int, object_ids, view_ids, H: int, W: int, *, aa: int = 3, return_aux: bool = False):
    """``(img [n,3,H,W] f32, R [n,3,3], t [n,3], table [n,6,16])`` (and, with
    ``return_aux``, depth and prim) of the listed (object, view) pairs: the
    composition of ``procedural_scene``, ``procedural_pose`` and ``scene_render``."""
    n = procedural_render_check(seed, object_ids, view_ids, H, W, aa)
    dev = object_ids.device
    table = procedural_scene(seed, object_ids, dev)
    R, t = procedural_pose(seed, object_ids, view_ids, dev)
    K = srn_intrinsics(dev).expand(n, 3, 3).contiguous()
    out = scene_render(table, R, t, K, H, W, aa=aa, return_aux=return_aux)
    return (out[0], R, t, table, out[1], out[2]) if return_aux else (out, R, t, table)


def procedural_batch(seed: int, batch_index: int, B: int, H: int, W: int, *, n_objects: int, views: int, split: str,
                     example_offset: int = 0, aa: int = 3, device="cpu"):
    """``(obj [B] i64, view [B,2] i64, img [B,2,3,H,W] f32, R [B,2,3,3], t
    [B,2,3])`` of a training batch: ``procedural_draw``, then the render of the
    2 B (object, view) pairs."""
    procedural_batch_check(seed, batch_index, B, H, W, n_objects, views, split, example_offset, aa)
    obj, view = procedural_draw(seed, batch_index, B, n_objects=n_objects, views=views, split=split,
                                example_offset=example_offset, device=device)
    img, R, t, _ = procedural_render(seed, obj.repeat_interleave(2), view.reshape(-1), H, W, aa=aa)
    return obj, view, img.reshape(B, 2, 3, H, W), R.reshape(B, 2, 3, 3), t.reshape(B, 2, 3)


# ------------------------------------------------ geometry-aware evaluation ---
# Co-visible PSNR and reprojection consistency on the procedural scenes
# (csrc/consistency.hip holds the rule in full).
VC_STATS = 8
VC_DEPTH_TOL = 1e-9                  # |tau1 - dist|, the bound of test_views_are_3d_consistent


def view_consistency_check(table, K, R_src, t_src, img_src, R_tgt, t_tgt, img_tgt, ref=None):
    """Argument check shared by both backends (ValueError); returns (N, H, W)."""
    name = "view_consistency"
    opt = (("ref", ref),) if ref is not None else ()
    for nm, x in (("table", table), ("K", K), ("R_src", R_src), ("t_src", t_src), ("img_src", img_src),
                  ("R_tgt", R_tgt), ("t_tgt", t_tgt), ("img_tgt", img_tgt)) + opt:
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{name}: {nm} must be a tensor, got {type(x).__name__}")
        if x.device != table.device:
            raise ValueError(f"{name}: {nm} is on {x.device}, the table on {table.device}")
    if table.dim() != 3 or tuple(table.shape[1:]) != (SCENE_SLOTS, SCENE_WORDS):
        raise ValueError(f"{name}: table must be [N,{SCENE_SLOTS},{SCENE_WORDS}], got {tuple(table.shape)}")
    N = table.shape[0]
    for nm, x, shape in (("K", K, (N, 3, 3)), ("R_src", R_src, (N, 3, 3)), ("t_src", t_src, (N, 3)),
                         ("R_tgt", R_tgt, (N, 3, 3)), ("t_tgt", t_tgt, (N, 3))):
        if tuple(x.shape) != shape:
            raise ValueError(f"{name}: {nm} must be {list(shape)} for {N} pairs, got {tuple(x.shape)}")
    for nm, x in (("table", table), ("K", K), ("R_src", R_src), ("t_src", t_src), ("R_tgt", R_tgt), ("t_tgt", t_tgt)):
        if x.dtype != torch.float64:
            raise ValueError(f"{name}: {nm} must be float64, got {x.dtype}")
    if img_tgt.dim() != 4 or img_tgt.shape[0] != N or img_tgt.shape[1] != 3 or min(img_tgt.shape[2:]) < 1:
        raise ValueError(f"{name}: img_tgt must be [{N},3,H,W], got {tuple(img_tgt.shape)}")
    for nm, x in (("img_src", img_src), ("img_tgt", img_tgt)) + opt:
        if x.shape != img_tgt.shape:
            raise ValueError(f"{name}: {nm} must be {list(img_tgt.shape)} like img_tgt, got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise ValueError(f"{name}: {nm} must be float32, got {x.dtype}")
        if not x.is_contiguous():
            raise ValueError(f"{name}: {nm} must be contiguous")
    return N, int(img_tgt.shape[2]), int(img_tgt.shape[3])


def view_consistency(table, K, R_src, t_src, img_src, R_tgt, t_tgt, img_tgt, ref=None, *, return_class=False):
    """stats [N,8] fp64 (and, with ``return_class``, the class plane [N,H,W]
    int32: 0 background, 1 disoccluded, 2 co-visible, 3 clean) of N pairs: the
    float64 torch form of csrc/consistency.hip, which states the rule.  Every
    pixel runs all 15 traces; the kernel's early exits only skip work whose
    result the masks here discard."""
    N, H, W = view_consistency_check(table, K, R_src, t_src, img_src, R_tgt, t_tgt, img_tgt, ref)
    dt, dev = torch.float64, table.device
    e = lambda x: x[:, None, None]  # noqa: E731
    s = torch.tensor([W / SCENE_REF, H / SCENE_REF, 1.0], dtype=dt, device=dev)
    Ks = K * s[None, :, None]
    Kinv = _inv3(Ks)
    prims_t, prims_s = _scene_prims(table, t_tgt), _scene_prims(table, t_src)
    py, px = torch.meshgrid(torch.arange(H, dtype=dt, device=dev), torch.arange(W, dtype=dt, device=dev),
                            indexing="ij")

    def surface(prims, d):
        t, p, _, f = _scene_nearest(prims, d)
        return t, torch.where(p >= 0, 8 * p + f, p)

    d = _scene_dirs(Kinv, R_tgt, px + 0.5, py + 0.5)
    tau, s0 = surface(prims_t, d)
    hit = s0 >= 0
    tau = torch.where(hit, tau, torch.zeros_like(tau))              # (a miss: any finite point; masked below)
    ev = [e(t_tgt[:, k]) + tau * d[k] - e(t_src[:, k]) for k in range(3)]
    dist = torch.sqrt(ev[0] * ev[0] + ev[1] * ev[1] + ev[2] * ev[2])
    c = [e(R_src[:, 0, k]) * ev[0] + e(R_src[:, 1, k]) * ev[1] + e(R_src[:, 2, k]) * ev[2] for k in range(3)]
    kc = [e(Ks[:, k, 0]) * c[0] + e(Ks[:, k, 1]) * c[1] + e(Ks[:, k, 2]) * c[2] for k in range(3)]
    u, v = kc[0] / kc[2], kc[1] / kc[2]
    x0, y0 = torch.floor(u - 0.5), torch.floor(v - 0.5)
    tau1, s1 = surface(prims_s, [x / dist for x in ev])
    inside = (x0 >= 0.0) & (x0 + 1.0 <= float(W - 1)) & (y0 >= 0.0) & (y0 + 1.0 <= float(H - 1))
    cov = hit & (c[2] > 0.0) & inside & ((tau1 - dist).abs() < VC_DEPTH_TOL) & (s1 == s0)
    zero = torch.zeros_like(u)
    x0, y0 = torch.where(cov, x0, zero), torch.where(cov, y0, zero)    # (elsewhere possibly NaN or outside)
    fx, fy = torch.where(cov, (u - 0.5) - x0, zero), torch.where(cov, (v - 0.5) - y0, zero)
    clean = cov
    for k in range(4):
        clean = clean & (surface(prims_t, _scene_dirs(Kinv, R_tgt, px + float(k & 1), py + float(k >> 1)))[1] == s0)
    for k in range(9):
        clean = clean & (surface(prims_s, _scene_dirs(Kinv, R_src, x0 + float(k % 3), y0 + float(k // 3)))[1] == s0)
    klass = hit.to(torch.int32) + cov.to(torch.int32) + clean.to(torch.int32)

    tg = img_tgt.double()
    stats = torch.zeros(N, VC_STATS, dtype=dt, device=dev)
    masks = [~hit, hit & ~cov, cov]
    for j, m in enumerate(masks):
        stats[:, j] = m.flatten(1).sum(1).to(dt)
    stats[:, 3] = clean.flatten(1).sum(1).to(dt)
    if ref is not None:
        se = ((tg - ref.double()) * 0.5).square().sum(1)               # [N,H,W]
        for j, m in enumerate(masks):
            stats[:, 4 + j] = torch.where(m, se, zero).flatten(1).sum(1)
    ix, iy = x0.long(), y0.long()
    flat = img_src.double().flatten(2)                                 # [N,3,HW]

    def take(dy, dx):                                                  # src at (y0 + dy, x0 + dx), [N,3,H,W]
        idx = ((iy + dy) * W + ix + dx).clamp(0, H * W - 1).flatten(1)
        return flat.gather(2, idx[:, None, :].expand(N, 3, H * W)).reshape(N, 3, H, W)

    w00, w01, w10, w11 = (1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy
    warp = w00[:, None] * take(0, 0) + w01[:, None] * take(0, 1) + w10[:, None] * take(1, 0) + w11[:, None] * take(1, 1)
    se = ((tg - warp) * 0.5).square().sum(1)
    stats[:, 7] = torch.where(clean, se, zero).flatten(1).sum(1)
    return (stats, klass) if return_class else stats


# ------------------------------------------------- multi-sample evaluation ---
# Ensemble bias, spread and per-sample error of C samples of one target view,
# per visibility class (csrc/ensemble.hip holds the rule in full).
ES_CLASSES, ES_COLS = 4, 4


def ensemble_stats_check(samples, target, klass=None):
    """Argument check shared by both backends (ValueError); returns (G, C, H, W)."""
    name = "ensemble_stats"
    opt = (("klass", klass),) if klass is not None else ()
    for nm, x in (("samples", samples), ("target", target)) + opt:
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{name}: {nm} must be a tensor, got {type(x).__name__}")
        if x.device != samples.device:
            raise ValueError(f"{name}: {nm} is on {x.device}, the samples on {samples.device}")
    if samples.dim() != 5 or samples.shape[2] != 3 or min(samples.shape[3:]) < 1:
        raise ValueError(f"{name}: samples must be [G,C,3,H,W], got {tuple(samples.shape)}")
    G, C, _, H, W = (int(s) for s in samples.shape)
    if C < 1:
        raise ValueError(f"{name}: needs at least one sample per group, got C = {C}")
    for nm, x, shape, dtype in (("samples", samples, (G, C, 3, H, W), torch.float32),
                                ("target", target, (G, 3, H, W), torch.float32)) + \
            ((("klass", klass, (G, H, W), torch.int32),) if klass is not None else ()):
        if tuple(x.shape) != shape:
            raise ValueError(f"{name}: {nm} must be {list(shape)} for samples {list(samples.shape)}, got "
                             f"{tuple(x.shape)}")
        if x.dtype != dtype:
            raise ValueError(f"{name}: {nm} must be {str(dtype).replace('torch.', '')}, got {x.dtype}")
        if not x.is_contiguous():
            raise ValueError(f"{name}: {nm} must be contiguous")
    return G, C, H, W


def ensemble_stats(samples, target, klass=None, *, quantize=True, return_maps=False):
    """stats [G,4,4] fp64 -- row k = [n_k, sum B, sum V, sum E] over the pixels
    of class k -- and, with ``return_maps``, mean [G,3,H,W] fp32 and std
    [G,H,W] fp32: the float64 torch form of csrc/ensemble.hip, which states the
    rule, written operation by operation in the kernel's order (the sums over
    the samples ascending, the channel sums 0, 1, 2)."""
    G, C, H, W = ensemble_stats_check(samples, target, klass)
    dt, dev = torch.float64, samples.device
    x, y = image_map01(samples, quantize), image_map01(target, quantize)
    s = x[:, 0]
    for c in range(1, C):
        s = s + x[:, c]
    m = s / float(C)                                                    # [G,3,H,W]
    v, e = torch.zeros_like(m), torch.zeros_like(m)
    for c in range(C):
        dv, de = x[:, c] - m, x[:, c] - y
        v = v + dv * dv
        e = e + de * de
    ch = lambda a: (a[:, 0] + a[:, 1]) + a[:, 2]  # noqa: E731
    db = m - y
    B, V, E = ch(db * db), ch(v / float(C)), ch(e / float(C))          # [G,H,W]
    stats = torch.zeros(G, ES_CLASSES, ES_COLS, dtype=dt, device=dev)
    zero = torch.zeros_like(B)
    for k in range(ES_CLASSES):
        mask = (klass == k) if klass is not None else torch.full_like(B, k == 0, dtype=torch.bool)
        stats[:, k, 0] = mask.flatten(1).sum(1).to(dt)
        for j, q in enumerate((B, V, E)):
            stats[:, k, 1 + j] = torch.where(mask, q, zero).flatten(1).sum(1)
    if return_maps:
        return stats, (2.0 * m - 1.0).float(), torch.sqrt(V / 3.0).float()
    return stats


# ------------------------------------------------ radiance-field consistency ---
# A dense voxel radiance field rendered by fixed-step quadrature, its squared
# error against target colours and the gradient on the grid (csrc/field.hip
# holds the rule in full).
FIELD_FIX_BITS = 36                  # the gradient's fixed-point scale, 2^36 (csrc/field.hip)
FIELD_FIX_BUDGET = float(1 << 23)    # R S M <= 2^23: 8 R S M 2^36 <= 2^62 < 2^63
FIELD_T_MAX = 3.0e38                 # the far end before the first slab (finite: no inf arithmetic)


def field_fix_load(R: int, samples: int, bound: float) -> float:
    """``R S M`` of the fixed-point bound: ``M = 6 max(1, delta_max)`` bounds
    one contribution (``|dL/dC| <= 2`` on 3 channels, ``|dC/dsigma| <=
    delta``), ``delta_max = 2 sqrt(3) bound / S`` the longest chord's step."""
    return float(R) * samples * 6.0 * max(1.0, 2.0 * math.sqrt(3.0) * bound / samples)


def field_check(name, grid, rays_o, rays_d, target=None, *, samples, bound, width=0):
    """Argument check shared by both backends (ValueError); returns (G, R)."""
    opt = (("target", target),) if target is not None else ()
    for nm, x in (("grid", grid), ("rays_o", rays_o), ("rays_d", rays_d)) + opt:
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{name}: {nm} must be a tensor, got {type(x).__name__}")
        if x.device != grid.device:
            raise ValueError(f"{name}: {nm} is on {x.device}, the grid on {grid.device}")
        if x.dtype != torch.float32:
            raise ValueError(f"{name}: {nm} must be float32, got {x.dtype}")
        if not x.is_contiguous():
            raise ValueError(f"{name}: {nm} must be contiguous")
    if grid.dim() != 4 or grid.shape[3] != 4 or not grid.shape[0] == grid.shape[1] == grid.shape[2]:
        raise ValueError(f"{name}: grid must be [G,G,G,4], got {tuple(grid.shape)}")
    G = int(grid.shape[0])
    if G < 2:
        raise ValueError(f"{name}: the grid needs at least 2 nodes per axis, got G = {G}")
    if rays_o.dim() != 2 or rays_o.shape[1] != 3:
        raise ValueError(f"{name}: rays_o must be [R,3], got {tuple(rays_o.shape)}")
    R = int(rays_o.shape[0])
    for nm, x in (("rays_d", rays_d),) + opt:
        if tuple(x.shape) != (R, 3):
            raise ValueError(f"{name}: {nm} must be [{R}, 3] as rays_o, got {tuple(x.shape)}")
    if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1:
        raise ValueError(f"{name}: samples must be an integer >= 1, got {samples!r}")
    if not (isinstance(bound, (int, float)) and 0.0 < float(bound) < float("inf")):
        raise ValueError(f"{name}: bound must be a positive finite number, got {bound!r}")
    if isinstance(width, bool) or not isinstance(width, int) or width < 0 or (width > 0 and R % width != 0):
        raise ValueError(f"{name}: width must be 0 or an image width that divides R = {R}, got {width!r}")
    if target is not None and field_fix_load(R, samples, float(bound)) > FIELD_FIX_BUDGET:
        raise ValueError(f"{name}: R * samples = {R * samples} is beyond the gradient's fixed-point range "
                         f"(R S 6 max(1, 2 sqrt(3) bound / S) <= 2^23); split the rays over several calls")
    return G, R


def _field_cells(G: int, o, d, S: int, bound: float, dt):
    """The samples of R rays in ``dt``: (hit [R], delta [R], t_i [R,S], the
    cell's corner (0, 0, 0) i0 [R,S,3] int64 as (ix, iy, iz), the weights
    toward the +1 corners f [R,S,3])."""
    o, d = o.to(dt), d.to(dt)
    b = torch.tensor(bound, dtype=dt, device=o.device)
    t0 = torch.zeros_like(o[:, 0])
    t1 = torch.full_like(t0, FIELD_T_MAX)
    hit = torch.ones_like(t0, dtype=torch.bool)
    for a in range(3):
        zero = d[:, a] == 0
        da = torch.where(zero, torch.ones_like(t0), d[:, a])
        ta, tb = (-b - o[:, a]) / da, (b - o[:, a]) / da
        t0 = torch.where(zero, t0, torch.maximum(t0, torch.minimum(ta, tb)))
        t1 = torch.where(zero, t1, torch.minimum(t1, torch.maximum(ta, tb)))
        hit = hit & (~zero | (o[:, a].abs() <= b))
    hit = hit & (t1 > t0)
    t0 = torch.where(hit, t0, torch.zeros_like(t0))
    delta = torch.where(hit, (t1 - t0) / S, torch.zeros_like(t0))
    ti = t0[:, None] + (torch.arange(S, dtype=dt, device=o.device) + 0.5) * delta[:, None]      # [R,S]
    pos = o[:, None, :] + ti[..., None] * d[:, None, :]                                          # [R,S,3]
    g = ((pos + b) * torch.tensor((G - 1) / (2.0 * bound), dtype=dt, device=o.device)).clamp(0, G - 1)
    i0 = g.detach().floor().clamp(max=G - 2).long()
    return hit, delta, ti, i0, g - i0.to(dt)


def _field_march(grid, o, d, S: int, bound: float, dt):
    """C [R,3] on the [0, 1] scale of csrc/field.hip's rule, in ``dt``."""
    G = grid.shape[0]
    flat = grid.reshape(-1, 4)
    hit, delta, ti, i0, f = _field_cells(G, o, d, S, bound, dt)
    v = torch.zeros(*ti.shape, 4, dtype=dt, device=o.device)
    for k in range(8):                     # corner k = (dz, dy, dx), ascending: the kernel's order
        dz, dy, dx = k >> 2, (k >> 1) & 1, k & 1
        wx = f[..., 0] if dx else 1 - f[..., 0]
        wy = f[..., 1] if dy else 1 - f[..., 1]
        wz = f[..., 2] if dz else 1 - f[..., 2]
        idx = ((i0[..., 2] + dz) * G + (i0[..., 1] + dy)) * G + (i0[..., 0] + dx)
        v = v + ((wz * wy) * wx)[..., None] * flat[idx]
    raw = v[..., 3]
    sigma = raw.clamp(min=0) + torch.log1p(torch.exp(-raw.abs()))
    rgb = torch.sigmoid(v[..., :3])
    alpha = -torch.expm1(-sigma * delta[:, None])
    T = torch.ones_like(delta)
    C = torch.zeros(o.shape, dtype=dt, device=o.device)
    for i in range(S):
        C = C + (T * alpha[:, i])[:, None] * rgb[:, i]
        T = T * (1 - alpha[:, i])
    C = C + T[:, None]
    return torch.where(hit[:, None], C, torch.ones_like(C))


def field_render(grid, rays_o, rays_d, *, samples, bound=1.0, width=0, dtype=torch.float64):
    """C [R,3] fp32 on the [0, 1] scale: the float64 torch form of
    csrc/field.hip (``dtype``: the precision it is evaluated in)."""
    field_check("field_render", grid, rays_o, rays_d, samples=samples, bound=bound, width=width)
    with torch.no_grad():
        return _field_march(grid.to(dtype), rays_o, rays_d, samples, float(bound), dtype).float()


def field_loss_grad(grid, rays_o, rays_d, target, *, samples, bound=1.0, width=0, dtype=torch.float64):
    """(L fp64 scalar, dL/dgrid fp32 [G,G,G,4]): the float64 torch form of
    csrc/field.hip, the gradient by autograd over the composition, rounded to
    fp32 at the end (``dtype``: the precision it is evaluated in)."""
    field_check("field_loss_grad", grid, rays_o, rays_d, target, samples=samples, bound=bound, width=width)
    with torch.enable_grad():
        g = grid.detach().to(dtype).requires_grad_(True)
        C = _field_march(g, rays_o, rays_d, samples, float(bound), dtype)
        L = (C - (target.to(dtype) + 1) * 0.5).square().sum()
        grad, = torch.autograd.grad(L, g)
    return L.detach().double(), grad.float()


# ------------------------------------------------------ batched field fits ---
# One iteration of F independent field fits as two ops: the data term over
# rays drawn by the counter hash, and Adam with a smoothness term on the grid
# (csrc/field_fit.hip holds the rule in full).
FIELD_MAX_BATCH = 65535              # the launch grid's second dimension


def field_draw(seed: int, it: int, n: int, N: int, device=None) -> torch.Tensor:
    """The rays of iteration ``it``: slot s < n takes ``hash_u32(seed, s + it n) % N``
    (with replacement, unsorted, the same for every field)."""
    return hash_u32(seed, torch.arange(n, dtype=torch.int64, device=device) + it * n) % N


def _field_tensors(name, named, dev):
    for nm, x in named:
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{name}: {nm} must be a tensor, got {type(x).__name__}")
        if x.device != dev:
            raise ValueError(f"{name}: {nm} is on {x.device}, the grid on {dev}")
        if x.dtype != torch.float32:
            raise ValueError(f"{name}: {nm} must be float32, got {x.dtype}")
        if not x.is_contiguous():
            raise ValueError(f"{name}: {nm} must be contiguous")


def _field_batch_grid(name, grid):
    if grid.dim() != 5 or grid.shape[4] != 4 or not grid.shape[1] == grid.shape[2] == grid.shape[3]:
        raise ValueError(f"{name}: grid must be [F,G,G,G,4], got {tuple(grid.shape)}")
    F, G = int(grid.shape[0]), int(grid.shape[1])
    if G < 2:
        raise ValueError(f"{name}: the grid needs at least 2 nodes per axis, got G = {G}")
    if F > FIELD_MAX_BATCH:
        raise ValueError(f"{name}: at most {FIELD_MAX_BATCH} fields per call, got {F}")
    return F, G


def _is_int(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


def field_batch_check(name, grid, rays_o, rays_d, target, *, n, it, seed, samples, bound):
    """Argument check shared by both backends (ValueError); returns (F, G, N)."""
    if not isinstance(grid, torch.Tensor):
        raise ValueError(f"{name}: grid must be a tensor, got {type(grid).__name__}")
    _field_tensors(name, (("grid", grid), ("rays_o", rays_o), ("rays_d", rays_d), ("target", target)), grid.device)
    F, G = _field_batch_grid(name, grid)
    if rays_o.dim() != 3 or rays_o.shape[0] != F or rays_o.shape[2] != 3:
        raise ValueError(f"{name}: rays_o must be [{F},N,3], got {tuple(rays_o.shape)}")
    N = int(rays_o.shape[1])
    for nm, x in (("rays_d", rays_d), ("target", target)):
        if tuple(x.shape) != (F, N, 3):
            raise ValueError(f"{name}: {nm} must be [{F}, {N}, 3] as rays_o, got {tuple(x.shape)}")
    if N < 1 or N >= 1 << 31:
        raise ValueError(f"{name}: every field needs between 1 and 2^31 - 1 stored rays, got N = {N}")
    if not _is_int(n) or n < 1 or n >= 1 << 31:
        raise ValueError(f"{name}: n must be an integer >= 1, got {n!r}")
    if not _is_int(it) or it < 0 or it >= 1 << 31:
        raise ValueError(f"{name}: it must be an integer >= 0, got {it!r}")
    if not _is_int(seed):
        raise ValueError(f"{name}: seed must be an integer, got {seed!r}")
    if not _is_int(samples) or samples < 1:
        raise ValueError(f"{name}: samples must be an integer >= 1, got {samples!r}")
    if not (isinstance(bound, (int, float)) and 0.0 < float(bound) < float("inf")):
        raise ValueError(f"{name}: bound must be a positive finite number, got {bound!r}")
    if field_fix_load(n, samples, float(bound)) > FIELD_FIX_BUDGET:
        raise ValueError(f"{name}: n * samples = {n * samples} is beyond the gradient's fixed-point range "
                         f"(n S 6 max(1, 2 sqrt(3) bound / S) <= 2^23 per field); draw fewer rays per iteration")
    return F, G, N


def field_batch_loss_grad(grid, rays_o, rays_d, target, *, n, it, seed, samples, bound=1.0, dtype=torch.float64):
    """(loss fp64 [F], grad fp32 [F,G,G,G,4]): the float64 torch form of
    csrc/field_fit.hip's data term -- per field, :func:`field_loss_grad` on the
    rows :func:`field_draw` names (``dtype``: the precision it is evaluated in)."""
    F, G, N = field_batch_check("field_batch_loss_grad", grid, rays_o, rays_d, target, n=n, it=it, seed=seed,
                                samples=samples, bound=bound)
    idx = field_draw(seed, it, n, N, grid.device)
    loss = torch.zeros(F, dtype=torch.float64, device=grid.device)
    grad = torch.zeros_like(grid)
    for f in range(F):
        loss[f], grad[f] = field_loss_grad(grid[f], rays_o[f][idx], rays_d[f][idx], target[f][idx], samples=samples,
                                           bound=bound, dtype=dtype)
    return loss, grad


def field_tv_grad(grid, tv_rgb: float, tv_sigma: float, dtype=torch.float64):
    """The gradient of ``L_tv = (1 / G^3) sum_c lambda_c sum_edges (v_a - v_b)^2``
    on ``grid`` [...,G,G,G,4] in ``dtype``: ``(2 lambda_c / G^3) sum_neighbours
    (v - v_n)`` over the neighbours inside the grid, in the kernel's order
    x-1, x+1, y-1, y+1, z-1, z+1."""
    v = grid.to(dtype)
    G = v.shape[-2]
    tv = torch.zeros_like(v)
    for dim in (-2, -3, -4):
        lo, hi = v.narrow(dim, 0, G - 1), v.narrow(dim, 1, G - 1)
        tv.narrow(dim, 1, G - 1).add_(hi - lo)
        tv.narrow(dim, 0, G - 1).add_(lo - hi)
    g3 = float(G) ** 3
    coef = torch.tensor([2.0 * tv_rgb / g3] * 3 + [2.0 * tv_sigma / g3], dtype=dtype, device=v.device)
    return coef * tv


def field_adam_tv_math(p, m, v, grad, *, step, lr, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, tv_rgb=0.0,
                       tv_sigma=0.0, dtype=torch.float64):
    """(p', m', v') in ``dtype``: one Adam step in torch's arithmetic order on
    ``grad_scale grad + grad L_tv(p)`` (csrc/field_fit.hip states it)."""
    b1, b2 = float(betas[0]), float(betas[1])
    p, m, v = p.to(dtype), m.to(dtype), v.to(dtype)
    g = grad.to(dtype) * grad_scale + field_tv_grad(p, tv_rgb, tv_sigma, dtype)
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    return p - (lr / (1.0 - b1 ** step)) * (m / denom), m, v


def field_adam_check(name, grid, grid_out, exp_avg, exp_avg_sq, grad, *, step, lr, betas, eps, grad_scale, tv_rgb,
                     tv_sigma):
    """Argument check shared by both backends (ValueError); returns (F, G)."""
    if not isinstance(grid, torch.Tensor):
        raise ValueError(f"{name}: grid must be a tensor, got {type(grid).__name__}")
    named = (("grid", grid), ("grid_out", grid_out), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq), ("grad", grad))
    _field_tensors(name, named, grid.device)
    F, G = _field_batch_grid(name, grid)
    for nm, x in named[1:]:
        if x.shape != grid.shape:
            raise ValueError(f"{name}: {nm} must be {tuple(grid.shape)} as grid, got {tuple(x.shape)}")
    span = [(nm, x.data_ptr(), x.data_ptr() + x.numel() * 4) for nm, x in named if x.numel()]
    for i, (na, a0, a1) in enumerate(span):
        for nb, b0, b1 in span[i + 1:]:
            if a0 < b1 and b0 < a1:
                raise ValueError(f"{name}: {na} and {nb} share memory; the new grid goes to a second buffer "
                                 f"(ping-pong two grids) and every state tensor is its own")
    if not _is_int(step) or step < 1:
        raise ValueError(f"{name}: step counts from 1, got {step!r}")
    try:
        b1, b2 = (float(b) for b in betas)
        scal = {"lr": float(lr), "eps": float(eps), "grad_scale": float(grad_scale), "tv_rgb": float(tv_rgb),
                "tv_sigma": float(tv_sigma)}
    except (TypeError, ValueError):
        raise ValueError(f"{name}: lr, betas, eps, grad_scale, tv_rgb and tv_sigma must be numbers") from None
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"{name}: betas must lie in [0, 1), got {betas!r}")
    for nm, x in scal.items():
        if not math.isfinite(x) or (nm != "grad_scale" and x < 0.0):
            raise ValueError(f"{name}: {nm} must be finite{'' if nm == 'grad_scale' else ' and not negative'}, got {x!r}")
    return F, G


def field_adam_tv(grid, grid_out, exp_avg, exp_avg_sq, grad, *, step, lr, betas=(0.9, 0.999), eps=1e-8,
                  grad_scale=1.0, tv_rgb=0.0, tv_sigma=0.0, dtype=torch.float64):
    """The float64 torch form of csrc/field_fit.hip's update: writes the new
    grid to ``grid_out`` and the moments in place, rounded to fp32 at the end."""
    kw = dict(step=step, lr=lr, betas=betas, eps=eps, grad_scale=grad_scale, tv_rgb=tv_rgb, tv_sigma=tv_sigma)
    field_adam_check("field_adam_tv", grid, grid_out, exp_avg, exp_avg_sq, grad, **kw)
    with torch.no_grad():
        p, m, v = field_adam_tv_math(grid, exp_avg, exp_avg_sq, grad, dtype=dtype, **kw)
        grid_out.copy_(p)
        exp_avg.copy_(m)
        exp_avg_sq.copy_(v)


# ------------------------------------------------------- field geometry ---
# Opacity, depth and normals of fitted fields along camera rays, and their
# score against a procedural scene's true surface (csrc/field_geom.hip holds
# the rule in full).
FG_ROWS, FG_PLANES = 7, 5            # the score row; the map planes (opacity, depth, n_x, n_y, n_z)
FG_HIT = 0.5                         # the field "hits" where its opacity is above this


def field_geometry_check(grid, K, R, t, H, W, *, samples, bound, rescale_from, table, return_maps):
    """Argument check shared by both backends (ValueError); returns (F, V, G)."""
    name = "field_geometry"
    if not isinstance(grid, torch.Tensor):
        raise ValueError(f"{name}: grid must be a tensor, got {type(grid).__name__}")
    _field_tensors(name, (("grid", grid),), grid.device)
    F, G = _field_batch_grid(name, grid)
    if not isinstance(R, torch.Tensor) or R.dim() != 4 or tuple(R.shape[2:]) != (3, 3) or R.shape[0] != F:
        raise ValueError(f"{name}: R must be a tensor [{F},V,3,3], got "
                         f"{tuple(R.shape) if isinstance(R, torch.Tensor) else type(R).__name__}")
    V = int(R.shape[1])
    named = (("K", K, (F, 3, 3)), ("R", R, (F, V, 3, 3)), ("t", t, (F, V, 3)))
    if table is not None:
        named += (("table", table, (F, SCENE_SLOTS, SCENE_WORDS)),)
    for nm, x, shape in named:
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{name}: {nm} must be a tensor, got {type(x).__name__}")
        if tuple(x.shape) != shape:
            raise ValueError(f"{name}: {nm} must be {list(shape)} for {F} fields of {V} views, got {tuple(x.shape)}")
        if x.dtype != torch.float64:
            raise ValueError(f"{name}: {nm} must be float64, got {x.dtype}")
        if x.device != grid.device:
            raise ValueError(f"{name}: {nm} is on {x.device}, the grid on {grid.device}")
    for nm, v, lo in (("H", H, 1), ("W", W, 1), ("samples", samples, 1), ("rescale_from", rescale_from, 0)):
        if not _is_int(v) or v < lo:
            raise ValueError(f"{name}: {nm} must be an integer >= {lo}, got {v!r}")
    if V > FIELD_MAX_BATCH or H * W >= 1 << 31:
        raise ValueError(f"{name}: at most {FIELD_MAX_BATCH} views per field and 2^31 - 1 pixels per view, got "
                         f"{V} views of {H} x {W}")
    if not (isinstance(bound, (int, float)) and 0.0 < float(bound) < float("inf")):
        raise ValueError(f"{name}: bound must be a positive finite number, got {bound!r}")
    if table is None and not return_maps:
        raise ValueError(f"{name}: without a table there are no scores: pass return_maps=True")
    return F, V, G


def field_geometry(grid, K, R, t, H, W, *, samples, bound=1.0, rescale_from=128, table=None, return_maps=False,
                   dtype=torch.float64):
    """scores fp64 [F,V,7] (with a table) and maps fp32 [F,V,5,H,W] (with
    ``return_maps``): the torch form of csrc/field_geom.hip, which states the
    rule.  The rays and the truth are float64 whatever ``dtype`` is; the walk
    through the field -- from the ray rounded to fp32 -- the opacity, depth
    and normal are evaluated in ``dtype`` (float64: the CPU path and the
    kernel's oracle)."""
    return _field_geometry(grid, K, R, t, H, W, samples=samples, bound=bound, rescale_from=rescale_from, table=table,
                           return_maps=return_maps, dtype=dtype)


def _field_geometry(grid, K, R, t, H, W, *, samples, bound, rescale_from, table, return_maps, dtype, cond=None):
    """:func:`field_geometry`; ``cond`` (a dict) also receives how well a
    pixel's values are conditioned, each [F,V,H,W] in ``dtype``: ``gnorm``,
    ``|g|`` before the normalisation; ``face``, the smallest distance in grid
    units of one of the ray's samples from a cell face, where the gradient
    jumps; and with a table ``n_true`` [F,V,3,H,W] fp64, the true normals."""
    F, V, G = field_geometry_check(grid, K, R, t, H, W, samples=samples, bound=bound, rescale_from=rescale_from,
                                   table=table, return_maps=return_maps)
    dt, dev, S, bound = torch.float64, grid.device, int(samples), float(bound)
    ref = float(rescale_from) if rescale_from else None
    s = torch.tensor([W / ref, H / ref, 1.0] if ref else [1.0, 1.0, 1.0], dtype=dt, device=dev)
    py, px = torch.meshgrid(torch.arange(H, dtype=dt, device=dev), torch.arange(W, dtype=dt, device=dev),
                            indexing="ij")
    scale = torch.tensor((G - 1) / (2.0 * bound), dtype=dtype, device=dev)
    e = lambda x: x[:, None, None]  # noqa: E731
    scores = torch.zeros(F, V, FG_ROWS, dtype=dt, device=dev)
    maps = torch.zeros(F, V, FG_PLANES, H, W, dtype=torch.float32, device=dev)
    if cond is not None:
        cond.update(gnorm=torch.zeros(F, V, H, W, dtype=dtype, device=dev),
                    face=torch.zeros(F, V, H, W, dtype=dtype, device=dev),
                    n_true=torch.zeros(F, V, 3, H, W, dtype=dt, device=dev))
    with torch.no_grad():
        for f in range(F):
            Kinv = _inv3((K[f] * s[:, None])[None]).expand(V, 3, 3)
            d = _scene_dirs(Kinv, R[f], px + 0.5, py + 0.5)                        # 3 x [V,H,W] fp64
            o32 = t[f].float()[:, None, :].expand(V, H * W, 3).reshape(-1, 3)
            d32 = torch.stack(d, -1).float().reshape(-1, 3)
            hit, delta, ti, i0, fr = _field_cells(G, o32, d32, S, bound, dtype)
            sig = grid[f].reshape(-1, 4)[:, 3].to(dtype)
            raw = torch.zeros_like(ti)
            gr = [torch.zeros_like(ti) for _ in range(3)]
            for k in range(8):             # corner k = (dz, dy, dx), ascending: the kernel's order
                dz, dy, dx = k >> 2, (k >> 1) & 1, k & 1
                wx = fr[..., 0] if dx else 1 - fr[..., 0]
                wy = fr[..., 1] if dy else 1 - fr[..., 1]
                wz = fr[..., 2] if dz else 1 - fr[..., 2]
                v = sig[((i0[..., 2] + dz) * G + (i0[..., 1] + dy)) * G + (i0[..., 0] + dx)]
                raw = raw + ((wz * wy) * wx) * v
                gr[0] = gr[0] + (wz * wy) * (v if dx else -v)
                gr[1] = gr[1] + (wz * wx) * (v if dy else -v)
                gr[2] = gr[2] + (wy * wx) * (v if dz else -v)
            sigma = raw.clamp(min=0) + torch.log1p(torch.exp(-raw.abs()))
            alpha = -torch.expm1(-sigma * delta[:, None])
            T = torch.ones_like(delta)
            A, Dn = torch.zeros_like(delta), torch.zeros_like(delta)
            g = [torch.zeros_like(delta) for _ in range(3)]
            for i in range(S):
                w = T * alpha[:, i]
                A = A + w
                Dn = Dn + w * ti[:, i]
                g = [g[a] + w * (gr[a][:, i] * scale) for a in range(3)]
                T = T * (1 - alpha[:, i])
            P = hit & (A > FG_HIT)
            zero = torch.zeros_like(A)
            A = torch.where(hit, A, zero)
            D = torch.where(P, Dn / torch.where(P, A, torch.ones_like(A)), torch.full_like(A, float("inf")))
            gn = torch.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            ok = P & (gn > 0)
            n = [torch.where(ok, -g[a] / torch.where(ok, gn, torch.ones_like(gn)), zero) for a in range(3)]
            planes = [x.reshape(V, H, W) for x in (A, D, *n)]
            maps[f] = torch.stack(planes, 1).float()
            if cond is not None:
                cond["gnorm"][f] = gn.reshape(V, H, W)
                cond["face"][f] = torch.minimum(fr, 1 - fr).flatten(1).min(1).values.reshape(V, H, W)
            if table is None:
                continue
            prims = _scene_prims(table[f][None].expand(V, SCENE_SLOTS, SCENE_WORDS), t[f])
            ts, prim, nl, _ = _scene_nearest(prims, d)
            M = prim >= 0
            ns = [torch.zeros_like(ts) for _ in range(3)]
            for p, (Am, _, _, _) in enumerate(prims):                  # n* = normalize(A^T n_local), as scene_shade
                w = [e(Am[:, 0, k]) * nl[0] + e(Am[:, 1, k]) * nl[1] + e(Am[:, 2, k]) * nl[2] for k in range(3)]
                wn = torch.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
                ns = [torch.where(prim == p, w[k] / wn, ns[k]) for k in range(3)]
            if cond is not None:
                cond["n_true"][f] = torch.stack(ns, 1)
            Ad, Dd, nd = planes[0].to(dt), planes[1].to(dt), [x.to(dt) for x in planes[2:]]
            Pm = P.reshape(V, H, W)
            both = M & Pm
            z = torch.zeros_like(ts)
            df = torch.where(both, Dd - torch.where(both, ts, z), z)
            cos = (nd[0] * ns[0] + nd[1] * ns[1]) + nd[2] * ns[2]
            sil = Ad - M.to(dt)
            for k, q in enumerate((M.to(dt), Pm.to(dt), both.to(dt), df.abs(), df * df,
                                   torch.where(both, 1.0 - cos, z), sil * sil)):
                scores[f, :, k] = q.flatten(1).sum(1)
    if table is None:
        return maps
    return (scores, maps) if return_maps else scores


# ------------------------------------------------ depth reprojection score ---
# Consistency between the views of one object under per-view depth planes
# (csrc/depth_consistency.hip holds the rule in full).
DC_STATS, DC_MAX_VIEWS = 7, 64


def depth_consistency_check(depth, images, K, R, t, *, tol, rescale_from):
    """Argument check shared by both backends (ValueError); returns (F, V, H, W)."""
    name = "depth_consistency"
    for nm, x in (("depth", depth), ("images", images), ("K", K), ("R", R), ("t", t)):
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{name}: {nm} must be a tensor, got {type(x).__name__}")
        if x.device != depth.device:
            raise ValueError(f"{name}: {nm} is on {x.device}, the depth on {depth.device}")
        if not x.is_contiguous():
            raise ValueError(f"{name}: {nm} must be contiguous")
    if depth.dim() != 4 or min(depth.shape[1:]) < 1:
        raise ValueError(f"{name}: depth must be [F,V,H,W] with V, H, W >= 1, got {tuple(depth.shape)}")
    F, V, H, W = (int(s) for s in depth.shape)
    for nm, x, shape, dtype in (("depth", depth, (F, V, H, W), torch.float32),
                                ("images", images, (F, V, 3, H, W), torch.float32), ("K", K, (F, 3, 3), torch.float64),
                                ("R", R, (F, V, 3, 3), torch.float64), ("t", t, (F, V, 3), torch.float64)):
        if tuple(x.shape) != shape:
            raise ValueError(f"{name}: {nm} must be {list(shape)} like the depth, got {tuple(x.shape)}")
        if x.dtype != dtype:
            raise ValueError(f"{name}: {nm} must be {dtype}, got {x.dtype}")
    if V > DC_MAX_VIEWS or H * W >= 1 << 31:
        raise ValueError(f"{name}: at most {DC_MAX_VIEWS} views per field and 2^31 - 1 pixels per view, got {V} views "
                         f"of {H} x {W}")
    if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not 0.0 < float(tol) < float("inf"):
        raise ValueError(f"{name}: tol must be a positive finite number, got {tol!r}")
    if not _is_int(rescale_from) or rescale_from < 0:
        raise ValueError(f"{name}: rescale_from must be an integer >= 0, got {rescale_from!r}")
    return F, V, H, W


def depth_consistency(depth, images, K, R, t, *, tol, rescale_from=128, return_class=False):
    """stats fp64 [F,V,V,7] (and, with ``return_class``, the class planes
    [F,V,V,H,W] int32: 0 background, 1 hidden, 2 co-visible, 3 clean, -1 on the
    diagonal) of the ordered view pairs [f, target, source]: the float64 torch
    form of csrc/depth_consistency.hip, which states the rule.  The CPU path
    and the kernel's oracle."""
    return _depth_consistency(depth, images, K, R, t, tol=tol, rescale_from=rescale_from, return_class=return_class)


def _depth_consistency(depth, images, K, R, t, *, tol, rescale_from, return_class, cond=None):
    """:func:`depth_consistency`; ``cond`` (a dict) also receives ``margin``,
    the smallest relative distance of one of the rule's decisions from its
    threshold over all pixels where that decision is taken: the ``tol`` tests
    (of q_n, of the q_k of co-visible pixels, of the neighbour depths) against
    ``tol dist`` / ``tol D``, the ``floor`` arguments against the nearest
    integer, ``fx`` / ``fy`` against 1/2 and ``c_z`` against 0 (over dist)."""
    F, V, H, W = depth_consistency_check(depth, images, K, R, t, tol=tol, rescale_from=rescale_from)
    dt, dev, tol = torch.float64, depth.device, float(tol)
    ref = float(rescale_from) if rescale_from else None
    s = torch.tensor([W / ref, H / ref, 1.0] if ref else [1.0, 1.0, 1.0], dtype=dt, device=dev)
    py, px = torch.meshgrid(torch.arange(H, dtype=dt, device=dev), torch.arange(W, dtype=dt, device=dev),
                            indexing="ij")
    stats = torch.zeros(F, V, V, DC_STATS, dtype=dt, device=dev)
    cls = torch.full((F, V, V, H, W), -1, dtype=torch.int32, device=dev)
    margin = [float("inf")]

    def near(x, mask):                           # the decisions' distances from their thresholds
        if cond is not None and bool(mask.any()):
            margin[0] = min(margin[0], float(x[mask].abs().min()))

    off = ~torch.eye(V, dtype=torch.bool, device=dev)[:, :, None, None]
    src = lambda x: x[None, :, None, None]       # noqa: E731  per source view
    for f in range(F):
        Ks = K[f] * s[:, None]
        d = _scene_dirs(_inv3(Ks[None]).expand(V, 3, 3), R[f], px + 0.5, py + 0.5)         # 3 x [V,H,W]
        Dp = depth[f].to(dt)
        hit = torch.isfinite(Dp)
        D = torch.where(hit, Dp, torch.zeros_like(Dp))           # (a miss: any finite point; masked below)
        X = [t[f, :, k, None, None] + D * d[k] for k in range(3)]
        smooth = torch.ones_like(hit)
        lo, hi, al = slice(None, -1), slice(1, None), slice(None)
        for sl_p, sl_n in (((..., hi), (..., lo)), ((..., lo), (..., hi)),             # the pixel, its neighbour
                           ((..., hi, al), (..., lo, al)), ((..., lo, al), (..., hi, al))):
            fin, dn, lim = hit[sl_n], (Dp[sl_n] - D[sl_p]).abs(), tol * D[sl_p]
            smooth[sl_p] &= fin & (dn <= lim)
            near((dn - lim) / lim, hit[sl_p] & fin)
        P = [[Ks[i, 0] * R[f, :, j, 0] + Ks[i, 1] * R[f, :, j, 1] + Ks[i, 2] * R[f, :, j, 2] for j in range(3)]
             for i in range(3)]                                   # P_b = Ks R_b^T, [V] each
        e = [X[k][:, None] - src(t[f, :, k]) for k in range(3)]  # [Va,Vb,H,W]
        dist = torch.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
        cz = src(R[f, :, 0, 2]) * e[0] + src(R[f, :, 1, 2]) * e[1] + src(R[f, :, 2, 2]) * e[2]
        kc = [src(P[i][0]) * e[0] + src(P[i][1]) * e[1] + src(P[i][2]) * e[2] for i in range(3)]
        u, v = kc[0] / kc[2], kc[1] / kc[2]
        x0, y0 = torch.floor(u - 0.5), torch.floor(v - 0.5)
        inside = (x0 >= 0.0) & (x0 + 1.0 <= float(W - 1)) & (y0 >= 0.0) & (y0 + 1.0 <= float(H - 1))
        seen = hit[:, None] & off & (cz > 0.0) & inside
        zero = torch.zeros_like(u)
        near(cz / dist, (hit[:, None] & off).expand_as(cz))
        front = hit[:, None] & off & (cz > 0.0)
        for w_ in (u - 0.5, v - 0.5):
            near((w_ - torch.round(w_)) / w_.abs().clamp_min(1.0), front & torch.isfinite(w_))
        x0, y0 = torch.where(seen, x0, zero), torch.where(seen, y0, zero)      # (elsewhere possibly NaN or outside)
        fx, fy = torch.where(seen, (u - 0.5) - x0, zero), torch.where(seen, (v - 0.5) - y0, zero)
        near(fx - 0.5, seen)
        near(fy - 0.5, seen)
        base = (torch.arange(V, device=dev) * (H * W))[None, :, None, None] + y0.long() * W + x0.long()
        take = lambda plane, dy, dx: plane[(base + (dy * W + dx)).clamp(0, V * H * W - 1)]   # noqa: E731
        dflat = Dp.reshape(-1)
        q = [take(dflat, 0, 0), take(dflat, 0, 1), take(dflat, 1, 0), take(dflat, 1, 1)]
        qn = torch.where(fy >= 0.5, torch.where(fx >= 0.5, q[3], q[2]), torch.where(fx >= 0.5, q[1], q[0]))
        lim = tol * dist
        ok = lambda x: torch.isfinite(x) & ((dist - x).abs() <= lim)           # noqa: E731
        cov = seen & ok(qn)
        near(((dist - qn).abs() - lim) / lim, seen & torch.isfinite(qn))
        clean = cov & smooth[:, None]
        for x in q:
            clean = clean & ok(x)
            near(((dist - x).abs() - lim) / lim, cov & torch.isfinite(x))
        w00, w01, w10, w11 = (1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy
        se = torch.zeros_like(u)
        for c in range(3):
            plane = images[f, :, c].to(dt).reshape(-1)
            warp = w00 * take(plane, 0, 0) + w01 * take(plane, 0, 1) + w10 * take(plane, 1, 0) + w11 * take(plane, 1, 1)
            r = (images[f, :, c].to(dt)[:, None] - warp) * 0.5
            se = se + r * r
        qbar = w00 * q[0] + w01 * q[1] + w10 * q[2] + w11 * q[3]
        bg, hid = (~hit)[:, None] & off, hit[:, None] & off & ~cov
        for k, m in enumerate((bg, hid, cov, clean)):
            stats[f, :, :, k] = m.flatten(2).sum(2).to(dt)
        stats[f, :, :, 4] = torch.where(cov, se, zero).flatten(2).sum(2)
        stats[f, :, :, 5] = torch.where(clean, se, zero).flatten(2).sum(2)
        stats[f, :, :, 6] = torch.where(clean, (dist - qbar).abs(), zero).flatten(2).sum(2)
        klass = (hit[:, None] & off).to(torch.int32) + cov.to(torch.int32) + clean.to(torch.int32)
        cls[f] = torch.where(off.expand_as(klass), klass, cls[f])
    if cond is not None:
        cond["margin"] = margin[0]
    return (stats, cls) if return_class else stats


# -------------------------------------------- sliced Wasserstein distance ---
# The distance between two image sets on Laplacian-pyramid patches (Karras et
# al. 2018), one number per pyramid level (csrc/swd.hip holds the rule in full).
SWD_PATCH = 7                        # patch side
SWD_DIM = 3 * SWD_PATCH * SWD_PATCH  # descriptor length, 147
SWD_MAX_N = 16384                    # descriptors per set and level: both sets' fp32 keys in one workgroup's LDS
SWD_MAX_SIDE = 128
SWD_K_PATCH, SWD_K_DIR = 0x1234567, 0x7654321
_SWD_TAPS = (1.0, 4.0, 6.0, 4.0, 1.0)


def swd_default_levels(H: int, W: int) -> int:
    """The largest L whose coarsest level has both sides >= 16 (at least 1)."""
    L = 1
    while H % (1 << L) == 0 and W % (1 << L) == 0 and min(H, W) >> L >= 16:
        L += 1
    return L


def swd_directions(seed: int, levels: int, dirs: int, device="cpu") -> torch.Tensor:
    """fp64 ``[levels, dirs, 147]`` unit vectors: ``normal01(seed ^ 0x7654321,
    (l * dirs + k) * 147 + j)`` upcast and divided by its fp64 norm.  Built on
    the CPU (one rule for both backends: the kernel takes it as a tensor)."""
    if int(levels) < 1 or int(dirs) < 1:
        raise ValueError(f"swd_directions: levels and dirs must be at least 1, got {levels} and {dirs}")
    idx = torch.arange(int(levels) * int(dirs) * SWD_DIM, dtype=torch.int64)
    g = normal01((int(seed) ^ SWD_K_DIR) & _M64, idx).double().view(int(levels), int(dirs), SWD_DIM)
    return (g / g.square().sum(-1, keepdim=True).sqrt()).contiguous().to(device)


def sliced_wasserstein_check(a, b, dirs, *, levels, patches, seed):
    """Argument check shared by both backends (ValueError); returns (N, H, W, L, P, D)."""
    name = "sliced_wasserstein"
    for nm, x in (("a", a), ("b", b), ("dirs", dirs)):
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{name}: {nm} must be a tensor, got {type(x).__name__}")
        if x.device != a.device:
            raise ValueError(f"{name}: {nm} is on {x.device}, a on {a.device}")
    if a.dim() != 4 or a.shape[1] != 3 or a.shape[0] < 1:
        raise ValueError(f"{name}: a must be [N,3,H,W] with N >= 1, got {tuple(a.shape)}")
    N, _, H, W = (int(s) for s in a.shape)
    if isinstance(levels, bool) or not isinstance(levels, int) or levels < 1:
        raise ValueError(f"{name}: levels must be an integer >= 1, got {levels!r}")
    if isinstance(patches, bool) or not isinstance(patches, int) or patches < 1:
        raise ValueError(f"{name}: patches must be an integer >= 1, got {patches!r}")
    if not isinstance(seed, int) or isinstance(seed, bool):
        raise ValueError(f"{name}: seed must be an integer, got {seed!r}")
    L, P = levels, patches
    if max(H, W) > SWD_MAX_SIDE or H % (1 << (L - 1)) or W % (1 << (L - 1)) or \
            min(H, W) >> (L - 1) < SWD_PATCH:
        raise ValueError(f"{name}: H and W must be at most {SWD_MAX_SIDE}, divisible by 2^(levels - 1) and at least "
                         f"{SWD_PATCH} at the coarsest level, got {H} x {W} with levels = {L}")
    if N * P > SWD_MAX_N:
        raise ValueError(f"{name}: N * patches = {N * P} descriptors per set, at most {SWD_MAX_N} fit: use fewer "
                         f"patches per image")
    if dirs.dim() != 3 or dirs.shape[0] != L or dirs.shape[1] < 1 or dirs.shape[2] != SWD_DIM:
        raise ValueError(f"{name}: dirs must be [{L},D,{SWD_DIM}] with D >= 1, got {tuple(dirs.shape)}")
    for nm, x, shape, dtype in (("a", a, (N, 3, H, W), torch.float32), ("b", b, (N, 3, H, W), torch.float32),
                                ("dirs", dirs, tuple(dirs.shape), torch.float64)):
        if tuple(x.shape) != shape:
            raise ValueError(f"{name}: {nm} must be {list(shape)} as a is, got {tuple(x.shape)}")
        if x.dtype != dtype:
            raise ValueError(f"{name}: {nm} must be {str(dtype).replace('torch.', '')}, got {x.dtype}")
        if not x.is_contiguous():
            raise ValueError(f"{name}: {nm} must be contiguous")
    return N, H, W, L, P, int(dirs.shape[1])


def _swd_blur(x: torch.Tensor, gain: float) -> torch.Tensor:
    """The separable 5-tap [1,4,6,4,1] / 16 blur of [...,H,W] with reflect
    borders, along W and then along H, taps ascending, times ``gain``."""
    import torch.nn.functional as F
    shape = x.shape
    x = x.reshape(-1, 1, shape[-2], shape[-1])
    d = 16.0 / math.sqrt(gain)
    p = F.pad(x, (2, 2, 0, 0), mode="reflect")
    s = _SWD_TAPS[0] * p[..., 0:shape[-1]]
    for k in range(1, 5):
        s = s + _SWD_TAPS[k] * p[..., k:k + shape[-1]]
    p = F.pad(s / d, (0, 0, 2, 2), mode="reflect")
    s = _SWD_TAPS[0] * p[..., 0:shape[-2], :]
    for k in range(1, 5):
        s = s + _SWD_TAPS[k] * p[..., k:k + shape[-2], :]
    return (s / d).reshape(shape)


def swd_laplacian(x: torch.Tensor, levels: int) -> list:
    """The Laplacian pyramid of fp64 planes [...,H,W]: ``levels`` tensors, the
    last the coarsest Gaussian level."""
    g = [x]
    for _ in range(levels - 1):
        g.append(_swd_blur(g[-1], 1.0)[..., ::2, ::2])
    out = []
    for l in range(levels - 1):
        z = torch.zeros_like(g[l])
        z[..., ::2, ::2] = g[l + 1]
        out.append(g[l] - _swd_blur(z, 4.0))
    return out + [g[-1]]


def swd_corners(seed: int, l: int, N: int, P: int, Hl: int, Wl: int, device="cpu"):
    """(x0, y0) int64 [N * P] of level ``l``'s patches, image-major."""
    q = (l * N * P + torch.arange(N * P, dtype=torch.int64, device=device))
    s = (int(seed) ^ SWD_K_PATCH) & _M64
    return hash_u32(s, 2 * q) % (Wl - SWD_PATCH + 1), hash_u32(s, 2 * q + 1) % (Hl - SWD_PATCH + 1)


def sliced_wasserstein(a, b, *, dirs, levels, patches, seed, quantize=True, return_kmax=False):
    """swd fp64 [L]: the float64 torch form of csrc/swd.hip, which states the
    rule -- the keys are NOT rounded to fp32 here (this is the oracle; the
    kernel's one rounding is within ``2^-23 kmax``).  ``return_kmax``: also the
    largest ``|key|`` per level, fp64 [L]."""
    N, H, W, L, P, D = sliced_wasserstein_check(a, b, dirs, levels=levels, patches=patches, seed=seed)
    dev, n = a.device, N * P
    lap = [swd_laplacian(image_map01(x, quantize), L) for x in (a, b)]
    img = torch.arange(N, device=dev).repeat_interleave(P)[:, None, None, None]
    ch = torch.arange(3, device=dev)[None, :, None, None]
    ar = torch.arange(SWD_PATCH, device=dev)
    swd = torch.zeros(L, dtype=torch.float64, device=dev)
    kmax = torch.zeros(L, dtype=torch.float64, device=dev)
    for l in range(L):
        Hl, Wl = H >> l, W >> l
        x0, y0 = swd_corners(seed, l, N, P, Hl, Wl, dev)
        yy = (y0[:, None] + ar)[:, None, :, None]
        xx = (x0[:, None] + ar)[:, None, None, :]
        keys = []
        for s in range(2):
            v = lap[s][l][img, ch, yy, xx]                                  # [n,3,7,7]
            mu = v.mean(dim=(0, 2, 3), keepdim=True)
            sd = (v - mu).square().mean(dim=(0, 2, 3), keepdim=True).sqrt()
            inv = torch.where(sd > 0, 1.0 / torch.where(sd > 0, sd, torch.ones_like(sd)), torch.zeros_like(sd))
            keys.append(((v - mu) * inv).reshape(n, SWD_DIM) @ dirs[l].t())    # [n,D]
        kmax[l] = torch.maximum(keys[0].abs().max(), keys[1].abs().max())
        diff = (keys[0].sort(0).values - keys[1].sort(0).values).abs()
        swd[l] = (diff.sum(0) / n).sum() / D
    return (swd, kmax) if return_kmax else swd


# ------------------------------------------------------- exact image k-NN ---
KNN_MAX_K = 8
KNN_MAX_D = 131071                   # D 2^14 < 2^31: the kernel's int32 accumulators and row norms cannot overflow


def image_map_u8(x: torch.Tensor) -> torch.Tensor:
    """[-1, 1] fp32 -> the uint8 value ``sampling.py:save_png`` writes (fp32
    add, fp32 multiply, truncation): the integer form of ``image_map01``."""
    return ((x.float().clamp(-1.0, 1.0) + 1.0) * 127.5).to(torch.uint8)


def image_knn_check(a, b, *, k, exclude_self, radius):
    """Argument check shared by both backends (ValueError); returns (N, M, D)."""
    name = "image_knn"
    for nm, x in (("a", a), ("b", b)):
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{name}: {nm} must be a tensor, got {type(x).__name__}")
        if x.dim() != 4 or x.shape[1] != 3 or min(x.shape) < 1:
            raise ValueError(f"{name}: {nm} must be a non-empty [n,3,H,W] tensor, got {tuple(x.shape)}")
        if x.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"{name}: {nm} must be float32 in [-1, 1] or uint8, got {x.dtype}")
    if b.device != a.device or a.shape[1:] != b.shape[1:]:
        raise ValueError(f"{name}: a and b must share a device and [3,H,W], got {tuple(a.shape)} on {a.device} and "
                         f"{tuple(b.shape)} on {b.device}")
    N, M, D = int(a.shape[0]), int(b.shape[0]), int(a.shape[1] * a.shape[2] * a.shape[3])
    if D > KNN_MAX_D:
        raise ValueError(f"{name}: 3 H W = {D} is above {KNN_MAX_D}, the limit of the exact int32 accumulation")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"{name}: k must be an integer in 1 .. {KNN_MAX_K}, got {k!r}")
    if k > M - (1 if exclude_self else 0):
        raise ValueError(f"{name}: k = {k} neighbours among {M} candidates" + (" without self" if exclude_self else ""))
    if radius is not None:
        if not isinstance(radius, torch.Tensor) or radius.dtype != torch.int64 or tuple(radius.shape) != (M,) \
                or radius.device != a.device:
            raise ValueError(f"{name}: radius must be an int64 [{M}] tensor on {a.device}")
    return N, M, D


def image_knn(a, b, *, k, exclude_self=False, radius=None, chunk=2048):
    """(d2 [N,k], idx [N,k][, inside [N]]) int64: the torch form of
    csrc/knn.hip, which states the rule.  The distances are exact integers:
    the shifted bytes ``u - 128`` are multiplied in float64, where every
    partial sum is an integer below 2^53, over chunks of ``b``; the running
    best k and the chunk are ranked by a stable sort on d2 with the lower
    indices first, which is the total order on (d2, j)."""
    N, M, D = image_knn_check(a, b, k=k, exclude_self=exclude_self, radius=radius)
    dev = a.device

    def shifted(x):
        u = x if x.dtype == torch.uint8 else image_map_u8(x)
        return u.reshape(x.shape[0], D).double() - 128.0

    sa = shifted(a)
    na = (sa * sa).sum(1).long()
    rows = torch.arange(N, device=dev)[:, None]
    best_d = torch.empty(N, 0, dtype=torch.int64, device=dev)
    best_i = torch.empty(N, 0, dtype=torch.int64, device=dev)
    inside = torch.zeros(N, dtype=torch.int64, device=dev)
    for j0 in range(0, M, chunk):
        sb = shifted(b[j0:j0 + chunk])
        j = torch.arange(j0, j0 + sb.shape[0], device=dev)[None, :]
        d2 = na[:, None] + (sb * sb).sum(1).long()[None, :] - 2 * (sa @ sb.t()).long()
        skip = (j == rows) if exclude_self else torch.zeros_like(d2, dtype=torch.bool)
        if radius is not None:
            inside += ((d2 <= radius[j0:j0 + sb.shape[0]][None, :]) & ~skip).sum(1)
        cand_d = torch.cat([best_d, d2.masked_fill(skip, 1 << 62)], 1)
        cand_i = torch.cat([best_i, j.expand(N, -1)], 1)
        cand_d, order = cand_d.sort(dim=1, stable=True)
        best_d, best_i = cand_d[:, :k].contiguous(), cand_i.gather(1, order[:, :k])
    return (best_d, best_i) if radius is None else (best_d, best_i, inside)
