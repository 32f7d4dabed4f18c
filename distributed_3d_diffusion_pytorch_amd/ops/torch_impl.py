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
    c = x.float().clamp(-1.0, 1.0)
    if quantize:
        return ((c + 1.0) * 127.5).to(torch.uint8).double() / 255.0
    return (c.double() + 1.0) * 0.5


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
