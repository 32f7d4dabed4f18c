"""Evaluation: novel-view synthesis scored against ground truth (the 3DiM
protocol) and the held-out training loss.

For every held-out object one input view is given and the listed target views
are generated -- with ``autoregressive`` each generated view joins the object's
record (stochastic conditioning), otherwise every view is generated from the
input view alone.  Up to ``batch`` objects run as ONE graph-replayed sampler
step (:meth:`DiffusionSampler.sample_groups`: one chain per (object, guidance
weight), the conditioning computed once per object and class), and the results
are scored on the device by ``ops.image_metrics(quantize=True)``, i.e. exactly
as the PNGs a writer would store.  Objects that carry their geometry (the
procedural scenes) can also be scored with it: ``ops.view_consistency`` splits
every generated view into background, disoccluded and co-visible pixels and
measures how well the views reproject into each other.  With ``samples`` > 1
every (object, guidance weight) runs that many independent chains and
``ops.ensemble_stats`` scores them as an ensemble: the error of their mean
image, their spread, and both by visibility class.  Single process.
"""
from __future__ import annotations

import math
import os
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import torch

from .. import ops
from .sampler import DiffusionSampler, RecordEntry

_VAL_KEY = 0x76616C6964617465      # "validate": keeps the validation draw apart from every training step's
_M64 = (1 << 64) - 1


# ------------------------------------------------------------ held-out loss
def validation_seed(seed: int, i: int) -> int:
    """RNG seed of validation batch ``i``: a function of (seed, the validation
    constant, i) only, so every call scores the same (t, eps, CFG-drop) draw."""
    base = (int(seed) * 0x2545F4914F6CDD1D + _VAL_KEY) & _M64
    return (base + (i + 1) * 0x9E3779B97F4A7C15) & _M64


@torch.no_grad()
def heldout_loss(model, batches: Iterable, seed: int, diffusion_cfg, dtype, bins=None) -> torch.Tensor:
    """Mean training loss (``ops.diffusion_inputs`` -> forward ->
    ``ops.diff_loss_nhwc``) of ``model`` in eval mode over ``batches`` of
    (img [B,2,3,H,W], R, T, K) on the model's device -- the configured
    objective: the target of ``diffusion_cfg.prediction`` under its
    ``loss_weight`` -- batch i drawn with
    ``validation_seed(seed, i)``.  ``bins``: an fp64 [NB,5] table on the
    model's device that every batch is added to (``ops.diff_loss_rows`` ->
    ``ops.loss_bins_add``: the loss by noise level).  Returns a device scalar;
    the model's train / eval mode is restored, nothing else is touched."""
    dc = diffusion_cfg
    was_training = model.training
    model.eval()
    total, n = None, 0
    try:
        for i, (img, R, T, K) in enumerate(batches):
            xz, eps, logsnr, keep = ops.diffusion_inputs(img, validation_seed(seed, i), 0, dc.cond_prob,
                                                         dc.logsnr_min, dc.logsnr_max, dtype,
                                                         prediction=dc.prediction)
            y = model({"xz": xz, "logsnr": logsnr, "R": R, "t": T, "K": K}, cond_mask=keep, head_nhwc=True)
            loss = ops.diff_loss_nhwc(y, eps, dc.loss_type, logsnr=logsnr, prediction=dc.prediction,
                                      loss_weight=dc.loss_weight, gamma=dc.min_snr_gamma).detach().float()
            if bins is not None:
                ops.loss_bins_add(bins, ops.diff_loss_rows(y, eps, dc.loss_type), logsnr, prediction=dc.prediction,
                                  loss_weight=dc.loss_weight, gamma=dc.min_snr_gamma, logsnr_min=dc.logsnr_min,
                                  logsnr_max=dc.logsnr_max)
            total = loss if total is None else total + loss
            n += 1
    finally:
        if was_training:
            model.train()
    if n == 0:
        raise ValueError("the held-out loss needs at least one batch")
    return total / n


# ------------------------------------------------------------------ objects
class EvalObject:
    """One object: ``imgs[v]`` [3,H,W] fp32 in [-1, 1], ``R[v]`` [3,3], ``T[v]``
    [3] for the views v the evaluation touches, and its intrinsics K [3,3].
    ``scene``: the object's analytic geometry, an fp64 [6,16] table of
    ``data.procedural`` (None for objects that carry none, such as SRN files);
    the geometry-aware scores (``consistency=True``) need it."""

    def __init__(self, name: str, imgs: Dict[int, torch.Tensor], R: Dict[int, torch.Tensor],
                 T: Dict[int, torch.Tensor], K: torch.Tensor, scene: Optional[torch.Tensor] = None):
        self.name, self.imgs, self.R, self.T, self.K, self.scene = name, imgs, R, T, K, scene


def load_objects(root: str, index: str = "", split: str = "val", instances: int = 0, imgsize: int = 64,
                 views: Sequence[int] = (0, 1)) -> List[EvalObject]:
    """The first ``instances`` (0 = all) objects of ``split`` under the SRN
    root -- the 90 / 10 split rule of :class:`SRNDataset` -- with the listed
    views (positions in the object's sorted view list)."""
    from ..data.srn import load_image, load_index, read_matrix, scan_index, split_ids
    idx = load_index(index) if index and os.path.exists(index) else scan_index(root)
    ids = split_ids(list(idx.keys()), split)
    if instances:
        ids = ids[:instances]
    out = []
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)  # noqa: E731
    for inst in ids:
        names = sorted(idx[inst])
        if max(views) >= len(names):
            raise ValueError(f"{inst} has {len(names)} views, view {max(views)} requested")
        imgs, Rs, Ts = {}, {}, {}
        for v in views:
            stem = names[v][:-4]
            imgs[v] = f32(load_image(os.path.join(root, inst, "rgb", names[v]), imgsize))
            pose = read_matrix(os.path.join(root, inst, "pose", stem + ".txt"), (4, 4))
            Rs[v], Ts[v] = f32(pose[:3, :3]), f32(pose[:3, 3])
        K = read_matrix(os.path.join(root, inst, "intrinsics", names[0][:-4] + ".txt"), (3, 3))
        out.append(EvalObject(inst, imgs, Rs, Ts, f32(K)))
    return out


# --------------------------------------------------------------- evaluation
_CLASSES = ("background", "disoccluded", "covisible")


def _ratio(total: float, count: float):
    """(mse, psnr) of a sum over ``count`` pixels x 3 channels; None where the
    count or the mse is 0."""
    if not count > 0 or not total > 0:
        return None, None
    mse = total / (3.0 * count)
    return mse, 10.0 * math.log10(1.0 / mse)


def _consistency_fields(st: Sequence[float]) -> dict:
    """The row fields of one ``ops.view_consistency`` stats row."""
    out = {"n_background": int(st[0]), "n_disoccluded": int(st[1]), "n_covisible": int(st[2]), "n_clean": int(st[3])}
    for j, name in enumerate(_CLASSES):
        out[f"mse_{name}"], out[f"psnr_{name}"] = _ratio(st[4 + j], st[j])
    out["reproj_mse"], out["reproj_psnr"] = _ratio(st[7], st[3])
    return out


def _scenes(objects: Sequence[EvalObject]) -> None:
    missing = [o.name for o in objects if getattr(o, "scene", None) is None]
    if missing:
        raise ValueError(f"consistency needs every object's scene table (procedural objects carry one); "
                         f"{len(missing)} of {len(objects)} have none, the first is {missing[0]!r}")


def _pose64(objs: Sequence[EvalObject], v: int, dev, rep: int = 1):
    """(R [G * rep,3,3], T [G * rep,3]) fp64 of view ``v``: the objects' stored values, upcast."""
    R = torch.stack([o.R[v] for o in objs]).to(dev).double().repeat_interleave(rep, 0)
    T = torch.stack([o.T[v] for o in objs]).to(dev).double().repeat_interleave(rep, 0)
    return R, T


@torch.no_grad()
def evaluate_objects(model, objects: Sequence[EvalObject], input_view: int = 0, views: Sequence[int] = (1,),
                     w: Sequence[float] = (3.0,), timesteps: int = 256, batch: int = 64,
                     autoregressive: bool = False, seed: int = 0, device=None, ref_quirk: bool = False,
                     graph: Optional[bool] = None, keep_images: bool = False,
                     on_view: Optional[Callable] = None, solver: str = "ancestral", eta: float = 0.0,
                     spacing: str = "t", prediction: str = "eps", consistency: bool = False, samples: int = 1):
    """Generate ``views`` of every object from its ``input_view`` and score
    them.  Returns ``(rows, images)``: one row ``{instance, view, w, chain,
    mse, psnr, ssim}`` per (object, view, w) -- ``chain`` the global chain
    index, ``psnr`` None where the images are identical (mse == 0) -- and,
    with ``keep_images``, ``images[(instance, view)]`` = the generated
    [len(w),3,H,W] batch on the CPU.  ``on_view(objects, view, out, gt)`` is
    called with each generated batch ([G * len(w),3,H,W], object-major) and
    its ground truth [G,3,H,W].  ``solver`` / ``eta`` / ``spacing``: the
    update rule and step spacing of :class:`DiffusionSampler`, ``prediction``
    what the model outputs (eps or v).

    ``consistency`` (every object needs a ``scene``, else ValueError): each
    generated batch also goes through ``ops.view_consistency`` with the input
    view's ground truth and pose as the source, and every row gains
    ``n_background`` / ``n_disoccluded`` / ``n_covisible`` / ``n_clean``,
    ``mse_<class>`` / ``psnr_<class>`` of the generated image against the
    ground truth on each class's pixels, and ``reproj_mse`` / ``reproj_psnr``
    of the generated image against the input view warped into it (None where
    the count or the mse is 0).  The poses are the objects' fp32 values upcast
    to fp64, what the model was conditioned on.  The function then returns
    ``(rows, images, pair_rows)``: with more than one view, one ``{instance,
    w, chain, src_view, tgt_view, n_clean, mse, psnr}`` per ordered pair of
    generated views of a chain, the reprojection error of one into the other.

    ``samples`` = C > 1 runs C independent chains per (object, w): chains are
    object-major, then w, then sample -- chain ``(object * len(w) + i) * C + c``
    -- so every per-chain row (which gains ``sample`` = c, as the pair rows do),
    ``images`` ([len(w) * C,3,H,W]) and the batch ``on_view`` sees widen by C,
    and one sampler step runs ``batch * len(w) * C`` chains.  The function then
    also returns ``ensemble_rows`` as its last element: per (instance, view, w)
    the scores of ``ops.ensemble_stats(quantize=True)`` over the C samples --
    ``samples``, ``n`` (pixels), ``mse_mean_image`` / ``psnr_mean_image`` (the
    error of the samples' mean image, sum B / (3 n)), ``mse_samples`` (the mean
    of the samples' errors, sum E / (3 n)), ``spread`` (their variance around
    the mean image, sum V / (3 n); ``mse_samples = mse_mean_image + spread``),
    ``psnr_best`` (the best per-chain ``psnr``; None where one is infinite) and
    ``spread_skill`` = sqrt(V (C + 1) / ((C - 1) B)) (None where B is 0): for
    samples and truth from one distribution E[B] = (1 + 1/C) sigma^2 and E[V]
    = (1 - 1/C) sigma^2, so 1 is calibrated and below 1 over-confident.  With
    ``consistency`` the pixels are split by the class plane of the batch's
    ``view_consistency`` call (geometry only: the first chain's plane serves
    all C) and the row gains ``n_<class>``, ``bias_<class>``,
    ``spread_<class>`` and ``mse_samples_<class>`` for background, disoccluded
    and covisible (None where the count is 0).  ``samples = 1`` is the path
    above, chain numbering and return value included."""
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    nw, C = len(w), int(samples)
    if C < 1:
        raise ValueError(f"samples must be at least 1, got {samples}")
    nc = nw * C                                    # chains per object
    rows: List[dict] = []
    pair_rows: List[dict] = []
    ensemble_rows: List[dict] = []
    images: Dict[tuple, torch.Tensor] = {}
    if consistency:
        _scenes(objects)
    for s in range(0, len(objects), max(int(batch), 1)):
        objs = objects[s:s + max(int(batch), 1)]
        G = len(objs)
        # chains are object-major and numbered globally, so a row (and its noise) does not depend on `batch`
        smp = DiffusionSampler(model, timesteps, ref_quirk, seed=seed, device=dev, chain_offset=s * nc, graph=graph,
                               solver=solver, eta=eta, spacing=spacing, prediction=prediction)
        group = torch.arange(G).repeat_interleave(nc)
        wv = torch.tensor([float(x) for x in w]).repeat_interleave(C).repeat(G)
        K = torch.stack([o.K for o in objs]).to(dev)
        records = [[RecordEntry(o.imgs[input_view].to(dev)[None].expand(nc, -1, -1, -1).contiguous(),
                                o.R[input_view].to(dev), o.T[input_view].to(dev))] for o in objs]
        if consistency:
            table = torch.stack([o.scene for o in objs]).to(dev).double().repeat_interleave(nc, 0)
            K64 = K.double().repeat_interleave(nc, 0)
            src = torch.stack([o.imgs[input_view] for o in objs]).to(dev).float().repeat_interleave(nc, 0)
            sR, sT = _pose64(objs, input_view, dev, nc)
            kept = {}
        for v in views:
            tR = torch.stack([o.R[v] for o in objs]).to(dev)
            tT = torch.stack([o.T[v] for o in objs]).to(dev)
            out = smp.sample_groups(records, tR, tT, K, wv, group).float()
            gt = torch.stack([o.imgs[v] for o in objs]).to(dev)
            mse, ssim = ops.image_metrics(out, gt.repeat_interleave(nc, 0), quantize=True)
            mse_l, ssim_l = mse.double().cpu().tolist(), ssim.double().cpu().tolist()
            klass = None
            if consistency:
                kept[int(v)] = out.contiguous()
                st = ops.view_consistency(table, K64, sR, sT, src, *_pose64(objs, v, dev, nc), kept[int(v)],
                                          gt.float().repeat_interleave(nc, 0), return_class=C > 1)
                if C > 1:
                    st, klass = st[0], st[1][::C].contiguous()
                st_l = st.cpu().tolist()
            if C > 1:
                H, W = out.shape[-2:]
                es_l = ops.ensemble_stats(out.contiguous().view(G * nw, C, 3, H, W),
                                          gt.float().repeat_interleave(nw, 0).contiguous(), klass,
                                          quantize=True).cpu().tolist()
            for gi, o in enumerate(objs):
                for i in range(nw):
                    for c in range(C):
                        j = (gi * nw + i) * C + c
                        rows.append({"instance": o.name, "view": int(v), "w": float(w[i]), "chain": s * nc + j,
                                     "mse": mse_l[j],
                                     "psnr": 10.0 * math.log10(1.0 / mse_l[j]) if mse_l[j] > 0 else None,
                                     "ssim": ssim_l[j]})
                        if C > 1:
                            rows[-1]["sample"] = c
                        if consistency:
                            rows[-1].update(_consistency_fields(st_l[j]))
                    if C > 1:
                        ensemble_rows.append({"instance": o.name, "view": int(v), "w": float(w[i]),
                                              **_ensemble_fields(es_l[gi * nw + i], C, [r["psnr"] for r in rows[-C:]],
                                                                 consistency)})
                if keep_images:
                    images[(o.name, int(v))] = out[gi * nc:(gi + 1) * nc].cpu()
                if autoregressive:
                    records[gi].append(RecordEntry(out[gi * nc:(gi + 1) * nc].contiguous(), o.R[v].to(dev),
                                                   o.T[v].to(dev)))
            if on_view is not None:
                on_view(objs, int(v), out, gt)
        if consistency:
            for va in kept:
                for vb in kept:
                    if va == vb:
                        continue
                    st_l = ops.view_consistency(table, K64, *_pose64(objs, va, dev, nc), kept[va],
                                                *_pose64(objs, vb, dev, nc), kept[vb]).cpu().tolist()
                    for gi, o in enumerate(objs):
                        for i in range(nw):
                            for c in range(C):
                                j = (gi * nw + i) * C + c
                                m, p = _ratio(st_l[j][7], st_l[j][3])
                                pair_rows.append({"instance": o.name, "w": float(w[i]), "chain": s * nc + j,
                                                  "src_view": va, "tgt_view": vb, "n_clean": int(st_l[j][3]),
                                                  "mse": m, "psnr": p})
                                if C > 1:
                                    pair_rows[-1]["sample"] = c
    res = (rows, images, pair_rows) if consistency else (rows, images)
    return res + (ensemble_rows,) if C > 1 else res


def _spread_skill(V: float, B: float, C: int):
    """sqrt(V (C + 1) / ((C - 1) B)); None where B is 0 (or C is 1)."""
    if C < 2 or not B > 0:
        return None
    return math.sqrt(V * (C + 1) / ((C - 1) * B))


def _ensemble_fields(st: Sequence[Sequence[float]], C: int, psnrs: Sequence, by_class: bool) -> dict:
    """The row fields of one ``ops.ensemble_stats`` [4,4] block; ``psnrs`` the
    group's per-chain PSNRs."""
    n, B, V, E = (math.fsum(st[k][j] for k in range(4)) for j in range(4))
    per = (lambda x: x / (3.0 * n)) if n > 0 else (lambda x: None)  # noqa: E731
    out = {"samples": C, "n": int(n), "mse_mean_image": per(B),
           "psnr_mean_image": 10.0 * math.log10(3.0 * n / B) if n > 0 and B > 0 else None,
           "mse_samples": per(E), "spread": per(V),
           "psnr_best": None if any(p is None for p in psnrs) else max(psnrs),
           "spread_skill": _spread_skill(V, B, C)}
    if by_class:
        for name, ks in zip(_CLASSES, ((0,), (1,), (2, 3))):
            nk, Bk, Vk, Ek = (math.fsum(st[k][j] for k in ks) for j in range(4))
            out[f"n_{name}"] = int(nk)
            for field, x in ((f"bias_{name}", Bk), (f"spread_{name}", Vk), (f"mse_samples_{name}", Ek)):
                out[field] = x / (3.0 * nk) if nk > 0 else None
    return out


def _pool(sel: Sequence[dict], count: str, mse: str) -> dict:
    """Pooled over rows: the sum of the rows' sums (mse x 3 count) over the sum of 3 count."""
    n = sum(int(r[count]) for r in sel)
    total = math.fsum(r[mse] * 3.0 * r[count] for r in sel if r[mse] is not None)
    m, p = _ratio(total, n)
    return {"n": n, "mse": m, "psnr": p}


def summarize_consistency(rows: Sequence[dict], pair_rows: Sequence[dict] = ()) -> dict:
    """Per guidance weight the pooled scores of ``evaluate_objects(...,
    consistency=True)``: ``{"<w>": {name: {n, mse, psnr}}}`` for ``covisible``,
    ``disoccluded``, ``background`` (generated against ground truth on the
    class's pixels), ``reproj`` (generated against the warped input view on
    the clean pixels) and ``pairs`` (generated views against each other).
    Pooled -- the sum of the rows' sums over the sum of their counts x 3, then
    the PSNR -- because a single pair may have no clean pixel; ``n`` is the
    pixel count, ``mse`` / ``psnr`` None where it or the error is 0."""
    out = {}
    for wv in sorted({r["w"] for r in rows}):
        sel = [r for r in rows if r["w"] == wv]
        d = {name: _pool(sel, f"n_{name}", f"mse_{name}") for name in ("covisible", "disoccluded", "background")}
        d["reproj"] = _pool(sel, "n_clean", "reproj_mse")
        d["pairs"] = _pool([r for r in pair_rows if r["w"] == wv], "n_clean", "mse")
        out[f"{wv:g}"] = d
    return out


def summarize_ensemble(ensemble_rows: Sequence[dict]) -> dict:
    """Per guidance weight the pooled scores of ``evaluate_objects(...,
    samples=C)``: ``{"<w>": {samples, n, mse_mean_image, psnr_mean_image,
    mse_samples, psnr_samples, spread, spread_skill}}`` and, where the rows
    carry the classes, ``{name: {n, bias, spread, mse_samples, spread_skill}}``
    for ``covisible``, ``disoccluded`` and ``background``.  Pooled as
    :func:`summarize_consistency` pools -- the sum of the rows' sums over the
    sum of their counts x 3, then the PSNRs and ``spread_skill`` from the
    pooled sums; None where the count (for a PSNR or the skill: the error) is 0."""
    def pooled(sel, count, fields):
        n = sum(int(r[count]) for r in sel)
        sums = [math.fsum(r[f] * 3.0 * r[count] for r in sel if r[f] is not None) for f in fields]
        return n, sums

    out = {}
    for wv in sorted({r["w"] for r in ensemble_rows}):
        sel = [r for r in ensemble_rows if r["w"] == wv]
        C = int(sel[0]["samples"])
        n, (B, V, E) = pooled(sel, "n", ("mse_mean_image", "spread", "mse_samples"))
        per = (lambda x: x / (3.0 * n)) if n > 0 else (lambda x: None)  # noqa: E731
        d = {"samples": C, "n": n, "mse_mean_image": per(B), "psnr_mean_image": _ratio(B, n)[1],
             "mse_samples": per(E), "psnr_samples": _ratio(E, n)[1], "spread": per(V),
             "spread_skill": _spread_skill(V, B, C)}
        for name in _CLASSES:
            if f"n_{name}" not in sel[0]:
                continue
            nk, (Bk, Vk, Ek) = pooled(sel, f"n_{name}", (f"bias_{name}", f"spread_{name}", f"mse_samples_{name}"))
            pk = (lambda x: x / (3.0 * nk)) if nk > 0 else (lambda x: None)  # noqa: E731
            d[name] = {"n": nk, "bias": pk(Bk), "spread": pk(Vk), "mse_samples": pk(Ek),
                       "spread_skill": _spread_skill(Vk, Bk, C)}
        out[f"{wv:g}"] = d
    return out


@torch.no_grad()
def gt_ceiling(objects: Sequence[EvalObject], input_view: int = 0, views: Sequence[int] = (1,), device=None) -> dict:
    """The consistency scores of the ground-truth images themselves, pooled
    over the objects: ``reproj`` (the input view warped into each of ``views``)
    and ``pairs`` (every ordered pair of ``views``), each ``{n, mse, psnr}``.
    This is the interpolation floor of the metric -- a pixel is the mean of
    its area, the warp a bilinear sample -- not zero error: what a perfect
    model would score."""
    _scenes(objects)
    dev = torch.device(device) if device is not None else torch.device("cpu")
    table = torch.stack([o.scene for o in objects]).to(dev).double()
    K64 = torch.stack([o.K for o in objects]).to(dev).double()
    img = lambda v: torch.stack([o.imgs[v] for o in objects]).to(dev).float().contiguous()  # noqa: E731

    def pooled(pairs):
        n, total = 0, 0.0
        for a, b in pairs:
            st = ops.view_consistency(table, K64, *_pose64(objects, a, dev), img(a), *_pose64(objects, b, dev), img(b))
            n += int(st[:, 3].sum())
            total += float(st[:, 7].sum())
        m, p = _ratio(total, n)
        return {"n": n, "mse": m, "psnr": p}

    views = [int(v) for v in views]
    return {"reproj": pooled([(int(input_view), v) for v in views]),
            "pairs": pooled([(a, b) for a in views for b in views if a != b])}


def summarize(rows: Sequence[dict]) -> dict:
    """Per guidance weight: ``psnr_mean`` over the images with mse > 0 (the
    rest are counted in ``n_identical``; their PSNR is infinite) and
    ``ssim_mean`` over all images."""
    out = {"n_images": len(rows), "n_identical": sum(1 for r in rows if not r["mse"] > 0), "psnr_mean": {},
           "ssim_mean": {}}
    for wv in sorted({r["w"] for r in rows}):
        sel = [r for r in rows if r["w"] == wv]
        ps = [r["psnr"] for r in sel if r["mse"] > 0]
        out["psnr_mean"][f"{wv:g}"] = sum(ps) / len(ps) if ps else None
        out["ssim_mean"][f"{wv:g}"] = sum(r["ssim"] for r in sel) / len(sel)
    return out


# ------------------------------------------------------------------ loading
def resolve_prediction(choice: str, cfg) -> str:
    """The ``--prediction`` of the sampling CLIs: ``auto`` reads the
    checkpoint's ``config.diffusion.prediction`` (``cfg`` None -- a checkpoint
    without a config, such as a reference checkpoint -- means eps)."""
    from ..diffusion import check_prediction
    if choice == "auto":
        choice = cfg.diffusion.prediction if cfg is not None else "eps"
    return check_prediction(choice)


def load_model(path: str, imgsize: int, device, ema: bool = False):
    """The model of a checkpoint, as ``sampling.py`` loads it: our checkpoints
    carry their config, reference checkpoints (with or without ``module.``)
    are ``XUNet(H, W, ch=128)``.  Returns (model in eval mode, TrainConfig or None)."""
    from ..models import XUNet
    from ..utils import load_checkpoint, load_model_weights
    dev = torch.device(device)
    ck = load_checkpoint(path)
    cfg = None
    if isinstance(ck.get("config"), dict):
        from ..config import from_dict
        cfg = from_dict(ck["config"])
        cfg.model.H = cfg.model.W = imgsize
        model = XUNet(cfg.model).to(dev)
    else:
        model = XUNet(H=imgsize, W=imgsize, ch=128).to(dev)
    load_model_weights(model, ck.get("ema") if (ema and ck.get("ema")) else ck["model"])
    model.compute_dtype = torch.bfloat16 if dev.type == "cuda" else torch.float32
    model.eval()
    return model, cfg
