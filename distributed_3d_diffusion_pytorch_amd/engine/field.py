"""Radiance-field consistency: 3DiM's "3D consistency scoring".

The views a sampler generated for one object are split into training and
held-out views; a dense voxel radiance field is fitted to the training views
(``ops.field_loss_grad``, one fused kernel pass per iteration, Adam on the
grid) and its renders of the held-out poses (``ops.field_render``) are scored
against the held-out generated views with ``ops.image_metrics``.  Views that
agree with one 3D object score high; views that each look plausible but
disagree score low.  Only the poses are needed, no geometry, so the score
exists for SRN data as well as for the procedural scenes.  Single process.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence

import torch

from .. import ops
from ..ops.torch_impl import hash_u32

# Chosen on procedural ground-truth views at 64 x 64 (profiles/field/README.md holds the sweep).
FIT_ITERS, FIT_RAYS, FIT_LR = 300, 4096, 0.1


def _rays(R, t, K, H: int, W: int, rescale_from: int):
    """(o, d) fp32 [V * H * W, 3] of V cameras, in image order."""
    pos, dirs = ops.camera_rays(R[None], t[None], K[None], H, W, rescale_from)
    return pos.reshape(-1, 3).contiguous(), dirs.reshape(-1, 3).contiguous()


def fit_field(images, R, t, K, *, grid: int = 48, samples: int = 64, bound: float = 1.0, iters: int = FIT_ITERS,
              rays_per_iter: int = FIT_RAYS, lr: float = FIT_LR, seed: int = 0, rescale_from: int = 128):
    """Fit a voxel radiance field ``[grid,grid,grid,4]`` (the layout of
    ``ops.field_render``) to ``images`` [V,3,H,W] in [-1, 1] seen by the
    cameras ``R`` [V,3,3] cam-to-world, ``t`` [V,3] and ``K`` [3,3] (the
    intrinsics of the ``rescale_from``-pixel image, as ``ops.camera_rays``
    takes them; 0: of this size).  Iteration i draws ``rays_per_iter`` of the V
    H W rays, with replacement, by the counter hash of ``(seed, i)`` and takes
    one Adam step of rate ``lr`` on the mean squared error of
    ``ops.field_loss_grad`` from a zero grid, so a fit is a pure function of its
    arguments on a given backend.  Returns ``(grid, history)``: ``history``
    fp64 [iters] on the images' device, the per-iteration mean loss (over rays
    and channels)."""
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"fit_field: images must be [V,3,H,W], got {tuple(images.shape)}")
    V, _, H, W = (int(s) for s in images.shape)
    if tuple(R.shape) != (V, 3, 3) or tuple(t.shape) != (V, 3) or tuple(K.shape) != (3, 3):
        raise ValueError(f"fit_field: R, t, K must be [{V},3,3], [{V},3], [3,3], got {tuple(R.shape)}, "
                         f"{tuple(t.shape)}, {tuple(K.shape)}")
    if iters < 1 or rays_per_iter < 1:
        raise ValueError(f"fit_field: iters and rays_per_iter must be at least 1, got {iters} and {rays_per_iter}")
    dev = images.device
    o, d = _rays(R.to(dev), t.to(dev), K.to(dev), H, W, rescale_from)
    y = images.float().permute(0, 2, 3, 1).reshape(-1, 3).contiguous()
    N, n = V * H * W, int(rays_per_iter)
    g = torch.zeros(grid, grid, grid, 4, dtype=torch.float32, device=dev)
    opt = torch.optim.Adam([g], lr=lr)
    history = torch.zeros(iters, dtype=torch.float64, device=dev)
    lane = torch.arange(n, dtype=torch.int64, device=dev)
    for it in range(iters):
        # sorted: neighbouring lanes of the kernel then hold neighbouring pixels of one view
        idx = torch.sort(hash_u32(seed, lane + it * n) % N).values
        loss, grad = ops.field_loss_grad(g, o[idx], d[idx], y[idx], samples=samples, bound=bound)
        g.grad = grad / (3.0 * n)
        opt.step()
        history[it] = loss / (3.0 * n)
    return g.detach(), history


def fit_fields(images, R, t, K, *, tv_rgb: float = 0.0, tv_sigma: float = 0.0, grid: int = 48, samples: int = 64,
               bound: float = 1.0, iters: int = FIT_ITERS, rays_per_iter: int = FIT_RAYS, lr: float = FIT_LR,
               seed: int = 0, rescale_from: int = 128):
    """F independent field fits at once: ``images`` [F,V,3,H,W] in [-1, 1],
    ``R`` [F,V,3,3], ``t`` [F,V,3] and one ``K`` [3,3] as :func:`fit_field`
    takes them.  The rays of all fields are computed once; after that
    iteration i is two ops for all fields together, with no host synchronise:
    ``ops.field_batch_loss_grad`` draws ``rays_per_iter`` of the V H W rays by
    the counter hash of ``(seed, i)`` (with replacement, unsorted -- unlike
    :func:`fit_field`, which sorts its draw -- and the same for every field)
    and ``ops.field_adam_tv`` takes the Adam step of rate ``lr`` on the mean
    squared error plus the smoothness term ``tv_rgb`` / ``tv_sigma`` (the
    weights of ``L_tv``, see the op) between two ping-ponged grids, from zero.
    A batched fit equals the F single fits bit for bit on a given backend.
    Returns ``(grids [F,grid,grid,grid,4], history fp64 [iters,F])``, the
    per-iteration mean loss (over rays and channels) of every field."""
    if images.dim() != 5 or images.shape[2] != 3:
        raise ValueError(f"fit_fields: images must be [F,V,3,H,W], got {tuple(images.shape)}")
    F, V, _, H, W = (int(s) for s in images.shape)
    if tuple(R.shape) != (F, V, 3, 3) or tuple(t.shape) != (F, V, 3) or tuple(K.shape) != (3, 3):
        raise ValueError(f"fit_fields: R, t, K must be [{F},{V},3,3], [{F},{V},3], [3,3], got {tuple(R.shape)}, "
                         f"{tuple(t.shape)}, {tuple(K.shape)}")
    if iters < 1 or rays_per_iter < 1:
        raise ValueError(f"fit_fields: iters and rays_per_iter must be at least 1, got {iters} and {rays_per_iter}")
    dev = images.device
    n = int(rays_per_iter)
    g = [torch.zeros(F, grid, grid, grid, 4, dtype=torch.float32, device=dev) for _ in range(2)]
    if F == 0:
        return g[0], torch.zeros(iters, 0, dtype=torch.float64, device=dev)
    # per field, so that a field's rays do not depend on the batch it is fitted in
    rays = [_rays(R[f].to(dev), t[f].to(dev), K.to(dev), H, W, rescale_from) for f in range(F)]
    o = torch.stack([r[0] for r in rays]).contiguous()
    d = torch.stack([r[1] for r in rays]).contiguous()
    y = images.float().permute(0, 1, 3, 4, 2).reshape(F, -1, 3).contiguous()
    m, v = torch.zeros_like(g[0]), torch.zeros_like(g[0])
    losses = []
    for it in range(iters):
        cur, nxt = g[it & 1], g[1 - (it & 1)]
        loss, grad = ops.field_batch_loss_grad(cur, o, d, y, n=n, it=it, seed=seed, samples=samples, bound=bound)
        ops.field_adam_tv(cur, nxt, m, v, grad, step=it + 1, lr=lr, grad_scale=1.0 / (3.0 * n), tv_rgb=tv_rgb,
                          tv_sigma=tv_sigma)
        losses.append(loss)
    return g[iters & 1], torch.stack(losses) / (3.0 * n)


def _score(grid, fit_loss: float, images, R, t, K, train, test, fit) -> dict:
    """The row of one fitted field: its renders of the poses of ``test`` against ``images[test]``."""
    H, W = (int(s) for s in images.shape[-2:])
    dev = images.device
    o, d = _rays(R[test].to(dev), t[test].to(dev), K.to(dev), H, W, fit.get("rescale_from", 128))
    C = ops.field_render(grid, o, d, samples=fit.get("samples", 64), bound=fit.get("bound", 1.0), width=W)
    pred = (C.view(len(test), H, W, 3).permute(0, 3, 1, 2) * 2.0 - 1.0).contiguous()
    mse, ssim = ops.image_metrics(pred, images[test].float().contiguous(), quantize=True)
    psnr = [10.0 * math.log10(1.0 / m) if m > 0 else 100.0 for m in mse.double().cpu().tolist()]
    ssim = ssim.double().cpu().tolist()
    return {"field_psnr": sum(psnr) / len(psnr), "field_ssim": sum(ssim) / len(ssim), "field_psnr_views": psnr,
            "field_ssim_views": ssim, "fit_loss": fit_loss, "n_train": len(train), "n_test": len(test)}


GEOM_KEYS = ("geom_n_truth", "geom_n_field", "geom_n_both", "geom_iou", "geom_depth_mae", "geom_depth_rmse",
             "geom_normal_cos", "geom_sil_mse")


def _geom_fields(sums: Sequence[float], pixels: int) -> dict:
    """The ``geom_*`` fields of pooled ``ops.field_geometry`` rows: ``sums`` the
    7 sums over all their views, ``pixels`` the pixels of those views.  Every
    value is sum / count, None where its count is 0."""
    nt, nf, nb = (int(round(x)) for x in sums[:3])
    per = lambda x: x / nb if nb else None  # noqa: E731
    mse = per(sums[4])
    return {"geom_n_truth": nt, "geom_n_field": nf, "geom_n_both": nb,
            "geom_iou": nb / (nt + nf - nb) if nt + nf - nb else None,
            "geom_depth_mae": per(sums[3]), "geom_depth_rmse": None if mse is None else math.sqrt(mse),
            "geom_normal_cos": None if nb == 0 else 1.0 - sums[5] / nb,
            "geom_sil_mse": sums[6] / pixels if pixels else None,
            "geom_sums": [float(x) for x in sums], "geom_pixels": int(pixels)}


def _geometry(grids, scenes, R, t, K, H: int, W: int, fit) -> List[dict]:
    """The ``geom_*`` fields of F fitted ``grids`` [F,G,G,G,4] seen from their
    held-out cameras ``R`` [F,V,3,3], ``t`` [F,V,3] against the scene tables
    ``scenes`` [F,6,16]: one ``ops.field_geometry`` call."""
    F, V = int(R.shape[0]), int(R.shape[1])
    dev = grids.device
    scores = ops.field_geometry(grids.contiguous(), K.to(dev).double()[None].expand(F, 3, 3).contiguous(),
                                R.to(dev).double(), t.to(dev).double(), H, W, samples=fit.get("samples", 64),
                                bound=fit.get("bound", 1.0), rescale_from=fit.get("rescale_from", 128),
                                table=scenes.to(dev).double().contiguous())
    return [_geom_fields(row, V * H * W) for row in scores.sum(1).cpu().tolist()]


# Chosen on procedural ground-truth views at 64 x 64 (profiles/field/README.md holds the sweep).
REPROJ_TOL = 0.05
REPROJ_KEYS = ("reproj_n_covisible", "reproj_n_clean", "reproj_mse", "reproj_psnr", "reproj_covis_mse",
               "reproj_covis_psnr", "reproj_depth_mae")


def _reproj_fields(sums: Sequence[float]) -> dict:
    """The ``reproj_*`` fields of pooled ``ops.depth_consistency`` rows: ``sums``
    the 7 sums over all their ordered view pairs.  Every value is sum / count,
    None where its count is 0; a zero error counts with 100 dB, as in
    ``field_psnr``."""
    ncov, ncl = int(round(sums[2])), int(round(sums[3]))
    mse, cmse = (sums[5] / (3 * ncl) if ncl else None), (sums[4] / (3 * ncov) if ncov else None)
    db = lambda m: None if m is None else 10.0 * math.log10(1.0 / m) if m > 0 else 100.0  # noqa: E731
    return {"reproj_n_covisible": ncov, "reproj_n_clean": ncl, "reproj_mse": mse, "reproj_psnr": db(mse),
            "reproj_covis_mse": cmse, "reproj_covis_psnr": db(cmse),
            "reproj_depth_mae": sums[6] / ncl if ncl else None, "reproj_sums": [float(x) for x in sums]}


def _reproj(grids, images, R, t, K, fit, tol: float) -> List[dict]:
    """The ``reproj_*`` fields of F fitted ``grids`` [F,G,G,G,4] and the views
    ``images`` [F,V,3,H,W] they belong to, training and held-out, under the
    cameras ``R`` [F,V,3,3], ``t`` [F,V,3]: one ``ops.field_geometry`` call
    reads the fields' depth at all V poses, one ``ops.depth_consistency`` call
    scores the V (V - 1) ordered pairs of every field under those depths."""
    F, V, _, H, W = (int(s) for s in images.shape)
    dev = grids.device
    Kf = K.to(dev).double()[None].expand(F, 3, 3).contiguous()
    Rd, td = R.to(dev).double().contiguous(), t.to(dev).double().contiguous()
    ref = fit.get("rescale_from", 128)
    maps = ops.field_geometry(grids.contiguous(), Kf, Rd, td, H, W, samples=fit.get("samples", 64),
                              bound=fit.get("bound", 1.0), rescale_from=ref, return_maps=True)
    stats = ops.depth_consistency(maps[:, :, 1].contiguous(), images.to(dev).float().contiguous(), Kf, Rd, td, tol=tol,
                                  rescale_from=ref)
    return [_reproj_fields(row) for row in stats.sum((1, 2)).cpu().tolist()]


def _need_scene(scene, name: str):
    if scene is None:
        raise ValueError(f"geometry needs the object's scene table (procedural objects carry one); {name} has none")
    return scene


def _split(train, test):
    train, test = [int(v) for v in train], [int(v) for v in test]
    if len(train) < 3:
        raise ValueError(f"field_consistency needs at least 3 training views, got {len(train)}")
    if not test:
        raise ValueError("field_consistency needs at least one held-out view")
    return train, test


def _batched(batch: int, tv_rgb: float, tv_sigma: float) -> bool:
    if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
        raise ValueError(f"batch must be an integer >= 1, got {batch!r}")
    return batch > 1 or tv_rgb != 0.0 or tv_sigma != 0.0


def field_consistency(images, R, t, K, train: Sequence[int], test: Sequence[int], *, batch: int = 1,
                      tv_rgb: float = 0.0, tv_sigma: float = 0.0, geometry: bool = False, scene=None,
                      reproj: bool = False, reproj_tol: float = REPROJ_TOL, **fit) -> dict:
    """The score of one set of views: fit a field (:func:`fit_field`, ``fit``
    its keywords) to ``images[train]``, render the poses of ``test`` and score
    the renders against ``images[test]`` with ``ops.image_metrics`` (as 8-bit
    PNGs).  With ``batch > 1`` or a non-zero ``tv_rgb`` / ``tv_sigma`` the fit
    is :func:`fit_fields` (here of one field) with that smoothness term.
    Returns ``field_psnr`` / ``field_ssim`` (the means over the test
    views; a view rendered exactly counts with 100 dB), ``field_psnr_views`` /
    ``field_ssim_views``, ``fit_loss`` (the last iteration's mean loss) and
    ``n_train`` / ``n_test``.  ``geometry``: the fitted grid is also read out
    with ``ops.field_geometry`` at the held-out poses against ``scene`` (the
    object's fp64 [6,16] table; ValueError without one) and the row gains
    ``geom_n_truth`` / ``geom_n_field`` / ``geom_n_both`` (pixels the scene,
    the field, both hit), ``geom_iou``, ``geom_depth_mae`` /
    ``geom_depth_rmse`` and ``geom_normal_cos`` over the pixels both hit and
    ``geom_sil_mse``, each pooled over the held-out views as sum / count (None
    where the count is 0; ``geom_sums`` / ``geom_pixels`` keep the sums for
    further pooling).  ``reproj``: the fitted field's depth is read at the poses
    of ALL views (``ops.field_geometry``) and the views themselves are warped
    into each other under it (``ops.depth_consistency`` with ``tol =
    reproj_tol``), so appearance never goes through the grid; the row gains,
    pooled over the V (V - 1) ordered pairs as sum / count (None at count 0),
    ``reproj_n_covisible`` / ``reproj_n_clean``, ``reproj_mse`` /
    ``reproj_psnr`` over the clean pixels (the [0, 1] scale of
    ``ops.image_metrics``, unquantized), ``reproj_covis_mse`` /
    ``reproj_covis_psnr`` over all co-visible pixels, ``reproj_depth_mae`` (the
    fields' own depth disagreement at the clean pixels) and ``reproj_sums``.
    Fewer than 3 training views, or no test view, is a ValueError."""
    train, test = _split(train, test)
    if geometry:
        _need_scene(scene, "the object")
    if _batched(batch, tv_rgb, tv_sigma):
        grids, history = fit_fields(images[train][None], R[train][None], t[train][None], K, tv_rgb=tv_rgb,
                                    tv_sigma=tv_sigma, **fit)
        grid, history = grids[0], history[:, 0]
    else:
        grid, history = fit_field(images[train], R[train], t[train], K, **fit)
    row = _score(grid, float(history[-1]), images, R, t, K, train, test, fit)
    if geometry:
        H, W = (int(s) for s in images.shape[-2:])
        row.update(_geometry(grid[None], scene[None], R[test][None], t[test][None], K, H, W, fit)[0])
    if reproj:
        row.update(_reproj(grid[None], images[None], R[None], t[None], K, fit, reproj_tol)[0])
    return row


def field_rows(objects, images: Dict[tuple, torch.Tensor], views: Sequence[int], holdout: Sequence[int],
               w: Sequence[float], device=None, *, batch: int = 1, tv_rgb: float = 0.0, tv_sigma: float = 0.0,
               geometry: bool = False, reproj: bool = False, reproj_tol: float = REPROJ_TOL, **fit) -> List[dict]:
    """One :func:`field_consistency` row per (object, guidance weight) of an
    ``evaluate_objects(..., keep_images=True)`` run: ``images[(instance, view)]``
    the generated ``[len(w),3,H,W]`` batch; the views in ``holdout`` are held
    out, the other generated views are the training set.  ``images`` None:
    the objects' own (ground-truth) images, one row per object with ``w``
    None -- the ceiling of the score at this grid and view count.  With
    ``batch > 1`` or a non-zero ``tv_rgb`` / ``tv_sigma`` the fields are fitted
    by :func:`fit_fields`, at most ``batch`` (object, weight) pairs per call.
    ``geometry``: every row also gets the ``geom_*`` fields of
    :func:`field_consistency` against the object's ``scene`` (ValueError for
    an object without one); the batched path reads all grids of a
    ``fit_fields`` call out in one ``ops.field_geometry`` call.  ``reproj``:
    every row also gets the ``reproj_*`` fields of :func:`field_consistency`;
    the batched path makes one ``ops.field_geometry`` and one
    ``ops.depth_consistency`` call per ``fit_fields`` call."""
    views, holdout = [int(v) for v in views], [int(v) for v in holdout]
    bad = [v for v in holdout if v not in views]
    if bad or len(set(holdout)) != len(holdout):
        raise ValueError(f"the held-out views must be distinct views of {views}, got {holdout}")
    train = [i for i, v in enumerate(views) if v not in holdout]
    test = [i for i, v in enumerate(views) if v in holdout]
    dev = torch.device(device) if device is not None else torch.device("cpu")
    batched = _batched(batch, tv_rgb, tv_sigma)
    rows, todo = [], []

    def flush():
        """Fit and score the pending (object, weight) pairs in one fit_fields call."""
        tr, te = _split(train, test)
        grids, history = fit_fields(torch.stack([p[2][tr] for p in todo]), torch.stack([p[3][tr] for p in todo]),
                                    torch.stack([p[4][tr] for p in todo]), todo[0][5], tv_rgb=tv_rgb,
                                    tv_sigma=tv_sigma, **fit)
        last = history[-1].cpu().tolist()
        geom = [{}] * len(todo)
        if geometry:
            H, W = (int(s) for s in todo[0][2].shape[-2:])
            geom = _geometry(grids, torch.stack([p[6] for p in todo]), torch.stack([p[3][te] for p in todo]),
                             torch.stack([p[4][te] for p in todo]), todo[0][5], H, W, fit)
        if reproj:
            rp = _reproj(grids, torch.stack([p[2] for p in todo]), torch.stack([p[3] for p in todo]),
                         torch.stack([p[4] for p in todo]), todo[0][5], fit, reproj_tol)
            geom = [{**g, **r} for g, r in zip(geom, rp)]
        for f, (name, wv, img, R, t, K, _) in enumerate(todo):
            rows.append({"instance": name, "w": wv, **_score(grids[f], last[f], img, R, t, K, tr, te, fit), **geom[f]})
        todo.clear()

    for o in objects:
        scene = _need_scene(getattr(o, "scene", None), o.name) if geometry else None
        R = torch.stack([o.R[v] for v in views]).to(dev)
        t = torch.stack([o.T[v] for v in views]).to(dev)
        for i, wv in enumerate(w if images is not None else (None,)):
            img = torch.stack([o.imgs[v] if images is None else images[(o.name, v)][i] for v in views]).to(dev)
            wv = None if wv is None else float(wv)
            if not batched:
                rows.append({"instance": o.name, "w": wv,
                             **field_consistency(img.float(), R, t, o.K.to(dev), train, test, geometry=geometry,
                                                 scene=scene, reproj=reproj, reproj_tol=reproj_tol, **fit)})
                continue
            K = o.K.to(dev)
            if todo and (len(todo) == batch or not torch.equal(K, todo[0][5])):     # one K per fit_fields call
                flush()
            todo.append((o.name, wv, img.float(), R, t, K, scene))
    if todo:
        flush()
    return rows


def summarize_field(rows: Sequence[dict]) -> dict:
    """Per guidance weight (``"gt"`` for the ground-truth rows) the means of
    ``field_psnr``, ``field_ssim`` and ``fit_loss`` over the objects; for rows
    with ``geom_*`` / ``reproj_*`` fields also those, pooled over the objects as
    sum / count."""
    out = {}
    for wv in sorted({r["w"] for r in rows}, key=lambda x: -math.inf if x is None else x):
        sel = [r for r in rows if r["w"] == wv]
        d = {"n": len(sel), **{k: sum(r[k] for r in sel) / len(sel) for k in ("field_psnr", "field_ssim", "fit_loss")}}
        if sel and all("geom_sums" in r for r in sel):
            pooled = _geom_fields([sum(r["geom_sums"][k] for r in sel) for k in range(7)],
                                  sum(r["geom_pixels"] for r in sel))
            d.update({k: pooled[k] for k in GEOM_KEYS})
        if sel and all("reproj_sums" in r for r in sel):
            pooled = _reproj_fields([sum(r["reproj_sums"][k] for r in sel) for k in range(7)])
            d.update({k: pooled[k] for k in REPROJ_KEYS})
        out["gt" if wv is None else f"{wv:g}"] = d
    return out
