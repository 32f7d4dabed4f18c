#!/usr/bin/env python
"""Evaluation CLI: PSNR / SSIM of generated novel views on held-out objects
(the 3DiM protocol) and, optionally, the held-out training loss.

    python evaluate.py --model runs/cars64/latest.pt --data data/SRN/cars_train --instances 64
    python evaluate.py --model runs/proc64/latest.pt --procedural --instances 64

Takes the first ``--instances`` objects of the split (the 90 / 10 rule of the
training set), conditions on ``--input_view`` of each and generates the views
listed in ``--views``, one chain per (object, guidance weight); up to
``--batch`` objects run as one graph-replayed sampler step.  With
``--autoregressive`` each generated view joins its object's record
(stochastic conditioning); otherwise every view is generated from the input
view alone.  The results are scored on the device as the 8-bit PNGs would be,
and ``<out>/metrics.json`` gets the arguments, one row per (instance, view, w)
and the per-w means.  ``--save_png`` also writes
``<out>/<instance>/<view>/{gt,<w>}.png``.  ``--procedural`` scores the held-out
objects of the ray-cast procedural scenes against their exact renders instead
of an SRN tree; there ``--consistency`` adds the geometry-aware scores of
``ops.view_consistency``: PSNR on the co-visible, disoccluded and background
pixels, the reprojection error against the input view and between the
generated views, and the same on the ground truth (``gt_ceiling``).
``--samples C`` runs C independent chains per (object, guidance weight) -- one
sampler step then runs ``batch * len(w) * C`` chains -- and adds the ensemble
scores of ``ops.ensemble_stats``: the error of the samples' mean image, their
spread and the spread-skill ratio, per visibility class with
``--consistency``; ``--save_png`` then writes ``<w>_s<c>.png``,
``mean_<w>.png`` and ``std_<w>.png``.  ``--field_holdout a,b`` adds 3DiM's 3D
consistency score (``engine.field_consistency``): per (object, guidance
weight) a voxel radiance field is fitted to the generated ``--views`` that are
not held out and its renders are scored against the held-out generated views;
it needs only the poses, so it works on SRN data, and with ``--procedural``
the same score of the ground-truth images (``gt_field``) gives its ceiling.
``--swd`` adds a distribution score that needs no trained network: the sliced
Wasserstein distance (``ops.sliced_wasserstein``) of each guidance weight's
generated set against the ground-truth set, one number per Laplacian-pyramid
level, and the same between the two halves of the ground truth as its floor.
``--knn`` separates fidelity from diversity: precision, recall, density and
coverage of each generated set against the ground-truth set from exact nearest
neighbours in 8-bit pixel space (``ops.image_knn``); ``--knn_train N`` searches
the nearest images of the first N training objects for every generated image:
one that is closer to a training image than to its own ground truth is
regurgitated.
Single process.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="./trained_model.pt")
    ap.add_argument("--data", default="./data/SRN/cars_train", help="SRN instance root")
    ap.add_argument("--index", default="", help="index pickle/json {instance: [views]}; default: scan --data")
    ap.add_argument("--procedural", action="store_true",
                    help="score ray-cast procedural objects (data/procedural.py) instead of --data: the first "
                         "--instances objects of the split, --views are view ids")
    ap.add_argument("--proc_seed", type=int, default=0, help="--procedural: the scene family's seed")
    ap.add_argument("--proc_objects", type=int, default=0,
                    help="--procedural: object ids [0, N) (0 = [0, 2^31)); ids with id %% 10 == 9 are the val split")
    ap.add_argument("--consistency", action="store_true",
                    help="--procedural: also score with the scenes' geometry (co-visible / disoccluded / background "
                         "PSNR, reprojection consistency); metrics.json gets the row fields and a consistency block")
    ap.add_argument("--split", default="val", choices=["train", "val"])
    ap.add_argument("--instances", type=int, default=64, help="first N objects of the split (0 = all)")
    ap.add_argument("--input_view", type=int, default=0)
    ap.add_argument("--views", default="1,2,3", help="target views (positions in the sorted view list)")
    ap.add_argument("--w", default="3.0", help="guidance weights, one chain per object each")
    ap.add_argument("--samples", type=int, default=1,
                    help="independent chains per (object, guidance weight), C >= 1: one sampler step runs "
                         "batch * len(w) * C chains; with C > 1 metrics.json gets an ensemble block (the error of the "
                         "samples' mean image, their spread, the spread-skill ratio; per visibility class with "
                         "--consistency)")
    ap.add_argument("--field_holdout", default="",
                    help="views of --views to hold out for the radiance-field consistency score: a field is fitted "
                         "to the other generated views (at least 3) of each (object, w) and its renders are scored "
                         "against the held-out generated views; metrics.json gets a field block")
    ap.add_argument("--field_grid", type=int, default=48, help="--field_holdout: nodes per axis of the field")
    ap.add_argument("--field_iters", type=int, default=0, help="--field_holdout: fit iterations (0 = the default)")
    ap.add_argument("--field_batch", type=int, default=1,
                    help="--field_holdout: fit this many (object, w) fields per call (engine.fit_fields); 1 with "
                         "--field_tv 0 is the one-by-one fit of engine.fit_field")
    ap.add_argument("--field_tv", type=float, default=0.0,
                    help="--field_holdout: weight of the smoothness term on the grid (colour and density alike); "
                         "not 0 fits through engine.fit_fields (profiles/field/README.md recommends a value)")
    ap.add_argument("--timesteps", type=int, default=256)
    ap.add_argument("--swd", action="store_true",
                    help="also score each guidance weight's generated set against the ground-truth set with the sliced "
                         "Wasserstein distance on Laplacian-pyramid patches (ops.sliced_wasserstein): a distribution "
                         "metric that needs no trained network; metrics.json gets an swd block.  With --samples C > 1 "
                         "the set is sample 0 of every view")
    ap.add_argument("--swd_patches", type=int, default=128,
                    help="--swd: patches per image and level (capped so that images x patches <= 16384)")
    ap.add_argument("--swd_dirs", type=int, default=512, help="--swd: projection directions per level")
    ap.add_argument("--swd_seed", type=int, default=0, help="--swd: seed of the patch corners and the directions")
    ap.add_argument("--knn", action="store_true",
                    help="also score each guidance weight's generated set against the ground-truth set by improved "
                         "precision / recall and density / coverage from exact k-nearest neighbours in 8-bit pixel "
                         "space (ops.image_knn); metrics.json gets a knn block.  With --samples C > 1 the set is "
                         "sample 0 of every view")
    ap.add_argument("--knn_k", type=int, default=5, help="--knn: the neighbour that sets an image's radius (1..8)")
    ap.add_argument("--knn_train", type=int, default=0,
                    help="search the nearest training images (the input view and --views of the first N objects of "
                         "the train split, 0 = off) of every generated and ground-truth image; metrics.json gets a "
                         "memorisation block")
    ap.add_argument("--knn_train_top", type=int, default=4, help="--knn_train: neighbours kept per image (1..8)")
    ap.add_argument("--field_geometry", action="store_true",
                    help="--field_holdout with --procedural: also read depth, silhouette and normals out of every "
                         "fitted field at the held-out poses (ops.field_geometry) and score them against the scenes' "
                         "true surface; the field block's rows, per_w and gt_field get the geom_* fields")
    ap.add_argument("--field_reproj", action="store_true",
                    help="--field_holdout: also read every fitted field's depth at the poses of all generated views and "
                         "warp the generated views into each other under it (ops.depth_consistency); the field block's "
                         "rows, per_w and gt_field get the reproj_* fields.  Needs only poses: works on SRN data")
    ap.add_argument("--field_reproj_tol", type=float, default=None,
                    help="--field_reproj: relative depth tolerance of a co-visible pixel (default: the engine's, "
                         "chosen in profiles/field/README.md)")
    ap.add_argument("--sampler", default="ancestral", choices=["ancestral", "ddim", "dpmpp2m"],
                    help="update rule: the 256-step ancestral chain, DDIM or DPM-Solver++(2M) for few steps")
    ap.add_argument("--eta", type=float, default=0.0, help="DDIM noise level in [0, 1] (1 = ancestral variance)")
    ap.add_argument("--spacing", default="t", choices=["t", "logsnr"], help="steps uniform in t or in logSNR")
    ap.add_argument("--prediction", default="auto", choices=["auto", "eps", "v"],
                    help="what the model outputs; auto: the checkpoint's config.diffusion.prediction (eps without one)")
    ap.add_argument("--imgsize", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64, help="objects per sampler batch")
    ap.add_argument("--autoregressive", action="store_true", help="generated views join the record")
    ap.add_argument("--val_batches", type=int, default=0, help="also score the training loss on this many batches")
    ap.add_argument("--val_batch_size", type=int, default=16)
    ap.add_argument("--loss_bins", type=int, default=0,
                    help="with --val_batches: also write the loss by noise level in this many bins (val_loss_bins)")
    ap.add_argument("--ema", action="store_true", help="use EMA weights when the checkpoint has them")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="evaluation")
    ap.add_argument("--save_png", action="store_true")
    ap.add_argument("--backend", default="auto")
    args = ap.parse_args(argv)
    if args.samples < 1:
        ap.error(f"--samples must be at least 1, got {args.samples}")
    if args.swd_patches < 1 or args.swd_dirs < 1:
        ap.error(f"--swd_patches and --swd_dirs must be at least 1, got {args.swd_patches} and {args.swd_dirs}")
    if not 1 <= args.knn_k <= 8 or not 1 <= args.knn_train_top <= 8 or args.knn_train < 0:
        ap.error(f"--knn_k and --knn_train_top must be in 1..8 and --knn_train at least 0, got {args.knn_k}, "
                 f"{args.knn_train_top} and {args.knn_train}")
    if args.field_batch < 1 or not 0.0 <= args.field_tv < float("inf"):
        ap.error(f"--field_batch must be at least 1 and --field_tv at least 0, got {args.field_batch} and "
                 f"{args.field_tv}")
    if args.field_holdout:
        views = [int(v) for v in args.views.split(",")]
        hold = [int(v) for v in args.field_holdout.split(",")]
        if args.samples > 1:
            ap.error("--field_holdout together with --samples C > 1 is not supported")
        if len(set(hold)) != len(hold) or any(v not in views for v in hold):
            ap.error(f"--field_holdout must name distinct views of --views {views}, got {hold}")
        if len(set(views)) != len(views) or len(views) - len(hold) < 3:
            ap.error(f"--field_holdout needs at least 3 distinct --views that are not held out, got {views} "
                     f"without {hold}")
    return args


def val_loss(model, cfg, args, dev, prediction: str):
    """The training loss (the checkpoint's configured, weighted objective, for
    the target of ``prediction``) on the first ``val_batches * val_batch_size``
    pairs of the split, with the fixed validation draw of
    ``Trainer.validation_loss``.  Returns ``(loss, report)``: ``report`` the
    loss by noise level in ``--loss_bins`` bins (None without them)."""
    import dataclasses
    import torch
    from distributed_3d_diffusion_pytorch_amd.config import DiffusionConfig
    from distributed_3d_diffusion_pytorch_amd.diffusion import loss_bins_report
    from distributed_3d_diffusion_pytorch_amd.data import SRNDataset, collate
    from distributed_3d_diffusion_pytorch_amd.engine import heldout_loss
    if args.procedural:
        import itertools
        from distributed_3d_diffusion_pytorch_amd.data import ProceduralBatches
        batches = itertools.islice(ProceduralBatches(args.val_batch_size, args.imgsize, dev, seed=args.proc_seed,
                                                     objects=args.proc_objects, split=args.split), args.val_batches)
    else:
        ds = SRNDataset(args.split, args.data, args.index, args.imgsize, seed=args.seed)
        n = min(len(ds), args.val_batches * args.val_batch_size)
        if n == 0:
            raise ValueError(f"no instances in the {args.split} split of {args.data}")
        batches = (tuple(t.to(dev) for t in collate([ds[i] for i in range(s, min(s + args.val_batch_size, n))]))
                   for s in range(0, n, args.val_batch_size))
    dc = dataclasses.replace(cfg.diffusion if cfg is not None else DiffusionConfig(), prediction=prediction)
    table = torch.zeros(args.loss_bins, 5, dtype=torch.float64, device=dev) if args.loss_bins > 0 else None
    loss = float(heldout_loss(model, batches, args.seed, dc, model.compute_dtype, bins=table))
    return loss, (loss_bins_report(table, dc.logsnr_min, dc.logsnr_max) if table is not None else None)


def train_chunks(args, views, dev, objects_per_chunk: int = 64):
    """The images of the first ``--knn_train`` objects of the train split at
    ``views`` as ``engine.nearest_train`` takes them: ``(uint8 [m,3,H,W] on
    ``dev``, [(instance, view)] * m)`` for at most ``objects_per_chunk``
    objects at a time, so a large N never sits on the device at once."""
    from distributed_3d_diffusion_pytorch_amd.ops.torch_impl import image_map_u8
    import torch
    for s in range(0, args.knn_train, objects_per_chunk):
        m = min(objects_per_chunk, args.knn_train - s)
        if args.procedural:
            from distributed_3d_diffusion_pytorch_amd.data import procedural_objects
            objs = procedural_objects(args.proc_seed, m, views, args.imgsize, objects=args.proc_objects, split="train",
                                      device=dev, offset=s)
        else:
            from distributed_3d_diffusion_pytorch_amd.engine import load_objects
            objs = load_objects(args.data, args.index, "train", m, args.imgsize, views, offset=s)
        if not objs:
            return
        yield (image_map_u8(torch.stack([o.imgs[v] for o in objs for v in views])).to(dev),
               [(o.name, v) for o in objs for v in views])


def run(args) -> dict:
    import torch
    from distributed_3d_diffusion_pytorch_amd import ops
    from distributed_3d_diffusion_pytorch_amd.engine import evaluate_objects, load_objects, summarize
    from distributed_3d_diffusion_pytorch_amd.engine.evaluate import load_model, resolve_prediction

    if args.consistency and not args.procedural:
        raise ValueError("--consistency needs --procedural: SRN data carries no geometry to score against")
    if args.field_geometry and not (args.procedural and args.field_holdout):
        raise ValueError("--field_geometry needs --procedural and --field_holdout: it scores the fitted fields against "
                         "the scenes' geometry, which SRN data does not carry")
    if args.field_reproj:
        from distributed_3d_diffusion_pytorch_amd.engine.field import REPROJ_TOL
        if not args.field_holdout:
            raise ValueError("--field_reproj needs --field_holdout: it scores the generated views under the depth of the "
                             "field fitted to them")
        if args.field_reproj_tol is None:
            args.field_reproj_tol = REPROJ_TOL
        if not 0.0 < args.field_reproj_tol < float("inf"):
            raise ValueError(f"--field_reproj_tol must be positive, got {args.field_reproj_tol}")
    if args.backend != "auto":
        ops.set_backend(args.backend)
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    t0 = time.time()
    views = [int(v) for v in args.views.split(",")]
    w = [float(x) for x in args.w.split(",")]
    model, cfg = load_model(args.model, args.imgsize, dev, args.ema)
    prediction = resolve_prediction(args.prediction, cfg)
    print(f"[evaluate] prediction {prediction}", flush=True)
    if args.procedural:
        from distributed_3d_diffusion_pytorch_amd.data import procedural_objects
        objects = procedural_objects(args.proc_seed, args.instances, sorted({args.input_view, *views}), args.imgsize,
                                     objects=args.proc_objects, split=args.split, device=dev)
    else:
        objects = load_objects(args.data, args.index, args.split, args.instances, args.imgsize,
                               sorted({args.input_view, *views}))
    if not objects:
        raise ValueError(f"no instances in the {args.split} split of {args.data}")
    os.makedirs(args.out, exist_ok=True)

    C = args.samples

    def write_pngs(objs, v, out, gt):
        from sampling import save_png
        if C > 1:                                  # the samples' mean image and their spread, grey min(1, 4 std)
            _, mean, std = ops.ensemble_stats(out.contiguous().view(len(objs) * len(w), C, *out.shape[1:]),
                                              gt.float().repeat_interleave(len(w), 0).contiguous(), return_maps=True)
            mean = mean.cpu().numpy()
            grey = ((4.0 * std).clamp(max=1.0) * 2.0 - 1.0)[:, None].expand(-1, 3, -1, -1).cpu().numpy()
        out, gt = out.cpu().numpy(), gt.cpu().numpy()
        for gi, o in enumerate(objs):
            d = os.path.join(args.out, o.name, str(v))
            os.makedirs(d, exist_ok=True)
            save_png(gt[gi], os.path.join(d, "gt.png"))
            for i, wv in enumerate(w):
                j = gi * len(w) + i
                if C == 1:
                    save_png(out[j], os.path.join(d, f"{wv:g}.png"))
                    continue
                for c in range(C):
                    save_png(out[j * C + c], os.path.join(d, f"{wv:g}_s{c}.png"))
                save_png(mean[j], os.path.join(d, f"mean_{wv:g}.png"))
                save_png(grey[j], os.path.join(d, f"std_{wv:g}.png"))

    t1 = time.time()
    rows, kept, *rest = evaluate_objects(model, objects, args.input_view, views, w, args.timesteps, args.batch,
                                      args.autoregressive, args.seed, dev, keep_images=bool(args.field_holdout),
                                      on_view=write_pngs if args.save_png else None, solver=args.sampler,
                                      eta=args.eta, spacing=args.spacing, prediction=prediction,
                                      consistency=args.consistency, samples=C,
                                      swd=dict(patches=args.swd_patches, dirs=args.swd_dirs, seed=args.swd_seed)
                                      if args.swd else None, knn=dict(k=args.knn_k) if args.knn else None,
                                      knn_train=train_chunks(args, sorted({args.input_view, *views}), dev)
                                      if args.knn_train else None, knn_train_top=args.knn_train_top)
    memorisation = rest.pop() if args.knn_train else None
    knn = rest.pop() if args.knn else None
    swd = rest.pop() if args.swd else None
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t2 = time.time()
    data = f"procedural seed={args.proc_seed} objects={args.proc_objects}" if args.procedural else args.data
    result = {"args": vars(args), "data": data, "prediction": prediction, "per_image": rows, **summarize(rows)}
    if args.consistency:
        from distributed_3d_diffusion_pytorch_amd.engine import gt_ceiling, summarize_consistency
        result["consistency"] = {"per_w": summarize_consistency(rows, rest[0]), "pairs": rest[0],
                                 "gt_ceiling": gt_ceiling(objects, args.input_view, views, dev)}
    if C > 1:
        from distributed_3d_diffusion_pytorch_amd.engine import summarize_ensemble
        result["ensemble"] = {"per_w": summarize_ensemble(rest[-1]), "rows": rest[-1]}
    if swd is not None:
        result["swd"] = swd
    if knn is not None:
        result["knn"] = knn
    if memorisation is not None:
        result["memorisation"] = memorisation
    if args.field_holdout:
        from distributed_3d_diffusion_pytorch_amd.engine import field_rows, summarize_field
        hold = [int(v) for v in args.field_holdout.split(",")]
        fit = {"grid": args.field_grid, "seed": args.seed, **({"iters": args.field_iters} if args.field_iters else {}),
               "batch": args.field_batch, "tv_rgb": args.field_tv, "tv_sigma": args.field_tv,
               **({"geometry": True} if args.field_geometry else {}),
               **({"reproj": True, "reproj_tol": args.field_reproj_tol} if args.field_reproj else {})}
        frows = field_rows(objects, kept, views, hold, w, dev, **fit)
        result["field"] = {"per_w": summarize_field(frows), "rows": frows}
        if args.procedural:
            grows = field_rows(objects, None, views, hold, w, dev, **fit)
            result["field"]["gt_field"] = {**summarize_field(grows)["gt"], "rows": grows}
    if args.val_batches > 0:
        result["val_loss"], bins = val_loss(model, cfg, args, dev, prediction)
        if bins is not None:
            result["val_loss_bins"] = bins
    result["sample_seconds"] = t2 - t1
    result["wall_seconds"] = time.time() - t0
    tmp = os.path.join(args.out, "metrics.json.tmp")
    with open(tmp, "w") as f:
        json.dump(result, f, indent=1, allow_nan=False)
    os.replace(tmp, os.path.join(args.out, "metrics.json"))
    for k in sorted(result["psnr_mean"], key=float):
        p = result["psnr_mean"][k]
        print(f"[evaluate] w={k}: PSNR {'n/a' if p is None else format(p, '.3f')} dB  SSIM "
              f"{result['ssim_mean'][k]:.4f}", flush=True)
    if args.consistency:
        fmt = lambda d: "n/a" if d["psnr"] is None else f"{d['psnr']:.3f} dB ({d['n']} px)"  # noqa: E731
        for k, d in sorted(result["consistency"]["per_w"].items(), key=lambda kv: float(kv[0])):
            print(f"[evaluate] w={k}: PSNR co-visible {fmt(d['covisible'])}  disoccluded {fmt(d['disoccluded'])}  "
                  f"background {fmt(d['background'])}", flush=True)
            print(f"[evaluate] w={k}: reprojection PSNR against the input view {fmt(d['reproj'])}  between generated "
                  f"views {fmt(d['pairs'])}", flush=True)
        c = result["consistency"]["gt_ceiling"]
        print(f"[evaluate] ground-truth ceiling: reprojection PSNR {fmt(c['reproj'])}  pairs {fmt(c['pairs'])}",
              flush=True)
    if C > 1:
        db = lambda x: "n/a" if x is None else f"{x:.3f} dB"  # noqa: E731
        num = lambda x, f: "n/a" if x is None else format(x, f)  # noqa: E731
        for k, d in sorted(result["ensemble"]["per_w"].items(), key=lambda kv: float(kv[0])):
            print(f"[evaluate] w={k}: {C} samples: PSNR of the mean image {db(d['psnr_mean_image'])}  of the samples "
                  f"{db(d['psnr_samples'])}  spread {num(d['spread'], '.3e')}  spread-skill "
                  f"{num(d['spread_skill'], '.3f')}", flush=True)
            if args.consistency:
                print(f"[evaluate] w={k}: spread co-visible {num(d['covisible']['spread'], '.3e')}  disoccluded "
                      f"{num(d['disoccluded']['spread'], '.3e')}  background "
                      f"{num(d['background']['spread'], '.3e')}", flush=True)
    if swd is not None:
        x1000 = lambda d: (" ".join(f"{1e3 * v:.2f}" for v in d["levels"]) +  # noqa: E731
                           f" (mean {1e3 * d['mean']:.2f})")
        for k, d in sorted(swd["per_w"].items(), key=lambda kv: float(kv[0])):
            print(f"[evaluate] w={k}: SWD x 1000, fine to coarse: {x1000(d)}", flush=True)
        if "split_floor" in swd:
            print(f"[evaluate] SWD x 1000 between the halves of the ground truth: {x1000(swd['split_floor'])}",
                  flush=True)
    if knn is not None:
        four = lambda d: (f"precision {d['precision']:.3f}  recall {d['recall']:.3f}  density "  # noqa: E731
                          f"{d['density']:.3f}  coverage {d['coverage']:.3f}")
        for k, d in sorted(knn["per_w"].items(), key=lambda kv: float(kv[0])):
            print(f"[evaluate] w={k}: k={knn['k']} pixel-space {four(d)}", flush=True)
        if "split_floor" in knn:
            print(f"[evaluate] between the halves of the ground truth: {four(knn['split_floor'])}", flush=True)
    if memorisation is not None:
        for k, d in sorted(memorisation["per_w"].items(), key=lambda kv: float(kv[0])):
            print(f"[evaluate] w={k}: nearest training image at mse {d['mse_nn_mean']:.3e} (ground truth's: "
                  f"{memorisation['gt_mse_nn_mean']:.3e}); {100 * d['frac_closer_to_train']:.1f}% closer to a "
                  f"training image than to their own ground truth", flush=True)
    if args.field_holdout:
        for k, d in sorted(result["field"]["per_w"].items(), key=lambda kv: float(kv[0])):
            print(f"[evaluate] w={k}: field PSNR {d['field_psnr']:.3f} dB  SSIM {d['field_ssim']:.4f} on the held-out "
                  f"views {args.field_holdout}", flush=True)
        if args.procedural:
            d = result["field"]["gt_field"]
            print(f"[evaluate] ground-truth ceiling: field PSNR {d['field_psnr']:.3f} dB  SSIM "
                  f"{d['field_ssim']:.4f}", flush=True)
        if args.field_reproj:
            rp = lambda d: ("n/a" if d["reproj_psnr"] is None else f"{d['reproj_psnr']:.3f} dB") + \
                f" ({d['reproj_n_clean']} clean px)"  # noqa: E731
            for k, d in sorted(result["field"]["per_w"].items(), key=lambda kv: float(kv[0])):
                print(f"[evaluate] w={k}: reprojection PSNR under the field's depth {rp(d)}", flush=True)
            if args.procedural:
                print(f"[evaluate] ground-truth ceiling: reprojection PSNR under the field's depth "
                      f"{rp(result['field']['gt_field'])}", flush=True)
    print(f"[evaluate] {result['n_images']} images ({result['n_identical']} identical) in "
          f"{result['wall_seconds']:.2f}s -> {os.path.join(args.out, 'metrics.json')}", flush=True)
    return result


def main(argv=None) -> None:
    run(parse(argv))


if __name__ == "__main__":
    main()
