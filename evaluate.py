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
``mean_<w>.png`` and ``std_<w>.png``.  Single process.
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
    ap.add_argument("--timesteps", type=int, default=256)
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


def run(args) -> dict:
    import torch
    from distributed_3d_diffusion_pytorch_amd import ops
    from distributed_3d_diffusion_pytorch_amd.engine import evaluate_objects, load_objects, summarize
    from distributed_3d_diffusion_pytorch_amd.engine.evaluate import load_model, resolve_prediction

    if args.consistency and not args.procedural:
        raise ValueError("--consistency needs --procedural: SRN data carries no geometry to score against")
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
    rows, _, *rest = evaluate_objects(model, objects, args.input_view, views, w, args.timesteps, args.batch,
                                      args.autoregressive, args.seed, dev,
                                      on_view=write_pngs if args.save_png else None, solver=args.sampler,
                                      eta=args.eta, spacing=args.spacing, prediction=prediction,
                                      consistency=args.consistency, samples=C)
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
    print(f"[evaluate] {result['n_images']} images ({result['n_identical']} identical) in "
          f"{result['wall_seconds']:.2f}s -> {os.path.join(args.out, 'metrics.json')}", flush=True)
    return result


def main(argv=None) -> None:
    run(parse(argv))


if __name__ == "__main__":
    main()
