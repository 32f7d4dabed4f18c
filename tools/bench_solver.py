#!/usr/bin/env python
"""Per-step time of the graph-replayed sampler for each update rule.

    python tools/bench_solver.py --solvers ancestral,ddim,dpmpp2m --timesteps 256

The set-up of ``bench.py --mode sample`` (random-init X-UNet ch128 at 64x64, 64
chains, two record entries, shared conditioning, a short warm-up run through
the same path and one timed ``sample``), with the solver as the only variable.
``--repeat N`` times every solver N times in turn (A/A spread).  Prints one
JSON line per run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--solvers", default="ancestral,ddim,dpmpp2m")
    ap.add_argument("--eta", type=float, default=0.0, help="DDIM noise level")
    ap.add_argument("--spacing", default="t", choices=["t", "logsnr"])
    ap.add_argument("--timesteps", type=int, default=256)
    ap.add_argument("--sample_batch", type=int, default=64)
    ap.add_argument("--imgsize", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=1)
    args = ap.parse_args(argv)

    import torch
    from distributed_3d_diffusion_pytorch_amd.models import XUNet
    from distributed_3d_diffusion_pytorch_amd.engine import DiffusionSampler, RecordEntry
    from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    if not torch.cuda.is_available():
        raise SystemExit("bench_solver needs a GPU")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    S, b = args.imgsize, args.sample_batch
    model = XUNet(H=S, W=S, ch=128).to(dev)
    model.compute_dtype = torch.bfloat16
    model.eval()
    img, R, T, K = next(SyntheticBatches(b, S, dev, seed=0))
    record = [RecordEntry(img[:, 0].contiguous(), R[0, 0].float(), T[0, 0].float()),
              RecordEntry(img[:, 1].contiguous(), R[0, 1].float(), T[0, 1].float())]
    w = torch.arange(b, dtype=torch.float32) % 8
    target = (R[1, 0].float(), T[1, 0].float(), K[0].float(), w)
    for rep in range(args.repeat):
        for solver in args.solvers.split(","):
            kw = {"device": dev, "solver": solver, "spacing": args.spacing,
                  "eta": args.eta if solver == "ddim" else 0.0}
            DiffusionSampler(model, max(2, args.warmup), seed=1, **kw).sample(record, *target)
            smp = DiffusionSampler(model, args.timesteps, seed=0, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = smp.sample(record, *target)       # includes this sampler's graph capture, as bench.py does
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"solver": solver, "eta": kw["eta"], "spacing": args.spacing, "repeat": rep,
                              "timesteps": args.timesteps, "chains": b, "image_size": S, "seconds": round(dt, 3),
                              "ms_per_step": round(1e3 * dt / args.timesteps, 3),
                              "finite": bool(torch.isfinite(out).all()),
                              "fallbacks": dict(hip_impl.FALLBACKS)}), flush=True)


if __name__ == "__main__":
    main()
