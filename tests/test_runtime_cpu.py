"""Runtime pieces added for the multi-GPU headline path and the training
epilogue: the bench launcher, resume state (EMA, RNG, mid-epoch position),
gradient clipping, the metrics stream and the counter-based input draw."""
import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_3d_diffusion_pytorch_amd.config import make_config
from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches, write_synthetic_srn
from distributed_3d_diffusion_pytorch_amd.engine import Trainer
from distributed_3d_diffusion_pytorch_amd.parallel import DistContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY_OV = {"model.ch": 32, "model.emb_ch": 64, "model.H": 16, "model.W": 16, "data.imgsize": 16,
           "global_batch": 2, "dtype": "fp32", "backend": "torch", "log_every": 0, "ckpt_every": 0,
           "data.num_workers": 0, "data.synthetic": True}


def _tiny_bench(gpus, extra=(), omp=2, cwd=ROOT):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env["OMP_NUM_THREADS"] = str(omp)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--device", "cpu", "--ch", "32",
           "--emb_ch", "64", "--imgsize", "16", "--global_batch", "4", "--steps", "2", "--warmup", "1",
           "--dtype", "fp32", "--backend", "torch", *extra]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=cwd)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout          # only rank 0 prints
    return json.loads(lines[0])


def test_bench_self_spawns_ranks():
    """`bench.py --gpus 2` without torchrun launches 2 ranks itself; the JSON
    reports the world size the process group actually has."""
    r = _tiny_bench(2)
    assert r["n_gpus"] == 2 and r["config"]["parallelism"] == "dp2"
    assert r["config"]["dist_backend"] == "gloo" and r["config"]["per_gpu_batch"] == 2
    assert r["value"] > 0 and r["vs_baseline"] is None      # not the headline architecture
    for k in ("metric", "unit", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "dtype", "data"):
        assert k in r


def test_bench_reports_comm_diagnostics_four_ranks():
    """`bench.py --gpus 4 --full`: the JSON carries the gradient-communication record
    a scaling run needs for diagnosis -- the process group's own world size
    and backend, step path, bucket count / sizes / payload, and the exposed
    all-reduce time per step (max over ranks)."""
    r = _tiny_bench(4, ("--grad_dtype", "bf16", "--full"))
    assert r["n_gpus"] == 4
    c = r["comm"]
    assert c["world_pg"] == 4 and c["backend_pg"] == "gloo" and c["active"]
    assert c["step"] == "eager" and c["comm_mode"] == "eager" and "error" not in c, c
    assert c["buckets"] == len(c["bucket_mib"]) >= 1 and abs(sum(c["bucket_mib"]) - c["total_mib"]) < 0.1
    assert c["payload"] == "bf16"
    assert c["exposed_allreduce_ms"] >= 0.0


def test_bench_eight_ranks_full_node_layout():
    """The 8-GPU launch shape of the scaling run, rehearsed with 8 gloo ranks
    on the host: `bench.py --gpus 8 --full` self-spawns 8 ranks, the global batch is
    split 8 ways, every rank's process group has world size 8, and the comm
    record carries the bucket layout (sizes summing to the flat gradient, the
    small first bucket first) and an exposed all-reduce time."""
    r = _tiny_bench(8, ("--global_batch", "8", "--bucket_mb", "0.25", "--full"), omp=1)
    assert r["n_gpus"] == 8 and r["config"]["parallelism"] == "dp8" and r["config"]["per_gpu_batch"] == 1
    c = r["comm"]
    assert c["world_pg"] == 8 and c["backend_pg"] == "gloo" and c["active"] and "error" not in c, c
    assert c["buckets"] == len(c["bucket_mib"]) >= 2, c
    assert abs(sum(c["bucket_mib"]) - c["total_mib"]) < 0.05
    assert c["exposed_allreduce_ms"] >= 0.0 and r["value"] > 0


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run takes no comm record (that is `--full`); `--dump-outputs`
    writes the last timed step's loss, parameters and first moment as float32
    .npy files, and two runs with the same arguments agree exactly (same
    inputs, same sample positions).  The run writes nothing else: its working
    directory (which need not be writable) stays empty."""
    import numpy as np
    runs = []
    cwd = tmp_path / "cwd"
    cwd.mkdir()
    for d in ("a", "b"):
        r = _tiny_bench(1, ("--dump-outputs", str(tmp_path / d)), cwd=str(cwd))
        assert os.listdir(cwd) == []
        assert r["comm"] is None and r["steps"] == 2 and r["ms_per_step"] > 0
        runs.append({n: np.load(tmp_path / d / f"{n}.npy") for n in ("loss", "params", "exp_avg")})
    a, b = runs
    assert sorted(os.listdir(tmp_path / "a")) == ["exp_avg.npy", "loss.npy", "params.npy"]
    for n in a:
        assert a[n].dtype == np.float32 and np.isfinite(a[n]).all() and np.array_equal(a[n], b[n]), n
    assert a["loss"].shape == (1,) and a["params"].shape == a["exp_avg"].shape
    assert np.abs(a["exp_avg"]).max() > 0           # the steps ran: the moment holds gradients


def test_bench_launcher_fails_when_a_rank_dies():
    env = dict(os.environ, D3D_FAULT_AT_STEP="0", D3D_FAULT_RANK="1", OMP_NUM_THREADS="2")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--device", "cpu", "--ch", "32",
           "--emb_ch", "64", "--imgsize", "16", "--global_batch", "4", "--steps", "1", "--warmup", "1",
           "--dtype", "fp32", "--backend", "torch"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode != 0


def _trainer(tmp_path, **ov):
    cfg = make_config(None, dict(TINY_OV, out_dir=str(tmp_path), **ov))
    return Trainer(cfg, DistContext())


def test_grad_clip_matches_torch_clip_grad_norm(tmp_path):
    tr = _trainer(tmp_path, **{"optim.grad_clip": 1e-3, "model.dropout": 0.0, "optim.lr": 1e-3})
    ref = _trainer(tmp_path, **{"model.dropout": 0.0, "optim.lr": 1e-3})
    ref.flat.data.copy_(tr.flat.data)
    batch = next(SyntheticBatches(2, 16, "cpu", seed=3))
    # reference: the same step with torch's clip_grad_norm_ applied to the gradient
    loss = ref.loss_fn(*batch)
    loss.backward()
    total = torch.nn.utils.clip_grad_norm_(ref.model.parameters(), 1e-3)
    assert float(total) > 1e-3                  # the clip is active
    ref.optim.step()
    tr.train_step(*batch)
    torch.testing.assert_close(tr.flat.data, ref.flat.data, rtol=1e-5, atol=1e-7)
    assert abs(float(tr.last_grad_norm) - float(total)) < 1e-5 * float(total)


def test_ema_restarts_from_loaded_weights_and_resumes(tmp_path):
    src = _trainer(tmp_path / "a", **{"optim.ema_halflife_examples": 100.0})
    batch = next(SyntheticBatches(2, 16, "cpu", seed=1))
    for _ in range(3):
        src.train_step(*batch)
    src.save("latest.pt", epoch=0)
    ema_saved = src.optim.ema.clone()
    assert not torch.equal(ema_saved, src.flat.data)
    # resume: the EMA comes back exactly
    res = _trainer(tmp_path / "b", **{"optim.ema_halflife_examples": 100.0, "transfer": str(tmp_path / "a")})
    torch.testing.assert_close(res.optim.ema, ema_saved, rtol=0, atol=0)
    # fine-tune from a checkpoint file: the EMA starts at the loaded weights
    ft = _trainer(tmp_path / "c", **{"optim.ema_halflife_examples": 100.0,
                                     "pretrained": str(tmp_path / "a" / "latest.pt")})
    torch.testing.assert_close(ft.optim.ema, ft.flat.data, rtol=0, atol=0)


def test_mid_epoch_resume_continues_where_it_stopped(tmp_path):
    root = str(tmp_path / "srn")
    write_synthetic_srn(root, num_instances=12, num_views=4, size=16, seed=0)
    ov = dict(TINY_OV, **{"data.synthetic": False, "data.path": root, "global_batch": 2, "num_epochs": 1})
    cfg = make_config(None, dict(ov, out_dir=str(tmp_path / "r"), ckpt_every=2, max_steps=2))
    tr = Trainer(cfg, DistContext())
    tr.fit()
    ck = torch.load(str(tmp_path / "r" / "after_warmup.pt"), weights_only=True)
    assert ck["sampler_epoch"] == 0 and ck["epoch_pos"] == 2 and len(ck["rng"]) == 1
    # the max_steps stop wrote latest.pt at the same mid-epoch position
    ck = torch.load(str(tmp_path / "r" / "latest.pt"), weights_only=True)
    assert ck["sampler_epoch"] == 0 and ck["epoch_pos"] == 2 and ck["epoch_examples"] == 4 and ck["epoch"] == -1
    # resume (find_resume picks latest.pt): epoch 0 continues at batch 2
    cfg2 = make_config(None, dict(ov, out_dir=str(tmp_path / "r"), transfer=str(tmp_path / "r")))
    tr2 = Trainer(cfg2, DistContext())
    assert tr2.step == 2 and tr2.epoch == 0 and tr2.epoch_pos == 2
    tr2.fit()
    # 10 training instances / batch 2 = 5 steps in epoch 0: 2 done before, 3 after
    assert tr2.step == 5


def test_metrics_stream_has_observability_fields(tmp_path):
    cfg = make_config(None, dict(TINY_OV, out_dir=str(tmp_path), log_every=1, max_steps=2, num_epochs=1))
    tr = Trainer(cfg, DistContext())
    tr.fit(steps_per_epoch=2)
    rows = [json.loads(l) for l in open(tmp_path / "metrics.jsonl")]
    assert len(rows) == 2
    for k in ("loss", "lr", "grad_norm", "examples_per_s", "tflops", "allreduce_wait_ms", "data_wait_ms",
              "hbm_peak_gib"):
        assert k in rows[-1], k
    assert rows[-1]["grad_norm"] > 0


def test_input_draw_is_counter_based():
    """Same (seed, global example index) -> same numbers, whatever the split;
    statistics of the draw match train.py:80-100."""
    from distributed_3d_diffusion_pytorch_amd import ops
    img = torch.rand(64, 2, 3, 8, 8) * 2 - 1
    xz, eps, lam, keep = ops.diffusion_inputs(img, 99)
    xz2, eps2, lam2, keep2 = ops.diffusion_inputs(img[40:], 99, e0=40)
    assert torch.equal(eps[40:], eps2) and torch.equal(lam[40:], lam2) and torch.equal(keep[40:], keep2)
    assert torch.equal(xz.view(64, 2, 8, 8, 8)[40:], xz2.view(24, 2, 8, 8, 8))
    assert abs(float(eps.mean())) < 0.05 and abs(float(eps.std()) - 1) < 0.05
    assert torch.all(lam[:, 0] == lam[0, 0]) and abs(float(lam[0, 0]) - 20.0) < 1e-3
    assert torch.all(lam[:, 1] <= 20.0) and torch.all(lam[:, 1] >= -20.01)
    # z_t = alpha z + sigma eps; dropped examples get noise instead of x
    a = torch.sigmoid(lam[:, 1]).sqrt().view(-1, 1, 1, 1)
    s = torch.sigmoid(-lam[:, 1]).sqrt().view(-1, 1, 1, 1)
    zt = xz.view(64, 2, 8, 8, 8)[:, 1, ..., :3].permute(0, 3, 1, 2)
    torch.testing.assert_close(zt, a * img[:, 1] + s * eps)
    x0 = xz.view(64, 2, 8, 8, 8)[:, 0, ..., :3].permute(0, 3, 1, 2)
    assert torch.equal(x0[keep], img[keep, 0]) and not torch.equal(x0[~keep], img[~keep, 0])
    assert 0 < int((~keep).sum()) < 20
    assert float(xz[..., 3:].abs().max()) == 0.0


def test_graph_dropout_seed_matches_eager_formula():
    from distributed_3d_diffusion_pytorch_amd.models.xunet import _next_seed, _GOLDEN
    from helpers import tiny_model
    m = tiny_model()
    blk = m.xunetblocks[0][0].resnetblock
    m.set_dropout_seed(0)
    baked = _next_seed(blk)
    m.set_dropout_seed(12345)
    assert _next_seed(blk) == (baked + 12345 * _GOLDEN) & 0xFFFFFFFFFFFFFFFF


def test_multi_rank_sampling_matches_single_rank(tmp_path):
    """`sampling.py --gpus 2` (gloo ranks, chains sharded, rank 0 gathers)
    writes the same PNG set as the single-rank run with the same seed."""
    import numpy as np
    from PIL import Image
    tr = _trainer(tmp_path / "ck", **{"model.dropout": 0.0})
    with torch.no_grad():               # non-trivial output: un-zero the zero-init layers
        g = torch.Generator().manual_seed(0)
        for p in tr.model.parameters():
            if p.abs().sum() == 0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    tr.save("latest.pt", epoch=0)
    root = str(tmp_path / "srn")
    write_synthetic_srn(root, num_instances=1, num_views=3, size=16, seed=2)
    inst = os.path.join(root, sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))[0])
    # host ranks on every machine: with a GPU visible sampling.py would put both ranks of the 2-rank run on
    # device 0 of a one-GPU host, which RCCL refuses
    env = dict(os.environ, OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    env.pop("WORLD_SIZE", None)
    outs = {}
    for gpus in (1, 2):
        out = str(tmp_path / f"s{gpus}")
        cmd = [sys.executable, os.path.join(ROOT, "sampling.py"), "--model", str(tmp_path / "ck" / "latest.pt"),
               "--target", inst, "--out", out, "--imgsize", "16", "--timesteps", "3", "--w", "0,1,2",
               "--max_views", "2", "--backend", "torch", "--gpus", str(gpus), "--seed", "5"]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[gpus] = out
    for k in (1, 2):
        for i in range(3):
            a = np.asarray(Image.open(os.path.join(outs[1], str(k), f"{i}.png")), dtype=np.int32)
            b = np.asarray(Image.open(os.path.join(outs[2], str(k), f"{i}.png")), dtype=np.int32)
            assert np.abs(a - b).max() <= 1, (k, i, np.abs(a - b).max())
    # the chains differ from each other (the test is not vacuous)
    c0 = np.asarray(Image.open(os.path.join(outs[1], "1", "0.png")), dtype=np.int32)
    c2 = np.asarray(Image.open(os.path.join(outs[1], "1", "2.png")), dtype=np.int32)
    assert np.abs(c0 - c2).max() > 5
