"""v-prediction and min-SNR loss weighting, CPU side: the eps <-> v identities
in fp64 through cfg_posterior / solver_step, the v target of the training-input
draw, the weights against an fp64 oracle, micro-batching, the CLIs and the
compat module."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from distributed_3d_diffusion_pytorch_amd.config import DiffusionConfig, make_config, to_dict, from_dict
from distributed_3d_diffusion_pytorch_amd.diffusion import (cfg_posterior, solver_step, solver_row, sampler_logsnrs,
                                                            diffusion_loss, min_snr_weight, v_target)
from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T
from distributed_3d_diffusion_pytorch_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
LAMBDAS = [-20.0, math.log(5.0) - 0.01, math.log(5.0) + 0.01, 0.0, 20.0]
TINY_OV = {"model.ch": 32, "model.emb_ch": 64, "model.H": 16, "model.W": 16, "data.imgsize": 16,
           "global_batch": 2, "dtype": "fp32", "backend": "torch", "log_every": 1, "ckpt_every": 2,
           "data.num_workers": 0}
V_MINSNR = {"diffusion.prediction": "v", "diffusion.loss_weight": "min_snr"}


def _sig(x):
    return 1.0 / (1.0 + math.exp(-x)) if x >= 0 else math.exp(x) / (1.0 + math.exp(x))


# ------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("spacing", ["t", "logsnr"])
def test_v_and_eps_routes_agree_fp64(spacing):
    """eps = sigma z + alpha v at fixed z, and CFG is linear in either output:
    the posterior and every solver step computed from (v_c, v_u) equal those
    from the matching (eps_c, eps_u), at every step of a 16-step schedule --
    step 0 (lambda = -20) included.  1e-8: the eps route's own cancellation
    there is ~2^-53 / alpha = 2.5e-12; a swapped alpha / sigma or a sign is O(1)."""
    torch.manual_seed(0)
    b, S, steps = 4, 8, 16
    w = torch.tensor([0.0, 1.0, 3.0, 5.0], dtype=F64)
    lam, lam_next = (t.tolist() for t in sampler_logsnrs(steps, dtype=F64, spacing=spacing))
    z = torch.randn(b, 3, S, S, dtype=F64)
    vc, vu = torch.randn(b, 3, S, S, dtype=F64), torch.randn(b, 3, S, S, dtype=F64)
    hist = torch.rand(b, 3, S, S, dtype=F64) * 2 - 1
    noise = torch.randn(b, 3, S, S, dtype=F64)
    seen_inside = 0
    for k in range(steps):
        alpha, sigma = math.sqrt(_sig(lam[k])), math.sqrt(_sig(-lam[k]))
        ec, eu = sigma * z + alpha * vc, sigma * z + alpha * vu
        mv, varv = cfg_posterior(z, vc, vu, w, torch.tensor(lam[k], dtype=F64), torch.tensor(lam_next[k], dtype=F64),
                                 prediction="v")
        me, vare = cfg_posterior(z, ec, eu, w, torch.tensor(lam[k], dtype=F64), torch.tensor(lam_next[k], dtype=F64))
        assert (mv - me).abs().max().item() < 1e-8, (k, (mv - me).abs().max().item())
        assert torch.equal(varv, vare)
        rows = [solver_row(lam, lam_next, k, "ddim", 0.0), solver_row(lam, lam_next, k, "ddim", 0.7),
                solver_row(lam, lam_next, k, "dpmpp2m"), solver_row(lam, lam_next, k, "dpmpp2m", first_order=True)]
        for i, row in enumerate(rows):
            row = torch.tensor(row, dtype=F64)
            for h in (hist, None):
                if h is None and float(row[5]) != 0.0:
                    continue
                zv, xv = solver_step(z, vc, vu, w, h, row, noise, prediction="v")
                ze, xe = solver_step(z, ec, eu, w, h, row, noise)
                dz, dx = (zv - ze).abs().max().item(), (xv - xe).abs().max().item()
                assert dz < 1e-8 and dx < 1e-8, (k, i, dz, dx)
                x_direct = (alpha * z - sigma * ((1 + w.view(-1, 1, 1, 1)) * vc - w.view(-1, 1, 1, 1) * vu))
                assert (xv - x_direct.clamp(-1, 1)).abs().max().item() < 1e-12
                seen_inside += int((xv.abs() < 1).any())
    assert seen_inside > 0                     # the clamp did not hide everything
    with pytest.raises(ValueError):
        cfg_posterior(z, vc, vu, w, torch.tensor(0.0), torch.tensor(1.0), prediction="x0")
    with pytest.raises(ValueError):
        solver_step(z, vc, vu, w, None, solver_row(lam, lam_next, 0), None, prediction="x0")


# --------------------------------------------------------------- 2. target
def test_v_target_of_training_input_draw():
    torch.manual_seed(1)
    seed = 0xDEADBEEF12345678
    img = torch.rand(5, 2, 3, 12, 12) * 2 - 1
    xz, v, lam, keep = T.diffusion_inputs(img, seed, e0=5, prediction="v")
    xe, eps, le, ke = T.diffusion_inputs(img, seed, e0=5)
    assert torch.equal(xz, xe) and torch.equal(lam, le) and torch.equal(keep, ke)
    l64 = le[:, 1].double()
    alpha = torch.sqrt(torch.sigmoid(l64)).float().view(5, 1, 1, 1)
    sigma = torch.sqrt(torch.sigmoid(-l64)).float().view(5, 1, 1, 1)
    assert torch.equal(v, alpha * eps - sigma * img[:, 1])
    assert (v - eps).abs().max().item() > 0.1
    # with z_t of the draw: eps = sigma z_t + alpha v and z = alpha z_t - sigma v
    zt = alpha * img[:, 1] + sigma * eps
    assert (sigma * zt + alpha * v - eps).abs().max().item() < 1e-5
    assert (alpha * zt - sigma * v - img[:, 1]).abs().max().item() < 1e-5
    xs, vs, ls, ks = T.diffusion_inputs(img[3:], seed, e0=8, prediction="v")
    assert torch.equal(vs, v[3:]) and torch.equal(xs, xz[6:]) and torch.equal(ls, lam[3:]) and torch.equal(ks, keep[3:])
    # the public entry point and the schedule helper give the same target
    assert torch.equal(ops.diffusion_inputs(img, seed, e0=5, prediction="v")[1], v)
    assert (v_target(img[:, 1], le[:, 1], eps) - v).abs().max().item() < 1e-5
    with pytest.raises(ValueError):
        T.diffusion_inputs(img, seed, prediction="x0")


# -------------------------------------------------------------- 3. weights
def _oracle_weight(lam: float, prediction: str, gamma: float) -> float:
    if prediction == "eps":
        return min(1.0, gamma * math.exp(-lam))
    return min(_sig(lam), gamma * _sig(-lam))


def _oracle_loss(y, target, lams, prediction, loss_type, gamma):
    d = (y.double() - target.double())
    if loss_type == "l2":
        el = d * d
    elif loss_type == "l1":
        el = d.abs()
    else:
        el = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)
    per = el.flatten(1).mean(1)
    return sum(_oracle_weight(l, prediction, gamma) * float(p) for l, p in zip(lams, per)) / len(lams)


@pytest.mark.parametrize("gamma", [1.0, 5.0])
@pytest.mark.parametrize("loss_type", ["l2", "l1", "huber"])
@pytest.mark.parametrize("prediction", ["eps", "v"])
def test_min_snr_weights_match_fp64_oracle(prediction, loss_type, gamma):
    torch.manual_seed(2)
    B, S = len(LAMBDAS), 6
    y = torch.zeros(B, S, S, 8)
    y[..., :3] = torch.randn(B, S, S, 3) * 1.5
    target = torch.randn(B, 3, S, S)
    lam = torch.tensor(LAMBDAS)
    logsnr = torch.stack([torch.full_like(lam, 20.0), lam], 1)
    kw = dict(prediction=prediction, loss_weight="min_snr", gamma=gamma)
    want = _oracle_loss(y[..., :3].permute(0, 3, 1, 2), target, LAMBDAS, prediction, loss_type, gamma)
    got_ops = float(ops.diff_loss_nhwc(y, target, loss_type, logsnr=logsnr, **kw))
    got_sched = float(diffusion_loss(target, y[..., :3].permute(0, 3, 1, 2), loss_type, logsnr=lam, **kw))
    assert abs(got_ops - want) <= 1e-6 * abs(want), (got_ops, want)
    assert abs(got_sched - want) <= 1e-6 * abs(want), (got_sched, want)
    # the weights themselves, where neither form may overflow or cancel
    wts = min_snr_weight(torch.tensor(LAMBDAS, dtype=F64), prediction, gamma).tolist()
    for l, wv in zip(LAMBDAS, wts):
        o = _oracle_weight(l, prediction, gamma)
        assert math.isfinite(wv) and abs(wv - o) <= 1e-12 * o, (l, wv, o)
    # the kink at SNR = gamma sits between the two lambdas around ln 5
    if gamma == 5.0:
        o = [_oracle_weight(l, prediction, gamma) * (math.exp(l) if prediction == "eps" else 1.0 / _sig(-l))
             for l in LAMBDAS[1:3]]                       # = min(SNR, gamma)
        assert o[0] < 5.0 and abs(o[1] - 5.0) < 1e-9
    # "none" is exactly the unweighted call, with or without a logsnr
    plain = ops.diff_loss_nhwc(y, target, loss_type)
    assert torch.equal(ops.diff_loss_nhwc(y, target, loss_type, logsnr=logsnr, prediction=prediction,
                                          loss_weight="none", gamma=gamma), plain)
    assert torch.equal(diffusion_loss(target, y[..., :3].permute(0, 3, 1, 2), loss_type, logsnr=lam,
                                      prediction=prediction), diffusion_loss(target, y[..., :3].permute(0, 3, 1, 2),
                                                                             loss_type))
    with pytest.raises(ValueError):
        ops.diff_loss_nhwc(y, target, loss_type, **kw)
    with pytest.raises(ValueError):
        diffusion_loss(target, y[..., :3].permute(0, 3, 1, 2), loss_type, **kw)
    with pytest.raises(ValueError):
        ops.diff_loss_nhwc(y, target, loss_type, logsnr=logsnr, loss_weight="sigmoid")
    with pytest.raises(ValueError):
        ops.diff_loss_nhwc(y, target, loss_type, logsnr=logsnr, prediction="x0", loss_weight="min_snr")


def test_config_fields_defaults_and_validation():
    dc = DiffusionConfig()
    assert (dc.prediction, dc.loss_weight, dc.min_snr_gamma) == ("eps", "none", 5.0)
    cfg = make_config(None, dict(TINY_OV, **V_MINSNR, **{"diffusion.min_snr_gamma": "3.5"}))
    assert (cfg.diffusion.prediction, cfg.diffusion.loss_weight, cfg.diffusion.min_snr_gamma) == ("v", "min_snr", 3.5)
    d = to_dict(cfg)
    assert from_dict(d).diffusion.prediction == "v"
    for key in ("prediction", "loss_weight", "min_snr_gamma"):       # a checkpoint from before the fields
        del d["diffusion"][key]
    old = from_dict(d).diffusion
    assert (old.prediction, old.loss_weight, old.min_snr_gamma) == ("eps", "none", 5.0)
    from distributed_3d_diffusion_pytorch_amd.engine import Trainer, DiffusionSampler
    from distributed_3d_diffusion_pytorch_amd.parallel import DistContext
    for bad in ({"diffusion.prediction": "x0"}, {"diffusion.loss_weight": "p2"}):
        with pytest.raises(ValueError):
            Trainer(make_config(None, dict(TINY_OV, **bad)), DistContext())
    with pytest.raises(ValueError):
        DiffusionSampler(torch.nn.Linear(1, 1), timesteps=4, prediction="x0")


# ------------------------------------------------------- 4. micro-batching
def test_micro_batching_matches_full_batch_v_min_snr():
    """The weights are not normalised by their sum, so two micro-batches of 2
    reproduce the full batch of 4 under v + min_snr too (the pattern of
    test_micro_batching_matches_full_batch); and the objective is another one
    than the default."""
    from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches
    from distributed_3d_diffusion_pytorch_amd.engine import Trainer
    from distributed_3d_diffusion_pytorch_amd.parallel import DistContext
    batch = next(SyntheticBatches(4, 16, "cpu", seed=0))
    grads, losses, params = [], [], []
    for mb, extra in ((0, V_MINSNR), (2, V_MINSNR), (0, {})):
        cfg = make_config(None, dict(TINY_OV, **{"global_batch": 4, "micro_batch": mb, "model.dropout": 0.0,
                                                 "optim.lr": 1e-3}, **extra))
        tr = Trainer(cfg, DistContext())
        grads_step = {}
        tr.optim.on_step.insert(0, lambda tr=tr, d=grads_step: d.setdefault("g", tr.flat.grad.clone()))
        losses.append(float(tr.train_step(*batch)))
        grads.append(grads_step["g"])
        params.append(tr.flat.data.clone())
    assert abs(losses[0] - losses[1]) < 1e-6 * max(1.0, abs(losses[0])), losses
    assert grads[0].abs().max() > 0
    torch.testing.assert_close(grads[1], grads[0], rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(params[1], params[0], rtol=1e-5, atol=1e-7)
    assert abs(losses[2] - losses[0]) > 0.05 * abs(losses[2]), losses


# --------------------------------------------------------- 5. CLI round trip
def test_cli_round_trip_v_min_snr(tmp_path, capsys):
    import train as train_cli
    import sampling as sampling_cli
    from distributed_3d_diffusion_pytorch_amd.data import write_synthetic_srn
    root = str(tmp_path / "srn")
    write_synthetic_srn(root, num_instances=5, num_views=4, size=32, seed=1)
    out = str(tmp_path / "run")
    ov = [f"{k}={v}" for k, v in dict(TINY_OV, **V_MINSNR).items()]
    train_cli.main(["--preset", "chairs32_cpu", "--train_data", root, "--out_dir", out, "--steps", "2",
                    "num_epochs=100"] + ov)
    ck = torch.load(os.path.join(out, "latest.pt"), weights_only=True)
    assert ck["step"] == 2
    dc = ck["config"]["diffusion"]
    assert (dc["prediction"], dc["loss_weight"], dc["min_snr_gamma"]) == ("v", "min_snr", 5.0)
    inst = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))[0]
    common = ["--model", os.path.join(out, "latest.pt"), "--target", os.path.join(root, inst), "--imgsize", "16",
              "--timesteps", "2", "--w", "0,2", "--max_views", "1", "--backend", "torch", "--metrics"]
    capsys.readouterr()
    sampling_cli.main(common + ["--out", str(tmp_path / "auto")])
    assert "prediction v" in capsys.readouterr().out
    sampling_cli.main(common + ["--out", str(tmp_path / "eps"), "--prediction", "eps"])
    assert "prediction eps" in capsys.readouterr().out
    sampling_cli.main(common + ["--out", str(tmp_path / "v"), "--prediction", "v"])
    png = {d: open(str(tmp_path / d / "1" / "1.png"), "rb").read() for d in ("auto", "eps", "v")}
    assert png["auto"] == png["v"] and png["auto"] != png["eps"]
    assert json.load(open(str(tmp_path / "auto" / "metrics.json")))["prediction"] == "v"
    assert json.load(open(str(tmp_path / "eps" / "metrics.json")))["prediction"] == "eps"
    # resuming under the other objective must fail, naming both
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--preset", "chairs32_cpu", "--train_data",
                        root, "--transfer", out, "--steps", "3", "num_epochs=100"] +
                       [f"{k}={v}" for k, v in dict(TINY_OV, **{"diffusion.prediction": "eps"}).items()],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode != 0
    assert "'v'" in r.stderr and "'eps'" in r.stderr and "prediction" in r.stderr, r.stderr[-2000:]
    assert torch.load(os.path.join(out, "latest.pt"), weights_only=True)["step"] == 2
    # ... and under its own it continues
    train_cli.main(["--preset", "chairs32_cpu", "--train_data", root, "--transfer", out, "--steps", "3",
                    "num_epochs=100"] + ov)
    assert torch.load(os.path.join(out, "latest.pt"), weights_only=True)["step"] == 3


def test_checkpoint_without_config_means_eps():
    from distributed_3d_diffusion_pytorch_amd.engine.evaluate import resolve_prediction
    from distributed_3d_diffusion_pytorch_amd.utils import checkpoint_prediction
    assert checkpoint_prediction({"model": {}}) == "eps"
    assert checkpoint_prediction({"config": {"diffusion": {"loss_type": "l2"}}}) == "eps"
    assert checkpoint_prediction({"config": {"diffusion": {"prediction": "v"}}}) == "v"
    assert resolve_prediction("auto", None) == "eps" and resolve_prediction("v", None) == "v"
    cfg = make_config(None, V_MINSNR)
    assert resolve_prediction("auto", cfg) == "v" and resolve_prediction("eps", cfg) == "eps"


# ---------------------------------------------------------------- 6. compat
def test_compat_diff3d_v_prediction():
    from distributed_3d_diffusion_pytorch_amd.compat import Diff3D
    from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches
    torch.manual_seed(3)
    m = Diff3D(image_size=16, batch_size=2, prediction="v")
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().sum() == 0:
                p.normal_(0, 0.02)
    batch = next(SyntheticBatches(2, 16, "cpu", seed=0))
    seen = {}
    fwd = m.forward

    def spy(in_x, noise=None, cond_prob=0.1):
        seen["noise"] = noise
        seen["pred"] = fwd(in_x, noise=noise, cond_prob=cond_prob)
        return seen["pred"]

    m.forward = spy
    loss = m.training_step(batch)
    want_target = v_target(batch[0][:, 1], m.last_logsnr, seen["noise"])
    assert torch.equal(loss, diffusion_loss(want_target, seen["pred"]))
    assert not torch.equal(loss, diffusion_loss(seen["noise"], seen["pred"]))
    assert torch.isfinite(loss) and loss.requires_grad
    out = m.sample(None, batch[0][:, 0], batch[1], batch[2], batch[3], 2.0, 2, return_all=False)
    assert out.shape == (2, 3, 16, 16) and torch.isfinite(out).all()
    with pytest.raises(ValueError):
        Diff3D(image_size=16, prediction="x0")
