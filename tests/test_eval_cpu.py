"""Evaluation path on the CPU (tiny model): grouped sampling, the evaluate.py
and sampling.py --metrics CLIs, and the validation loss."""
import json
import os

import numpy as np
import pytest
import torch

from distributed_3d_diffusion_pytorch_amd.config import from_dict, make_config, to_dict
from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches, write_synthetic_srn
from distributed_3d_diffusion_pytorch_amd.engine import DiffusionSampler, RecordEntry, Trainer
from distributed_3d_diffusion_pytorch_amd.parallel import DistContext
from helpers import tiny_model
from metrics_oracle import metrics01

TINY_OV = {"model.ch": 32, "model.emb_ch": 64, "model.H": 16, "model.W": 16, "data.imgsize": 16,
           "global_batch": 2, "dtype": "fp32", "backend": "torch", "log_every": 1, "ckpt_every": 0,
           "data.num_workers": 0}
K = torch.tensor([[20.0, 0, 8], [0, 20.0, 8], [0, 0, 1]])


def _rot(a):
    c, s = float(np.cos(a)), float(np.sin(a))
    return torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _signal_model():
    m = tiny_model().eval()
    torch.manual_seed(3)
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().sum() == 0:
                p.normal_(0, 0.05)
    return m


# ------------------------------------------------------------ sample_groups
SPANS = [(0, 2), (2, 5)]
POSES = [[(_rot(0.1), torch.tensor([0.0, 0.0, 1.3])), (_rot(0.5), torch.tensor([0.0, 1.3, 0.0]))],
         [(_rot(-0.7), torch.tensor([1.3, 0.0, 0.0])), (_rot(1.1), torch.tensor([0.5, 0.5, 1.0]))]]
TARGET_R = torch.stack([_rot(0.9), _rot(-0.3)])
TARGET_T = torch.tensor([[1.3, 0.0, 0.0], [0.0, -1.3, 0.0]])


def _records(img, g, swap=False):
    lo, hi = SPANS[g]
    p = POSES[1 - g] if swap else POSES[g]
    return [RecordEntry(img[lo:hi], *p[0]), RecordEntry(img[lo:hi].flip(-1), *p[1])]


def test_sample_groups_equals_per_object_sample():
    """Two objects (chains [0,1] and [2,3,4], two record entries and different
    poses each) in one grouped run == two `sample` runs from fresh samplers
    with the same seed and chain_offset 0 / 2."""
    m = _signal_model()
    g = torch.Generator().manual_seed(11)
    img = torch.rand(5, 3, 16, 16, generator=g) * 2 - 1
    w = torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0])
    group = torch.tensor([0, 0, 1, 1, 1])
    ref = []
    for gi, (lo, hi) in enumerate(SPANS):
        smp = DiffusionSampler(m, timesteps=3, seed=7, chain_offset=lo)
        ref.append(smp.sample(_records(img, gi), TARGET_R[gi], TARGET_T[gi], K, w[lo:hi]))
    ref = torch.cat(ref)
    smp = DiffusionSampler(m, timesteps=3, seed=7)
    out = smp.sample_groups([_records(img, 0), _records(img, 1)], TARGET_R, TARGET_T, K, w, group)
    torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-5)
    # per-group intrinsics [G,3,3] and per-chain conditioning (share_cond=False): same result
    smp = DiffusionSampler(m, timesteps=3, seed=7, share_cond=False)
    out2 = smp.sample_groups([_records(img, 0), _records(img, 1)], TARGET_R, TARGET_T, K[None].expand(2, 3, 3), w,
                             group)
    torch.testing.assert_close(out2, ref, rtol=1e-4, atol=1e-5)
    # the poses matter: groups with swapped record poses differ
    smp = DiffusionSampler(m, timesteps=3, seed=7)
    sw = smp.sample_groups([_records(img, 0, True), _records(img, 1, True)], TARGET_R, TARGET_T, K, w, group)
    assert (sw - ref).abs().max() > 1e-2
    # and so does the chain -> group map (an interleaved map, records in chain order)
    smp = DiffusionSampler(m, timesteps=3, seed=7)
    perm = torch.tensor([0, 2, 1, 3, 4])               # chain order [obj0, obj1, obj0, obj1, obj1]
    rec0 = [RecordEntry(e.img, e.R, e.T) for e in _records(img, 0)]
    rec1 = [RecordEntry(e.img, e.R, e.T) for e in _records(img, 1)]
    out3 = smp.sample_groups([rec0, rec1], TARGET_R, TARGET_T, K, w, torch.tensor([0, 1, 0, 1, 1]))
    assert out3.shape == ref.shape and torch.isfinite(out3).all()
    assert (out3[perm] - ref).abs().max() > 1e-3       # other chain indices -> other noise and weights


def test_sample_groups_rejects_bad_input():
    m = _signal_model()
    img = torch.zeros(5, 3, 16, 16)
    w = torch.zeros(5)
    smp = DiffusionSampler(m, timesteps=2, seed=0)
    with pytest.raises(ValueError):        # group 1 has no chain
        smp.sample_groups([_records(img, 0), _records(img, 1)], TARGET_R, TARGET_T, K, w, torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError):        # records of different lengths
        smp.sample_groups([_records(img, 0), _records(img, 1)[:1]], TARGET_R, TARGET_T, K, w,
                          torch.tensor([0, 0, 1, 1, 1]))


def test_step_group_equals_per_chain_step():
    m = _signal_model()
    g = torch.Generator().manual_seed(5)
    b = 5
    group = torch.tensor([0, 1, 1, 0, 1])
    x = torch.rand(b, 3, 16, 16, generator=g) * 2 - 1
    z = torch.randn(b, 3, 16, 16, generator=g)
    w = torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0])
    Rg = torch.stack([torch.stack([POSES[0][0][0], TARGET_R[0]]), torch.stack([POSES[1][1][0], TARGET_R[1]])])
    Tg = torch.stack([torch.stack([POSES[0][0][1], TARGET_T[0]]), torch.stack([POSES[1][1][1], TARGET_T[1]])])
    Kg = torch.stack([K, K * torch.tensor([[1.1], [0.9], [1.0]])])
    smp = DiffusionSampler(m, timesteps=8, seed=3)
    for k in (0, 4, 7):
        a = smp.step(z, x, Rg, Tg, Kg, w, k, group=group)
        ref = smp.step(z, x, Rg[group], Tg[group], Kg[group], w, k, shared=False)
        torch.testing.assert_close(a, ref, rtol=1e-4, atol=1e-5)
    with pytest.raises(ValueError):
        smp.step(z, x, Rg, Tg, Kg, w, 0, group=torch.tensor([0, 0, 0, 0, 2]))


# -------------------------------------------------------------------- CLIs
@pytest.fixture(scope="module")
def srn_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("srn_eval"))
    write_synthetic_srn(root, num_instances=20, num_views=4, size=16, seed=2)
    return root


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ckpt"))
    cfg = make_config(None, dict(TINY_OV, **{"data.synthetic": True, "out_dir": out}))
    tr = Trainer(cfg, DistContext())
    with torch.no_grad():
        for p in tr.model.parameters():
            if p.abs().sum() == 0:
                p.normal_(0, 0.05)
    tr.save("latest.pt", epoch=0)
    tr.logger.close()
    return os.path.join(out, "latest.pt")


def _png01(path):
    from PIL import Image
    a = np.asarray(Image.open(path), dtype=np.float64) / 255.0
    return torch.from_numpy(a.transpose(2, 0, 1))[None]


def test_evaluate_cli(srn_root, checkpoint, tmp_path):
    import evaluate as evaluate_cli
    out = str(tmp_path / "ev")
    common = ["--model", checkpoint, "--data", srn_root, "--split", "val", "--instances", "2", "--views", "1,3",
              "--w", "0,2", "--timesteps", "2", "--imgsize", "16", "--backend", "torch", "--seed", "4"]
    evaluate_cli.main(common + ["--out", out, "--batch", "2", "--save_png", "--val_batches", "1",
                                "--val_batch_size", "2"])
    res = json.load(open(os.path.join(out, "metrics.json")))
    rows = res["per_image"]
    assert res["n_images"] == len(rows) == 2 * 2 * 2
    assert {(r["instance"], r["view"], r["w"]) for r in rows} == \
        {(i, v, w) for i in {r["instance"] for r in rows} for v in (1, 3) for w in (0.0, 2.0)}
    assert len({r["instance"] for r in rows}) == 2 and len({r["chain"] for r in rows}) == 4
    assert res["args"]["timesteps"] == 2 and np.isfinite(res["val_loss"]) and res["wall_seconds"] > 0
    # every row == the fp64 oracle on the PNGs that were written
    for r in rows:
        d = os.path.join(out, r["instance"], str(r["view"]))
        rm, rs = metrics01(_png01(os.path.join(d, f"{r['w']:g}.png")), _png01(os.path.join(d, "gt.png")))
        assert abs(r["mse"] - float(rm)) <= 1e-6 * float(rm) + 1e-12, (r, float(rm))
        assert abs(r["ssim"] - float(rs)) <= 2e-6, (r, float(rs))
        assert abs(r["psnr"] - 10 * np.log10(1 / float(rm))) < 1e-4
    # the means match the rows
    for w in (0.0, 2.0):
        sel = [r for r in rows if r["w"] == w]
        assert abs(res["psnr_mean"][f"{w:g}"] - np.mean([r["psnr"] for r in sel])) < 1e-9
        assert abs(res["ssim_mean"][f"{w:g}"] - np.mean([r["ssim"] for r in sel])) < 1e-12
    assert res["n_identical"] == 0
    # rows do not depend on how the objects are batched; the autoregressive protocol changes later views only
    out1 = str(tmp_path / "ev1")
    evaluate_cli.main(common + ["--out", out1, "--batch", "1"])
    rows1 = json.load(open(os.path.join(out1, "metrics.json")))["per_image"]
    key = lambda r: (r["instance"], r["view"], r["w"])  # noqa: E731
    for a, b_ in zip(sorted(rows, key=key), sorted(rows1, key=key)):
        assert key(a) == key(b_) and a["chain"] == b_["chain"]
        assert abs(a["ssim"] - b_["ssim"]) < 1e-3 and abs(a["psnr"] - b_["psnr"]) < 0.05
    assert not os.path.exists(os.path.join(out1, rows1[0]["instance"]))      # no PNGs without --save_png
    out2 = str(tmp_path / "ev2")
    evaluate_cli.main(common + ["--out", out2, "--batch", "2", "--autoregressive"])
    rows2 = json.load(open(os.path.join(out2, "metrics.json")))["per_image"]
    same = [abs(a["mse"] - b_["mse"]) < 1e-9 for a, b_ in zip(sorted(rows, key=key), sorted(rows2, key=key))]
    views = [key(a)[1] for a in sorted(rows, key=key)]
    assert all(s for s, v in zip(same, views) if v == 1)


def test_summarize_identical_images():
    from distributed_3d_diffusion_pytorch_amd.engine import summarize
    rows = [{"w": 1.0, "mse": 0.0, "psnr": None, "ssim": 1.0}, {"w": 1.0, "mse": 0.01, "psnr": 20.0, "ssim": 0.5},
            {"w": 2.0, "mse": 0.0, "psnr": None, "ssim": 1.0}]
    s = summarize(rows)
    assert s["n_images"] == 3 and s["n_identical"] == 2
    assert s["psnr_mean"] == {"1": 20.0, "2": None} and s["ssim_mean"] == {"1": 0.75, "2": 1.0}
    json.dumps(s, allow_nan=False)


def test_sampling_cli_metrics(srn_root, checkpoint, tmp_path):
    import sampling as sampling_cli
    inst = sorted(d for d in os.listdir(srn_root) if os.path.isdir(os.path.join(srn_root, d)))[0]
    base = ["--model", checkpoint, "--target", os.path.join(srn_root, inst), "--imgsize", "16", "--timesteps", "2",
            "--w", "0,2", "--max_views", "2", "--backend", "torch"]
    a, b = str(tmp_path / "plain"), str(tmp_path / "scored")
    sampling_cli.main(base + ["--out", a])
    sampling_cli.main(base + ["--out", b, "--metrics"])

    def tree(root):
        return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read()
                for d, _, fs in os.walk(root) for f in fs}

    ta, tb = tree(a), tree(b)
    assert "metrics.json" not in ta and all(k.endswith(".png") for k in ta)
    assert {k: v for k, v in tb.items() if k != "metrics.json"} == ta          # PNG set unchanged, byte for byte
    rows = json.loads(tb["metrics.json"])["per_image"]
    assert [(r["view"], r["chain"]) for r in rows] == [(1, 0), (1, 1), (2, 0), (2, 1)]
    for r in rows:
        d = os.path.join(b, str(r["view"]))
        rm, rs = metrics01(_png01(os.path.join(d, f"{r['chain']}.png")), _png01(os.path.join(d, "gt.png")))
        assert abs(r["mse"] - float(rm)) <= 1e-6 * float(rm) + 1e-12 and abs(r["ssim"] - float(rs)) <= 2e-6


# --------------------------------------------------------- validation loss
def _fit(tmp, val_every):
    cfg = make_config(None, dict(TINY_OV, **{"data.synthetic": True, "out_dir": str(tmp), "max_steps": 4,
                                             "val_every": val_every, "val_batches": 2, "optim.lr": 1e-3}))
    tr = Trainer(cfg, DistContext())
    tr.fit()
    return tr


def test_validation_loss_is_repeatable_and_side_effect_free(tmp_path):
    cfg = make_config(None, dict(TINY_OV, **{"data.synthetic": True, "out_dir": str(tmp_path / "v")}))
    tr = Trainer(cfg, DistContext())
    tr.train_step(*next(SyntheticBatches(2, 16, "cpu", seed=0)))
    batches = tr.make_val_data()[:2]
    cpu_rng, gen = torch.get_rng_state(), tr.gen.get_state()
    before = (tr.flat.data.clone(), tr.flat.grad.clone(), tr.optim.exp_avg.clone(), tr.optim.step_count, tr.step)
    a, b = tr.validation_loss(batches), tr.validation_loss(batches)
    assert a == b and np.isfinite(a) and a > 0
    assert tr.model.training
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(tr.gen.get_state(), gen)
    assert torch.equal(tr.flat.data, before[0]) and torch.equal(tr.flat.grad, before[1])
    assert torch.equal(tr.optim.exp_avg, before[2]) and (tr.optim.step_count, tr.step) == before[3:]
    # another batch order is another draw per batch: the seed follows the batch index
    assert tr.validation_loss(batches[::-1]) != a
    tr.logger.close()


def test_val_every_does_not_change_training(tmp_path):
    t0, t2 = _fit(tmp_path / "a", 0), _fit(tmp_path / "b", 2)
    assert t0.step == t2.step == 4 and t0.optim.step_count == t2.optim.step_count
    assert torch.equal(t0.flat.data, t2.flat.data)
    assert torch.equal(t0.optim.exp_avg, t2.optim.exp_avg) and torch.equal(t0.optim.exp_avg_sq, t2.optim.exp_avg_sq)
    logs = [json.loads(l) for l in open(tmp_path / "b" / "metrics.jsonl")]
    val = [(r["step"], r["val_loss"]) for r in logs if "val_loss" in r]
    assert [s for s, _ in val] == [2, 4] and all(np.isfinite(v) for _, v in val)
    assert not any("val_loss" in json.loads(l) for l in open(tmp_path / "a" / "metrics.jsonl"))


def test_val_data_from_srn_root_and_train_cli(srn_root, tmp_path):
    import train as train_cli
    out = str(tmp_path / "run")
    train_cli.main(["--train_data", srn_root, "--val_data", srn_root, "--out_dir", out, "--steps", "2",
                    "num_epochs=100", "val_every=1", "val_batches=1"] + [f"{k}={v}" for k, v in TINY_OV.items()])
    logs = [json.loads(l) for l in open(os.path.join(out, "metrics.jsonl"))]
    assert [r["step"] for r in logs if "val_loss" in r] == [1, 2]
    ck = torch.load(os.path.join(out, "latest.pt"), weights_only=True)
    assert ck["config"]["data"]["val_path"] == srn_root and ck["config"]["val_every"] == 1


def test_old_checkpoint_config_loads():
    d = to_dict(make_config(None, {"model.ch": 32, "global_batch": 4}))
    for k in ("val_every", "val_batches"):
        d.pop(k)
    d["data"].pop("val_path")
    cfg = from_dict(d)
    assert (cfg.val_every, cfg.val_batches, cfg.data.val_path) == (0, 8, "")
    assert cfg.model.ch == 32 and cfg.global_batch == 4
