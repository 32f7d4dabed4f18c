"""The radiance-field consistency score on the CPU (the float64 torch form of
csrc/field.hip): closed forms, the gradient against central differences,
consistent views against views with shifted poses, and the CLI."""
import json
import math
import os

import pytest
import torch

from distributed_3d_diffusion_pytorch_amd import ops
from distributed_3d_diffusion_pytorch_amd.data import procedural as P
from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T

O = torch.tensor([[0.3, 0.1, -2.0], [0.1, -0.2, 0.3], [5.0, 5.0, 5.0], [1.5, 0.0, -3.0]])
D = torch.tensor([[0.0, 0.0, 1.0], [0.36, 0.48, -0.8], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


@pytest.mark.parametrize("S", [1, 7, 64])
def test_closed_forms(S):
    raw = 0.3
    grid = torch.full((4, 4, 4, 4), raw)
    o = torch.tensor([[0.25, 0.125, -2.0], [0.125, -0.25, 0.25], [5.0, 5.0, 5.0], [1.5, 0.0, -3.0]])
    d = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    C = T._field_march(grid.double(), o, d, S, 1.0, torch.float64)
    sigma, c = math.log1p(math.exp(float(torch.tensor(raw)))), 1 / (1 + math.exp(-float(torch.tensor(raw))))
    # chords: straight through (2), from inside to the face z = -1 (1.25), and two misses
    for r, chord in ((0, 2.0), (1, 1.25)):
        e = math.exp(-sigma * chord)
        assert (C[r] - ((1 - e) * c + e)).abs().max() <= 1e-12
    assert torch.equal(C[2:], torch.ones(2, 3, dtype=torch.float64))
    empty = grid.clone()
    empty[..., 3] = -40.0
    assert (ops.field_render(empty, o, d, samples=S) == 1).all()
    L, g = ops.field_loss_grad(grid, o[2:], d[2:], torch.zeros(2, 3), samples=S)
    assert L.item() == 2 * 3 * 0.25 and L.dtype == torch.float64 and g.dtype == torch.float32 and not g.any()


def test_gradient_matches_central_differences():
    G, S = 3, 5
    grid = (T.u01(3, torch.arange(G ** 3 * 4)) * 4 - 2).reshape(G, G, G, 4).contiguous()
    y = (T.u01(4, torch.arange(12)) * 2 - 1).reshape(4, 3)
    L, g = ops.field_loss_grad(grid, O, D, y, samples=S)

    def loss(gr):
        return (T._field_march(gr, O, D, S, 1.0, torch.float64) - (y.double() + 1) / 2).square().sum()

    assert L.item() == loss(grid.double()).item()
    num, eps = torch.zeros(grid.numel(), dtype=torch.float64), 1e-6
    for i in range(grid.numel()):
        e = torch.zeros(grid.numel(), dtype=torch.float64)
        e[i] = eps
        num[i] = (loss(grid.double() + e.view_as(grid)) - loss(grid.double() - e.view_as(grid))) / (2 * eps)
    # central differences: O(eps^2) truncation + 1e-16 / eps rounding; the op's gradient is rounded to fp32
    assert g.abs().max() > 1e-2
    assert (num - g.flatten().double()).abs().max() <= 1e-8 + 6e-8 * g.abs().max().item()


def test_consistent_views_beat_shifted_poses():
    """Procedural ground truth of 2 objects at 24 x 24, 10 train / 2 test views, G = 24: the same images with
    the training poses shifted by one view score lower (profiles/field/README.md records the values)."""
    from distributed_3d_diffusion_pytorch_amd.engine import field_consistency
    fit = dict(grid=24, samples=32, iters=60, rays_per_iter=1024, lr=0.3)
    train, test = list(range(10)), [10, 11]
    K = P.srn_intrinsics().float()
    for obj in (1, 3):
        img, R, t, _ = P.render_views(1234, [obj] * 12, list(range(12)), 24, "cpu", 3)
        img, R, t = img.float(), R.float(), t.float()
        good = field_consistency(img, R, t, K, train, test, **fit)
        Rs, ts = R.clone(), t.clone()
        Rs[train], ts[train] = R[train].roll(1, 0), t[train].roll(1, 0)
        bad = field_consistency(img, Rs, ts, K, train, test, **fit)
        print(f"object {obj}: consistent {good['field_psnr']:.3f} dB, shifted {bad['field_psnr']:.3f} dB")
        assert good["field_psnr"] > bad["field_psnr"]
        assert (good["n_train"], good["n_test"]) == (10, 2) and math.isfinite(good["fit_loss"])
    with pytest.raises(ValueError):
        field_consistency(img, R, t, K, [0, 1], [2], **fit)


def test_cli(tmp_path):
    """evaluate.py --field_holdout: the field block and gt_field; refused together with --samples 2."""
    import evaluate as evaluate_cli
    from distributed_3d_diffusion_pytorch_amd.config import make_config
    from distributed_3d_diffusion_pytorch_amd.engine import Trainer
    from distributed_3d_diffusion_pytorch_amd.parallel import DistContext
    for bad in (["--samples", "2"], ["--views", "1,2,3"], ["--field_holdout", "9"]):
        with pytest.raises(SystemExit) as ex:
            evaluate_cli.parse(["--views", "1,2,3,4", "--field_holdout", "4"] + bad)
        assert ex.value.code != 0
    run = str(tmp_path / "run")
    tr = Trainer(make_config(None, {"model.ch": 32, "model.emb_ch": 64, "model.H": 16, "model.W": 16,
                                    "data.imgsize": 16, "global_batch": 2, "dtype": "fp32", "backend": "torch",
                                    "log_every": 1, "ckpt_every": 0, "data.num_workers": 0, "data.procedural": True,
                                    "out_dir": run}), DistContext())
    tr.save("latest.pt", epoch=0)
    tr.logger.close()
    ev = str(tmp_path / "eval")
    res = evaluate_cli.run(evaluate_cli.parse(
        ["--model", os.path.join(run, "latest.pt"), "--procedural", "--proc_seed", "4", "--proc_objects", "40",
         "--instances", "2", "--views", "1,2,3,4", "--field_holdout", "4", "--field_grid", "8", "--field_iters", "3",
         "--w", "0,2", "--timesteps", "2", "--imgsize", "16", "--backend", "torch", "--out", ev]))
    with open(os.path.join(ev, "metrics.json")) as f:
        block = json.load(f)["field"]
    assert block == res["field"] and set(block) == {"per_w", "rows", "gt_field"}
    assert set(block["per_w"]) == {"0", "2"} and len(block["rows"]) == 4 and len(block["gt_field"]["rows"]) == 2
    for r in block["rows"] + block["gt_field"]["rows"] + list(block["per_w"].values()) + [block["gt_field"]]:
        assert math.isfinite(r["field_psnr"]) and math.isfinite(r["field_ssim"]) and math.isfinite(r["fit_loss"])
    assert all((r["n_train"], r["n_test"]) == (3, 1) for r in block["rows"])
