"""ops.depth_consistency on the CPU (the float64 torch form of
csrc/depth_consistency.hip): closed-form properties on a view paired with its
exact copy, the argument checks, and the score end to end through evaluate.py."""
import json
import math
import os

import pytest
import torch

from distributed_3d_diffusion_pytorch_amd import ops
from distributed_3d_diffusion_pytorch_amd.data import procedural as P

H, W, TOL = 12, 20, 0.05


@pytest.fixture(scope="module")
def twin():
    """One rendered view, twice: same pose, image and true depth."""
    R, t = P.procedural_pose(1234, [1], [0])
    K = P.srn_intrinsics()[None]
    img, depth, _ = ops.scene_render(P.procedural_scene(1234, [1]), R, t, K, H, W, aa=2, return_aux=True)
    two = lambda x: x[None].expand(1, 2, *x.shape[1:]).contiguous()  # noqa: E731
    return dict(depth=two(depth), images=two(img), K=K, R=two(R), t=two(t))


@pytest.mark.parametrize("nudge", [0.0, 1e-6])
def test_copy_is_covisible_and_exact(twin, nudge):
    """A pixel of an exact copy lands on its own centre up to the rounding of u, v (a few ulp of W: below 1e-12
    pixels), so its footprint starts at the pixel with fx = 1e-12 or one tap lower with fx = 1 - 1e-12: the warp is
    the target pixel within 1e-12 of the colour range, but which tap the floor names -- and so the inside rule at the
    image border -- is decided by that rounding.  nudge moves the source camera by 1e-6 along its own -x and -y: every
    landing moves by 1e-5 pixels (focal 12 to 20 pixels over a depth of about 1.3) towards +x, +y, every footprint
    starts at its pixel, and the border is decided: the last row and column are hidden, all other hit pixels
    co-visible.  Bounds: ((fx + fy) 2 / 2)^2 per channel over 3 H W terms, and the depth likewise."""
    a = dict(twin)
    if nudge:
        a["t"] = twin["t"].clone()
        a["t"][0, 1] -= nudge * (twin["R"][0, 1, :, 0] + twin["R"][0, 1, :, 1])
    stats, cls = ops.depth_consistency(**a, tol=TOL, return_class=True)
    hit = torch.isfinite(twin["depth"][0, 0])
    inner, core = torch.zeros_like(hit), torch.zeros_like(hit)
    inner[:-1, :-1], core[1:-1, 1:-1] = True, True
    shift = 4e-5 if nudge else 1e-12
    assert 0 < hit.sum() < hit.numel() and "depth_consistency" in ops.__all__
    assert (cls[0, 0, 1][hit & core] >= 2).all() and (cls[0, 0, 1][~hit] == 0).all() and stats[0, 0, 1, 3] > 0
    assert (stats[0, 0, 1, 4:6] <= 3 * H * W * shift ** 2).all() and stats[0, 0, 1, 6] <= H * W * (shift + 1e-15)
    assert stats[0, 0, 1, :3].sum() == H * W and stats[0, 0, 1, 5] <= stats[0, 0, 1, 4]
    if nudge:
        assert (cls[0, 0, 1][hit & inner] >= 2).all() and (cls[0, 0, 1][hit & ~inner] == 1).all()
        assert stats[0, 0, 1, 2] == (hit & inner).sum()
    assert not stats[0, 0, 0].any() and (cls[0, 1, 1] == -1).all()


def test_no_surface_and_scaled_depth(twin):
    empty = {**twin, "depth": torch.full_like(twin["depth"], float("inf"))}
    stats = ops.depth_consistency(**empty, tol=TOL)
    assert (stats[0, [0, 1], [1, 0], 0] == H * W).all() and not stats[..., 1:].any()
    far = twin["depth"].clone()
    far[0, 1] *= 1.0 + 2.0 * TOL                             # as a source, view 1 now lies behind every point
    stats = ops.depth_consistency(**{**twin, "depth": far}, tol=TOL)
    assert stats[0, 0, 1, 2] == 0 and stats[0, 0, 1, 1] == torch.isfinite(far[0, 0]).sum()


@pytest.mark.parametrize("change", [dict(tol=0.0), dict(tol=-1.0), dict(tol=True), dict(tol=None), dict(rescale_from=-1),
                                    dict(depth=torch.zeros(1, 2, H, W, dtype=torch.float64)),
                                    dict(depth=torch.zeros(1, 65, 1, 1)), dict(images=torch.zeros(1, 2, 3, H, W + 1)),
                                    dict(images=torch.zeros(1, 2, W, H, 3).permute(0, 1, 4, 3, 2)),
                                    dict(K=torch.zeros(1, 3, 3)), dict(R=torch.zeros(1, 3, 3, 3, dtype=torch.float64)),
                                    dict(t=[0.0])], ids=lambda c: next(iter(c)))
def test_bad_arguments(twin, change):
    with pytest.raises(ValueError, match="depth_consistency"):
        ops.depth_consistency(**{**twin, "tol": TOL, **change})


def test_tol_is_required(twin):
    with pytest.raises(TypeError):
        ops.depth_consistency(**twin)


def test_cli(tmp_path):
    """evaluate.py --field_reproj: refused without --field_holdout; with it finite reproj_* fields in rows, per_w
    and gt_field; without it none of the new keys."""
    import evaluate as evaluate_cli
    from distributed_3d_diffusion_pytorch_amd.config import make_config
    from distributed_3d_diffusion_pytorch_amd.engine import Trainer
    from distributed_3d_diffusion_pytorch_amd.engine.field import REPROJ_KEYS, REPROJ_TOL
    from distributed_3d_diffusion_pytorch_amd.parallel import DistContext
    with pytest.raises(ValueError, match="field_holdout"):
        evaluate_cli.run(evaluate_cli.parse(["--field_reproj", "--model", str(tmp_path / "none.pt"), "--out",
                                             str(tmp_path / "refused")]))
    run = str(tmp_path / "run")
    tr = Trainer(make_config(None, {"model.ch": 32, "model.emb_ch": 64, "model.H": 16, "model.W": 16,
                                    "data.imgsize": 16, "global_batch": 2, "dtype": "fp32", "backend": "torch",
                                    "log_every": 1, "ckpt_every": 0, "data.num_workers": 0, "data.procedural": True,
                                    "out_dir": run}), DistContext())
    tr.save("latest.pt", epoch=0)
    tr.logger.close()
    common = ["--model", os.path.join(run, "latest.pt"), "--procedural", "--proc_seed", "4", "--proc_objects", "40",
              "--instances", "2", "--views", "1,2,3,4", "--field_holdout", "4", "--field_grid", "8", "--field_iters", "6",
              "--field_batch", "2", "--w", "0", "--timesteps", "2", "--imgsize", "16", "--backend", "torch"]
    evaluate_cli.run(evaluate_cli.parse(common + ["--field_reproj", "--out", str(tmp_path / "on")]))
    with open(tmp_path / "on" / "metrics.json") as f:
        on = json.load(f)
    assert on["args"]["field_reproj"] is True and on["args"]["field_reproj_tol"] == REPROJ_TOL
    block = on["field"]
    for r in block["rows"] + [block["per_w"]["0"]] + block["gt_field"]["rows"] + [block["gt_field"]]:
        assert all(r[k] is None or math.isfinite(r[k]) for k in REPROJ_KEYS)
        assert r["reproj_n_covisible"] >= r["reproj_n_clean"] >= 0
    assert all(len(r["reproj_sums"]) == 7 and sum(r["reproj_sums"][:3]) == 4 * 3 * 256 for r in block["rows"])
    evaluate_cli.run(evaluate_cli.parse(common + ["--out", str(tmp_path / "off")]))
    with open(tmp_path / "off" / "metrics.json") as f:
        off = json.load(f)
    assert off["args"]["field_reproj"] is False and "reproj" not in json.dumps(off["field"])
    assert [r["field_psnr"] for r in off["field"]["rows"]] == [r["field_psnr"] for r in block["rows"]]
