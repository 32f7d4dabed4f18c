"""ops.field_geometry on the CPU (the float64 torch form of csrc/field_geom.hip):
a grid whose surface is a known sphere, an empty grid, and the read-out end to
end through engine.field_rows and evaluate.py."""
import math

import pytest
import torch

from distributed_3d_diffusion_pytorch_amd import ops
from distributed_3d_diffusion_pytorch_amd.data import procedural as P

G, S, HW, R0, SHARP = 24, 96, 24, 0.6, 1000.0
# profiles/field/README.md, "The sphere": the reference gives a smallest cosine of 0.99753 and an IoU of 0.96800;
# each bound allows twice the reference's own distance from the ideal 1.
COS_MIN, IOU_MIN = 1.0 - 2.0 * (1.0 - 0.99753), 1.0 - 2.0 * (1.0 - 0.96800)


def cameras(V=3):
    R, t = P.procedural_pose(1234, [1] * V, list(range(V)))
    return dict(K=P.srn_intrinsics()[None], R=R[None], t=t[None])


def test_sphere_depth_normals_iou():
    """sigma = SHARP (R0 - |p|) at the nodes: D within a voxel plus a step of the sphere, n radial, IoU near 1."""
    x = torch.linspace(-1.0, 1.0, G, dtype=torch.float64)
    z, y, xx = torch.meshgrid(x, x, x, indexing="ij")
    grid = torch.zeros(1, G, G, G, 4)
    grid[0, ..., 3] = (SHARP * (R0 - torch.sqrt(xx * xx + y * y + z * z))).float()
    table = torch.zeros(1, 6, 16, dtype=torch.float64)
    table[0, 0, [0, 4, 8]] = 1.0 / R0                                  # A = I / R0: the sphere as slot 0
    table[0, 0, 12:15], table[0, 0, 15] = 0.5, 1.0
    cam = cameras()
    scores, maps = ops.field_geometry(grid, **cam, H=HW, W=HW, samples=S, table=table, return_maps=True)
    pos, dirs = ops.camera_rays(cam["R"], cam["t"], cam["K"], HW, HW, 128)          # [1,V,H,W,3]
    b = (pos * dirs).sum(-1).double()
    disc = b * b - ((pos * pos).sum(-1).double() - R0 * R0)
    hit = maps[0, :, 0] > 0.5
    assert 0 < hit.sum() < hit.numel() and (disc[0][hit] > 0).all()
    want = (-b - disc.clamp_min(0).sqrt())[0][hit]
    chord = 2.0 * math.sqrt(3.0)                                       # the longest ray through the cube
    assert ((maps[0, :, 1][hit].double() - want).abs() <= 2.0 / (G - 1) + chord / S).all()
    assert torch.isinf(maps[0, :, 1][~hit]).all() and not maps[0, :, 2:].permute(0, 2, 3, 1)[~hit].any()
    p = (pos[0] + maps[0, :, 1, :, :, None] * dirs[0])[hit].double()            # the field's surface point
    cos = (maps[0, :, 2:].permute(0, 2, 3, 1)[hit].double() * p / p.norm(dim=-1, keepdim=True)).sum(-1)
    s = scores[0].sum(0)
    iou = (s[2] / (s[0] + s[1] - s[2])).item()
    print(f"smallest cosine {cos.min().item():.5f} (bound {COS_MIN:.5f}), IoU {iou:.5f} (bound {IOU_MIN:.5f})")
    assert cos.min().item() >= COS_MIN and iou >= IOU_MIN


def test_empty_grid():
    grid = torch.zeros(1, 8, 8, 8, 4)
    grid[..., 3] = -20.0
    table = P.procedural_scene(1234, [1])
    scores, maps = ops.field_geometry(grid, **cameras(2), H=16, W=16, samples=16, table=table, return_maps=True)
    assert not scores[..., 1].any() and not scores[..., 2:6].any() and scores[..., 0].sum() > 0
    assert torch.isinf(maps[:, :, 1]).all() and not maps[:, :, 2:].any()
    assert (scores[..., 6] - scores[..., 0]).abs().max() <= 1e-6 * scores[..., 0].max()


def test_end_to_end(tmp_path):
    """field_rows(geometry=True) adds finite geom_* fields and leaves field_psnr alone; the CLI refuses the flag
    without --procedural."""
    import evaluate as evaluate_cli
    from distributed_3d_diffusion_pytorch_amd.engine import field_rows, summarize_field
    from distributed_3d_diffusion_pytorch_amd.engine.field import GEOM_KEYS
    views = list(range(5))
    objects = P.procedural_objects(1234, 2, views, 16, device="cpu")
    fit = dict(grid=8, samples=16, iters=6, rays_per_iter=256, lr=0.3)
    for batch in (1, 2):
        plain = field_rows(objects, None, views, [4], [0.0], batch=batch, **fit)
        rows = field_rows(objects, None, views, [4], [0.0], batch=batch, geometry=True, **fit)
        assert [r["field_psnr"] for r in rows] == [r["field_psnr"] for r in plain]
        assert not any(k.startswith("geom_") for r in plain for k in r)
        for r in rows + [summarize_field(rows)["gt"]]:
            assert all(r[k] is None or math.isfinite(r[k]) for k in GEOM_KEYS) and r["geom_n_truth"] > 0
        assert set(summarize_field(plain)["gt"]) == {"n", "field_psnr", "field_ssim", "fit_loss"}
    with pytest.raises(ValueError, match="geometry"):
        evaluate_cli.run(evaluate_cli.parse(["--field_geometry", "--views", "1,2,3,4", "--field_holdout", "4", "--model",
                                             str(tmp_path / "none.pt"), "--out", str(tmp_path / "refused")]))
