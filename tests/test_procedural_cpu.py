"""Procedural scenes on the CPU (data/procedural.py, the float64 torch form of
ops.scene_render): the renderer follows the ray convention the model
conditions on, the views of an object are 3D-consistent, the batches are
deterministic and shard like the training-input draw, bad arguments raise,
the SRN tree round-trips and the CLIs run."""
import json
import os

import numpy as np
import pytest
import torch

from distributed_3d_diffusion_pytorch_amd import ops
from distributed_3d_diffusion_pytorch_amd.data import (ProceduralBatches, SRNDataset, procedural_objects,
                                                       procedural_pose, procedural_scene, write_procedural_srn)
from distributed_3d_diffusion_pytorch_amd.data import procedural as P
from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T

F64 = torch.float64
SEED, S = 1234, 16
OBJ = [o for o in range(24) for _ in range(2)]          # objects 0..23, views 0 and 1 of each
VIEW = [0, 1] * 24

TINY_OV = {"model.ch": 32, "model.emb_ch": 64, "model.H": 32, "model.W": 32, "data.imgsize": 32,
           "global_batch": 2, "dtype": "fp32", "backend": "torch", "log_every": 1, "ckpt_every": 2,
           "data.num_workers": 0}


@pytest.fixture(scope="module")
def scene():
    """The shared reference: 48 images of 16 x 16 at aa = 1 with aux, computed once."""
    table = procedural_scene(SEED, OBJ)
    R, t = procedural_pose(SEED, OBJ, VIEW)
    K = P.srn_intrinsics().expand(len(OBJ), 3, 3).contiguous()
    img, depth, prim = ops.scene_render(table, R, t, K, S, S, aa=1, return_aux=True)
    return {"table": table, "R": R, "t": t, "K": K, "img": img, "depth": depth, "prim": prim}


def test_scene_family_rule():
    table = procedural_scene(SEED, list(range(24)))
    assert table.shape == (24, 6, 16) and table.dtype == F64
    kind = table[..., 15]
    count = 3 + T.hash_u32(SEED ^ 0x5BD1E995, torch.arange(24)) % 4
    assert ((kind > 0).sum(1) == count).all() and set(count.tolist()) == {3, 4, 5, 6}
    assert {0.0, 1.0, 2.0} == set(kind.flatten().tolist())
    live = kind > 0
    assert (table[~live] == 0).all()                                   # empty slots hold nothing
    assert (live[:, :-1] >= live[:, 1:]).all()                         # ... and come last
    A = table[..., :9].reshape(24, 6, 3, 3)[live]
    inv_axes = (A @ A.transpose(-1, -2)).diagonal(dim1=-2, dim2=-1).sqrt()    # A A^T = diag(1 / axes^2)
    assert (1 / inv_axes).min() >= 0.08 and (1 / inv_axes).max() <= 0.30
    off = A @ A.transpose(-1, -2) - torch.diag_embed(inv_axes ** 2)
    assert off.abs().max() < 1e-9
    assert (table[..., 9:12][live].abs() <= torch.tensor([0.35, 0.25, 0.2], dtype=F64)).all()
    alb = table[..., 12:15][live]
    assert alb.min() >= 0.1 and alb.max() <= 0.9
    # a pure function of (seed, id): any subset, any order
    again = procedural_scene(SEED, [7, 3])
    assert torch.equal(again, table[[7, 3]])
    assert not torch.equal(procedural_scene(SEED + 1, [7]), table[[7]])


def test_pose_is_the_orbit_look_at():
    R, t = procedural_pose(SEED, OBJ, VIEW)
    assert R.dtype == F64 and t.dtype == F64
    assert (t.norm(dim=-1) - 1.3).abs().max() < 1e-12
    assert (R @ R.transpose(-1, -2) - torch.eye(3, dtype=F64)).abs().max() < 1e-12
    assert (torch.linalg.det(R) - 1).abs().max() < 1e-12
    assert (R[:, :, 2] + t / 1.3).abs().max() < 1e-12                  # z looks at the origin
    assert R[:, 2, 0].abs().max() < 1e-12 and (R[:, 2, 1] < 0).all()   # x horizontal, y down (z is up)
    el = torch.asin(t[:, 2] / 1.3)
    assert el.min() >= 0.05 and el.max() <= 1.0


def test_coverage(scene):
    """The rule's foreground coverage at 16 x 16: 17 - 52 % per image, mean 31 %."""
    cov = (scene["prim"] >= 0).double().flatten(1).mean(1)
    assert 0.15 < cov.min() and cov.max() < 0.55 and 0.28 < cov.mean() < 0.34, (cov.min(), cov.mean(), cov.max())


def test_rays_follow_camera_rays(scene):
    """X = t + depth * dir with the fp32 directions of ops.camera_rays(...,
    rescale_from=128) lies on the hit primitive's surface: | ||A (X - c)|| - 1 |
    (ellipsoid) and | ||A (X - c)||_inf - 1 | (box) stay below 5e-6 (direction
    rounding 6e-8, depth at most 2.3, ||A|| at most 12.5)."""
    table, R, t, K = scene["table"], scene["R"], scene["t"], scene["K"]
    depth, prim = scene["depth"], scene["prim"]
    _, dirs = ops.camera_rays(R[:, None], t[:, None], K, S, S, rescale_from=128)
    assert dirs.dtype == torch.float32
    X = t[:, None, None, :] + depth.double()[..., None] * dirs[:, 0].double()
    hit = prim >= 0
    assert torch.isinf(depth[~hit]).all() and (depth[hit] > 0).all() and depth[hit].max() < 2.3
    n, y, x = hit.nonzero(as_tuple=True)
    row = table[n, prim[n, y, x].long()]                               # [M,16]
    local = torch.einsum("mij,mj->mi", row[:, :9].reshape(-1, 3, 3), X[n, y, x] - row[:, 9:12])
    kind = row[:, 15]
    assert set(kind.tolist()) == {1.0, 2.0}
    r = torch.where(kind == 1, local.norm(dim=-1), local.abs().max(-1).values)
    print(f"surface residual: max {float((r - 1).abs().max()):.3e} over {r.numel()} hits")
    assert (r - 1).abs().max() < 5e-6


def test_views_are_3d_consistent(scene):
    """Every surface point seen from view 0 that view 1 also sees (the ray
    from view 1's origin reaches it: depth = distance to 1e-9) has the same
    colour there to 1e-9; at least 30 % of the points are visible."""
    table, R, t, K = scene["table"], scene["R"], scene["t"], scene["K"]
    v0, v1 = slice(0, None, 2), slice(1, None, 2)
    sK = K[v0] * torch.tensor([S / 128, S / 128, 1.0], dtype=F64)[None, :, None]
    py, px = torch.meshgrid(torch.arange(S, dtype=F64), torch.arange(S, dtype=F64), indexing="ij")
    d0 = torch.stack(T._scene_dirs(T._inv3(sK), R[v0], px + 0.5, py + 0.5), -1)
    t0, p0, c0 = T.scene_trace(table[v0], t[v0], d0)
    assert torch.equal(p0.int(), scene["prim"][v0])
    X = t[v0][:, None, None, :] + torch.where(p0 >= 0, t0, torch.zeros_like(t0))[..., None] * d0
    to = X - t[v1][:, None, None, :]
    dist = to.norm(dim=-1)
    t1, p1, c1 = T.scene_trace(table[v1], t[v1], to / dist[..., None])
    fg = p0 >= 0
    seen = fg & ((t1 - dist).abs() < 1e-9)
    frac = float(seen.sum()) / float(fg.sum())
    err = (c0 - c1).abs().amax(1)[seen].max()
    print(f"visible from view 1: {int(seen.sum())} of {int(fg.sum())} points ({frac:.1%}); colour difference "
          f"{float(err):.2e}")
    assert frac >= 0.30
    assert (p0[seen] == p1[seen]).all()
    assert err < 1e-9
    # the image is that colour
    assert (scene["img"][v0].double() - (2 * c0 - 1)).abs().max() < 1e-7


def test_antialiasing_is_the_subpixel_mean(scene):
    """aa = 2: the mean of the 4 rays at offsets 0.25 / 0.75; aux stays the pixel-centre ray's."""
    table, R, t, K = (scene[k][:6] for k in ("table", "R", "t", "K"))
    img, depth, prim = ops.scene_render(table, R, t, K, S, S, aa=2, return_aux=True)
    assert torch.equal(depth, scene["depth"][:6]) and torch.equal(prim, scene["prim"][:6])
    Kinv = T._inv3(K * torch.tensor([S / 128, S / 128, 1.0], dtype=F64)[None, :, None])
    py, px = torch.meshgrid(torch.arange(S, dtype=F64), torch.arange(S, dtype=F64), indexing="ij")
    acc = 0
    for dy in (0.25, 0.75):
        for dx in (0.25, 0.75):
            acc = acc + T.scene_trace(table, t, torch.stack(T._scene_dirs(Kinv, R, px + dx, py + dy), -1))[2]
    assert (img.double() - (2 * (acc / 4) - 1)).abs().max() < 1e-7
    assert not torch.equal(img, scene["img"][:6])
    assert img.min() >= -1 and img.max() <= 1


def test_non_square_uses_both_scales(scene):
    """H != W: rows scale by H / 128, columns by W / 128 (camera_rays' rescale)."""
    table, R, t, K = (scene[k][:4] for k in ("table", "R", "t", "K"))
    H, W = 8, 24
    _, depth, prim = ops.scene_render(table, R, t, K, H, W, aa=1, return_aux=True)
    _, dirs = ops.camera_rays(R[:, None], t[:, None], K, H, W, rescale_from=128)
    d, p, _ = T.scene_trace(table, t, dirs[:, 0].double())
    assert (prim.long() != p).float().mean() < 0.01 and (p >= 0).any()
    same = (prim.long() == p) & (p >= 0)
    assert (depth.double() - d)[same].abs().max() < 5e-6


def test_batches_deterministic_and_sharded():
    B = 6
    kw = dict(imgsize=8, device="cpu", seed=5, objects=200, views=7, aa=1)
    a, b = ProceduralBatches(B, **kw), ProceduralBatches(B, **kw)
    lo, hi = ProceduralBatches(B // 2, **kw), ProceduralBatches(B // 2, example_offset=B // 2, **kw)
    first = None
    for step in range(2):
        x, y = next(a), next(b)
        assert [tuple(v.shape) for v in x] == [(B, 2, 3, 8, 8), (B, 2, 3, 3), (B, 2, 3), (B, 3, 3)]
        assert [v.dtype for v in x] == [torch.float32, F64, F64, F64]
        for u, v in zip(x, y):
            assert torch.equal(u, v)
        for u, l, h in zip(x, next(lo), next(hi)):
            assert torch.equal(u, torch.cat([l, h]))
        first = x if first is None else first
    assert not torch.equal(first[0], x[0])                             # batch 1 is another draw
    assert torch.equal(x[3][0], P.srn_intrinsics())                    # the 128^2 K, unrescaled
    # what the batch holds is the render of the drawn (object, view) pairs
    obj, view = a.draw(1)
    assert (view[:, 0] != view[:, 1]).all() and view.min() >= 0 and view.max() < 7
    (img, R, t, _) = P.render_views(5, obj.repeat_interleave(2), view.reshape(-1), 8, aa=1)
    assert torch.equal(img.reshape(B, 2, 3, 8, 8), x[0]) and torch.equal(R.reshape(B, 2, 3, 3), x[1])
    assert not torch.equal(x[0][:, 0], x[0][:, 1])


def test_views_distinct_and_splits_disjoint():
    tr = ProceduralBatches(64, 8, seed=3, objects=50, views=2, split="train")
    va = ProceduralBatches(64, 8, seed=3, objects=50, views=2, split="val")
    ids = {"train": set(), "val": set()}
    for i in range(8):
        for name, it in (("train", tr), ("val", va)):
            obj, view = it.draw(i)
            assert (view[:, 0] != view[:, 1]).all()                    # 2 views: always both
            ids[name] |= set(obj.tolist())
    assert ids["val"] == {9, 19, 29, 39, 49}
    assert ids["train"] == set(range(50)) - ids["val"]
    big = ProceduralBatches(256, 8, seed=3, split="val").draw(0)[0]
    assert (big % 10 == 9).all() and big.max() < 2 ** 31 and big.unique().numel() > 250
    big = ProceduralBatches(256, 8, seed=3, split="train").draw(0)[0]
    assert (big % 10 != 9).all() and big.max() < 2 ** 31 and big.max() > 2 ** 27
    assert P.split_size(0, "train") + P.split_size(0, "val") == 2 ** 31
    for kw in (dict(objects=5, split="val"), dict(views=1), dict(aa=5), dict(split="test")):
        with pytest.raises(ValueError):
            ProceduralBatches(2, 8, **kw)


def test_all_miss_and_empty_slots(scene):
    table, R, t, K = (scene[k][:2].clone() for k in ("table", "R", "t", "K"))
    R[0, :, 0] *= -1
    R[0, :, 2] *= -1                                                   # image 0 looks away from the object
    img, depth, prim = ops.scene_render(table, R, t, K, S, S, aa=3, return_aux=True)
    assert (img[0] == 1).all() and (prim[0] == -1).all() and torch.isinf(depth[0]).all()
    assert (prim[1] >= 0).any() and torch.equal(prim[1], scene["prim"][1])
    # whatever an empty slot holds is ignored; a table of empty slots is white
    assert (table[:, :, 15] == 0).any()
    junk = table.clone()
    junk[..., :15] = torch.where((table[..., 15:] == 0), torch.full_like(table[..., :15], 0.37), table[..., :15])
    out = ops.scene_render(junk, R, t, K, S, S, aa=3, return_aux=True)
    for u, v in zip(out, (img, depth, prim)):
        assert torch.equal(u, v)
    blank = ops.scene_render(torch.zeros_like(table), scene["R"][:2], t, K, S, S)
    assert (blank == 1).all()
    # only the live primitives of an object are ever hit
    count = (scene["table"][..., 15] > 0).sum(1)
    assert (scene["prim"].flatten(1).max(1).values < count).all()


def test_bad_arguments_raise(scene):
    table, R, t, K = (scene[k][:2] for k in ("table", "R", "t", "K"))
    ok = ops.scene_render(table, R, t, K, 4, 4, aa=4)
    assert ok.shape == (2, 3, 4, 4) and ok.dtype == torch.float32
    assert ops.scene_render(table[:0], R[:0], t[:0], K[:0], 4, 4).shape == (0, 3, 4, 4)
    bad = [dict(aa=0), dict(aa=5), dict(aa=2.0), dict(H=0), dict(W=-1), dict(table=table[:, :5]),
           dict(table=table[..., :15]), dict(table=table[0]), dict(table=table.float()), dict(R=R[:1]),
           dict(R=R.float()), dict(t=t[:, :2]), dict(t=t.float()), dict(K=K[0]), dict(K=K.float())]
    for kw in bad:
        a = dict(table=table, R=R, t=t, K=K, H=4, W=4, aa=3)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.scene_render(a.pop("table"), a.pop("R"), a.pop("t"), a.pop("K"), a.pop("H"), a.pop("W"), **a)
    assert "scene_render" in ops.__all__


def test_eval_objects():
    objs = procedural_objects(SEED, 3, [0, 2], 8, objects=100, device="cpu")
    assert [o.name for o in objs] == [f"proc-{SEED}-{i}" for i in (9, 19, 29)]
    (img, R, t, K) = P.render_views(SEED, [19, 19], [0, 2], 8)
    o = objs[1]
    assert sorted(o.imgs) == [0, 2] and torch.equal(o.imgs[2], img[1]) and o.imgs[0].dtype == torch.float32
    assert torch.equal(o.R[2], R[1].float()) and torch.equal(o.T[0], t[0].float())
    assert torch.equal(o.K, P.srn_intrinsics().float())
    assert [o.name for o in procedural_objects(SEED, 2, [0], 8, split="train", device="cpu")] == \
        [f"proc-{SEED}-0", f"proc-{SEED}-1"]
    with pytest.raises(ValueError):
        procedural_objects(SEED, 11, [0], 8, objects=100, device="cpu")     # 10 held-out objects among 100


@pytest.fixture(scope="module")
def srn_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("proc_srn"))
    index = write_procedural_srn(root, num_instances=5, num_views=4, size=32, seed=2)
    return root, index


def test_srn_tree_round_trip(srn_root):
    root, index = srn_root
    assert len(index) == 5 and all(len(v) == 4 for v in index.values())
    with open(os.path.join(root, "index.json")) as f:
        assert json.load(f) == index
    from distributed_3d_diffusion_pytorch_amd.data.srn import load_image, load_index, read_matrix
    assert load_index(os.path.join(root, "index.pkl")) == index
    ds = SRNDataset("train", root, "", 32)
    assert len(ds) == 4
    imgs, R, t, K = ds[0]
    assert imgs.shape == (2, 3, 32, 32) and R.shape == (2, 3, 3) and K.shape == (3, 3)
    assert np.allclose(K, [[131.25 / 4, 0, 16], [0, 131.25 / 4, 16], [0, 0, 1]])
    # every file is the 8-bit render of its (object, view) at the tree's size, with its pose
    for o, inst in enumerate(sorted(index)):
        img, Rr, tr, _ = P.render_views(2, [o] * 4, [0, 1, 2, 3], 32)
        want = torch.from_numpy(P.to_uint8(img)).double().permute(0, 3, 1, 2) / 255 * 2 - 1
        for v, name in enumerate(index[inst]):
            got = load_image(os.path.join(root, inst, "rgb", name), 32)
            assert np.array_equal(got, want[v].numpy().astype(np.float32))
            pose = read_matrix(os.path.join(root, inst, "pose", name[:-4] + ".txt"), (4, 4))
            assert np.abs(pose[:3, :3] - Rr[v].numpy()).max() < 1e-8
            assert np.abs(pose[:3, 3] - tr[v].numpy()).max() < 1e-8
    assert any(np.array_equal(imgs[0], load_image(os.path.join(root, ds.ids[0], "rgb", n), 32))
               for n in index[ds.ids[0]])


def test_clis(srn_root, tmp_path):
    """train.py --procedural -> evaluate.py --procedural and sampling.py
    --procedural on that checkpoint; the directory-based CLIs on the written tree."""
    import evaluate as evaluate_cli
    import sampling as sampling_cli
    import train as train_cli
    root, index = srn_root
    ov = [f"{k}={v}" for k, v in TINY_OV.items()]
    with pytest.raises((SystemExit, ValueError)):
        train_cli.main(["--procedural", "--synthetic", "--steps", "1"] + ov)
    out = str(tmp_path / "run")
    train_cli.main(["--procedural", "--out_dir", out, "--steps", "2", "val_every=2", "val_batches=1",
                    "data.procedural_objects=40", "data.procedural_views=5"] + ov)
    model = os.path.join(out, "latest.pt")
    ck = torch.load(model, weights_only=True)
    assert ck["step"] == 2 and ck["config"]["data"]["procedural"] is True

    ev = str(tmp_path / "eval")
    res = evaluate_cli.run(evaluate_cli.parse(
        ["--model", model, "--procedural", "--proc_seed", "4", "--proc_objects", "40", "--instances", "2",
         "--views", "1,3", "--w", "0,2", "--timesteps", "2", "--imgsize", "32", "--val_batches", "1",
         "--val_batch_size", "2", "--backend", "torch", "--out", ev]))
    with open(os.path.join(ev, "metrics.json")) as f:
        saved = json.load(f)
    assert saved["args"]["procedural"] is True and saved["data"] == "procedural seed=4 objects=40"
    rows = saved["per_image"]
    assert len(rows) == 2 * 2 * 2 and {r["instance"] for r in rows} == {"proc-4-9", "proc-4-19"}
    assert all(np.isfinite([r["mse"], r["psnr"], r["ssim"]]).all() and r["mse"] > 0 for r in rows)
    assert np.isfinite(res["val_loss"]) and res["val_loss"] > 0

    so = str(tmp_path / "samples")
    sampling_cli.main(["--model", model, "--procedural", "7", "--proc_seed", "4", "--proc_views", "3", "--out", so,
                       "--imgsize", "32", "--timesteps", "2", "--w", "0,2", "--backend", "torch", "--metrics"])
    for k in (1, 2):
        assert os.path.exists(os.path.join(so, str(k), "gt.png")) and os.path.exists(os.path.join(so, str(k), "1.png"))
    from PIL import Image
    gt = np.asarray(Image.open(os.path.join(so, "1", "gt.png")))
    assert np.array_equal(gt, P.to_uint8(P.render_views(4, [7], [1], 32)[0])[0])
    with open(os.path.join(so, "metrics.json")) as f:
        assert json.load(f)["target"] == "proc-4-7"

    # the written tree through the directory-based CLIs
    inst = sorted(index)[0]
    so2 = str(tmp_path / "samples_dir")
    sampling_cli.main(["--model", model, "--target", os.path.join(root, inst), "--out", so2, "--imgsize", "32",
                       "--timesteps", "2", "--w", "1", "--max_views", "1", "--backend", "torch"])
    assert os.path.exists(os.path.join(so2, "1", "0.png"))
    ev2 = str(tmp_path / "eval_dir")
    res2 = evaluate_cli.run(evaluate_cli.parse(
        ["--model", model, "--data", root, "--split", "train", "--instances", "2", "--views", "1", "--w", "1",
         "--timesteps", "2", "--imgsize", "32", "--backend", "torch", "--out", ev2]))
    assert res2["n_images"] == 2 and all(np.isfinite(r["ssim"]) for r in res2["per_image"])
