"""Procedural multi-view scenes: a dataset the project generates itself.

An object is a handful of analytic primitives (ellipsoids and boxes) drawn
from the counter hash of ``ops.torch_impl`` (``hash_u32`` / ``u01``), a view an
SRN-style orbit camera drawn the same way, and the image the ray-cast render
of ``ops.scene_render`` (``csrc/scene.hip`` on the GPU).  Shading does not
depend on the view, so the views of an object are 3D-consistent by
construction; objects and views are pure functions of ``(seed, object id,
view id)`` on any device and any rank, unlimited in number, and need no files.

The rule (everything float64):

* object ``o`` has ``3 + hash_u32(seed ^ 0x5bd1e995, o) % 4`` primitives out of
  ``P_MAX = 6`` slots; primitive ``p`` reads ``u_k = u01(seed, (6 o + p) 64 + k)``,
  ``k < 14``: centre ``(u0..2 - 0.5) * (0.7, 0.5, 0.4)``, semi-axes ``0.08 +
  0.22 u3..5``, orientation the unit quaternion ``(w, x, y, z)`` proportional
  to ``2 u6..9 - 1 + 1e-3``, albedo ``0.1 + 0.8 u10..12``, an ellipsoid if
  ``u13 < 0.5``, else a box;
* view ``v`` of object ``o`` reads ``u = u01(seed ^ 0x7f4a7c15, 2 (4096 o + v) +
  {0, 1})``: azimuth ``2 pi u0``, elevation ``0.05 + 0.95 u1`` rad, radius
  ``SRN_RADIUS``, the look-at pose of ``random_orbit_poses``;
* intrinsics: the SRN 128 x 128 pinhole, unrescaled -- what the SRN files and
  ``SyntheticBatches`` hand the model; an image of size S is rendered with the
  camera of the downsized SRN image (``camera_rays(..., rescale_from=128)``);
* the image: see ``ops.scene_render``.

Split: object ids with ``o % 10 == 9`` are held out (``split="val"``).
"""
from __future__ import annotations

import json
import math
import os
import pickle
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from .. import ops
from ..ops.torch_impl import hash_u32, u01, GOLDEN
from .synthetic import SRN_FOCAL_128, SRN_RADIUS, orbit_look_at

P_MAX = 6
MAX_VIEWS = 4096                     # views of one object (the pose counter's stride)
MAX_OBJECTS = 1 << 31
_K_COUNT = 0x5BD1E995
_K_POSE = 0x7F4A7C15
_K_BATCH = 0x70726F6365647572        # "procedur": keeps the batch draw apart from the scene and pose draws
_M64 = (1 << 64) - 1
_CENTRE = (0.7, 0.5, 0.4)


def _ids(x, device) -> torch.Tensor:
    return torch.as_tensor(x, dtype=torch.int64, device=device).reshape(-1)


def srn_intrinsics(device="cpu") -> torch.Tensor:
    """The SRN 128 x 128 pinhole K [3,3] (float64)."""
    return torch.tensor([[SRN_FOCAL_128, 0.0, 64.0], [0.0, SRN_FOCAL_128, 64.0], [0.0, 0.0, 1.0]],
                        dtype=torch.float64, device=device)


def procedural_scene(seed: int, object_ids, device="cpu") -> torch.Tensor:
    """Scene tables [N,6,16] (float64) of the objects: per slot the 3 x 3 map
    ``A = diag(1 / axes) R^T`` (world to the unit primitive, row-major), the
    centre, the albedo and the kind (0 empty, 1 ellipsoid, 2 box)."""
    dt = torch.float64
    o = _ids(object_ids, device)
    N = o.numel()
    count = 3 + hash_u32(seed ^ _K_COUNT, o) % 4                                  # [N]
    p = torch.arange(P_MAX, device=o.device)
    k = torch.arange(14, device=o.device)
    u = u01(seed, ((o[:, None, None] * P_MAX + p[None, :, None]) * 64 + k[None, None, :])).to(dt)   # [N,6,14]
    centre = (u[..., 0:3] - 0.5) * torch.tensor(_CENTRE, dtype=dt, device=o.device)
    axes = 0.08 + 0.22 * u[..., 3:6]
    q = 2.0 * u[..., 6:10] - 1.0 + 1e-3
    q = q / torch.sqrt((q * q).sum(-1, keepdim=True))
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(N, P_MAX, 3, 3)
    A = R.transpose(-1, -2) / axes[..., :, None]                                  # diag(1 / axes) R^T
    albedo = 0.1 + 0.8 * u[..., 10:13]
    kind = torch.where(u[..., 13] < 0.5, 1.0, 2.0).to(dt)
    table = torch.cat([A.reshape(N, P_MAX, 9), centre, albedo, kind[..., None]], -1)
    live = p[None, :] < count[:, None]
    return torch.where(live[..., None], table, torch.zeros_like(table))


def procedural_pose(seed: int, object_ids, view_ids, device="cpu") -> Tuple[torch.Tensor, torch.Tensor]:
    """Cam-to-world poses of views ``view_ids`` [n] of objects ``object_ids``
    [n]: R [n,3,3], t [n,3] (float64; OpenCV axes, z up, looking at the origin)."""
    o, v = _ids(object_ids, device), _ids(view_ids, device)
    if o.shape != v.shape:
        raise ValueError(f"procedural_pose: {o.numel()} object ids and {v.numel()} view ids")
    c = 2 * (o * MAX_VIEWS + v)
    az = 2.0 * math.pi * u01(seed ^ _K_POSE, c).to(torch.float64)
    el = 0.05 + 0.95 * u01(seed ^ _K_POSE, c + 1).to(torch.float64)
    return orbit_look_at(az, el, SRN_RADIUS)


def render_views(seed: int, object_ids, view_ids, imgsize: int, device="cpu", aa: int = 3, return_aux: bool = False):
    """``(img [n,3,S,S] fp32, R [n,3,3], t [n,3], K [n,3,3])`` of the listed
    (object, view) pairs (``return_aux``: ``img`` is ``ops.scene_render``'s
    (img, depth, prim))."""
    o = _ids(object_ids, device)
    table = procedural_scene(seed, o, device)
    R, t = procedural_pose(seed, o, view_ids, device)
    K = srn_intrinsics(o.device).expand(o.numel(), 3, 3).contiguous()
    return ops.scene_render(table, R, t, K, imgsize, imgsize, aa=aa, return_aux=return_aux), R, t, K


def split_size(objects: int, split: str) -> int:
    """Objects of the split among ids ``[0, objects)`` (0: ``[0, 2^31)``)."""
    if split not in ("train", "val"):
        raise ValueError(f"split {split!r}: expected 'train' or 'val'")
    if not 0 <= objects <= MAX_OBJECTS:
        raise ValueError(f"objects must be in [0, 2^31], got {objects}")
    n = objects or MAX_OBJECTS
    return n // 10 if split == "val" else n - n // 10


def split_object(rank, split: str):
    """The id of the split's ``rank``-th object (int or int64 tensor): ids with
    ``o % 10 == 9`` are the held-out split, the rest the training split."""
    return 10 * rank + 9 if split == "val" else rank + rank // 9


class ProceduralBatches:
    """Infinite iterator of on-device batches of rendered scenes, the tuple
    ``SyntheticBatches`` yields: ``(img[B,2,3,S,S] f32 in [-1,1], R[B,2,3,3]
    f64, T[B,2,3] f64, K[B,3,3] f64)``.

    Example ``g = example_offset + j`` of batch ``i`` draws its object (of the
    split, among ids ``[0, objects)``; 0: ``[0, 2^31)``) and its two distinct
    views (of ``views``) from the counter hash keyed by ``(seed, i, g)``, so a
    rank's shard or a micro-batch split reproduces its rows of the full batch."""

    def __init__(self, batch_size: int, imgsize: int = 64, device="cpu", seed: int = 0, objects: int = 0,
                 views: int = 50, split: str = "train", example_offset: int = 0, aa: int = 3):
        if not 2 <= views <= MAX_VIEWS:
            raise ValueError(f"views must be in 2..{MAX_VIEWS}, got {views}")
        if not 1 <= aa <= 4:
            raise ValueError(f"aa must be in 1..4, got {aa}")
        self.n_objects = split_size(objects, split)
        if self.n_objects == 0:
            raise ValueError(f"no {split} objects among ids [0, {objects})")
        self.B, self.S = int(batch_size), int(imgsize)
        self.device = torch.device(device)
        self.seed, self.views, self.split, self.aa = int(seed), int(views), split, int(aa)
        self.example_offset = int(example_offset)
        self.i = 0
        self.K = srn_intrinsics(self.device)

    def __iter__(self):
        return self

    def draw(self, i: int):
        """(object ids [B], view ids [B,2]) of batch ``i`` (int64, on the device)."""
        s = ((self.seed * 0x2545F4914F6CDD1D + _K_BATCH) + (i + 1) * GOLDEN) & _M64
        g = torch.arange(self.B, dtype=torch.int64, device=self.device) + self.example_offset
        obj = split_object(hash_u32(s, 4 * g) % self.n_objects, self.split)
        v0 = hash_u32(s, 4 * g + 1) % self.views
        v1 = (v0 + 1 + hash_u32(s, 4 * g + 2) % (self.views - 1)) % self.views
        return obj, torch.stack([v0, v1], 1)

    def __next__(self):
        B, S = self.B, self.S
        obj, view = self.draw(self.i)
        self.i += 1
        table = procedural_scene(self.seed, obj, self.device)
        R, t = procedural_pose(self.seed, obj.repeat_interleave(2), view.reshape(-1), self.device)
        K = self.K.expand(B, 3, 3).contiguous()
        img = ops.scene_render(table.repeat_interleave(2, 0), R, t, K.repeat_interleave(2, 0), S, S, aa=self.aa)
        return img.reshape(B, 2, 3, S, S), R.reshape(B, 2, 3, 3), t.reshape(B, 2, 3), K


def procedural_objects(seed: int, instances: int, views: Sequence[int], imgsize: int, objects: int = 0,
                       split: str = "val", aa: int = 3, device=None) -> List:
    """The first ``instances`` objects of the split with the listed views, as
    the ``EvalObject`` list ``engine.evaluate_objects`` and the sampler take
    (CPU fp32 tensors, names ``proc-<seed>-<id>``; ``scene`` is the object's
    fp64 table, which the geometry-aware scores read).  Rendered on ``device``
    (default: the GPU when there is one)."""
    from ..engine.evaluate import EvalObject
    n = split_size(objects, split)
    if instances <= 0 or instances > n:
        raise ValueError(f"instances must be in 1..{n} (the {split} objects among ids [0, {objects or MAX_OBJECTS})), "
                         f"got {instances}")
    views = [int(v) for v in views]
    if not views or min(views) < 0 or max(views) >= MAX_VIEWS:
        raise ValueError(f"views must be in [0, {MAX_VIEWS}), got {views}")
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    ids = [split_object(r, split) for r in range(instances)]
    nv = len(views)
    img, R, t, _ = render_views(seed, [o for o in ids for _ in views], views * len(ids), imgsize, device, aa)
    img, R, t = img.cpu(), R.float().cpu(), t.float().cpu()
    K = srn_intrinsics().float()
    scene = procedural_scene(seed, ids)                 # the geometry, for the geometry-aware scores
    return [EvalObject(f"proc-{seed}-{o}", {v: img[j * nv + i] for i, v in enumerate(views)},
                       {v: R[j * nv + i] for i, v in enumerate(views)},
                       {v: t[j * nv + i] for i, v in enumerate(views)}, K.clone(), scene=scene[j].clone())
            for j, o in enumerate(ids)]


def to_uint8(img: torch.Tensor) -> np.ndarray:
    """[..,3,H,W] in [-1, 1] -> [..,H,W,3] uint8, the value ``sampling.py:save_png`` writes."""
    x = ((img.float().clamp(-1.0, 1.0) + 1.0) * 127.5).to(torch.uint8)
    return x.movedim(-3, -1).cpu().numpy()


def write_procedural_srn(root: str, num_instances: int = 10, num_views: int = 6, size: int = 128, seed: int = 0,
                         device="cpu", aa: int = 3) -> Dict[str, list]:
    """Write objects ``0 .. num_instances - 1`` with views ``0 .. num_views - 1``
    as an SRN tree in ``write_synthetic_srn``'s format: ``root/<id>/{rgb,pose,
    intrinsics}`` (RGBA PNGs of ``size``, 4 x 4 cam-to-world poses, K scaled to
    ``size``) plus ``root/index.pkl|.json``."""
    from PIL import Image
    os.makedirs(root, exist_ok=True)
    f = SRN_FOCAL_128 * size / 128.0
    K = np.array([[f, 0, size / 2], [0, f, size / 2], [0, 0, 1.0]])
    index = {}
    views = list(range(num_views))
    for o in range(num_instances):
        inst = f"proc{seed}_{o:08d}"
        for sub in ("rgb", "pose", "intrinsics"):
            os.makedirs(os.path.join(root, inst, sub), exist_ok=True)
        img, R, t, _ = render_views(seed, [o] * num_views, views, size, device, aa)
        rgb, R, t = to_uint8(img), R.cpu().numpy(), t.cpu().numpy()
        names = []
        for v in views:
            name = f"{v:06d}.png"
            rgba = np.concatenate([rgb[v], np.full((size, size, 1), 255, np.uint8)], -1)
            Image.fromarray(rgba, "RGBA").save(os.path.join(root, inst, "rgb", name))
            pose = np.eye(4)
            pose[:3, :3], pose[:3, 3] = R[v], t[v]
            np.savetxt(os.path.join(root, inst, "pose", name[:-4] + ".txt"), pose.reshape(1, 16), fmt="%.8f")
            np.savetxt(os.path.join(root, inst, "intrinsics", name[:-4] + ".txt"), K.reshape(1, 9), fmt="%.6f")
            names.append(name)
        index[inst] = names
    with open(os.path.join(root, "index.pkl"), "wb") as fh:
        pickle.dump(index, fh)
    with open(os.path.join(root, "index.json"), "w") as fh:
        json.dump(index, fh)
    return index
