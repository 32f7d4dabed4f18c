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

On a HIP device a batch (``ProceduralBatches``) and a list of views
(``render_views``, ``procedural_objects``) are one fused launch each,
``ops.procedural_batch`` / ``ops.procedural_render`` (``csrc/procedural.hip``:
draw, tables, poses and render in one kernel); ``D3D_PROC_FUSED=0`` keeps the
torch composition of the rule's functions in front of ``ops.scene_render``,
which is also the CPU path.
"""
from __future__ import annotations

import json
import os
import pickle
from typing import Dict, List, Sequence

import numpy as np
import torch

from .. import ops
from ..ops import torch_impl as _t
from ..ops.torch_impl import (hash_u32, u01, GOLDEN, SRN_FOCAL_128, SRN_RADIUS, orbit_look_at,  # noqa: F401
                              procedural_scene, procedural_pose, split_object, srn_intrinsics)

# The rule's pure functions (procedural_scene, procedural_pose, split_object,
# the batch draw) live in ops.torch_impl, next to the renderer they feed: they
# are the CPU form of ops.procedural_render / ops.procedural_batch.
P_MAX = _t.SCENE_SLOTS
MAX_VIEWS = _t.PROC_MAX_VIEWS        # views of one object (the pose counter's stride)
MAX_OBJECTS = _t.PROC_MAX_OBJECTS
_K_COUNT, _K_POSE, _K_BATCH = _t.PROC_K_COUNT, _t.PROC_K_POSE, _t.PROC_K_BATCH
_M64 = (1 << 64) - 1
_CENTRE = _t.PROC_CENTRE
_ids = _t.proc_ids


def _fused(device) -> bool:
    """One fused HIP launch (ops.procedural_render / procedural_batch) instead
    of the torch composition in front of ops.scene_render: on a HIP device,
    unless ``D3D_PROC_FUSED=0`` (A/B runs)."""
    return torch.device(device).type == "cuda" and os.environ.get("D3D_PROC_FUSED", "1") != "0"


def render_views(seed: int, object_ids, view_ids, imgsize: int, device="cpu", aa: int = 3, return_aux: bool = False,
                 return_table: bool = False):
    """``(img [n,3,S,S] fp32, R [n,3,3], t [n,3], K [n,3,3])`` of the listed
    (object, view) pairs (``return_aux``: ``img`` is ``ops.scene_render``'s
    (img, depth, prim); ``return_table``: also the scene tables [n,6,16])."""
    o = _ids(object_ids, device)
    K = srn_intrinsics(o.device).expand(o.numel(), 3, 3).contiguous()
    if _fused(o.device) and o.numel():
        out = ops.procedural_render(seed, o, _ids(view_ids, device), imgsize, imgsize, aa=aa, return_aux=return_aux)
        img, R, t, table = out[:4]
        img = (img, out[4], out[5]) if return_aux else img
    else:
        table = procedural_scene(seed, o, device)
        R, t = procedural_pose(seed, o, view_ids, device)
        img = ops.scene_render(table, R, t, K, imgsize, imgsize, aa=aa, return_aux=return_aux)
    return (img, R, t, K, table) if return_table else (img, R, t, K)


def split_size(objects: int, split: str) -> int:
    """Objects of the split among ids ``[0, objects)`` (0: ``[0, 2^31)``)."""
    if split not in ("train", "val"):
        raise ValueError(f"split {split!r}: expected 'train' or 'val'")
    if not 0 <= objects <= MAX_OBJECTS:
        raise ValueError(f"objects must be in [0, 2^31], got {objects}")
    n = objects or MAX_OBJECTS
    return n // 10 if split == "val" else n - n // 10


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
        return _t.procedural_draw(self.seed, i, self.B, n_objects=self.n_objects, views=self.views, split=self.split,
                                  example_offset=self.example_offset, device=self.device)

    def __next__(self):
        B, S = self.B, self.S
        i, self.i = self.i, self.i + 1
        K = self.K.expand(B, 3, 3).contiguous()
        if _fused(self.device) and B > 0:           # draw, tables, poses and render: one launch
            _, _, img, R, t = ops.procedural_batch(self.seed, i, B, S, S, n_objects=self.n_objects, views=self.views,
                                                   split=self.split, example_offset=self.example_offset, aa=self.aa,
                                                   device=self.device)
            return img, R, t, K
        obj, view = self.draw(i)
        table = procedural_scene(self.seed, obj, self.device)
        R, t = procedural_pose(self.seed, obj.repeat_interleave(2), view.reshape(-1), self.device)
        img = ops.scene_render(table.repeat_interleave(2, 0), R, t, K.repeat_interleave(2, 0), S, S, aa=self.aa)
        return img.reshape(B, 2, 3, S, S), R.reshape(B, 2, 3, 3), t.reshape(B, 2, 3), K


def procedural_objects(seed: int, instances: int, views: Sequence[int], imgsize: int, objects: int = 0,
                       split: str = "val", aa: int = 3, device=None, offset: int = 0) -> List:
    """The first ``instances`` objects of the split (after skipping ``offset``
    of them) with the listed views, as
    the ``EvalObject`` list ``engine.evaluate_objects`` and the sampler take
    (CPU fp32 tensors, names ``proc-<seed>-<id>``; ``scene`` is the object's
    fp64 table, which the geometry-aware scores read).  Rendered on ``device``
    (default: the GPU when there is one)."""
    from ..engine.evaluate import EvalObject
    n = split_size(objects, split)
    if instances <= 0 or offset < 0 or offset + instances > n:
        raise ValueError(f"instances must be in 1..{n} (the {split} objects among ids [0, {objects or MAX_OBJECTS})), "
                         f"got {instances}" + (f" after {offset}" if offset else ""))
    views = [int(v) for v in views]
    if not views or min(views) < 0 or max(views) >= MAX_VIEWS:
        raise ValueError(f"views must be in [0, {MAX_VIEWS}), got {views}")
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    ids = [split_object(r, split) for r in range(offset, offset + instances)]
    nv = len(views)
    img, R, t, _, table = render_views(seed, [o for o in ids for _ in views], views * len(ids), imgsize, device, aa,
                                       return_table=True)
    img, R, t = img.cpu(), R.float().cpu(), t.float().cpu()
    K = srn_intrinsics().float()
    scene = table[::nv].cpu()                           # the geometry, for the geometry-aware scores
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
