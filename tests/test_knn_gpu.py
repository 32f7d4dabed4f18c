"""csrc/knn.hip (ops.image_knn on the GPU) against the exact torch form on the
CPU.  Everything is an integer: every output is compared with torch.equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
from distributed_3d_diffusion_pytorch_amd import ops  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.data import procedural as P  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.engine import knn_block  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T  # noqa: E402

DEV = "cuda"


def rnd(n, h, w, seed, u8=False):
    g = torch.Generator().manual_seed(seed)
    if u8:
        return torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, generator=g)
    return torch.rand(n, 3, h, w, generator=g) * 2.0 - 1.0


def ties():
    """b: 70 distinct images, each 10 times -- every distance ties across column tiles and across splits of M."""
    return rnd(20, 16, 16, 5), rnd(70, 16, 16, 6, u8=True).repeat(10, 1, 1, 1)


def extremes():
    """all -1 against all +1 among random images: d2 = 3 128 128 255^2 > 2^31.  Four of the five candidates are all +1,
    so the second neighbour of the all -1 query is one of them."""
    a, b = rnd(3, 128, 128, 7), rnd(5, 128, 128, 8)
    a[1], b[:4] = -1.0, 1.0
    return a, b


def mapping():
    """fp32 a: +-1, values beyond the clamp and the (k + 0.5) / 127.5 - 1 boundaries of the 8-bit map; uint8 b."""
    edge = (torch.arange(256, dtype=torch.float32) + 0.5) / 127.5 - 1.0
    vals = torch.cat([edge, torch.nextafter(edge, torch.tensor(2.0)), torch.nextafter(edge, torch.tensor(-2.0)),
                      torch.tensor([-1.0, 1.0, -3.0, 2.5, 0.0])])
    a = vals[torch.randint(0, vals.numel(), (6, 3, 8, 8), generator=torch.Generator().manual_seed(9))]
    return a, rnd(40, 8, 8, 10, u8=True)


# name -> (a, b, k, exclude_self, splits); b None: b is a
CASES = {"1x9 D75 k8": lambda: (rnd(1, 5, 5, 1), rnd(9, 5, 5, 2), 8, False, 0),
         "17x130 ragged": lambda: (rnd(17, 8, 8, 3), rnd(130, 8, 8, 4, u8=True), 3, False, 0),
         "130x17 ragged": lambda: (rnd(130, 8, 8, 11), rnd(17, 8, 8, 12), 5, False, 0),
         "33 within-set": lambda: (rnd(33, 8, 8, 13), None, 5, True, 0),
         "ties, own splits": lambda: (*ties(), 4, False, 0),
         "ties, 3 splits": lambda: (*ties(), 4, False, 3),
         "int64 epilogue": lambda: (*extremes(), 2, False, 0),
         "mapping": lambda: (*mapping(), 4, False, 0)}


@pytest.fixture(scope="module")
def H():
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    return hip_impl


@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_oracle(H, name):
    a, b, k, excl, splits = CASES[name]()
    ref = T.image_knn(a, a if b is None else b, k=k, exclude_self=excl)
    # radii from the oracle's own k-th distances (equality counts as inside), some -1, over all M and not the top k
    M = a.shape[0] if b is None else b.shape[0]
    radius = ref[0][:, k - 1].repeat(M // a.shape[0] + 1)[:M].clone()
    radius[::3] = -1
    ref_r = T.image_knn(a, a if b is None else b, k=k, exclude_self=excl, radius=radius)
    assert name != "17x130 ragged" or int(ref_r[2].max()) > k
    da = a.to(DEV)
    db = da if b is None else b.to(DEV)
    if "ties" in name:
        assert H._lib.d3d_knn_splits(a.shape[0], M, splits) > 1 and int((ref[0][:, 1:] == ref[0][:, :-1]).sum()) > 0
    got = H.image_knn(da, db, k=k, exclude_self=excl, splits=splits)
    got_r = H.image_knn(da, db, k=k, exclude_self=excl, radius=radius.to(DEV), splits=splits)
    for x, y in zip(got + got_r, ref + ref_r):
        assert x.dtype == torch.int64 and torch.equal(x.cpu(), y)
    if name == "int64 epilogue":
        assert int(got[0][1, 1]) == 3 * 128 * 128 * 255 ** 2 > 2 ** 31 and int(got[1][1, 1]) == 0
    again = ops.image_knn(da, db, k=k, exclude_self=excl, radius=radius.to(DEV))      # the public op; the same bits
    assert all(torch.equal(x, y) for x, y in zip(again, got_r))


def test_image_knn_guarded(H):
    """tests/guarded.py over the panels, norms, split lists and results at a ragged shape with several splits."""
    a, b, k, _, _ = CASES["17x130 ragged"]()
    radius = torch.full((130,), 2100000, dtype=torch.int64)               # about the mean d2 of random 8 x 8 images
    ref = T.image_knn(a, b, k=k, radius=radius)
    got = guarded.run_guarded(lambda: {"a": a.to(DEV), "b": b.to(DEV), "radius": radius.to(DEV)},
                              lambda **t: H.image_knn(**t, k=k))
    assert all(torch.equal(x.cpu(), y) for x, y in zip(got, ref))


def test_knn_block_equals_cpu():
    n, size = 24, 32
    objs = list(range(1, n + 1))
    K = P.srn_intrinsics()[None].expand(n, 3, 3).contiguous()
    table = P.procedural_scene(1234, objs)
    real, gen = (T.scene_render(table, *P.procedural_pose(1234, objs, [v] * n), K, size, size, aa=2).contiguous()
                 for v in (0, 1))
    ref = knn_block([gen, real.flip(0)], real, [0.0, 3.0], k=3)
    assert knn_block([gen.to(DEV), real.flip(0).to(DEV)], real.to(DEV), [0.0, 3.0], k=3) == ref
    assert ref["per_w"]["3"] == {"precision": 1.0, "recall": 1.0, "density": ref["per_w"]["3"]["density"],
                                 "coverage": 1.0} and "split_floor" in ref
