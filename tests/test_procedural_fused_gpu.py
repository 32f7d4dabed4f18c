"""csrc/procedural.hip (ops.procedural_render / ops.procedural_batch on the GPU)
against the float64 torch composition on the CPU (procedural_scene,
procedural_pose, torch_impl.scene_render, ProceduralBatches(device="cpu").draw),
at scene.hip's smallest shapes: one partial block, a ragged last block, a
non-square image with fewer pixels than a block.  The bounds are those of
tests/test_procedural_gpu.py.  The id sets hold objects of 3, 4, 5 and 6
primitives and both kinds under both seeds, object 2^31 - 1 (the 64-bit hash
index) and view 4095; rendered on the CPU from tables and poses perturbed by
1e-12 they keep every primitive id (checked when they were chosen), so no case
sits on a silhouette.  GPU only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded as G  # noqa: E402
from distributed_3d_diffusion_pytorch_amd import ops  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.data import ProceduralBatches, procedural_pose, procedural_scene  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.data.procedural import srn_intrinsics  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T  # noqa: E402

DEV = "cuda"
BIG = 2 ** 31 - 1
SEEDS = [0, 2 ** 40 + 3]
CASES = {(1, 16, 16): ([BIG], [4095]), (5, 24, 24): ([0, 1, 2, 4, 6], [0, 7, 4095, 3, 49]),
         (3, 8, 24): ([9, BIG, 14], [1, 2, 4095])}
ID_RANGE = {("train", 1): 1, ("val", 1): 10, ("train", 1000): 1111, ("val", 1000): 10000}   # ids [0, x) hold that many
_REF = {}


def ids(shape, dev="cpu"):
    return tuple(torch.tensor(x, dtype=torch.int64, device=dev) for x in CASES[shape])


def render_reference(seed, obj, view, h, w, aa):
    """(img, depth, prim, R, t, table) of the CPU composition."""
    table, (R, t) = procedural_scene(seed, obj), procedural_pose(seed, obj, view)
    K = srn_intrinsics().expand(len(obj), 3, 3).contiguous()
    return (*T.scene_render(table, R, t, K, h, w, aa=aa, return_aux=True), R, t, table)


def reference(seed, shape, aa):
    """Computed once per case and shared."""
    if (seed, shape, aa) not in _REF:
        _REF[(seed, shape, aa)] = render_reference(seed, *ids(shape), shape[1], shape[2], aa)
    return _REF[(seed, shape, aa)]


def close(got, want, tag):
    """Poses and tables: 1e-12 absolute, the project's bound for poses."""
    for name, a, b in zip("R t table".split(), got, want):
        err = (a.cpu() - b).abs().max().item()
        print(f"{tag}: {name} {err:.3e}")
        assert a.dtype == torch.float64 and a.shape == b.shape and err <= 1e-12, name


def compare(img, depth, prim, want, tag):
    rimg, rdepth, rprim = want[:3]
    img, depth, prim = img.cpu(), depth.cpu(), prim.cpu()
    assert img.dtype == torch.float32 and depth.dtype == torch.float32 and prim.dtype == torch.int32
    same = prim == rprim
    bad = int((~same).sum())
    hit = same & (rprim >= 0)
    derr = ((depth.double() - rdepth.double()).abs() / rdepth.double())[hit].max().item() if hit.any() else 0.0
    cerr = (img.double() - rimg.double()).abs()[same[:, None].expand_as(img)].max().item()
    print(f"{tag}: {bad} of {prim.numel()} ids differ, depth rel {derr:.3e}, colour {cerr:.3e}")
    assert bad * 10000 <= prim.numel(), bad
    assert (depth[same & (rprim < 0)] == float("inf")).all()
    assert derr <= 1.2e-7 and cerr <= 2.5e-7


def test_cases_cover_the_counts_and_kinds():
    for seed in SEEDS:
        kind = torch.cat([procedural_scene(seed, o) for o, _ in CASES.values()])[..., 15]
        assert set((kind > 0).sum(1).tolist()) == {3, 4, 5, 6} and set(kind.flatten().tolist()) == {0.0, 1.0, 2.0}


@pytest.mark.parametrize("aa", [1, 3])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("shape", list(CASES), ids=lambda s: "x".join(map(str, s)))
def test_render_matches_the_cpu_composition(shape, seed, aa):
    n, h, w = shape
    obj, view = ids(shape, DEV)
    want = reference(seed, shape, aa)
    img, R, t, table, depth, prim = ops.procedural_render(seed, obj, view, h, w, aa=aa, return_aux=True)
    tag = f"{shape} seed={seed} aa={aa}"
    close((R, t, table), want[3:], tag)
    compare(img, depth, prim, want, tag)
    assert (prim[0] >= 0).any()
    plain = ops.procedural_render(seed, obj, view, h, w, aa=aa)          # without aux: the same numbers
    assert len(plain) == 4 and all(torch.equal(a, b) for a, b in zip(plain, (img, R, t, table)))
    for i in range(n):                                                   # image i reads entry i of the ids only
        one = ops.procedural_render(seed, obj[i:i + 1], view[i:i + 1], h, w, aa=aa, return_aux=True)
        assert all(torch.equal(a[0], b[i]) for a, b in zip(one, (img, R, t, table, depth, prim))), i


@pytest.mark.parametrize("index", [0, 3])
@pytest.mark.parametrize("offset", [0, 7])
@pytest.mark.parametrize("objects", [1, 1000])
@pytest.mark.parametrize("split", ["train", "val"])
@pytest.mark.parametrize("views", [2, 50])
@pytest.mark.parametrize("B", [1, 5])
def test_batch_matches_the_cpu_draw_and_render(B, views, split, objects, offset, index):
    S, seed = 16, 11
    kw = dict(n_objects=objects, views=views, split=split, aa=3)
    obj, view, img, R, t = ops.procedural_batch(seed, index, B, S, S, example_offset=offset, device=DEV, **kw)
    cpu = ProceduralBatches(B, S, "cpu", seed, objects=ID_RANGE[split, objects], views=views, split=split,
                            example_offset=offset)
    assert cpu.n_objects == objects
    robj, rview = cpu.draw(index)
    assert torch.equal(obj.cpu(), robj) and torch.equal(view.cpu(), rview)               # ids are exact
    assert obj.dtype == view.dtype == torch.int64 and (view[:, 0] != view[:, 1]).all()
    rimg, _, _, rR, rt, _ = render_reference(seed, robj.repeat_interleave(2), rview.reshape(-1), S, S, 3)
    close((R, t), (rR.reshape(B, 2, 3, 3), rt.reshape(B, 2, 3)), "batch")
    cerr = (img.cpu().double() - rimg.reshape(B, 2, 3, S, S).double()).abs().max().item()
    print(f"batch colour {cerr:.3e}")
    assert img.dtype == torch.float32 and cerr <= 2.5e-7
    assert not torch.equal(R[:, 0], R[:, 1])                  # one object (the reference above) from two views
    if B == 5:                                                # a shard reproduces its rows bit for bit
        part = ops.procedural_batch(seed, index, 3, S, S, example_offset=offset + 2, device=DEV, **kw)
        assert all(torch.equal(a[2:5], b) for a, b in zip((obj, view, img, R, t), part))


@pytest.mark.parametrize("op", ["render", "batch"])
def test_guarded(op):
    """Guards intact, every output element written, two poisoned runs identical
    (tests/guarded.py).  The harness wants finite results and a miss's depth is
    +inf by definition, so the depth goes through it as (depth with misses at
    0, the miss mask), as in test_scene_render_guarded."""
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl as H
    shape = (5, 24, 24)

    def render(obj, view):
        img, R, t, table, depth, prim = H.procedural_render(SEEDS[1], obj, view, 24, 24, aa=3, return_aux=True)
        miss = depth == float("inf")
        return img, R, t, table, torch.where(miss, torch.zeros_like(depth), depth), miss, prim

    if op == "render":
        img, R, t, table, depth, miss, prim = G.run_guarded(lambda: dict(zip(("obj", "view"), ids(shape, DEV))), render)
        want = reference(SEEDS[1], shape, 3)
        assert torch.equal(miss, prim < 0)
        close((R, t, table), want[3:], "guarded")
        compare(img, torch.where(miss, torch.full_like(depth, float("inf")), depth), prim, want, "guarded")
    else:
        kw = dict(n_objects=1000, views=50, split="train", example_offset=7, aa=3)
        got = G.run_guarded(dict, lambda: H.procedural_batch(11, 3, 5, 24, 24, device=DEV, **kw))
        assert all(torch.equal(a, b) for a, b in zip(got, ops.procedural_batch(11, 3, 5, 24, 24, device=DEV, **kw)))


RENDER_OK = dict(seed=0, object_ids=[1, 2], view_ids=[0, 1], H=8, W=8)
BATCH_OK = dict(seed=0, batch_index=0, B=2, H=8, W=8, n_objects=10, views=5, split="train")


@pytest.mark.parametrize("op,kw", [
    ("render", dict(aa=0)), ("render", dict(aa=5)), ("batch", dict(aa=0)), ("batch", dict(aa=5)),
    ("batch", dict(views=1)), ("batch", dict(views=4097)),
    ("render", dict(object_ids=[1, -1])), ("render", dict(object_ids=[2 ** 31, 1])),
    ("render", dict(view_ids=[-1, 0])), ("render", dict(view_ids=[0, 4096])), ("render", dict(view_ids=[0, 1, 2]))],
    ids=lambda x: x if isinstance(x, str) else "-".join(f"{k}={v}" for k, v in x.items()).replace(" ", ""))
def test_bad_arguments_raise_on_the_gpu(op, kw):
    a = dict(RENDER_OK if op == "render" else dict(BATCH_OK, device=DEV), **kw)
    if op == "render":
        a.update({k: torch.tensor(a[k], dtype=torch.int64, device=DEV) for k in ("object_ids", "view_ids")})
    with pytest.raises(ValueError):
        (ops.procedural_render if op == "render" else ops.procedural_batch)(**a)
