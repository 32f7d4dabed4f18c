"""csrc/scene.hip (ops.scene_render on the GPU) against the float64 torch form
on the same tables and cameras, at the smallest shapes that can go wrong:
exactly one block, a ragged third block, a non-square image; aa 1 and 3;
3- and 6-primitive objects, both kinds, an all-miss camera.  Then the
guard-band harness, the on-device batches and a training step.  GPU only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded as G  # noqa: E402
from distributed_3d_diffusion_pytorch_amd import ops  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.data import ProceduralBatches, procedural_pose, procedural_scene  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.data import procedural as P  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T  # noqa: E402

DEV = "cuda"
SEED = 1234
# objects 0 and 9 have 3 primitives, 1, 3 and 5 have 6 (test_cases_cover_the_kinds_and_counts checks it)
SHAPES = {(1, 16, 16): [1], (5, 24, 24): [0, 1, 2, 3, 4], (3, 8, 24): [9, 3, 5]}
_REF = {}


@pytest.fixture(scope="module")
def H():
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    yield hip_impl
    _REF.clear()


def inputs(shape):
    """CPU inputs of a shape; with more than one image, the last camera looks away (all-miss)."""
    objs = SHAPES[shape]
    table = procedural_scene(SEED, objs)
    R, t = procedural_pose(SEED, objs, list(range(len(objs))))
    if len(objs) > 1:
        R[-1, :, 0] *= -1
        R[-1, :, 2] *= -1
    return {"table": table, "R": R, "t": t, "K": P.srn_intrinsics().expand(len(objs), 3, 3).contiguous()}


def reference(shape, aa):
    """The float64 torch form on the CPU, computed once per case and shared."""
    if (shape, aa) not in _REF:
        _REF[(shape, aa)] = T.scene_render(**inputs(shape), H=shape[1], W=shape[2], aa=aa, return_aux=True)
    return _REF[(shape, aa)]


def compare(got, want, tag=""):
    """The issue's conditions on (img, depth, prim) against the oracle's."""
    img, depth, prim = (x.cpu() for x in got)
    rimg, rdepth, rprim = want
    assert img.dtype == torch.float32 and depth.dtype == torch.float32 and prim.dtype == torch.int32
    bad = int((prim != rprim).sum())
    same = prim == rprim
    hit = same & (rprim >= 0)
    derr = ((depth.double() - rdepth.double()).abs() / rdepth.double())[hit].max().item() if hit.any() else 0.0
    cerr = (img.double() - rimg.double()).abs().max().item()
    print(f"{tag}: {bad} of {prim.numel()} ids differ, depth rel {derr:.3e}, colour {cerr:.3e}, "
          f"coverage {float((rprim >= 0).float().mean()):.2f}")
    assert bad * 10000 <= prim.numel(), bad
    assert torch.isinf(depth[same & (rprim < 0)]).all() and (depth[same & (rprim < 0)] > 0).all()
    assert derr <= 1.2e-7
    assert cerr <= 2.5e-7
    return img, depth, prim


def test_cases_cover_the_kinds_and_counts():
    counts, kinds = [], set()
    for objs in SHAPES.values():
        kind = procedural_scene(SEED, objs)[..., 15]
        counts += (kind > 0).sum(1).tolist()
        kinds |= set(kind.flatten().tolist())
    assert {3, 6} <= set(counts) and kinds == {0.0, 1.0, 2.0}


@pytest.mark.parametrize("aa", [1, 3])
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_fp64_oracle(H, shape, aa):
    N, h, w = shape
    dev = {k: v.to(DEV) for k, v in inputs(shape).items()}
    got = H.scene_render(**dev, H=h, W=w, aa=aa, return_aux=True)
    img, depth, prim = compare(got, reference(shape, aa), f"{shape} aa={aa}")
    assert (prim[0] >= 0).any()
    if N > 1:                                                           # the all-miss camera
        assert (img[-1] == 1).all() and (prim[-1] == -1).all() and torch.isinf(depth[-1]).all()
    # the public op takes the same path; without aux it is the same image
    pub = ops.scene_render(**dev, H=h, W=w, aa=aa)
    assert torch.equal(pub.cpu(), img)
    # two runs are bitwise equal, and image i does not depend on the rest of the batch
    again = H.scene_render(**dev, H=h, W=w, aa=aa, return_aux=True)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    for i in range(N):
        one = H.scene_render(**{k: v[i:i + 1] for k, v in dev.items()}, H=h, W=w, aa=aa, return_aux=True)
        for a, b in zip(got, one):
            assert torch.equal(a[i:i + 1], b), i


@pytest.mark.parametrize("aux", [False, True])
def test_scene_render_guarded(H, aux):
    """Guards intact, inputs unchanged, two poisoned runs identical (tests/guarded.py).
    The harness wants finite results and a miss's depth is +inf by definition,
    so the depth goes through it as (depth with misses at 0, the miss mask):
    a poisoned (NaN) depth element is in neither and still fails."""
    shape = (5, 24, 24)
    make = lambda: {k: v.to(DEV) for k, v in inputs(shape).items()}  # noqa: E731

    def run(table, R, t, K):
        out = H.scene_render(table, R, t, K, 24, 24, aa=3, return_aux=aux)
        if not aux:
            return out
        img, depth, prim = out
        miss = depth == float("inf")
        return img, torch.where(miss, torch.zeros_like(depth), depth), miss, prim

    res = G.run_guarded(make, run)
    want = reference(shape, 3)
    if aux:
        img, depth, miss, prim = res
        assert torch.equal(miss, prim < 0)
        compare((img, torch.where(miss, torch.full_like(depth, float("inf")), depth), prim), want, "guarded")
    else:
        assert (res.cpu().double() - want[0].double()).abs().max() <= 2.5e-7


def test_bad_arguments_raise_on_the_gpu(H):
    dev = {k: v.to(DEV) for k, v in inputs((1, 16, 16)).items()}
    for kw in (dict(aa=0), dict(aa=5), dict(H=0), dict(R=dev["R"].float()), dict(K=dev["K"].cpu()),
               dict(table=dev["table"][:, :5])):
        a = dict(dev, H=4, W=4, aa=3)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.scene_render(**a)
    assert ops.scene_render(**{k: v[:0] for k, v in dev.items()}, H=4, W=4).shape == (0, 3, 4, 4)


def test_batches_match_the_torch_backend():
    """ProceduralBatches on the GPU (scene.hip) == the CPU iterator (the torch
    form), to the kernel's colour tolerance; a shard reproduces its rows."""
    kw = dict(imgsize=24, seed=11, objects=300, views=9)
    gpu, cpu = ProceduralBatches(6, device=DEV, **kw), ProceduralBatches(6, device="cpu", **kw)
    shard = ProceduralBatches(3, device=DEV, example_offset=3, **kw)
    for _ in range(2):
        g, c, s = next(gpu), next(cpu), next(shard)
        assert all(x.is_cuda for x in g) and [x.dtype for x in g] == [x.dtype for x in c]
        cerr = (g[0].cpu().double() - c[0].double()).abs().max().item()
        print(f"batch colour difference {cerr:.3e}")
        assert cerr <= 2.5e-7
        for a, b in zip(g[1:], c[1:]):
            assert (a.cpu() - b).abs().max() < 1e-12
        for a, b in zip(g, s):
            assert torch.equal(a[3:], b)
        assert 0.05 < float((g[0] < 0.999).float().mean()) < 0.7     # objects in front of the white background


def test_training_step_on_a_procedural_batch():
    """One eager and one graph-replayed training step at 32 x 32 on a
    procedural batch: finite losses that agree (the bound of
    test_graph_train_step_matches_eager), nothing falls back."""
    from distributed_3d_diffusion_pytorch_amd.config import make_config
    from distributed_3d_diffusion_pytorch_amd.engine import Trainer
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    from distributed_3d_diffusion_pytorch_amd.parallel import DistContext
    ov = {"model.H": 32, "model.W": 32, "model.dropout": 0.1, "data.imgsize": 32, "global_batch": 4,
          "data.procedural": True, "data.procedural_objects": 100, "log_every": 0, "ckpt_every": 0,
          "optim.warmup_examples": 8, "micro_batch": 0}
    try:
        losses = []
        for graph in (False, True):
            tr = Trainer(make_config(None, dict(ov, graph=graph)), DistContext(device=torch.device("cuda", 0)))
            data, _, _ = tr.make_data()
            assert isinstance(data, ProceduralBatches) and data.split == "train"
            batch = next(data)
            assert batch[0].shape == (4, 2, 3, 32, 32) and batch[0].is_cuda
            losses.append(tr.train_step(*batch).item())
            tr.sync()
            assert (tr._graphed is not None) == graph
        print(f"eager {losses[0]} graph {losses[1]}")
        assert all(x == x and abs(x) < 1e4 for x in losses), losses
        assert abs(losses[0] - losses[1]) <= 2e-3 * abs(losses[0]) + 1e-4, losses
        val = tr.make_val_data()
        assert len(val) >= 1 and val[0][0].shape == (4, 2, 3, 32, 32)
        v = tr.validation_loss(val)
        assert v == v and v > 0
    finally:
        hip_impl.set_device_seed(None)
    assert hip_impl.FALLBACKS == {}, hip_impl.FALLBACKS
