"""csrc/ensemble.hip (ops.ensemble_stats on the GPU) against the float64 torch
form on the CPU: exactly one block with one sample, a ragged third block with
an odd sample count and all four classes, a non-square image, eight samples.
target is the rendered ground truth of the renderer tests' objects, samples
the ground truth plus a fixed hash noise of amplitude 0.1 per sample, klass
the CPU class plane of view_consistency for those objects (view 0 -> view 1;
with more than one group the last source camera looks away).  Then
determinism and batch independence, the guard-band harness, bad arguments and
one evaluation run.  GPU only."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded as G  # noqa: E402
from distributed_3d_diffusion_pytorch_amd import ops  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.data import (procedural_objects, procedural_pose,  # noqa: E402
                                                       procedural_scene)
from distributed_3d_diffusion_pytorch_amd.data import procedural as P  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T  # noqa: E402

DEV = "cuda"
SEED = 1234
# (G, C, H, W) -> the objects
SHAPES = {(1, 1, 16, 16): [1], (5, 5, 24, 24): [0, 1, 2, 3, 4], (3, 2, 8, 24): [9, 3, 5], (2, 8, 16, 16): [1, 3]}
_IN, _REF = {}, {}


@pytest.fixture(scope="module")
def H():
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    yield hip_impl
    _IN.clear()
    _REF.clear()


def inputs(shape):
    """CPU inputs of a shape, computed once and shared."""
    if shape not in _IN:
        objs = SHAPES[shape]
        n, c, h, w = shape
        table = procedural_scene(SEED, objs)
        K = P.srn_intrinsics().expand(n, 3, 3).contiguous()
        Rs, ts = procedural_pose(SEED, objs, [0] * n)
        Rt, tt = procedural_pose(SEED, objs, [1] * n)
        src = T.scene_render(table, Rs, ts, K, h, w, aa=3)
        gt = T.scene_render(table, Rt, tt, K, h, w, aa=3)
        if n > 1:
            Rs[-1, :, 0] *= -1
            Rs[-1, :, 2] *= -1
        klass = T.view_consistency(table, K, Rs, ts, src, Rt, tt, gt, return_class=True)[1].contiguous()
        amp = (T.u01(78, torch.arange(n * c * gt[0].numel())).reshape(n, c, *gt.shape[1:]) * 2 - 1) * 0.1
        _IN[shape] = {"samples": (gt[:, None] + amp).contiguous(), "target": gt.contiguous(), "klass": klass}
    return _IN[shape]


def reference(shape, with_klass, quantize):
    """The float64 torch form on the CPU (with the maps), computed once per case and shared."""
    key = (shape, with_klass, quantize)
    if key not in _REF:
        a = inputs(shape)
        _REF[key] = T.ensemble_stats(a["samples"], a["target"], a["klass"] if with_klass else None, quantize=quantize,
                                     return_maps=True)
    return _REF[key]


def on_dev(shape, with_klass=True):
    a = {k: v.to(DEV) for k, v in inputs(shape).items()}
    if not with_klass:
        del a["klass"]
    return a


def compare(got, want, tag=""):
    """The issue's conditions on stats (and the maps, where given) against the oracle's."""
    stats, maps = (got[0], got[1:]) if isinstance(got, tuple) else (got, ())
    stats = stats.cpu()
    rstats = want[0]
    assert stats.dtype == torch.float64 and stats.shape == rstats.shape
    assert torch.equal(stats[..., 0], rstats[..., 0])
    d, r = (stats[..., 1:] - rstats[..., 1:]).abs(), rstats[..., 1:].abs()
    print(f"{tag}: sums relative {float((d / r.clamp_min(1e-300))[r != 0].max()) if (r != 0).any() else 0.0:.3e}")
    assert (d <= 1e-9 * r).all()
    for name, m, rm in zip(("mean", "std"), maps, want[1:]):
        m = m.cpu()
        assert m.dtype == torch.float32 and m.shape == rm.shape
        err = (m.double() - rm.double()).abs().max().item()
        print(f"{tag}: {name} absolute {err:.3e}")
        assert err <= 2.5e-7


@pytest.mark.parametrize("quantize", [True, False], ids=["png", "float"])
@pytest.mark.parametrize("with_klass", [True, False], ids=["klass", "noklass"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_fp64_oracle(H, shape, with_klass, quantize):
    n, c, h, w = shape
    dev = on_dev(shape, with_klass)
    want = reference(shape, with_klass, quantize)
    got = H.ensemble_stats(**dev, quantize=quantize, return_maps=True)
    tag = f"{shape} klass={with_klass} quantize={quantize}"
    compare(got, want, tag)
    stats = got[0]
    assert (stats[..., 0].sum(1) == h * w).all()
    if not with_klass:
        assert (stats[:, 1:] == 0).all()
    if c == 1:
        assert (stats[..., 2] == 0).all() and torch.equal(stats[..., 3], stats[..., 1]) and (got[2] == 0).all()
    else:
        assert (stats[:, 0, 2] > 0).all()
    e = (stats[..., 1] + stats[..., 2] - stats[..., 3]).abs()
    assert (e <= 1e-12 * stats[..., 3]).all()                          # E = B + V per (group, class)
    # without the maps: the same numbers; the public op takes the same path
    plain = H.ensemble_stats(**dev, quantize=quantize)
    assert torch.equal(plain, stats)
    pub = ops.ensemble_stats(**dev, quantize=quantize, return_maps=True)
    assert all(torch.equal(a, b) for a, b in zip(pub, got))


def test_all_classes_occur():
    k = inputs((5, 5, 24, 24))["klass"]
    assert set(k.flatten().tolist()) == {0, 1, 2, 3}
    assert (k[-1] < 2).all() and (k[-1] == 1).any()                    # its source camera looks away


@pytest.mark.parametrize("shape", [(5, 5, 24, 24), (2, 8, 16, 16)], ids=lambda s: "x".join(map(str, s)))
def test_reproducible_and_batch_independent(H, shape):
    dev = on_dev(shape)
    first = H.ensemble_stats(**dev, return_maps=True)
    again = H.ensemble_stats(**dev, return_maps=True)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for i in range(shape[0]):
        one = H.ensemble_stats(**{k: v[i:i + 1] for k, v in dev.items()}, return_maps=True)
        assert all(torch.equal(a, b[i:i + 1]) for a, b in zip(one, first)), i


@pytest.mark.parametrize("with_klass,with_maps", [(True, True), (False, True), (False, False)])
def test_ensemble_stats_guarded(H, with_klass, with_maps):
    """Guards intact, inputs unchanged, two poisoned runs identical (tests/guarded.py)."""
    shape = (5, 5, 24, 24)
    res = G.run_guarded(lambda: on_dev(shape, with_klass), lambda **a: H.ensemble_stats(**a, return_maps=with_maps))
    compare(res, reference(shape, with_klass, True), f"guarded klass={with_klass} maps={with_maps}")


def test_bad_arguments_raise_on_the_gpu(H):
    dev = on_dev((1, 1, 16, 16))
    for kw in (dict(samples=dev["samples"][0]), dict(samples=dev["samples"].double()),
               dict(samples=dev["samples"].cpu()), dict(samples=dev["samples"].transpose(-1, -2)),
               dict(samples=dev["samples"][:, :0]), dict(target=dev["target"][..., :15].contiguous()),
               dict(target=dev["target"].cpu()), dict(target=dev["target"].double()),
               dict(klass=dev["klass"].long()), dict(klass=dev["klass"].cpu()), dict(klass=dev["klass"][:, :15])):
        with pytest.raises(ValueError):
            ops.ensemble_stats(**dict(dev, **kw))
    st, mean, std = ops.ensemble_stats(**{k: v[:0] for k, v in dev.items()}, return_maps=True)
    assert st.shape == (0, 4, 4) and st.dtype == torch.float64 and st.is_cuda
    assert mean.shape == (0, 3, 16, 16) and mean.dtype == torch.float32 and mean.is_cuda
    assert std.shape == (0, 16, 16) and std.dtype == torch.float32 and std.is_cuda
    st = ops.ensemble_stats(dev["samples"][:0], dev["target"][:0])
    assert st.shape == (0, 4, 4) and st.dtype == torch.float64 and st.is_cuda


def test_evaluate_objects_end_to_end():
    """evaluate_objects(samples=2, consistency=True) on the HIP backend: 2
    procedural objects x 1 view at 32 x 32, dpmpp2m, 4 steps, 4 chains; the
    fields are finite or None, the counts add up, the samples differ, nothing
    falls back."""
    from distributed_3d_diffusion_pytorch_amd.engine import evaluate_objects, summarize_ensemble
    from distributed_3d_diffusion_pytorch_amd.models import XUNet
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    torch.manual_seed(14)
    m = XUNet(H=32, W=32, ch=128).to(DEV)
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().sum() == 0:
                p.normal_(0, 0.02)
    m.compute_dtype = torch.bfloat16
    m.eval()
    objs = procedural_objects(SEED, 2, [0, 1], 32, objects=100, device=DEV)
    rows, _, pair_rows, ens = evaluate_objects(m, objs, input_view=0, views=(1,), w=(3.0,), timesteps=4, batch=2,
                                               seed=3, device=DEV, solver="dpmpp2m", consistency=True, samples=2)
    assert len(rows) == 4 and pair_rows == [] and len(ens) == 2
    assert [(r["chain"], r["sample"]) for r in rows] == [(0, 0), (1, 1), (2, 0), (3, 1)]
    for e in ens:
        for k, v in e.items():
            assert v is None or isinstance(v, (str, int)) or math.isfinite(v), (k, e)
        assert e["samples"] == 2 and e["n"] == 1024
        assert e["n_background"] + e["n_disoccluded"] + e["n_covisible"] == 1024
        assert e["spread"] > 0
        grp = [r for r in rows if r["instance"] == e["instance"]]
        assert len(grp) == 2
        want = (grp[0]["mse"] + grp[1]["mse"]) / 2
        print(f"{e['instance']}: mse_samples {e['mse_samples']:.9e}, the rows' mean {want:.9e}")
        assert abs(e["mse_samples"] - want) <= 1e-6 * want
    print(f"pooled: {summarize_ensemble(ens)}")
    assert hip_impl.FALLBACKS == {}, hip_impl.FALLBACKS
