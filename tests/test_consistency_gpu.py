"""csrc/consistency.hip (ops.view_consistency on the GPU) against the float64
torch form on the CPU, at the renderer tests' shapes: exactly one block, a
ragged third block with the last pair's source camera turned away, a
non-square image with 3- and 6-primitive objects of both kinds.  src is the
ground truth, tgt the ground truth plus a fixed hash noise of amplitude 0.1,
ref the ground truth.  Then determinism and batch independence, the
guard-band harness, bad arguments and one evaluation run.  GPU only."""
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
SHAPES = {(1, 16, 16): [1], (5, 24, 24): [0, 1, 2, 3, 4], (3, 8, 24): [9, 3, 5]}
# (hit, co-visible, clean) of objects 0..4 at 24 x 24, view 0 -> view 1, on the CPU
COUNTS_24 = [(155, 2, 0), (259, 166, 48), (296, 233, 29), (224, 205, 65), (155, 92, 9)]
_IN, _REF = {}, {}


@pytest.fixture(scope="module")
def H():
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    yield hip_impl
    _IN.clear()
    _REF.clear()


def inputs(shape):
    """CPU inputs of a shape (view 0 -> view 1 of each object, rendered by the
    torch form); with more than one pair, the last source camera looks away."""
    if shape not in _IN:
        objs = SHAPES[shape]
        n, h, w = shape
        table = procedural_scene(SEED, objs)
        K = P.srn_intrinsics().expand(n, 3, 3).contiguous()
        Rs, ts = procedural_pose(SEED, objs, [0] * n)
        Rt, tt = procedural_pose(SEED, objs, [1] * n)
        src = T.scene_render(table, Rs, ts, K, h, w, aa=3)
        gt = T.scene_render(table, Rt, tt, K, h, w, aa=3)
        if n > 1:
            Rs[-1, :, 0] *= -1
            Rs[-1, :, 2] *= -1
        amp = (T.u01(77, torch.arange(gt.numel())).reshape(gt.shape) * 2 - 1) * 0.1
        _IN[shape] = {"table": table, "K": K, "R_src": Rs, "t_src": ts, "img_src": src, "R_tgt": Rt, "t_tgt": tt,
                      "img_tgt": (gt + amp).contiguous(), "ref": gt}
    return _IN[shape]


def reference(shape, with_ref):
    """The float64 torch form on the CPU, computed once per case and shared."""
    if (shape, with_ref) not in _REF:
        a = dict(inputs(shape))
        if not with_ref:
            a["ref"] = None
        _REF[(shape, with_ref)] = T.view_consistency(**a, return_class=True)
    return _REF[(shape, with_ref)]


def on_dev(shape, with_ref=True):
    a = {k: v.to(DEV) for k, v in inputs(shape).items()}
    if not with_ref:
        a["ref"] = None
    return a


def compare(stats, cls, want, tag=""):
    """The issue's conditions on (stats, class plane) against the oracle's."""
    rstats, rcls = want
    stats = stats.cpu()
    assert stats.dtype == torch.float64 and stats.shape == rstats.shape
    if cls is not None:
        cls = cls.cpu()
        assert cls.dtype == torch.int32 and cls.shape == rcls.shape
        bad = int((cls != rcls).sum())
        print(f"{tag}: {bad} of {cls.numel()} classes differ")
        assert bad * 10000 <= cls.numel(), bad
        if bad:                                 # (the counts and sums are compared where the planes agree everywhere)
            return
    assert torch.equal(stats[:, :4], rstats[:, :4])
    err = ((stats[:, 4:] - rstats[:, 4:]).abs() / (rstats[:, 4:].abs() + 1e-300))[rstats[:, 4:] != 0]
    print(f"{tag}: sums relative {float(err.max()) if err.numel() else 0.0:.3e}")
    assert ((stats[:, 4:] - rstats[:, 4:]).abs() <= 1e-9 * rstats[:, 4:].abs() + 1e-12).all()


@pytest.mark.parametrize("with_ref", [True, False], ids=["ref", "noref"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_fp64_oracle(H, shape, with_ref):
    N, h, w = shape
    dev = on_dev(shape, with_ref)
    want = reference(shape, with_ref)
    stats, cls = H.view_consistency(**dev, return_class=True)
    compare(stats, cls, want, f"{shape} ref={with_ref}")
    assert (stats[:, :3].sum(1) == h * w).all() and (stats[:, 3] <= stats[:, 2]).all()
    if not with_ref:
        assert (stats[:, 4:7] == 0).all()
    if N > 1:                                                          # the source camera that looks away
        assert stats[-1, 2] == 0 and stats[-1, 3] == 0 and stats[-1, 7] == 0 and stats[-1, 1] > 0
    # without the class plane: the same numbers; the public op takes the same path
    plain = H.view_consistency(**dev)
    assert torch.equal(plain, stats)
    compare(plain, None, want, f"{shape} ref={with_ref} no class plane")
    pub = ops.view_consistency(**dev, return_class=True)
    assert torch.equal(pub[0], stats) and torch.equal(pub[1], cls)
    # two runs are bitwise equal, and pair i does not depend on the rest of the batch
    again = H.view_consistency(**dev, return_class=True)
    assert torch.equal(again[0], stats) and torch.equal(again[1], cls)
    for i in range(N):
        one = H.view_consistency(**{k: (v[i:i + 1] if v is not None else None) for k, v in dev.items()},
                                 return_class=True)
        assert torch.equal(one[0], stats[i:i + 1]) and torch.equal(one[1], cls[i:i + 1]), i


def test_all_classes_occur(H):
    shape = (5, 24, 24)
    stats, cls = H.view_consistency(**on_dev(shape), return_class=True)
    stats = stats.cpu()
    got = [(int(stats[i, 1] + stats[i, 2]), int(stats[i, 2]), int(stats[i, 3])) for i in range(5)]
    print(f"(hit, co-visible, clean) per pair: {got}")
    assert set(cls.flatten().tolist()) == {0, 1, 2, 3}
    assert got[:4] == COUNTS_24[:4]
    assert got[4] == (COUNTS_24[4][0], 0, 0)                           # its source camera looks away
    # ground truth on both sides: the clean pixels reproject to better than 50 dB (57.6 dB over 24 objects)
    a = on_dev(shape)
    gt = H.view_consistency(**dict(a, img_tgt=a["ref"], ref=None)).cpu()
    psnr = 10 * math.log10(3 * gt[:, 3].sum().item() / gt[:, 7].sum().item())
    print(f"ground-truth clean reprojection PSNR over {int(gt[:, 3].sum())} pixels: {psnr:.2f} dB")
    assert psnr >= 50.0


@pytest.mark.parametrize("with_ref,with_cls", [(True, True), (False, False), (True, False), (False, True)])
def test_view_consistency_guarded(H, with_ref, with_cls):
    """Guards intact, inputs unchanged, two poisoned runs identical (tests/guarded.py)."""
    shape = (5, 24, 24)

    def make():
        a = on_dev(shape, with_ref)
        return a if with_ref else {k: v for k, v in a.items() if k != "ref"}

    res = G.run_guarded(make, lambda **a: H.view_consistency(**a, return_class=with_cls))
    stats, cls = res if with_cls else (res, None)
    compare(stats, cls, reference(shape, with_ref), f"guarded ref={with_ref} class={with_cls}")


def test_bad_arguments_raise_on_the_gpu(H):
    dev = on_dev((1, 16, 16))
    for kw in (dict(table=dev["table"][:, :5]), dict(K=dev["K"].float()), dict(R_src=dev["R_src"].cpu()),
               dict(img_src=dev["img_src"].double()), dict(img_tgt=dev["img_tgt"][..., :15]),
               dict(img_tgt=dev["img_tgt"].transpose(-1, -2)), dict(ref=dev["ref"].cpu()),
               dict(t_tgt=dev["t_tgt"][:, :2])):
        with pytest.raises(ValueError):
            ops.view_consistency(**dict(dev, **kw))
    st, cls = ops.view_consistency(**{k: v[:0] for k, v in dev.items()}, return_class=True)
    assert st.shape == (0, 8) and st.dtype == torch.float64 and st.is_cuda
    assert cls.shape == (0, 16, 16) and cls.dtype == torch.int32 and cls.is_cuda


def test_evaluate_objects_end_to_end():
    """evaluate_objects(consistency=True) on the HIP backend: 2 procedural
    objects x 2 views at 32 x 32, dpmpp2m, 4 steps; the fields are finite or
    None, the counts add up, nothing falls back."""
    from distributed_3d_diffusion_pytorch_amd.engine import evaluate_objects, gt_ceiling, summarize_consistency
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
    objs = procedural_objects(SEED, 2, [0, 1, 2], 32, objects=100, device=DEV)
    rows, _, pair_rows = evaluate_objects(m, objs, input_view=0, views=(1, 2), w=(3.0,), timesteps=4, batch=2, seed=3,
                                          device=DEV, solver="dpmpp2m", consistency=True)
    assert len(rows) == 4 and len(pair_rows) == 4
    for r in rows:
        assert r["n_background"] + r["n_disoccluded"] + r["n_covisible"] == 32 * 32
        assert r["n_clean"] <= r["n_covisible"]
        assert r["n_background"] > 0 and r["n_disoccluded"] + r["n_covisible"] > 0
        for k in ("mse_background", "psnr_background", "mse_disoccluded", "psnr_disoccluded", "mse_covisible",
                  "psnr_covisible", "reproj_mse", "reproj_psnr", "mse", "psnr", "ssim"):
            assert r[k] is None or math.isfinite(r[k]), (k, r)
        assert r["mse_background"] is not None
    for p in pair_rows:
        assert (p["mse"] is None and p["psnr"] is None) or (math.isfinite(p["mse"]) and math.isfinite(p["psnr"]))
        assert (p["n_clean"] == 0) == (p["mse"] is None)
    s = summarize_consistency(rows, pair_rows)
    c = gt_ceiling(objs, 0, (1, 2), DEV)
    print(f"pooled: {s}\nground-truth ceiling: {c}")
    assert set(s) == {"3"} and s["3"]["background"]["n"] == sum(r["n_background"] for r in rows)
    assert c["reproj"]["n"] == sum(r["n_clean"] for r in rows)       # the same geometry, the same clean pixels
    assert hip_impl.FALLBACKS == {}, hip_impl.FALLBACKS
