"""csrc/field.hip (ops.field_render, ops.field_loss_grad on the GPU) against the
float64 torch form on the CPU: a single cell where every sample is clamped, a
non-power-of-two grid, a ragged last block, more than one block; bound 0.5 and
1.  The rays are pixels of two procedural orbit cameras plus five by hand (a
miss, an origin inside the cube, a zero direction component inside and outside
its slab, a ray along a cube face); the grids hold hash values in [-6, 6].
Then reproducibility, rays that miss, the tiled ray layout, the guard-band
harness, bad arguments and one fit.  GPU only."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
from distributed_3d_diffusion_pytorch_amd import ops  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.data import procedural as P  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T  # noqa: E402

DEV = "cuda"
SEED = 1234
CASES = [(2, 1, 1), (5, 64, 7), (16, 257, 32), (8, 1024, 16)]           # (G, R, S)
BOUNDS = [0.5, 1.0]
# profiles/field/README.md, "Tolerances": the largest difference between the
# torch form evaluated in fp32 and in fp64 on the CPU over these 8 inputs; the
# kernel may differ from fp64 by 4 x that (another fp32 operation order, FMAs).
FP32_C, FP32_LOSS_REL, FP32_GRAD_REL = 5.318e-7, 3.172e-7, 1.366e-6
TOL_C, TOL_LOSS_REL, TOL_GRAD_REL = 4 * FP32_C, 4 * FP32_LOSS_REL, 4 * FP32_GRAD_REL
_IN, _REF = {}, {}


@pytest.fixture(scope="module")
def H():
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    yield hip_impl
    _IN.clear()
    _REF.clear()


def inputs(case, bound):
    """CPU inputs of a case, computed once and shared."""
    if (case, bound) not in _IN:
        G, R, S = case
        b = bound
        Rc, tc = P.procedural_pose(SEED, [1, 1], [0, 1])
        pos, dirs = T.camera_rays(Rc[None], tc[None], P.srn_intrinsics()[None], 24, 24, 128)
        n = max(R - 5, 1)
        sel = (torch.arange(n) * (2 * 24 * 24 // n) + 24 * 12 + 12) % (2 * 24 * 24)   # starts at a centre pixel
        hand_o = torch.tensor([[3, 3, 3], [0.1, -0.2, 0.3], [0.2, 0.3, -3], [1.5, 0, -3], [-3, 1, 0.1]]) * b
        hand_d = torch.tensor([[2 / 3, 2 / 3, 1 / 3], [0.36, 0.48, -0.8], [0, 0.28, 0.96], [0, 0, 1], [1, 0, 0]])
        o = torch.cat([pos.reshape(-1, 3)[sel], hand_o.float()])[:R].contiguous()
        d = torch.cat([dirs.reshape(-1, 3)[sel], hand_d.float()])[:R].contiguous()
        grid = (T.u01(SEED + G, torch.arange(G ** 3 * 4)) * 12 - 6).reshape(G, G, G, 4).contiguous()
        y = (T.u01(77, torch.arange(R * 3)) * 2 - 1).reshape(R, 3).contiguous()
        _IN[(case, bound)] = {"grid": grid, "rays_o": o, "rays_d": d, "target": y}
    return _IN[(case, bound)]


def reference(case, bound):
    """(C, L, grad) of the float64 torch form on the CPU, computed once per case and shared."""
    if (case, bound) not in _REF:
        a = inputs(case, bound)
        C = T._field_march(a["grid"].double(), a["rays_o"], a["rays_d"], case[2], bound, torch.float64)
        _REF[(case, bound)] = (C, *T.field_loss_grad(**a, samples=case[2], bound=bound))
    return _REF[(case, bound)]


def on_dev(case, bound):
    return {k: v.to(DEV) for k, v in inputs(case, bound).items()}


def compare(C, L, g, case, bound, tag):
    rC, rL, rg = reference(case, bound)
    if C is not None:
        eC = (C.cpu().double() - rC).abs().max().item()
        print(f"{tag}: C absolute {eC:.3e} (bound {TOL_C:.3e})")
        assert C.dtype == torch.float32 and eC <= TOL_C
    if L is not None:
        eL = abs(L.item() - rL.item()) / rL.item()
        eg = (g.cpu().double() - rg.double()).abs().max().item() / rg.abs().max().item()
        print(f"{tag}: loss relative {eL:.3e} (bound {TOL_LOSS_REL:.3e}), grad relative to its max {eg:.3e} "
              f"(bound {TOL_GRAD_REL:.3e})")
        assert L.dtype == torch.float64 and L.dim() == 0 and g.dtype == torch.float32 and g.shape == rg.shape
        assert eL <= TOL_LOSS_REL and eg <= TOL_GRAD_REL


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernels_match_fp64_oracle(H, case, bound):
    a, S = on_dev(case, bound), case[2]
    rays = {k: a[k] for k in ("grid", "rays_o", "rays_d")}
    C = H.field_render(**rays, samples=S, bound=bound)
    L, g = H.field_loss_grad(**a, samples=S, bound=bound)
    compare(C, L, g, case, bound, f"{case} bound={bound}")
    # the loss is the rendered colours' error; the public ops take the same path
    want = (C.double() - (a["target"].double() + 1) * 0.5).square().sum().item()
    assert abs(L.item() - want) <= 1e-12 * want
    assert torch.equal(ops.field_render(**rays, samples=S, bound=bound), C)
    pL, pg = ops.field_loss_grad(**a, samples=S, bound=bound)
    assert torch.equal(pL, L) and torch.equal(pg, g)


def test_reproducible_misses_and_tiles(H):
    case, bound = (16, 257, 32), 1.0
    a = on_dev(case, bound)
    L, g = H.field_loss_grad(**a, samples=32, bound=bound)
    L2, g2 = H.field_loss_grad(**a, samples=32, bound=bound)
    assert torch.equal(L, L2) and torch.equal(g, g2)
    # appended rays that all miss (their target is the white background) change neither output
    far = torch.tensor([[0.0, 0.0, 5.0]], device=DEV).expand(300, 3)
    more = {"grid": a["grid"], "rays_o": torch.cat([a["rays_o"], far]).contiguous(),
            "rays_d": torch.cat([a["rays_d"], far / 5]).contiguous(),
            "target": torch.cat([a["target"], torch.ones(300, 3, device=DEV)]).contiguous()}
    L3, g3 = H.field_loss_grad(**more, samples=32, bound=bound)
    assert torch.equal(L, L3) and torch.equal(g, g3)
    # image rows of width 19 (8 x 8 tiles, ragged in both directions): the same colours and gradient
    sub = {k: (v if k == "grid" else v[:247].contiguous()) for k, v in a.items()}
    rays = {k: sub[k] for k in ("grid", "rays_o", "rays_d")}
    assert torch.equal(H.field_render(**rays, samples=32, width=19), H.field_render(**rays, samples=32))
    (Lt, gt), (Ll, gl) = H.field_loss_grad(**sub, samples=32, width=19), H.field_loss_grad(**sub, samples=32)
    assert torch.equal(gt, gl) and abs(Lt.item() - Ll.item()) <= 1e-13 * Ll.item()


@pytest.mark.parametrize("op", ["render", "loss_grad"])
def test_field_guarded(H, op):
    """Guards intact, inputs unchanged, two poisoned runs identical (tests/guarded.py)."""
    case, bound = (5, 64, 7), 0.5
    H._FIELD_ACC.clear()                              # the accumulator is allocated inside the arena
    if op == "render":
        C = guarded.run_guarded(lambda: {k: v for k, v in on_dev(case, bound).items() if k != "target"},
                                lambda **a: H.field_render(**a, samples=7, bound=bound))
        compare(C, None, None, case, bound, "guarded render")
    else:
        L, g = guarded.run_guarded(lambda: on_dev(case, bound), lambda **a: H.field_loss_grad(**a, samples=7, bound=bound))
        compare(None, L, g, case, bound, "guarded loss_grad")
    H._FIELD_ACC.clear()


def test_bad_arguments_raise_on_the_gpu(H):
    a = on_dev((5, 64, 7), 1.0)
    big = {k: (v if k == "grid" else v[:1].expand(1024, 3).contiguous()) for k, v in a.items()}
    for kw, s in ((dict(grid=a["grid"].double()), 7), (dict(grid=a["grid"].cpu()), 7), (dict(grid=a["grid"][0]), 7),
                  (dict(grid=a["grid"].transpose(0, 1)), 7), (dict(grid=a["grid"][:1, :1, :1].contiguous()), 7),
                  (dict(rays_d=a["rays_d"][:63]), 7), (dict(target=a["target"].cpu()), 7),
                  (dict(rays_o=a["rays_o"].double()), 7), ({}, 0), (big, 4096)):
        with pytest.raises(ValueError):
            ops.field_loss_grad(**dict(a, **kw), samples=s)
    with pytest.raises(ValueError):
        ops.field_render(a["grid"], a["rays_o"], a["rays_d"][:, :2], samples=7)
    ops.field_render(big["grid"], big["rays_o"], big["rays_d"], samples=4096)          # no gradient: no limit
    L, g = ops.field_loss_grad(**{k: (v if k == "grid" else v[:0]) for k, v in a.items()}, samples=7)
    assert L.item() == 0 and L.dtype == torch.float64 and g.shape == a["grid"].shape and not g.any()
    assert ops.field_render(a["grid"], a["rays_o"][:0], a["rays_d"][:0], samples=7).shape == (0, 3)


def test_field_consistency_end_to_end(H):
    """field_consistency on the HIP backend: procedural ground truth at 32 x 32, 6 + 2 views, a short fit."""
    from distributed_3d_diffusion_pytorch_amd.engine import field_consistency, fit_field
    img, R, t, _ = P.render_views(SEED, [1] * 8, list(range(8)), 32, DEV, 3)
    K = P.srn_intrinsics(DEV).float()
    fit = dict(grid=24, samples=32, iters=40, rays_per_iter=2048, lr=0.3)
    res = field_consistency(img.float(), R.float(), t.float(), K, range(6), [6, 7], **fit)
    _, hist = fit_field(img[:6].float(), R[:6].float(), t[:6].float(), K, **fit)
    print(f"field_psnr {res['field_psnr']:.3f} dB, loss {hist[0].item():.4e} -> {hist[-1].item():.4e}")
    assert hist.is_cuda and hist.shape == (40,) and torch.isfinite(hist).all() and hist[-1] < hist[0]
    assert res["fit_loss"] == hist[-1].item()                                        # a fit is reproducible
    assert math.isfinite(res["field_psnr"]) and 0 < res["field_ssim"] <= 1
    assert (res["n_train"], res["n_test"], len(res["field_psnr_views"])) == (6, 2, 2)
    assert H.FALLBACKS == {}, H.FALLBACKS
