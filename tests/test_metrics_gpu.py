"""csrc/metrics.hip (ops.image_metrics on the GPU) against the test-local
float64 oracle.  Tolerances: fp32 rounding of the two outputs (6e-8 relative)
with margin -- |ssim - ref| <= 2e-6, |mse - ref| <= 1e-6 ref + 1e-12 -- which
fp64 window sums meet and the plain fp32 E[x^2] - mu^2 formula misses by 4e-4
on the flat pair."""
import pytest
import torch

from distributed_3d_diffusion_pytorch_amd import ops
from metrics_oracle import cases, oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"

# 11: one window; 26: exactly one tile; 27: one tile + a one-wide ragged tile both ways
SHAPES = [(11, 11), (12, 12), (26, 26), (27, 27), (27, 43), (64, 64), (128, 128)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_image_metrics_matches_fp64_oracle(H, W):
    assert ops.use_hip(torch.empty(1, device=DEV), any_dtype=True)
    bad = []
    for N in (1, 7):
        for name, (a, b) in cases(N, H, W).items():
            for q in (False, True):
                rm, rs = oracle(a, b, q)
                mse, ssim = ops.image_metrics(a.to(DEV), b.to(DEV), quantize=q)
                assert mse.dtype == torch.float32 and mse.shape == (N,) and ssim.shape == (N,)
                em = (mse.double().cpu() - rm).abs()
                es = (ssim.double().cpu() - rs).abs()
                print(f"{H}x{W} N={N} {name} q={int(q)}: mse rel err {float((em / rm.clamp_min(1e-30)).max()):.2e} "
                      f"ssim err {float(es.max()):.2e}")
                if not ((em <= 1e-6 * rm + 1e-12).all() and (es <= 2e-6).all()):
                    bad.append((N, name, q, float(em.max()), float(es.max())))
    assert not bad, bad


def test_identical_and_psnr():
    x = (torch.rand(3, 3, 40, 33, device=DEV) * 2 - 1)
    mse, ssim = ops.image_metrics(x, x.clone())
    assert (mse == 0).all() and (ssim == 1).all() and torch.isinf(ops.psnr(mse)).all()


def test_deterministic_and_batch_independent():
    """Fixed-order reductions, no atomics: two launches agree bitwise, and
    image i scored alone equals image i scored inside a batch of 7."""
    a, b = cases(7, 64, 64)["srn_like"]
    a, b = a.to(DEV), b.to(DEV)
    b[3] = torch.rand(3, 64, 64, device=DEV) * 2 - 1
    for q in (False, True):
        m0, s0 = ops.image_metrics(a, b, quantize=q)
        m1, s1 = ops.image_metrics(a, b, quantize=q)
        assert torch.equal(m0, m1) and torch.equal(s0, s1)
        for i in (0, 3, 6):
            mi, si = ops.image_metrics(a[i:i + 1], b[i:i + 1], quantize=q)
            assert torch.equal(mi, m0[i:i + 1]) and torch.equal(si, s0[i:i + 1])


def test_non_contiguous_input():
    g = torch.Generator().manual_seed(5)
    a = (torch.rand(2, 5, 27, 43, generator=g) * 2 - 1).to(DEV)
    b = (torch.rand(2, 5, 27, 43, generator=g) * 2 - 1).to(DEV)
    av, bv = a[:, 1:4], b[:, ::2]
    assert not av.is_contiguous() and not bv.is_contiguous()
    m0, s0 = ops.image_metrics(av, bv)
    m1, s1 = ops.image_metrics(av.contiguous(), bv.contiguous())
    assert torch.equal(m0, m1) and torch.equal(s0, s1)
    rm, rs = oracle(av.cpu(), bv.cpu(), True)
    assert ((s0.double().cpu() - rs).abs() <= 2e-6).all()


def test_small_images_rejected():
    with pytest.raises(ValueError):
        ops.image_metrics(torch.zeros(1, 3, 10, 16, device=DEV), torch.zeros(1, 3, 10, 16, device=DEV))
