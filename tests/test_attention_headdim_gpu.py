"""Attention at head dims 32 (head-pair kernels) and 256 (split-D kernels),
attention_hd.hip, against the fp32 torch composition (ops.torch_impl) on the
same bf16-rounded inputs, at the tolerances of the project's other attention
tests (max-abs error over max-abs reference: forward 2e-2, dqkv 4e-2).

Every image carries a boundary pair: query row L-1 and key row L-1 of every
head are the constant 2.0, so that key holds essentially all of query L-1's
softmax (q.k.scale = 4 sqrt(D) >= 22) and out[:, L-1] must equal v[L-1] of the
key image.  A kernel that drops, duplicates or mis-masks the last valid key is
off by O(1) there, where uniform random scores would hide it under 1/L.
GPU only."""
import pytest
import torch

import guarded as G

pytestmark = pytest.mark.gpu

from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
YTOL, GTOL = 2e-2, 4e-2
# D = 32: one pair, odd head count, the model's shape; D = 256
SHAPES = [(64, 2), (96, 3), (256, 8), (256, 1), (512, 2)]
# below one block; ragged and odd; one past a block; the all-keys limit; past it (slabs)
LENGTHS = [16, 49, 65, 256, 320]
_REF = {}


@pytest.fixture(scope="module")
def H():
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    hip_impl._ensure_impl()
    yield hip_impl
    _REF.clear()


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


def make(N, L, C):
    g = torch.Generator(device=DEV).manual_seed(1000 * L + C + N)
    qkv = 0.3 * torch.randn(N, L, 3 * C, device=DEV, generator=g)
    qkv[:, L - 1, :2 * C] = 2.0                       # the boundary pair: q and k of row L-1, every head
    go = torch.randn(N, L, C, device=DEV, generator=g)
    return {"qkv": qkv.to(BF).requires_grad_(True), "go": go}


def reference(N, L, C, heads, cross):
    """(out, dqkv) of the fp32 oracle, computed once per case and shared."""
    key = (N, L, C, heads, cross)
    if key not in _REF:
        inp = make(N, L, C)
        q = inp["qkv"].detach().float().requires_grad_(True)
        y = T.attention(q, heads, cross)
        y.backward(inp["go"])
        _REF[key] = (y.detach(), q.grad)
    return _REF[key]


def check(N, L, C, heads, cross, qkv, y, dqkv):
    yr, gr = reference(N, L, C, heads, cross)
    v_last = qkv.detach()[:, L - 1, 2 * C:].float()
    if cross:
        v_last = v_last.view(N // 2, 2, C).flip(1).reshape(N, C)
    ey, eg, eb = rel(y, yr), rel(dqkv, gr), rel(y[:, L - 1], v_last)
    print(f"C={C} heads={heads} L={L} N={N} cross={cross}: out {ey:.3e} dqkv {eg:.3e} boundary {eb:.3e}")
    assert ey < YTOL and eb < YTOL, (ey, eb)
    assert eg < GTOL, eg


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("N", [2, 4])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("C,heads", SHAPES)
def test_attention_headdim(H, C, heads, L, N, cross):
    inp = make(N, L, C)
    y = H.attention(inp["qkv"], heads, cross)
    y.backward(inp["go"].to(BF))
    assert y.dtype == BF and not H.FALLBACKS, H.FALLBACKS
    check(N, L, C, heads, cross, inp["qkv"], y, inp["qkv"].grad)


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("N", [2, 4])
@pytest.mark.parametrize("L", [49, 320])
@pytest.mark.parametrize("C,heads", SHAPES)
def test_attention_headdim_guarded(H, C, heads, L, N, cross):
    """Nothing outside out, lse, dqkv and the slab workspace is written and no
    uninitialised value is used (guard bands, two poison bytes)."""
    def fn(qkv, go):
        y = H.attention(qkv, heads, cross)
        y.backward(go.to(BF))
        return {"y": y, "dqkv": qkv.grad}
    got = G.run_guarded(lambda: make(N, L, C), fn)
    check(N, L, C, heads, cross, make(N, L, C)["qkv"], got["y"], got["dqkv"])


@pytest.mark.parametrize("heads", [8, 2])
def test_model_attn_heads_matches_fp32_oracle(H, heads):
    """X-UNet with 8 heads (head dims 32 / 64) and 2 heads (128 / 256) on the
    HIP backend against the fp32 oracle models/reference.py: output and every
    parameter gradient by relative L2, each no worse than twice the error of
    the torch backend's bf16 run of the same model, and no fallback."""
    from distributed_3d_diffusion_pytorch_amd import ops
    from distributed_3d_diffusion_pytorch_amd.models import XUNet, reference_forward_grad
    from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches
    torch.manual_seed(21)
    m = XUNet(H=32, W=32, ch=128, attn_heads=heads).to(DEV)
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().sum() == 0:
                p.normal_(0, 0.02)
    m.compute_dtype = BF
    m.eval()
    img, R, t, K = next(SyntheticBatches(2, 32, DEV, seed=4))
    batch = {"x": img[:, 0], "z": img[:, 1], "logsnr": torch.tensor([[20.0, 2.5], [20.0, -4.0]], device=DEV),
             "R": R, "t": t, "K": K}
    mask = torch.tensor([True, False], device=DEV)
    go = torch.randn(2, 3, 32, 32, device=DEV)
    sd = {n: p.detach().clone().float().requires_grad_(True) for n, p in m.named_parameters()}
    ref = reference_forward_grad(sd, batch, mask, attn_heads=heads)
    (ref * go).sum().backward()
    r2 = lambda a, b: ((a.float() - b).norm() / b.norm().clamp_min(1e-12)).item()  # noqa: E731
    res = {}
    for be in ("hip", "torch"):
        ops.set_backend(be)
        try:
            m.zero_grad(set_to_none=True)
            out = m(batch, cond_mask=mask)
            (out.float() * go).sum().backward()
        finally:
            ops.set_backend(None)
        res[be] = {n: r2(p.grad, sd[n].grad) for n, p in m.named_parameters()
                   if p.grad is not None and sd[n].grad.norm() > 0}
        res[be]["<output>"] = r2(out, ref)
    eh, et = res["hip"], res["torch"]
    worst = max(eh, key=lambda n: eh[n] / et[n])
    print(f"heads={heads}: output hip {eh['<output>']:.3e} torch {et['<output>']:.3e}; worst ratio "
          f"{worst} hip {eh[worst]:.3e} torch {et[worst]:.3e}")
    assert H.FALLBACKS == {}, H.FALLBACKS
    assert len(eh) == len(list(m.parameters())) + 1
    bad = {n: (eh[n], et[n]) for n in eh if not eh[n] <= 2 * et[n]}
    assert not bad, bad
