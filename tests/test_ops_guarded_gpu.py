"""Memory behaviour of every HIP op, under the guard-band instrument of
tests/guarded.py: each case runs the op twice inside a poisoned arena (0xFF,
then 0x4B) -- every output and workspace of hip_impl and every test input sits
between guard bands, starts out as poison, and afterwards the guards must be
intact, the inputs bitwise unchanged, the results finite and the two runs
bit-identical -- and then compares the result with the fp32 torch composition
(ops.torch_impl) on the same bf16-rounded inputs, at the tolerances
tests/test_ops_gpu.py uses for that op.  Shapes are the smallest at which each
path still has a tail.  GPU only."""
import ctypes
import math

import pytest
import torch

import guarded as G
from test_ops_gpu import (rel, leaf, CONV_SHAPES, HSM_SHAPES, S64_SHAPES, W8_SHAPES, WGRAD_W8_SHAPES, WG_JOBS,
                          _wg_ref)

pytestmark = pytest.mark.gpu

from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
_REF = {}


@pytest.fixture(scope="module")
def H():
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    hip_impl._ensure_impl()
    yield hip_impl
    _REF.clear()
    hip_impl.invalidate_weight_cache()
    hip_impl._ATTN_PAIRS.clear()             # (pairs registered on arena tensors)
    hip_impl._ATTN_TABLE[:] = [None, -1]


@pytest.fixture
def gn_img(H, request):
    """GroupNorm path of the case: 0 chunked kernels, else the whole-image
    kernels up to that many pixels."""
    prev = H._lib.d3d_gn_img_cfg(-1)
    H._lib.d3d_gn_img_cfg(request.param)
    yield request.param
    H._lib.d3d_gn_img_cfg(prev)


def ref_once(key, compute):
    """A reference is computed once and shared by the cases that need it."""
    if key not in _REF:
        _REF[key] = compute()
    return _REF[key]


def grad(t):
    return t.requires_grad_(True)


def _ref_in(v):
    if not torch.is_tensor(v):
        return v
    r = v.detach().clone()
    if r.dtype == BF:
        r = r.float()
    return r.requires_grad_(True) if v.requires_grad else r


def fwd_bwd(op):
    """fn for run_guarded: y = op(**inputs), backward with the placed ``go``,
    returns the output and the gradient of every differentiable input."""
    def fn(**p):
        go = p.pop("go")
        y = op(**p)
        y.backward(go.to(y.dtype))
        out = {"y": y}
        out.update({"d" + k: v.grad for k, v in p.items() if torch.is_tensor(v) and v.requires_grad})
        return out
    return fn


def guarded_vs_ref(key, make, hip, ref, ytol, gtol, **kw):
    got = G.run_guarded(make, fwd_bwd(hip), **kw)

    def compute():
        r = {k: _ref_in(v) for k, v in make().items()}
        go = r.pop("go")
        y = ref(**r)
        y.backward(go.float())
        out = {"y": y.detach()}
        out.update({"d" + k: v.grad for k, v in r.items() if torch.is_tensor(v) and v.requires_grad})
        return out
    want = ref_once(key, compute)
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in want:
        assert got[k] is not None and got[k].shape == want[k].shape, k
        e = rel(got[k], want[k])
        print(f"{key} {k}: rel {e:.3e}")
        assert e < (ytol if k == "y" else gtol), (k, e)
    return got


def test_instrument_on_device_buffers(H):
    """The arena works on device memory as it does in tests/test_guarded_cpu.py:
    a torch write one element past a guarded device buffer (inside the arena's
    own allocation) and a skipped output element are both reported."""
    import types
    fake = types.ModuleType("fake_dev_impl")
    fake.torch = torch

    def good(x):
        return fake.torch.empty_like(x).copy_(x * 2)

    def past_end(x):
        out = fake.torch.empty_like(x).copy_(x)
        torch.as_strided(out, (1,), (1,), out.storage_offset() + out.numel()).fill_(1.0)
        return out

    def skip_last(x):
        out = fake.torch.empty_like(x)
        out.view(-1)[:-1] = x.reshape(-1)[:-1]
        return out

    def make():
        torch.manual_seed(0)
        return {"x": torch.randn(5, 24, device=DEV).to(BF)}

    assert torch.equal(G.run_guarded(make, good, impl=fake), make()["x"] * 2)
    with pytest.raises(G.GuardError, match=r"back guard, first corrupted byte 0 bytes past"):
        G.run_guarded(make, past_end, impl=fake)
    with pytest.raises(G.GuardError, match=r"not finite \(poison 0xFF\): 1 of 120 elements, first at 119"):
        G.run_guarded(make, skip_last, impl=fake)
    assert fake.torch is torch


# ------------------------------------------------------------------ conv ----
def conv_case(N, Hh, W, Ci, Co, s, res, rb, scale):
    OH, OW = (Hh - 1) // s + 1, (W - 1) // s + 1

    def make():
        torch.manual_seed(3)
        d = {"x": grad(torch.randn(N, Hh, W, Ci, device=DEV).to(BF)),
             "w": grad(torch.randn(Co, Ci, 3, 3, device=DEV) / math.sqrt(9 * Ci)),
             "b": grad(torch.randn(Co, device=DEV) * 0.1)}
        if res:
            d["r"] = grad(torch.randn(N, OH, OW, Co, device=DEV).to(BF))
        if rb:
            d["rb"] = grad(torch.randn(N, Co, device=DEV))
        d["go"] = torch.randn(N, OH, OW, Co, device=DEV).to(BF)
        return d

    def op(M):
        return lambda x, w, b, r=None, rb=None: M.conv3x3(x, w, b, s, r, scale, rb)
    return make, op


def run_conv(H, shape):
    make, op = conv_case(*shape)
    return guarded_vs_ref(("conv",) + tuple(shape), make, op(H), op(T), 2e-2, 3e-2)


LADDER_SHAPES = [CONV_SHAPES[8]] + CONV_SHAPES[4:8] + [CONV_SHAPES[9], CONV_SHAPES[10], CONV_SHAPES[0]]
assert LADDER_SHAPES[0][:5] == (2, 12, 20, 384, 128) and [s[5] for s in LADDER_SHAPES[1:5]] == [1, 2, 4, 8]
assert all(s[3] == 144 and s[7] for s in LADDER_SHAPES[1:5]) and LADDER_SHAPES[7][:5] == (4, 16, 16, 128, 128)


@pytest.mark.parametrize("impl", ["halo", "bufl", "w8", "w8w", "w8n"])
@pytest.mark.parametrize("shape", LADDER_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:6]))
def test_conv3x3_ladder(H, impl, shape):
    """Forward, dx, dw, db, residual and row-bias gradients under every
    forward ceiling of _CONV_IMPLS ("halo" is the default ladder; a shape the
    ceiling's kernel does not take falls down the ladder)."""
    assert set(H._CONV_IMPLS) == {"bufl", "w8", "w8w", "w8n", "halo"}
    try:
        H.set_conv_impl(impl)
        run_conv(H, shape)
    finally:
        H.set_conv_impl("halo")


@pytest.mark.parametrize("impl", ["w8", "w8w", "w8n", "halo"])
@pytest.mark.parametrize("shape", [W8_SHAPES[2], W8_SHAPES[3]], ids=["partial-pixel-tile", "bm256-overhang"])
def test_conv3x3_eight_wave_and_halo(H, impl, shape):
    assert shape[:5] in ((300, 12, 20, 128, 384), (16, 64, 64, 64, 640))
    H.set_conv_impl(impl)
    try:
        run_conv(H, shape)
    finally:
        H.set_conv_impl("halo")


@pytest.mark.parametrize("cfg", [1, 2, 3, 4])
def test_conv3x3_small_tiles(H, cfg):
    assert S64_SHAPES[5][:5] == (20, 8, 8, 256, 512)
    H._lib.d3d_conv_s64_cfg(cfg)
    try:
        run_conv(H, S64_SHAPES[5])
    finally:
        H._lib.d3d_conv_s64_cfg(0)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4])
def test_conv3x3_small_halo(H, cfg):
    assert HSM_SHAPES[4][:5] == (32, 16, 16, 96, 128)           # IC < ICp
    H._lib.d3d_conv_hsm_cfg(cfg)
    try:
        run_conv(H, HSM_SHAPES[4])
    finally:
        H._lib.d3d_conv_hsm_cfg(1)


@pytest.mark.parametrize("impl", ["reg", "bufl", "w8"])
@pytest.mark.parametrize("shape", [WGRAD_W8_SHAPES[1], WGRAD_W8_SHAPES[2], CONV_SHAPES[5]],
                         ids=["partial-last-split", "ic-overhang", "stride2-144"])
def test_conv3x3_weight_gradient(H, impl, shape):
    assert shape[:6] in ((3, 16, 16, 128, 256, 1), (4, 16, 16, 384, 128, 1), (2, 16, 16, 144, 256, 2))
    H.set_wgrad_impl(impl)
    try:
        run_conv(H, shape)
    finally:
        H.set_wgrad_impl("w8")


@pytest.mark.parametrize("gn_img", [0], indirect=True)
def test_conv3x3_gn_epilogue_partials(H, gn_img):
    """The conv epilogue's GroupNorm partials (a torch.empty workspace the
    consuming GroupNorm reads whole) on (4,16,16,128,128)."""
    shape = CONV_SHAPES[0]
    make0, _ = conv_case(*shape)

    def make():
        d = make0()
        d.pop("go")
        torch.manual_seed(13)
        d["gam"] = torch.rand(128, device=DEV) + 0.5
        d["bet"] = torch.randn(128, device=DEV) * 0.1
        return {k: v.detach() for k, v in d.items()}

    def fn(x, w, b, r, gam, bet):
        y = H.conv3x3(x, w, b, 1, r, shape[8], gn_groups=32)
        assert hasattr(y, "_d3d_gnpart"), "fused GroupNorm partials not produced"
        return {"y": y, "part": y._d3d_gnpart[0], "h": H.group_norm(y, gam, bet, 32, 1e-5, True)}

    got = G.run_guarded(make, fn)
    r = {k: _ref_in(v) for k, v in make().items()}
    yr = T.conv3x3(r["x"], r["w"], r["b"], 1, r["r"], shape[8])
    assert rel(got["y"], yr) < 2e-2
    assert rel(got["h"], T.group_norm(yr, r["gam"], r["bet"], 32, 1e-5, True)) < 2e-2


# ------------------------------------------------------------- GroupNorm ----
GN_CASES = [(3, 8, 8, 384, 32, True, (0, 256)), (2, 4, 4, 1024, 32, False, (0, 256)),
            (2, 16, 16, 128, 1, True, (0, 256)), (2, 16, 16, 256, 64, True, (0, 256)),
            (3, 32, 32, 256, 32, True, (0, 1024))]
GN_PARAMS = [pytest.param(c[:6], m, id=f"{'x'.join(map(str, c[:5]))}-img{m}") for c in GN_CASES for m in c[6]]


def _gn_make(N, Hh, W, C, with_ss=False, seed=0):
    def make():
        torch.manual_seed(seed)
        d = {"x": grad((torch.randn(N, Hh, W, C, device=DEV) * 2 + 0.5).to(BF)),
             "w": grad(torch.randn(C, device=DEV) * 0.5 + 1), "b": grad(torch.randn(C, device=DEV) * 0.1)}
        if with_ss:
            d["ss"] = grad((torch.randn(N, Hh, W, 2 * C, device=DEV) * 0.5).to(BF))
        d["go"] = torch.randn(N, Hh, W, C, device=DEV).to(BF)
        return d
    return make


@pytest.mark.parametrize("case,gn_img", GN_PARAMS, indirect=["gn_img"])
def test_group_norm(H, case, gn_img):
    N, Hh, W, C, Gr, silu = case
    # the whole-image kernels take groups of whole 8-channel vectors (norm.hip img_plan); 12-channel groups
    # (C = 384) and 4-channel ones (G = 64) run the chunked kernels at either setting
    assert H.gn_img_ok(Hh * W, C, Gr, N) == bool(gn_img and (C // Gr) % 8 == 0)
    got = G.run_guarded(_gn_make(N, Hh, W, C), fwd_bwd(lambda x, w, b: H.group_norm(x, w, b, Gr, 1e-5, silu)))

    def compute():
        r = {k: _ref_in(v) for k, v in _gn_make(N, Hh, W, C)().items()}
        y = T.group_norm(r["x"], r["w"], r["b"], Gr, 1e-5, silu)
        y.backward(r["go"])
        return y.detach(), r["x"].grad, r["w"].grad, r["b"].grad
    yr, dx, dw, db = ref_once(("gn",) + tuple(case), compute)
    assert rel(got["y"], yr) < 2e-2
    assert rel(got["dx"], dx) < 3e-2
    assert rel(got["dw"], dw) < 1e-2
    assert rel(got["db"], db) < 1e-2


@pytest.mark.parametrize("shape,gn_img", [((2, 16, 16, 256), 0), ((2, 16, 16, 256), 256), ((3, 32, 32, 256), 0),
                                          ((3, 32, 32, 256), 1024)], indirect=["gn_img"])
def test_gn_film_dropout(H, shape, gn_img):
    """GN-FiLM with dropout 0.1 against the fp32 composition under the
    kernel's own mask (the convention of test_gn_whole_image)."""
    N, Hh, W, C = shape
    p, seed = 0.1, 77
    assert H.gn_img_ok(Hh * W, C, 32, N) == bool(gn_img)
    make = _gn_make(N, Hh, W, C, True, seed=31)
    got = G.run_guarded(make, fwd_bwd(lambda x, w, b, ss: H.gn_film(x, w, b, ss, 32, 1e-5, p, True, seed)))
    r = {k: _ref_in(v) for k, v in make().items()}
    src = make()
    keep = (H.gn_film(src["x"].detach(), torch.ones(C, device=DEV), torch.zeros(C, device=DEV),
                      torch.zeros_like(src["ss"]).detach(), 32, 1e-5, p, True, seed) != 0).float()
    assert 0.05 < 1 - keep.mean().item() < 0.15
    yr = T.gn_film(r["x"], r["w"], r["b"], r["ss"], 32, 1e-5, 0.0, False, 0) * keep / (1 - p)
    yr.backward(r["go"])
    assert rel(got["y"], yr) < 2e-2
    for k in ("x", "w", "b", "ss"):
        assert rel(got["d" + k], r[k].grad) < 3e-2, k


@pytest.mark.parametrize("gn_img", [0, 256], indirect=True)
def test_gn_film_ss_map_strided(H, gn_img):
    """Shared-conditioning GN-FiLM reading a channel slice (ld = 6C) of a
    level-batched modulation through ss_map."""
    N, Hh, C = 6, 8, 256

    def make():
        torch.manual_seed(4)
        return {"x": torch.randn(N, Hh, Hh, C, device=DEV).to(BF), "w": torch.randn(C, device=DEV) * 0.5 + 1,
                "b": torch.randn(C, device=DEV) * 0.1,
                "parent": (torch.randn(4, Hh, Hh, 3 * 2 * C, device=DEV) * 0.5).to(BF),
                "smap": torch.tensor([0, 1, 2, 3, 0, 3], dtype=torch.int32, device=DEV)}

    def fn(x, w, b, parent, smap):
        with torch.no_grad():
            return H.gn_film(x, w, b, parent[..., 2 * C:4 * C], 32, 1e-5, 0.0, False, 0, smap)

    y = G.run_guarded(make, fn)
    s = make()
    yr = T.gn_film(s["x"].float(), s["w"], s["b"], s["parent"][..., 2 * C:4 * C].float()[s["smap"].long()], 32, 1e-5,
                   0.0, False, 0)
    assert rel(y, yr) < 1e-2


@pytest.mark.parametrize("gn_img", [0, 256], indirect=True)
def test_cat_gn_silu_dense(H, gn_img):
    C1, C2, OC, N, Hh = 512, 256, 256, 4, 8

    def make():
        torch.manual_seed(11)
        return {"a": grad((torch.randn(N, Hh, Hh, C1, device=DEV) + 0.3).to(BF)),
                "b": grad((torch.randn(N, Hh, Hh, C2, device=DEV) * 2).to(BF)),
                "gw": grad(torch.rand(C1 + C2, device=DEV) + 0.5), "gb": grad(torch.randn(C1 + C2, device=DEV) * 0.1),
                "dw": grad(torch.randn(OC, C1 + C2, 1, 1, device=DEV) / 20), "db": grad(torch.randn(OC, device=DEV) * 0.1),
                "gy": torch.randn(N, Hh, Hh, C1 + C2, device=DEV).to(BF),
                "gs": torch.randn(N, Hh, Hh, OC, device=DEV).to(BF)}

    def run(M):
        def fn(gy, gs, **p):
            y, s = M.cat_gn_silu_dense(*p.values(), 32, 1e-5)
            ((y.float() * gy.float()).sum() + (s.float() * gs.float()).sum()).backward()
            return [y, s] + [t.grad for t in p.values()]
        return fn

    got = G.run_guarded(make, run(H))
    want = ref_once("cat_gn", lambda: run(T)(**{k: _ref_in(v) for k, v in make().items()}))
    for n, x, r in zip(["y", "skip", "da", "db", "dgw", "dgb", "ddw", "ddb"], got, want):
        assert rel(x, r) < 3e-2, (n, rel(x, r))


def test_gn_silu_conv_fused(H, monkeypatch):
    N, Hh, C, OC = 32, 32, 128, 256
    monkeypatch.setattr(H, "_GN_CONV", True)

    def make():
        torch.manual_seed(11)
        return {"x": grad((torch.randn(N, Hh, Hh, C, device=DEV) * 1.5 + 0.3).to(BF)),
                "gw": grad(torch.rand(C, device=DEV) + 0.5), "gb": grad(torch.randn(C, device=DEV) * 0.2),
                "cw": grad(torch.randn(OC, C, 3, 3, device=DEV) / (3 * C ** 0.5)),
                "cb": grad(torch.randn(OC, device=DEV) * 0.1), "go": torch.randn(N, Hh, Hh, OC, device=DEV).to(BF)}

    def hip(x, gw, gb, cw, cb):
        assert H.gn_silu_conv_ok(x, OC, 32)
        return H.gn_silu_conv3x3(x, gw, gb, cw, cb, 32, 1e-5, gn1_groups=32)

    guarded_vs_ref("gn_conv", make, hip,
                   lambda x, gw, gb, cw, cb: T.conv3x3(T.group_norm(x, gw, gb, 32, 1e-5, silu=True), cw, cb), 2e-2, 4e-2)


# ------------------------------------------------------------- attention ----
def _attn_make(N, L, C):
    def make():
        torch.manual_seed(5)
        return {"qkv": grad(torch.randn(N, L, 3 * C, device=DEV).to(BF)),
                "go": torch.randn(N, L, C, device=DEV).to(BF)}
    return make


def _attention(H, N, L, C, cross):
    try:
        for cfg in (0, 1 << 30):          # one-workgroup-per-head kernels forced / the 64-row workgroups + fp32 slabs
            H._lib.d3d_attn_fwd_cfg(cfg)
            H._lib.d3d_attn_bwd_cfg(cfg)
            guarded_vs_ref(("attn", N, L, C, cross), _attn_make(N, L, C), lambda qkv: H.attention(qkv, 4, cross),
                           lambda qkv: T.attention(qkv, 4, cross), 2e-2, 4e-2)
    finally:
        H._lib.d3d_attn_fwd_cfg(512)
        H._lib.d3d_attn_bwd_cfg(0)


@pytest.mark.parametrize("C", [256, 512])
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("N", [2, 4])
@pytest.mark.parametrize("L", [16, 49, 65, 100, 196])
def test_attention(H, L, N, cross, C):
    _attention(H, N, L, C, cross)


def test_attention_long(H):
    _attention(H, 2, 1024, 256, True)


# ------------------------------------------------------------ GEMM users ----
def _pad_is_poison(H, pad):
    torch.cuda.synchronize()
    assert bool((G._bits(pad) == H.torch._arena.byte).all()), "columns past M written"


@pytest.mark.parametrize("cfg", [8, 4, 2])
def test_gemm_nt_padded_rows(H, cfg):
    """M / N tails with row strides wider than K and M: the pad columns of a,
    b and res hold NaN (never to be used), those of out stay untouched."""
    M, N, K, lda, ldb, ldo = 200, 1000, 192, 200, 256, 208
    nan = float("nan")

    def make():
        torch.manual_seed(11)
        a = torch.randn(M, lda, device=DEV)
        b = torch.randn(N, ldb, device=DEV)
        r = torch.randn(N, ldo, device=DEV)
        a[:, K:], b[:, K:], r[:, M:] = nan, nan, nan
        return {"a": a.to(BF), "b": b.to(BF), "bias": torch.randn(M, device=DEV), "r": r.to(BF)}

    def fn(a, b, bias, r):
        out = H.torch.empty(N, ldo, dtype=BF, device=DEV)
        H.gemm_nt(a, b, out, M, N, K, lda, ldb, ldo, bias=bias, res=r, alpha=0.5, scale=0.7)
        _pad_is_poison(H, out[:, M:])
        return out[:, :M]

    H._lib.d3d_gemm_tune(cfg, 0, 0)
    try:
        out = G.run_guarded(make, fn)
    finally:
        H._lib.d3d_gemm_tune(1, 0, 0)

    def compute():
        s = make()
        ref = (s["a"][:, :K].float() @ s["b"][:, :K].float().t() * 0.5).t()
        return (ref + s["bias"] + s["r"][:, :M].float()) * 0.7
    assert rel(out, ref_once("gemm_nt", compute)) < 1e-2


@pytest.mark.parametrize("cfg", [8, 4, 2])
def test_gemm_dsilu_and_in_place_residual(H, cfg):
    M, N, K = 200, 1000, 192

    def make():
        torch.manual_seed(3)
        return {"a": torch.randn(M, K, device=DEV).to(BF), "b": torch.randn(N, K, device=DEV).to(BF),
                "e": (torch.randn(N, M, device=DEV) * 3).to(BF), "acc": torch.randn(N, M, device=DEV).to(BF)}

    def fn(a, b, e, acc):
        out = H.torch.empty(N, M, dtype=BF, device=DEV)
        H.gemm_nt(a, b, out, M, N, K, K, K, M, dsilu_of=e, ldr=M, alpha=0.5)
        H.gemm_nt(a, b, acc, M, N, K, K, K, M, res=acc)             # accumulate in place
        return out, acc

    H._lib.d3d_gemm_tune(cfg, 0, 0)
    try:
        out, acc = G.run_guarded(make, fn, mutated=("acc",))
    finally:
        H._lib.d3d_gemm_tune(1, 0, 0)
    s = make()
    prod = s["b"].float() @ s["a"].float().t()
    sg = torch.sigmoid(s["e"].float())
    assert rel(out, 0.5 * prod * sg * (1 + s["e"].float() * (1 - sg))) < 1e-2
    assert rel(acc, s["acc"].float() + prod) < 1e-2


@pytest.mark.parametrize("P,IC,OC", [(128, 256, 768), (4096, 384, 128)])
def test_linear(H, P, IC, OC):
    def make():
        torch.manual_seed(4)
        return {"x": grad(torch.randn(2, P // 2, IC, device=DEV).to(BF)),
                "w": grad(torch.randn(OC, IC, device=DEV) / math.sqrt(IC)), "b": grad(torch.randn(OC, device=DEV) * 0.1),
                "r": grad(torch.randn(2, P // 2, OC, device=DEV).to(BF)),
                "go": torch.randn(2, P // 2, OC, device=DEV).to(BF)}
    nfb = len(H.FALLBACKS)
    guarded_vs_ref(("linear", P, IC, OC), make, lambda x, w, b, r: H.linear(x, w, b, r, 0.7),
                   lambda x, w, b, r: T.linear(x, w, b, r, 0.7), 2e-2, 3e-2)
    assert len(H.FALLBACKS) == nfb, H.FALLBACKS


@pytest.mark.parametrize("gn_img", [0], indirect=True)
def test_linear_gn_partials(H, gn_img):
    N, L, C = 2, 64, 128
    sc = 1 / math.sqrt(2)

    def make():
        torch.manual_seed(17)
        return {"x": torch.randn(N, L, C, device=DEV).to(BF), "w": torch.randn(C, C, device=DEV) / math.sqrt(C),
                "b": torch.randn(C, device=DEV) * 0.2, "r": torch.randn(N, L, C, device=DEV).to(BF)}

    def fn(x, w, b, r):
        y = H.linear(x, w, b, r, sc, gn_groups=32)
        assert hasattr(y, "_d3d_gnpart")
        return y, y._d3d_gnpart[0]

    y, part = G.run_guarded(make, fn)
    s = make()
    assert rel(y, T.linear(s["x"].float(), s["w"], s["b"], s["r"].float(), sc)) < 2e-2
    # the partials are the sums / sums of squares of the WRITTEN output (test_gemm_gn_partials' layout and bound)
    v = y.float().view(N, L // 64, 64, 32, C // 32)
    got = part.view(N, 32, L // 64, 2)
    assert rel(got[..., 0], v.sum((2, 4)).permute(0, 2, 1)) < 1e-4
    assert rel(got[..., 1], (v * v).sum((2, 4)).permute(0, 2, 1)) < 1e-4


@pytest.mark.parametrize("split", [False, True])
def test_attn_out(H, split, monkeypatch):
    N, L, C = 3, 100, 256
    monkeypatch.setattr(H, "_ATTN_SPLIT", 0 if split else 1 << 30)
    monkeypatch.setattr(H, "_ATTN_SMALL", True)
    s = 1 / math.sqrt(2)

    def make():
        torch.manual_seed(23)
        return {"a": grad(torch.randn(N, L, C, device=DEV).to(BF)), "x": grad(torch.randn(N, L, C, device=DEV).to(BF)),
                "Wo": grad(torch.randn(C, C, device=DEV) / math.sqrt(C)), "bo": grad(torch.randn(C, device=DEV) * 0.1),
                "Wl": grad(torch.randn(C, C, 1, 1, device=DEV) / math.sqrt(C)),
                "bl": grad(torch.randn(C, device=DEV) * 0.1), "go": torch.randn(N, L, C, device=DEV).to(BF)}

    guarded_vs_ref("attn_out", make,
                   lambda a, x, Wo, bo, Wl, bl: H.attn_out(a, Wo, bo, Wl, bl, residual=x, out_scale=s),
                   lambda a, x, Wo, bo, Wl, bl: T.linear(T.linear(a, Wo, bo), Wl, bl, x, s), 2e-2, 3e-2)


@pytest.mark.parametrize("mode", ["tn", "blas", "seg"])
def test_film_batch(H, mode):
    chans, N, Hh, K = [128, 128, 256], 4, 8, 1024
    nb = len(chans)

    def make():
        torch.manual_seed(0)
        d = {"semb": grad((torch.randn(N, Hh, Hh, K, device=DEV) * 2).to(BF))}
        for i, c in enumerate(chans):
            d[f"W{i}"] = grad(torch.randn(2 * c, K, device=DEV) / 32)
            d[f"B{i}"] = grad(torch.randn(2 * c, device=DEV) * 0.1)
            d[f"x{i}"] = torch.randn(N, Hh, Hh, c, device=DEV).to(BF)
            d[f"g{i}"] = torch.rand(c, device=DEV) + 0.5
            d[f"b{i}"] = torch.randn(c, device=DEV) * 0.1
            d[f"go{i}"] = torch.randn(N, Hh, Hh, c, device=DEV).to(BF)
        return d

    def run(M):
        def fn(**p):
            ws, bs = [p[f"W{i}"] for i in range(nb)], [p[f"B{i}"] for i in range(nb)]
            if M is H:
                sss = H.film_batch(p["semb"], ws, bs)
            else:
                sss = [T.linear(torch.nn.functional.silu(p["semb"]), w, b) for w, b in zip(ws, bs)]
            loss = 0
            for i, ss in enumerate(sss):
                y = M.gn_film(p[f"x{i}"], p[f"g{i}"], p[f"b{i}"], ss, 32, 1e-5, 0.0, False, 0)
                loss = loss + (y.float() * p[f"go{i}"].float()).sum()
            loss.backward()
            return [p["semb"].grad] + [w.grad for w in ws] + [b.grad for b in bs]
        return fn

    prev = H._FILM_WGRAD
    H._FILM_WGRAD = mode
    try:
        got = G.run_guarded(make, run(H))
    finally:
        H._FILM_WGRAD = prev
    want = ref_once("film", lambda: run(T)(**{k: _ref_in(v) for k, v in make().items()}))
    for a, b in zip(got, want):
        assert rel(a, b) < 3e-2, rel(a, b)


@pytest.mark.parametrize("with_bias", [True, False])
def test_cat_gemm(H, with_bias):
    C, OC, N, Hh = 128, 128, 3, 10
    P = N * Hh * Hh

    def make():
        torch.manual_seed(5)
        d = {"a": torch.randn(P, C, device=DEV).to(BF), "b": (torch.randn(P, C, device=DEV) * 2).to(BF),
             "w": (torch.randn(OC, 2 * C, device=DEV) / 20).to(BF)}
        if with_bias:
            d["db"] = torch.randn(OC, device=DEV) * 0.1
        return d

    def fn(a, b, w, db=None):
        one = H.torch.empty(P, OC, dtype=BF, device=DEV)
        rc = H._lib.d3d_gemm_cat(w.data_ptr(), a.data_ptr(), b.data_ptr(), C, one.data_ptr(), H._ptr(db), OC, P,
                                 2 * C, 2 * C, OC, 1.0, 1.0, H._st())
        assert rc == 0, rc
        return one

    one = G.run_guarded(make, fn)
    s = make()
    ref = torch.cat([s["a"], s["b"]], -1).float() @ s["w"].float().t()
    assert rel(one, ref + s["db"] if with_bias else ref) < 1e-2


# --------------------------------------------- reductions, small kernels ----
@pytest.mark.parametrize("P,M,N,ldy,splits", [(128, 256, 256, 384, 1), (256, 200, 136, 384, 1)])
def test_wgrad_tn(H, P, M, N, ldy, splits):
    """ldy > M: a column slice of a wider dy whose other columns hold NaN."""
    def make():
        torch.manual_seed(3)
        dyw = torch.randn(P, ldy, device=DEV)
        dyw[:, M:] = float("nan")
        return {"dyw": dyw.to(BF), "x": torch.randn(P, N, device=DEV).to(BF)}

    def fn(dyw, x):
        ws, bws, used = H.wgrad_tn(dyw[:, :M], x, splits)
        assert used >= 1 and ws.shape == (used, M, N)
        return ws, bws

    ws, bws = G.run_guarded(make, fn)
    s = make()
    dy = s["dyw"][:, :M].float()
    assert rel(ws.sum(0), dy.t() @ s["x"].float()) < 1e-4
    rb = dy.sum(0)
    assert (bws.sum(0) - rb).abs().max().item() <= 1e-3 * rb.abs().max().item() + 1e-3


WG_PICK = [3, 4, 5, 6, 7, 8, 9]     # per-tap unsplit, channel tails, 1x1, 1x1 concat, split-K, halo concat, halo small


def test_wgrad_group_run(H):
    """One job of each kind of test_wgrad_group_matches_fp32 in one grouped
    launch (library default plan), accumulated onto existing gradients."""
    jobs_ = [WG_JOBS[i] for i in WG_PICK]

    def make():
        torch.manual_seed(5)
        d = {}
        for i, (N, Hh, W, IC, OC, taps, C1, bias) in enumerate(jobs_):
            d[f"g{i}"] = torch.randn(N, Hh, W, OC, device=DEV).to(BF)
            x = torch.randn(N, Hh, W, IC, device=DEV).to(BF)
            if C1:
                d[f"xa{i}"], d[f"xb{i}"] = x[..., :C1].contiguous(), x[..., C1:].contiguous()
            else:
                d[f"xa{i}"] = x
            d[f"dw{i}"] = torch.randn(OC, IC, taps, device=DEV)
            if bias:
                d[f"db{i}"] = torch.randn(OC, device=DEV)
        return d

    def fn(**p):
        jobs = []
        for i, (N, Hh, W, IC, OC, taps, C1, bias) in enumerate(jobs_):
            kw = dict(x2=p[f"xb{i}"], C1=C1) if C1 else {}
            j = H.wgrad_job(p[f"g{i}"], p[f"xa{i}"], OC, IC, N, Hh, W, taps, p[f"dw{i}"], p.get(f"db{i}"), 0.7, **kw)
            assert j is not None, jobs_[i]
            jobs.append(j)
        H.wgrad_group_run(jobs)
        torch.cuda.synchronize()
        return {k: v for k, v in p.items() if k[:2] in ("dw", "db")}

    names = [k for k in make() if k[:2] in ("dw", "db")]
    got = G.run_guarded(make, fn, mutated=names)
    s = make()
    for i, (N, Hh, W, IC, OC, taps, C1, bias) in enumerate(jobs_):
        x = torch.cat([s[f"xa{i}"], s[f"xb{i}"]], -1) if C1 else s[f"xa{i}"]
        assert rel(got[f"dw{i}"], s[f"dw{i}"] + 0.7 * _wg_ref(s[f"g{i}"], x, taps)) < 1e-4, jobs_[i]
        if bias:
            assert rel(got[f"db{i}"], s[f"db{i}"] + 0.7 * s[f"g{i}"].reshape(-1, OC).float().sum(0)) < 1e-4, jobs_[i]


def test_colsum_group_run(H):
    """A 32-row job, a 256-row job and an accumulating job (the kinds of
    test_colsum_jobs_batched) in one launch."""
    kinds = [(32, 256, 0), (256, 128, 0), (256, 256, 1)]

    def make():
        torch.manual_seed(7)
        d = {}
        for i, (R, C, acc) in enumerate(kinds):
            d[f"x{i}"] = torch.randn(R, 2 * C, device=DEV)
            d[f"p{i}"] = torch.randn(C, device=DEV)
            d[f"q{i}"] = torch.randn(C, device=DEV)
        return d

    def fn(**p):
        specs = [H._ColJob(p[f"x{i}"].data_ptr(), p[f"p{i}"].data_ptr(), p[f"q{i}"].data_ptr(), R, 2 * C, acc, 0)
                 for i, (R, C, acc) in enumerate(kinds)]
        H.colsum_group_run(specs)
        torch.cuda.synchronize()
        return {k: v for k, v in p.items() if k[0] in "pq"}

    outs = [k for k in make() if k[0] in "pq"]
    got = G.run_guarded(make, fn, mutated=outs)
    s = make()
    for i, (R, C, acc) in enumerate(kinds):
        for k, off in (("p", 0), ("q", 1)):
            ref = s[f"x{i}"][:, off::2].sum(0) + (s[f"{k}{i}"] if acc else 0)
            assert torch.allclose(got[f"{k}{i}"], ref, rtol=1e-5, atol=1e-4), (i, k)


@pytest.mark.parametrize("per_image", [True, False])
def test_chansum(H, per_image):
    """Channel sums of a bf16 gradient (the conv's bias / row-bias gradients;
    their bound in test_conv3x3)."""
    def make():
        torch.manual_seed(2)
        return {"g": torch.randn(3, 6, 10, 128, device=DEV).to(BF)}

    def fn(g):
        per, tot = H._chansum(g, per_image)
        return {"tot": tot, **({"per": per} if per_image else {})}

    got = G.run_guarded(make, fn)
    g = make()["g"].float()
    assert rel(got["tot"], g.sum((0, 1, 2))) < 3e-2
    if per_image:
        assert rel(got["per"], g.sum((1, 2))) < 3e-2


@pytest.mark.parametrize("N,period", [(5, 1), (6, 2)])
def test_period_sum(H, N, period):
    def make():
        torch.manual_seed(2)
        return {"g": torch.randn(N, 8, 8, 40, device=DEV).to(BF)}
    out = G.run_guarded(make, lambda g: H._period_sum(g, period))
    ref = make()["g"].float().reshape(N // period, period, 8, 8, 40).sum(0)
    assert out.shape == (period, 8, 8, 40) and out.dtype == BF
    assert (out.float() - ref).abs().max().item() <= 0.01 * ref.abs().max().item() + 1e-2


def test_logsnr_mlp(H):
    R, E = 200, 1024

    def make():
        torch.manual_seed(0)
        return {"logsnr": torch.rand(R // 2, 2, device=DEV) * 50 - 25, "w1": grad(torch.randn(E, E, device=DEV) / 32),
                "b1": grad(torch.randn(E, device=DEV) * 0.1), "w2": grad(torch.randn(E, E, device=DEV) / 32),
                "b2": grad(torch.randn(E, device=DEV) * 0.1), "go": torch.randn(R, E, device=DEV)}
    guarded_vs_ref("mlp", make, H.logsnr_mlp, T.logsnr_mlp, 1e-2, 1e-2)
    assert H.FALLBACKS.get(f"logsnr_mlp: E={E}") is None


@pytest.mark.parametrize("name", ["silu", "avgpool2", "upsample2"])
def test_elementwise(H, name):
    oshape = {"silu": (2, 6, 10, 128), "avgpool2": (2, 3, 5, 128), "upsample2": (2, 12, 20, 128)}[name]

    def make():
        torch.manual_seed(7)
        return {"x": grad(torch.randn(2, 6, 10, 128, device=DEV).to(BF)), "go": torch.randn(*oshape, device=DEV).to(BF)}
    guarded_vs_ref(name, make, getattr(H, name), getattr(T, name), 1e-2, 1e-2)


def test_ray_posenc(H):
    from distributed_3d_diffusion_pytorch_amd.data.synthetic import random_orbit_poses
    B, Hh, W = 3, 16, 16

    def make():
        g = torch.Generator(device=DEV)
        g.manual_seed(0)
        torch.manual_seed(0)
        R, t = random_orbit_poses(2 * B, g, DEV)
        K = torch.tensor([[131.25, 0, 64.0], [0, 131.25, 64.0], [0, 0, 1]], dtype=torch.float64, device=DEV)
        return {"R": R.reshape(B, 2, 3, 3).contiguous(), "t": t.reshape(B, 2, 3).contiguous(),
                "K": K.expand(B, 3, 3).contiguous(), "mask": torch.tensor([True, False, True], device=DEV),
                "pe": grad(torch.randn(144, Hh, W, device=DEV) * 0.1),
                "fe": grad(torch.randn(1, 1, 144, 1, 1, device=DEV) * 0.1),
                "oe": grad(torch.randn(1, 1, 144, 1, 1, device=DEV) * 0.1),
                "go": torch.randn(2 * B, Hh, W, 144, device=DEV).to(BF)}

    got = G.run_guarded(make, fwd_bwd(lambda R, t, K, mask, pe, fe, oe: H.ray_posenc(R, t, K, Hh, W, mask, pe, fe, oe)))
    r = {k: _ref_in(v) for k, v in make().items()}
    yr = T.ray_posenc(r["R"], r["t"], r["K"], Hh, W, r["mask"], r["pe"], r["fe"], r["oe"])
    yr.backward(r["go"])
    assert (got["y"].float() - yr).abs().max().item() < 2e-2
    for k in ("pe", "fe", "oe"):
        assert rel(got["d" + k], r[k].grad) < 1e-2, k


@pytest.mark.parametrize("rescale", [0, 128])
def test_ray_conditioning(H, rescale):
    B, Hh, W = 5, 32, 32

    def make():
        torch.manual_seed(3)
        R = torch.linalg.qr(torch.randn(B, 2, 3, 3, device=DEV))[0].contiguous()
        K = torch.tensor([[60.0, 0.0, 16.0], [0.0, 58.0, 15.5], [0.0, 0.0, 1.0]], device=DEV).repeat(B, 1, 1)
        t = torch.randn(B, 2, 3, device=DEV) * 2
        K[:, 0, 0] += torch.rand(B, device=DEV) * 5
        return {"R": R, "t": t, "K": K, "mask": torch.tensor([True, False, True, True, False], device=DEV)}

    dh, oh = G.run_guarded(make, lambda R, t, K, mask: H.ray_conditioning(R, t, K, Hh, W, mask, rescale))
    s = make()
    dr = T.ray_posenc_dir(s["R"], s["t"], s["K"], Hh, W, s["mask"], rescale)
    orr = T.ray_origin_pe(s["t"], s["mask"])
    assert oh.shape == orr.shape == (2 * B, 93) and (oh - orr).abs().max().item() < 1e-5
    assert dh.shape == dr.shape == (2 * B, Hh, W, 64) and rel(dh, dr) < 1e-2
    assert dh[..., 51:].abs().max().item() == 0.0


@pytest.mark.parametrize("s", [1, 8])
def test_cond_conv(H, s):
    N, Hh, OC, no = 4, 16, 256, 93
    OHs = (Hh - 1) // s + 1

    def make():
        torch.manual_seed(7)
        rays = torch.zeros(N, Hh, Hh, 64, device=DEV)
        rays[..., :51] = torch.randn(N, Hh, Hh, 51, device=DEV)
        return {"rays": rays.to(BF), "orig": torch.randn(N, no, device=DEV),
                "w": grad(torch.randn(OC, 144, 3, 3, device=DEV) / 36), "b": grad(torch.randn(OC, device=DEV) * 0.1),
                "rb": grad(torch.randn(N, OC, device=DEV)), "r": grad(torch.randn(2, OHs, OHs, OC, device=DEV).to(BF)),
                "go": torch.randn(N, OHs, OHs, OC, device=DEV).to(BF)}

    guarded_vs_ref(("cond_conv", s), make, lambda rays, orig, w, b, rb, r: H.cond_conv(rays, orig, w, b, s, rb, r, 2),
                   lambda rays, orig, w, b, rb, r: T.cond_conv(rays, orig, w, b, s, rb, r, 2), 2e-2, 3e-2)


@pytest.mark.parametrize("OC,IC", [(3, 128), (1024, 144)])
def test_weight_packers(H, OC, IC):
    """pack_w_k and the batched refresh (pack_all_k) write whole operands,
    their own zero padding included: [OCp][9][ICp] and [ICp][9][OCp] bf16."""
    def ref_packs(w):
        v = w.reshape(OC, IC, 9)
        f = torch.zeros(H._up(OC, 128), 9, H._up(IC, 64), device=DEV, dtype=BF)
        f[:OC, :, :IC] = v.permute(0, 2, 1).to(BF)
        t = torch.zeros(H._up(IC, 128), 9, H._up(OC, 64), device=DEV, dtype=BF)
        t[:IC, :, :OC] = v.permute(1, 2, 0).to(BF)
        return f.reshape(-1), t.reshape(-1)

    def make():
        torch.manual_seed(11)
        return {"w": torch.randn(OC, IC, 3, 3, device=DEV)}

    def fn(w):
        H.invalidate_weight_cache()
        try:
            p = torch.nn.Parameter(w)
            fwd, trn = H.packed_weight(p, False, 9), H.packed_weight(p, True, 9)
            first = (fwd.clone(), trn.clone())
            with torch.no_grad():
                p.mul_(-0.5).add_(0.25)               # an "optimizer step" on the fp32 master
            H.refresh_weights()
            torch.cuda.synchronize()
            return first + (fwd, trn)
        finally:
            H.invalidate_weight_cache()

    f0, t0, f1, t1 = G.run_guarded(make, fn, mutated=("w",))
    w = make()["w"]
    rf, rt = ref_packs(w)
    assert torch.equal(f0, rf) and torch.equal(t0, rt)
    rf, rt = ref_packs(w * -0.5 + 0.25)
    assert torch.equal(f1, rf) and torch.equal(t1, rt)


# ---------------------------------------------------------- step kernels ----
ADAM_SIZES = [(33, 7), (128,), (5, 5, 3)]          # the odd sizes of test_adam_matches_torch
ADAM_HP = dict(lr=1e-2, b1=0.9, b2=0.99, eps=1e-8, wd=0.01, t=3, grad_scale=0.5, ema_decay=0.999)


def _adam_make():
    from distributed_3d_diffusion_pytorch_amd.parallel.flat import FlatParams
    torch.manual_seed(8)
    flat = FlatParams([torch.nn.Parameter(torch.randn(s, device=DEV)) for s in ADAM_SIZES])
    n = flat.numel
    h = ADAM_HP
    hp = [h["b1"], h["b2"], h["eps"], h["wd"], h["lr"] / (1 - h["b1"] ** h["t"]), math.sqrt(1 - h["b2"] ** h["t"]),
          h["grad_scale"], 1 - h["ema_decay"]]
    return {"p": flat.data.clone(), "g": torch.randn(n, device=DEV), "m": torch.randn(n, device=DEV) * 0.1,
            "v": torch.rand(n, device=DEV) * 0.1, "ema": torch.randn(n, device=DEV),
            "hp": torch.tensor(hp, dtype=torch.float32, device=DEV)}


def _adam_ref():
    """The update of engine/optim.py's torch branch, in fp64."""
    s = {k: v.double() for k, v in _adam_make().items()}
    h = ADAM_HP
    g = s["g"] * h["grad_scale"] + h["wd"] * s["p"]
    m = torch.lerp(s["m"], g, 1 - h["b1"])
    v = s["v"] * h["b2"] + (1 - h["b2"]) * g * g
    p = s["p"] - h["lr"] / (1 - h["b1"] ** h["t"]) * m / (v.sqrt() / math.sqrt(1 - h["b2"] ** h["t"]) + h["eps"])
    return {"p": p, "m": m, "v": v, "ema": torch.lerp(s["ema"], p, 1 - h["ema_decay"])}


def _adam_check(got):
    for k, r in ref_once("adam", _adam_ref).items():
        assert torch.allclose(got[k], r.float(), atol=1e-6, rtol=1e-5), (k, (got[k] - r.float()).abs().max().item())


def test_adam_flat(H):
    h = ADAM_HP

    def fn(p, g, m, v, ema, hp):
        H.adam_flat(p, g, m, v, ema, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["lr"] / (1 - h["b1"] ** h["t"]),
                    math.sqrt(1 - h["b2"] ** h["t"]), h["grad_scale"], h["ema_decay"])
        torch.cuda.synchronize()
        return {"p": p, "m": m, "v": v, "ema": ema}
    H.invalidate_weight_cache()
    _adam_check(G.run_guarded(_adam_make, fn, mutated=("p", "m", "v", "ema")))


def test_adam_update_all(H):
    from distributed_3d_diffusion_pytorch_amd.parallel.flat import FlatParams

    def fn(p, g, m, v, ema, hp):
        flat = FlatParams([torch.nn.Parameter(torch.empty(s, device=DEV)) for s in ADAM_SIZES])
        assert flat.numel == p.numel()
        flat.data, flat.grad = p, g
        H.adam_update_all(flat, m, v, ema, hp)
        torch.cuda.synchronize()
        H._FUSED.pop(id(flat), None)
        return {"p": p, "m": m, "v": v, "ema": ema}
    H.invalidate_weight_cache()
    _adam_check(G.run_guarded(_adam_make, fn, mutated=("p", "m", "v", "ema")))


def test_diffusion_inputs(H):
    def make():
        torch.manual_seed(3)
        return {"img": torch.rand(6, 2, 3, 12, 12, device=DEV) * 2 - 1}
    seed = 0xDEADBEEF12345678
    xz, eps, lam, keep = G.run_guarded(make, lambda img: H.diffusion_inputs(img, seed, e0=5, cond_prob=0.3))
    xr, er, lr, kr = T.diffusion_inputs(make()["img"], seed, e0=5, cond_prob=0.3, dtype=torch.float32)
    assert torch.equal(keep, kr) and 0 < int((~keep).sum()) < 6
    assert (lam - lr).abs().max().item() < 2e-4 * 20
    assert (eps - er).abs().max().item() < 1e-3
    assert (xz.float() - xr).abs().max().item() < 2e-2


@pytest.mark.parametrize("loss_type", ["l2", "l1", "huber"])
def test_diff_loss(H, loss_type):
    def make():
        torch.manual_seed(4)
        y = torch.randn(5, 12, 12, 8, device=DEV).to(BF)
        y[..., 3:] = 0
        return {"y": grad(y), "eps": torch.randn(5, 3, 12, 12, device=DEV)}

    def run(M):
        def fn(y, eps):
            loss = M.diff_loss_nhwc(y, eps, loss_type)
            (loss * 0.37).backward()
            return loss, y.grad
        return fn

    lh, gh = G.run_guarded(make, run(H))
    lr_, gr = run(T)(**{k: _ref_in(v) for k, v in make().items()})
    assert abs(lh.item() - lr_.item()) < 1e-5 * abs(lr_.item())
    assert rel(gh, gr) < 1e-2
    assert float(gh[..., 3:].abs().max()) == 0.0


def _sampler(**kw):
    from distributed_3d_diffusion_pytorch_amd.engine import DiffusionSampler
    return DiffusionSampler(torch.nn.Linear(1, 1).to(DEV), timesteps=8, seed=3, chain_offset=4, **kw)


def _sampler_make(b=3, S=12):          # HW = 144: no multiple of the block
    def make():
        torch.manual_seed(12)
        return {"y": torch.randn(2 * b, S, S, 8, device=DEV).to(BF), "z": torch.randn(b, 3, S, S, device=DEV),
                "hist": torch.rand(b, 3, S, S, device=DEV) * 2 - 1, "xc": torch.rand(b, 3, S, S, device=DEV) * 2 - 1,
                "w": torch.tensor([0.0, 2.0, 5.0], device=DEV)}
    return make


def test_sampler_inputs(H):
    b, S, k, c0 = 3, 12, 2, 4
    smp = _sampler()
    row = smp.params(k)

    def fn(y, z, hist, xc, w):
        prm = G.place(H.torch._arena, torch.tensor(row, device=DEV), "prm")
        xz = H.torch.empty(4 * b, S, S, 8, dtype=BF, device=DEV)
        logsnr = H.torch.empty(2 * b, 2, dtype=torch.float32, device=DEV)
        H.sampler_inputs(xc, z, prm, None, smp.step_seed(k), c0, xz, logsnr)
        torch.cuda.synchronize()
        return xz, logsnr

    xz, logsnr = G.run_guarded(_sampler_make(b, S), fn)
    s = _sampler_make(b, S)()
    HW = S * S
    idx = (c0 + torch.arange(b, device=DEV))[:, None, None] * (3 * HW) + \
        torch.arange(3, device=DEV)[None, :, None] * HW + torch.arange(HW, device=DEV)[None, None, :]
    xu = T.normal01(smp.step_seed(k) ^ T.K_XU, idx).reshape(b, 3, S, S)
    ref = torch.zeros(2 * b, 2, S, S, 8, device=DEV)
    ref[:, 0, ..., :3] = torch.cat([s["xc"], xu]).permute(0, 2, 3, 1)
    ref[:, 1, ..., :3] = torch.cat([s["z"], s["z"]]).permute(0, 2, 3, 1)
    assert (xz.float() - ref.reshape(4 * b, S, S, 8)).abs().max().item() < 2e-2       # (test_diffusion_inputs' xz bound)
    want = torch.tensor([row[7], row[0]], dtype=torch.float32, device=DEV).expand(2 * b, 2)
    assert torch.equal(logsnr, want)


@pytest.mark.parametrize("k", [2, 7])
def test_sampler_step2(H, k):
    from distributed_3d_diffusion_pytorch_amd.diffusion import cfg_posterior
    b, S, c0 = 3, 12, 4
    smp = _sampler()

    def fn(y, z, hist, xc, w):
        prm = G.place(H.torch._arena, torch.tensor(smp.params(k), device=DEV), "prm")
        H.sampler_step2(z, y, w, prm, None, smp.step_seed(k), c0)
        torch.cuda.synchronize()
        return z

    zz = G.run_guarded(_sampler_make(b, S), fn, mutated=("z",))
    s = _sampler_make(b, S)()
    ec = s["y"][:b, ..., :3].float().permute(0, 3, 1, 2)
    eu = s["y"][b:, ..., :3].float().permute(0, 3, 1, 2)
    mean, var = cfg_posterior(s["z"], ec, eu, s["w"], torch.tensor(smp.lam[k]), torch.tensor(smp.lam_next[k]))
    if smp.add_noise(k):
        mean = mean + var.sqrt() * smp._noise(T.K_NZ, k, (b, 3, S, S), torch.device(DEV))
    assert (zz - mean).abs().max().item() < 1e-4


@pytest.mark.parametrize("solver,eta,k", [("ddim", 0.7, 3), ("dpmpp2m", 0.0, 4)])
def test_sampler_solve(H, solver, eta, k):
    from distributed_3d_diffusion_pytorch_amd.diffusion import solver_step
    b, S, c0 = 3, 12, 4
    smp = _sampler(solver=solver, eta=eta) if solver == "ddim" else _sampler(solver=solver)
    row = smp.solver_params(k)

    def fn(y, z, hist, xc, w):
        prm = G.place(H.torch._arena, torch.tensor(row, dtype=torch.float32, device=DEV), "prm")
        H.sampler_solve(z, hist, y, w, prm, None, smp.step_seed(k), c0)
        torch.cuda.synchronize()
        return z, hist

    zz, hh = G.run_guarded(_sampler_make(b, S), fn, mutated=("z", "hist"))
    s = _sampler_make(b, S)()
    F64 = torch.float64
    ec = s["y"][:b, ..., :3].permute(0, 3, 1, 2).to(F64)
    eu = s["y"][b:, ..., :3].permute(0, 3, 1, 2).to(F64)
    noise = smp._noise(T.K_NZ, k, (b, 3, S, S), torch.device(DEV)).to(F64)
    ref_z, ref_x0 = solver_step(s["z"].to(F64), ec, eu, s["w"].to(F64), s["hist"].to(F64),
                                torch.tensor(row, dtype=torch.float32), noise)
    assert (zz - ref_z).abs().max().item() < 1e-4 and (hh - ref_x0).abs().max().item() < 1e-4


def test_randn_hash(H):
    shape, seed, off = (5, 3, 7, 7), 0x1234567, 1000
    out = G.run_guarded(lambda: {}, lambda: H.randn_hash(shape, seed, off, DEV))
    n = math.prod(shape)
    ref = T.normal01(seed, off + torch.arange(n, device=DEV)).reshape(shape)
    assert (out - ref).abs().max().item() < 1e-3             # (the bound of the same draw in test_diffusion_inputs)


@pytest.mark.parametrize("quantize", [False, True])
def test_image_metrics(H, quantize):
    from metrics_oracle import oracle

    def make():
        torch.manual_seed(6)
        a = torch.rand(3, 3, 27, 43, device=DEV) * 2 - 1
        return {"a": a, "b": (a + torch.randn_like(a) * 0.1).clamp(-1, 1)}

    mse, ssim = G.run_guarded(make, lambda a, b: H.image_metrics(a, b, quantize))
    s = make()
    rm, rs = oracle(s["a"].cpu(), s["b"].cpu(), quantize)
    assert ((mse.double().cpu() - rm).abs() <= 1e-6 * rm + 1e-12).all()
    assert ((ssim.double().cpu() - rs).abs() <= 2e-6).all()
