"""csrc/field_geom.hip (ops.field_geometry on the GPU) against the float64 torch
form on the CPU, bound 0.5 and 1, with and without a table.  Hash grids in
[-6, 6] whose sigma channel is scaled and shifted by SIGMA until the
preconditions of reference() hold, the orbit cameras of data.procedural_pose,
the tables of data.procedural_scene.  The gradient of the trilinear cell jumps
at cell faces: the normal of a pixel with a sample within FACE_EPS of a face
(at G = 5, S = 7 the middle sample of every ray through opposite faces) is
only checked to be a unit vector; profiles/field/README.md has the story."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
from distributed_3d_diffusion_pytorch_amd import ops  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.data import procedural as P  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T  # noqa: E402

DEV, SEED = "cuda", 1234
CASES = [(1, 1, 2, 1, 1, 1), (2, 2, 5, 5, 7, 7), (1, 3, 16, 24, 8, 32), (3, 1, 9, 16, 16, 16)]   # (F, V, G, H, W, S)
BOUNDS = [0.5, 1.0]
SIGMA = {(CASES[2], 0.5): (1.75, 0.0), (CASES[2], 1.0): (1.0, -1.7), (CASES[3], 0.5): (2.0, 0.0)}   # else (1, 0)
# profiles/field/README.md: the largest difference of the torch form in fp32 and fp64 on the CPU over these 8 inputs
# (normal: pixels, row 5: rows without face samples); A and n absolute, D and rows relative; the kernel gets 4 x that.
FP32_A, FP32_D_REL, FP32_N = 6.855e-7, 1.185e-6, 2.104e-5
FP32_ROW_REL = {3: 2.585e-7, 4: 3.835e-7, 5: 7.916e-7, 6: 1.367e-6}
TOL_A, TOL_D_REL, TOL_N = 4 * FP32_A, 4 * FP32_D_REL, 4 * FP32_N
# grid units; an fp32 sample position is off by a few ulp of (|p| + bound) scale <= 2.3 * 7.5 * 6e-8 = 1e-6
FACE_EPS = 1e-5
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
        F, V, G = case[:3]
        objs = [1 + 2 * f for f in range(F)]
        R, t = P.procedural_pose(SEED, [o for o in objs for _ in range(V)], list(range(V)) * F)
        grid = (T.u01(SEED + G, torch.arange(F * G ** 3 * 4)) * 12 - 6).reshape(F, G, G, G, 4).contiguous()
        scale, shift = SIGMA.get((case, bound), (1.0, 0.0))
        grid[..., 3] = grid[..., 3] * scale + shift
        _IN[(case, bound)] = {"grid": grid, "K": P.srn_intrinsics()[None].expand(F, 3, 3).contiguous(),
                              "R": R.reshape(F, V, 3, 3).contiguous(), "t": t.reshape(F, V, 3).contiguous(),
                              "table": P.procedural_scene(SEED, objs)}
    return _IN[(case, bound)]


def reference(case, bound):
    """The float64 torch form on the CPU, once per input; asserts the preconditions: no opacity within 1e-3 of
    the threshold, no |g| on P below 1e-3 of the largest, pixels on both sides of P and of M."""
    if (case, bound) not in _REF:
        H_, W_, S = case[3:]
        cond = {}
        s, m = T._field_geometry(**inputs(case, bound), H=H_, W=W_, samples=S, bound=bound, rescale_from=128,
                                 return_maps=True, dtype=torch.float64, cond=cond)
        A, gn = m[:, :, 0].double(), cond["gnorm"]
        hit = A > T.FG_HIT
        assert (A - T.FG_HIT).abs().min() >= 1e-3 and gn[hit].min() >= 1e-3 * gn[hit].max()
        if A.numel() > 1:
            assert 0 < s[..., 0].sum() < A.numel() and 0 < s[..., 1].sum() < A.numel()
        _REF[(case, bound)] = (s, m, cond)
    return _REF[(case, bound)]


def on_dev(case, bound, table=True):
    return {k: v.to(DEV) for k, v in inputs(case, bound).items() if table or k != "table"}


def compare(scores, maps, case, bound, tag):
    rs, rm, cond = reference(case, bound)
    m, hit = maps.cpu().double(), rm[:, :, 0] > T.FG_HIT
    face = hit & (cond["face"] < FACE_EPS)                    # normals not defined to rounding
    eA = (m[:, :, 0] - rm[:, :, 0]).abs().max().item()
    assert torch.equal(torch.isinf(m[:, :, 1]), ~hit) and torch.isfinite(m[:, :, [0, 2, 3, 4]]).all()
    eD = ((m[:, :, 1] - rm[:, :, 1])[hit].abs() / rm[:, :, 1][hit]).max().item()
    eN = (m[:, :, 2:] - rm[:, :, 2:]).abs().amax(2)[~face].max().item()
    print(f"{tag}: opacity {eA:.3e} (bound {TOL_A:.3e}), depth relative {eD:.3e} (bound {TOL_D_REL:.3e}), normal "
          f"{eN:.3e} (bound {TOL_N:.3e}) off the {int(face.sum())} of {int(hit.sum())} hit pixels with face samples")
    assert maps.dtype == torch.float32 and eA <= TOL_A and eD <= TOL_D_REL and eN <= TOL_N
    assert ((m[:, :, 2:].square().sum(2).sqrt() - hit.double()).abs() <= 1e-6).all()        # unit on P, zero off it
    if scores is None:
        return
    s = scores.cpu()
    assert scores.dtype == torch.float64 and torch.equal(s[..., :3], rs[..., :3]) and torch.isfinite(s).all()
    # row 5 is the sum of the kernel's own normals against the true ones (fp64 terms <= 2, rounding only) ...
    both = hit & (cond["n_true"].square().sum(2) > 0.5)
    own = torch.where(both, 1.0 - (m[:, :, 2:] * cond["n_true"]).sum(2), torch.zeros(())).flatten(2).sum(2)
    print(f"{tag}: row 5 against its maps {(s[..., 5] - own).abs().max().item():.3e}")
    assert ((s[..., 5] - own).abs() <= 1e-10 * rs[..., 2].clamp_min(1.0)).all()
    clean = ~(face & both).flatten(2).any(2)                  # ... and the oracle's where no pixel has face samples
    for k, fp32 in FP32_ROW_REL.items():
        e = ((s[..., k] - rs[..., k]).abs() / rs[..., k].abs().clamp_min(1e-300))[clean if k == 5 else ...]
        print(f"{tag}: row {k} relative {e.max().item() if e.numel() else 0.0:.3e} (bound {4 * fp32:.3e})")
        assert (e <= 4 * fp32).all()


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_matches_fp64_oracle(H, case, bound):
    F, V, _, H_, W_, S = case
    a = on_dev(case, bound)
    kw = dict(H=H_, W=W_, samples=S, bound=bound)
    scores, maps = ops.field_geometry(**a, **kw, return_maps=True)
    compare(scores, maps, case, bound, f"{case} bound={bound}")
    # row 0 is the renderer's own hit count on the same cameras
    rep = lambda x: x.repeat_interleave(V, 0)  # noqa: E731
    prim = ops.scene_render(rep(a["table"]), a["R"].flatten(0, 1), a["t"].flatten(0, 1), rep(a["K"]), H_, W_, aa=1,
                            return_aux=True)[2]
    assert torch.equal(scores[..., 0], (prim >= 0).flatten(1).sum(1).view(F, V).double())
    # without a table: the same maps; scores alone: the same rows; twice: the same bits
    assert torch.equal(ops.field_geometry(**on_dev(case, bound, table=False), **kw, return_maps=True), maps)
    assert torch.equal(ops.field_geometry(**a, **kw), scores)
    # a batched call is the F single-field calls, bit for bit
    for f in range(F):
        s1, m1 = ops.field_geometry(**{k: v[f:f + 1].contiguous() for k, v in a.items()}, **kw, return_maps=True)
        assert torch.equal(s1[0], scores[f]) and torch.equal(m1[0], maps[f])


@pytest.mark.parametrize("table", [True, False])
def test_field_geometry_guarded(H, table):
    """tests/guarded.py (the +inf depths are masked for the helper's finiteness check only)."""
    case, bound = CASES[2], 0.5
    keep = {}

    def fn(**a):
        out = H.field_geometry(**a, H=case[3], W=case[4], samples=case[5], bound=bound, return_maps=True)
        keep["scores"], keep["maps"] = out if table else (None, out)
        finite = torch.where(torch.isinf(keep["maps"]), torch.zeros_like(keep["maps"]), keep["maps"])
        return finite if not table else (keep["scores"], finite)

    guarded.run_guarded(lambda: on_dev(case, bound, table), fn)
    compare(keep["scores"], keep["maps"], case, bound, "guarded")
