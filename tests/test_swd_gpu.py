"""csrc/swd.hip (ops.sliced_wasserstein on the GPU) against the float64 torch
form on the CPU.  The sets are procedural objects seen from views 0 and 1.

The tolerance is derived, not measured.  The oracle keeps its keys in fp64; the
kernel rounds each key once to fp32, at most half an ulp = 2^-24 |key|.  Sorting
is 1-Lipschitz in the sup norm, so each sorted array moves by at most 2^-24 kmax
and each |a_i - b_i| -- hence their mean -- by at most 2^-23 kmax, kmax the
largest |key| the oracle saw at that level; 1e-12 covers the fp64 reordering."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
from distributed_3d_diffusion_pytorch_amd import ops  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.data import procedural as P  # noqa: E402
from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T  # noqa: E402

DEV, SEED = "cuda", 7
# (N, H, W, L, P, D): n = 6 in one wave, no pyramid; n = 150 -> 256, non-square, several waves; n = 1152 -> 2048,
# several keys per thread, three levels; n = 16384, the LDS limit; the 128-wide pyramid
CASES = [(2, 8, 8, 1, 3, 2), (3, 16, 24, 2, 50, 5), (9, 32, 32, 3, 128, 3), (128, 16, 16, 1, 128, 2),
         (2, 128, 128, 2, 8, 2)]
_IN, _REF = {}, {}


@pytest.fixture(scope="module")
def H():
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    yield hip_impl
    _IN.clear()
    _REF.clear()


def inputs(case, const=False):
    """CPU inputs of a case, computed once and shared; ``const``: channel 2 of ``a`` is 1 everywhere (sigma = 0)."""
    if (case, const) not in _IN:
        N, H_, W_, L, _, D = case
        objs = list(range(1, N + 1))
        K = P.srn_intrinsics()[None].expand(N, 3, 3).contiguous()
        table = P.procedural_scene(1234, objs)
        a, b = (T.scene_render(table, *P.procedural_pose(1234, objs, [v] * N), K, H_, W_, aa=2).contiguous()
                for v in (0, 1))
        if const:
            a[:, 2] = 1.0
        _IN[(case, const)] = {"a": a, "b": b, "dirs": T.swd_directions(SEED, L, D)}
    return _IN[(case, const)]


def kwargs(case):
    return dict(levels=case[3], patches=case[4], seed=SEED)


def reference(case, const=False, quantize=True):
    key = (case, const, quantize)
    if key not in _REF:
        _REF[key] = T.sliced_wasserstein(**inputs(case, const), **kwargs(case), quantize=quantize, return_kmax=True)
    return _REF[key]


def on_dev(case, const=False):
    return {k: v.to(DEV) for k, v in inputs(case, const).items()}


def compare(swd, case, const=False, quantize=True):
    ref, kmax = reference(case, const, quantize)
    assert swd.dtype == torch.float64 and tuple(swd.shape) == (case[3],)
    err = (swd.cpu() - ref).abs()
    print(f"{case} const={const}: swd {ref.tolist()} kmax {kmax.tolist()} off by {err.tolist()}")
    assert torch.isfinite(ref).all() and (ref > 0).all()
    assert (err <= 2.0 ** -23 * kmax + 1e-12).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_matches_fp64_oracle(H, case):
    d = on_dev(case)
    swd = ops.sliced_wasserstein(d["a"], d["b"], dirs=d["dirs"], **kwargs(case))
    compare(swd, case)
    assert torch.equal(ops.sliced_wasserstein(d["a"], d["b"], dirs=d["dirs"], **kwargs(case)), swd)   # the same bits
    same = ops.sliced_wasserstein(d["a"], d["a"].clone(), dirs=d["dirs"], **kwargs(case))
    assert torch.equal(same, torch.zeros_like(same))


def test_constant_channel(H):
    """sigma_c = 0 in one set's channel (1 / sigma := 0), on the unquantized map."""
    case = CASES[1]
    d = on_dev(case, const=True)
    compare(ops.sliced_wasserstein(d["a"], d["b"], dirs=d["dirs"], quantize=False, **kwargs(case)), case, True, False)


def test_sliced_wasserstein_guarded(H):
    """tests/guarded.py over the planes, the statistics, the partials and the result at the ragged shape."""
    case = CASES[1]
    compare(guarded.run_guarded(lambda: on_dev(case), lambda **a: H.sliced_wasserstein(**a, **kwargs(case))), case)


def test_too_many_descriptors(H):
    a = torch.zeros(5, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.sliced_wasserstein(a, a, levels=1, patches=3277, dirs=2)          # n = 16385
