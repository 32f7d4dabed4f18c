"""Few-step solvers on the GPU: `sampler_solve_k` against the fp64 formula,
the graph-replayed solver step against the eager one (sample and
sample_groups), and the eta = 1 DDIM step against the ancestral HIP step."""
import pytest
import torch

from test_eval_gpu import rel

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64


@pytest.fixture(scope="module")
def model():
    from distributed_3d_diffusion_pytorch_amd.models import XUNet
    torch.manual_seed(14)
    m = XUNet(H=32, W=32, ch=128).to(DEV)
    with torch.no_grad():
        for p in m.parameters():
            if p.abs().sum() == 0:
                p.normal_(0, 0.02)
    m.compute_dtype = BF
    m.eval()
    return m


@pytest.mark.parametrize("b,S", [(3, 16), (5, 12)])
def test_sampler_solve_matches_fp64_formula(b, S):
    """`sampler_solve_k` == solver_step in fp64 with the same fp32 row and the
    same counter noise (chain offset 4); S = 12 gives HW = 144, no multiple of
    the block.  A k1 = 0 row must not read the history buffer (NaN-filled)."""
    from distributed_3d_diffusion_pytorch_amd.diffusion import solver_step
    from distributed_3d_diffusion_pytorch_amd.engine import DiffusionSampler
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl as H, torch_impl as T
    torch.manual_seed(12)
    c0 = 4
    y = torch.randn(2 * b, S, S, 8, device=DEV).to(BF)
    z = torch.randn(b, 3, S, S, device=DEV)
    hist = torch.rand(b, 3, S, S, device=DEV) * 2 - 1
    w = torch.tensor([0.0, 2.0, 5.0, 2.0, 0.0], device=DEV)[:b].contiguous()
    ec = y[:b, ..., :3].permute(0, 3, 1, 2).to(F64)
    eu = y[b:, ..., :3].permute(0, 3, 1, 2).to(F64)
    lin = torch.nn.Linear(1, 1).to(DEV)
    mk = lambda **kw: DiffusionSampler(lin, timesteps=8, seed=3, chain_offset=c0, **kw)  # noqa: E731
    nan = torch.full_like(hist, float("nan"))
    cases = [("ddim eta 0", mk(solver="ddim"), 3, hist, False),
             ("ddim eta 0.7", mk(solver="ddim", eta=0.7), 3, hist, False),
             ("dpmpp2m mid", mk(solver="dpmpp2m"), 4, hist, False),
             ("dpmpp2m mid logsnr", mk(solver="dpmpp2m", spacing="logsnr"), 5, hist, False),
             ("dpmpp2m last (first order), NaN history", mk(solver="dpmpp2m"), 7, nan, True),
             ("ddim eta 0.7, NaN history", mk(solver="ddim", eta=0.7), 2, nan, True)]
    for name, smp, k, h0, first in cases:
        row = smp.solver_params(k)
        assert (row[5] != 0.0) == ("dpmpp2m mid" in name) and (row[6] != 0.0) == ("0.7" in name), (name, row)
        assert row[5] == 0.0 or not first
        prm = torch.tensor(row, dtype=torch.float32, device=DEV)
        zz, hh = z.clone(), h0.clone()
        H.sampler_solve(zz, hh, y, w, prm, None, smp.step_seed(k), c0)
        noise = smp._noise(T.K_NZ, k, (b, 3, S, S), torch.device(DEV)).to(F64)
        ref_z, ref_x0 = solver_step(z.to(F64), ec, eu, w.to(F64), None if first else h0.to(F64), prm.cpu(), noise)
        dz, dx = (zz - ref_z).abs().max().item(), (hh - ref_x0).abs().max().item()
        print(f"b={b} S={S} {name}: max |dz'| {dz:.3e}  max |dx0| {dx:.3e}")
        assert torch.isfinite(zz).all() and torch.isfinite(hh).all(), name
        assert dz < 1e-4 and dx < 1e-4, (name, dz, dx)
        if not first:                  # the history is read: another one gives another step
            z2, h2 = z.clone(), -h0
            H.sampler_solve(z2, h2, y, w, prm, None, smp.step_seed(k), c0)
            assert ((z2 - zz).abs().max().item() > 1e-3) == (row[5] != 0.0), name
    # the device seed word of the graphed step gives the same draw as the host seed
    smp = mk(solver="ddim", eta=0.7)
    prm = torch.tensor(smp.solver_params(3), dtype=torch.float32, device=DEV)
    za, ha, zb, hb = z.clone(), hist.clone(), z.clone(), hist.clone()
    H.sampler_solve(za, ha, y, w, prm, None, smp.step_seed(3), c0)
    H.sampler_solve(zb, hb, y, w, prm, torch.tensor([4, 0, 0], dtype=torch.int64, device=DEV), smp.seed_base, c0)
    assert torch.equal(za, zb) and torch.equal(ha, hb)
    assert H.FALLBACKS == {}, H.FALLBACKS


def _single_args():
    from distributed_3d_diffusion_pytorch_amd.engine import RecordEntry
    from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches
    img, R, t, K = next(SyntheticBatches(5, 32, DEV, seed=1))
    R, t = R.float(), t.float()
    rec = [RecordEntry(img[:, 0].contiguous(), R[0, 0], t[0, 0]), RecordEntry(img[:, 1].contiguous(), R[1, 0], t[1, 0])]
    w = torch.tensor([0.0, 1.0, 2.0, 3.0, 1.5])
    return rec, [(R[2, 1], t[2, 1]), (R[4, 0], t[4, 0])], K[0].float(), w


def _group_args():
    from distributed_3d_diffusion_pytorch_amd.engine import RecordEntry
    from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches
    img, R, t, K = next(SyntheticBatches(5, 32, DEV, seed=1))
    R, t = R.float(), t.float()
    recs = [[RecordEntry(img[:2, 0].contiguous(), R[0, 0], t[0, 0]), RecordEntry(img[:2, 1].contiguous(), R[0, 1], t[0, 1])],
            [RecordEntry(img[2:, 0].contiguous(), R[1, 0], t[1, 0]), RecordEntry(img[2:, 1].contiguous(), R[1, 1], t[1, 1])]]
    w = torch.tensor([0.0, 1.0, 2.0, 3.0, 1.5])
    targets = [(torch.stack([R[2, 1], R[3, 1]]), torch.stack([t[2, 1], t[3, 1]])),
               (torch.stack([R[4, 0], R[4, 1]]), torch.stack([t[4, 0], t[4, 1]]))]
    return recs, targets, K[0].float(), w, torch.tensor([0, 0, 1, 1, 1])


@pytest.mark.parametrize("solver,eta", [("dpmpp2m", 0.0), ("ddim", 0.5)])
def test_solver_graph_replay_matches_eager(model, solver, eta):
    """sample and sample_groups, 5 steps: the HIP-graph replayed solver step
    (static history buffer, rows from the device table) == the eager step with
    the same kernels and seeds; a second call with new target poses reuses the
    captured graph -- its history restarts -- and still matches."""
    from distributed_3d_diffusion_pytorch_amd.engine import DiffusionSampler
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    rec, tg1, K1, w = _single_args()
    recs, tgG, KG, wG, group = _group_args()
    outs = {}
    for graph in (False, True):
        kw = dict(timesteps=5, seed=9, device=torch.device(DEV), graph=graph, solver=solver, eta=eta)
        smp = DiffusionSampler(model, **kw)
        o = [smp.sample(rec, *tg1[0], K1, w)]
        captured = smp._g["graph"] if graph else None
        assert (smp._g is not None) == graph
        o.append(smp.sample(rec, *tg1[1], K1, w))
        if graph:
            assert smp._g["graph"] is captured and "x0" in smp._g
        smp = DiffusionSampler(model, **kw)
        o.append(smp.sample_groups(recs, *tgG[0], KG, wG, group))
        captured = smp._gg["graph"] if graph else None
        assert (smp._gg is not None) == graph
        o.append(smp.sample_groups(recs, *tgG[1], KG, wG, group))
        if graph:
            assert smp._gg["graph"] is captured and "x0" in smp._gg
        outs[graph] = o
    for i, name in enumerate(("sample", "sample (2nd call)", "sample_groups", "sample_groups (2nd call)")):
        assert torch.isfinite(outs[False][i]).all()
        d = (outs[False][i] - outs[True][i]).abs().max().item()
        print(f"{solver} eta={eta} {name}: max |graph - eager| {d:.3e}")
        assert d < 1e-3, (name, d)
    assert (outs[True][0] - outs[True][1]).abs().max().item() > 1e-2     # the new target poses were used
    assert (outs[True][2] - outs[True][3]).abs().max().item() > 1e-2
    assert hip_impl.FALLBACKS == {}, hip_impl.FALLBACKS


def test_ddim_eta1_step_matches_ancestral_step(model):
    """Eager HIP steps from the same z: ddim at eta = 1 == the ancestral step
    (the same posterior, other kernel and coefficient form), mid-schedule steps
    of 256 -- the ancestral kernel forms 1 - c in fp32, inaccurate at the
    schedule's ends."""
    from distributed_3d_diffusion_pytorch_amd.engine import DiffusionSampler, SolverState
    from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    b = 4
    img, R, t, K = next(SyntheticBatches(b, 32, DEV, seed=2))
    Rb = R[:1].float().expand(b, 2, 3, 3).contiguous()
    Tb = t[:1].float().expand(b, 2, 3).contiguous()
    Kb = K[:1].float().expand(b, 3, 3).contiguous()
    w = torch.tensor([0.0, 1.0, 2.0, 3.0], device=DEV)
    kw = dict(timesteps=256, seed=9, device=torch.device(DEV))
    anc = DiffusionSampler(model, **kw)
    ddim = DiffusionSampler(model, solver="ddim", eta=1.0, **kw)
    assert anc._hip(img) and ddim._hip(img)
    z = torch.randn(b, 3, 32, 32, device=DEV)
    for k in (100, 128, 200):
        za = anc.step(z, img[:, 0], Rb, Tb, Kb, w, k, shared=True)
        st = SolverState()
        zd = ddim.step(z, img[:, 0], Rb, Tb, Kb, w, k, shared=True, state=st)
        assert torch.isfinite(zd).all() and st.x0_prev is not None and st.x0_prev.abs().max().item() <= 1.0
        print(f"k={k}: rel {rel(zd, za):.3e}")
        assert rel(zd, za) < 1e-2, (k, rel(zd, za))
    assert hip_impl.FALLBACKS == {}, hip_impl.FALLBACKS
