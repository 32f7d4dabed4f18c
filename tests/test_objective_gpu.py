"""v-prediction and min-SNR loss weighting on the GPU: the training-input
kernel's v target, the weighted loss kernels, the three sampler kernels with
``prediction="v"`` (step 0 included), and the switch reaching the
graph-replayed sampler, the graph-replayed training step and the validation
loss."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64
LAMBDAS = [-20.0, math.log(5.0) - 0.01, math.log(5.0) + 0.01, 0.0, 20.0]
V_MINSNR = {"diffusion.prediction": "v", "diffusion.loss_weight": "min_snr"}


@pytest.fixture(scope="module")
def H():
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    return hip_impl


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


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def leaf(t, dtype=None):
    t = t.detach().clone()
    if dtype is not None:
        t = t.to(dtype)
    return t.requires_grad_(True)


# ------------------------------------------------------------ 7. the target
@pytest.mark.parametrize("B,S", [(5, 12), (24, 32)])
def test_diffusion_inputs_kernel_v_target(H, B, S):
    """diffusion_fwd2_k<v>: slot 1 is v = alpha eps - sigma z_clean (the torch
    draw's, to the bound the eps test uses); everything else is bitwise the
    eps instantiation's; the device seed block gives the host seed's draw."""
    torch.manual_seed(3)
    seed = 0xDEADBEEF12345678
    img = torch.rand(B, 2, 3, S, S, device=DEV) * 2 - 1
    xz, v, lam, keep = H.diffusion_inputs(img, seed, e0=5, cond_prob=0.3, prediction="v")
    xe, eps, le, ke = H.diffusion_inputs(img, seed, e0=5, cond_prob=0.3)
    xr, vr, lr, kr = T.diffusion_inputs(img, seed, e0=5, cond_prob=0.3, dtype=torch.float32, prediction="v")
    d = (v - vr).abs().max().item()
    print(f"B={B} S={S}: max |v - v_torch| {d:.3e}")
    assert d < 1e-3
    assert (v - eps).abs().max().item() > 0.1                 # it is another target
    assert torch.equal(xz, xe) and torch.equal(lam, le) and torch.equal(keep, ke) and torch.equal(keep, kr)
    word, off = 7, 3
    seed_blk = torch.tensor([0, word, off], dtype=torch.int64, device=DEV)
    base = 0x1111
    H.set_device_seed(seed_blk)
    try:
        xg, vg, lg, kg = H.diffusion_inputs(img, base, e0=0, prediction="v")
    finally:
        H.set_device_seed(None)
    xh, vh, lh, kh = H.diffusion_inputs(img, (base + word * 0x9E3779B97F4A7C15) & (2 ** 64 - 1), e0=off,
                                        prediction="v")
    assert torch.equal(vg, vh) and torch.equal(xg, xh) and torch.equal(lg, lh) and torch.equal(kg, kh)
    with pytest.raises(ValueError):
        H.diffusion_inputs(img, seed, prediction="x0")
    assert H.FALLBACKS == {}, H.FALLBACKS


# -------------------------------------------------------------- 8. the loss
@pytest.mark.parametrize("loss_type", ["l2", "l1", "huber"])
@pytest.mark.parametrize("prediction", ["eps", "v"])
@pytest.mark.parametrize("shape", [(5, 12, 12, 8), (6, 32, 32, 8)])
def test_weighted_loss_kernel(H, shape, prediction, loss_type):
    """diff_loss_part_k / diff_loss_bwd_k with the min-SNR weight of
    logsnr[:, 1] against the torch composition: the loss, the gradient on the
    whole tensor and on every example's slice (the weights span 8 decades: a
    wrong weight on a 1e-8 row shows only there), zero padding channels,
    bitwise repeatability."""
    torch.manual_seed(4)
    B, S = shape[0], shape[1]
    y = torch.randn(*shape, device=DEV).to(BF)
    y[..., 3:] = 0
    target = torch.randn(B, 3, S, S, device=DEV)
    lam = torch.tensor((LAMBDAS * 2)[:B], device=DEV)
    logsnr = torch.stack([torch.full_like(lam, 20.0), lam], 1).contiguous()
    kw = dict(logsnr=logsnr, prediction=prediction, loss_weight="min_snr", gamma=5.0)
    yh, yr = leaf(y), leaf(y, torch.float32)
    lh = H.diff_loss_nhwc(yh, target, loss_type, **kw)
    lr_ = T.diff_loss_nhwc(yr, target, loss_type, **kw)
    err = abs(lh.item() - lr_.item()) / abs(lr_.item())
    print(f"{shape} {prediction} {loss_type}: loss {lh.item():.6e} ref {lr_.item():.6e} rel {err:.2e}")
    assert err < 1e-5
    (lh * 0.37).backward()
    (lr_ * 0.37).backward()
    assert rel(yh.grad, yr.grad) < 1e-2
    for i in range(B):
        assert yr.grad[i].abs().max().item() > 0
        r = rel(yh.grad[i], yr.grad[i])
        assert r < 1e-2, (i, LAMBDAS[i % 5], r)
    assert float(yh.grad[..., 3:].abs().max()) == 0.0
    y2 = leaf(y)
    l2 = H.diff_loss_nhwc(y2, target, loss_type, **kw)
    (l2 * 0.37).backward()
    assert torch.equal(l2, lh) and torch.equal(y2.grad, yh.grad)
    # the weighted value is another one, and "none" is the unweighted call
    plain = H.diff_loss_nhwc(y, target, loss_type)
    assert abs(plain.item() - lh.item()) > 1e-3 * plain.item()
    assert torch.equal(H.diff_loss_nhwc(y, target, loss_type, logsnr=logsnr, prediction=prediction), plain)
    with pytest.raises(ValueError):
        H.diff_loss_nhwc(y, target, loss_type, prediction=prediction, loss_weight="min_snr")
    assert H.FALLBACKS == {}, H.FALLBACKS


# ------------------------------------------------------ 9. sampler kernels
def _heads(b, S):
    torch.manual_seed(12)
    y = torch.randn(2 * b, S, S, 8, device=DEV).to(BF)
    z = torch.randn(b, 3, S, S, device=DEV)
    w = torch.tensor([0.0, 2.0, 5.0, 2.0, 0.0], device=DEV)[:b].contiguous()
    yc = y[:b, ..., :3].permute(0, 3, 1, 2).to(F64)
    yu = y[b:, ..., :3].permute(0, 3, 1, 2).to(F64)
    return y, z, w, yc, yu


@pytest.mark.parametrize("b,S", [(3, 16), (5, 12)])
def test_sampler_step2_v_matches_posterior(H, b, S):
    """sampler_step2_k<v> == the fp64 cfg_posterior(prediction="v") on the
    same bf16 head output plus the counter noise, at k = 0, 2 and 7 of 8.
    Step 0 (lambda = -20) is the one the eps form cannot hold: there
    1/alpha = 2.2e4 and the fp32 1 - c of the posterior has lost its digits,
    so the eps instantiation is held to the bound at k = 2 and 7, as in
    test_sampler_step2_matches_posterior."""
    from distributed_3d_diffusion_pytorch_amd.diffusion import cfg_posterior
    from distributed_3d_diffusion_pytorch_amd.engine import DiffusionSampler
    c0 = 4
    y, z, w, yc, yu = _heads(b, S)
    smp = DiffusionSampler(torch.nn.Linear(1, 1).to(DEV), timesteps=8, seed=3, chain_offset=c0)
    for prediction, ks in (("v", (0, 2, 7)), ("eps", (2, 7))):
        for k in ks:
            prm = torch.tensor(smp.params(k), device=DEV)
            zz = z.clone()
            H.sampler_step2(zz, y, w, prm, None, smp.step_seed(k), c0, prediction=prediction)
            mean, var = cfg_posterior(z.to(F64), yc, yu, w.to(F64), torch.tensor(smp.lam[k]),
                                      torch.tensor(smp.lam_next[k]), prediction=prediction)
            if smp.add_noise(k):
                mean = mean + var.sqrt() * smp._noise(T.K_NZ, k, (b, 3, S, S), torch.device(DEV)).to(F64)
            d = (zz - mean).abs().max().item()
            print(f"b={b} S={S} {prediction} k={k}: max |dz'| {d:.3e}")
            assert torch.isfinite(zz).all()
            assert d < 1e-4, (prediction, k, d)
    # the two instantiations are different steps
    za, zb = z.clone(), z.clone()
    prm = torch.tensor(smp.params(2), device=DEV)
    H.sampler_step2(za, y, w, prm, None, smp.step_seed(2), c0)
    H.sampler_step2(zb, y, w, prm, None, smp.step_seed(2), c0, prediction="v")
    assert (za - zb).abs().max().item() > 1e-2
    # the legacy out-of-place step takes the switch too
    k = 2
    p = smp.params(k)
    ycf, yuf = yc.float().contiguous(), yu.float().contiguous()
    out = H.sampler_step(z, ycf, yuf, w, p[1], p[2], p[3], p[4], p[5], 0, 0, prediction="v")
    mean, _ = cfg_posterior(z.to(F64), yc, yu, w.to(F64), torch.tensor(smp.lam[k]), torch.tensor(smp.lam_next[k]),
                            prediction="v")
    assert (out - mean).abs().max().item() < 1e-4
    assert H.FALLBACKS == {}, H.FALLBACKS


@pytest.mark.parametrize("b,S", [(3, 16), (5, 12)])
def test_sampler_solve_v_matches_fp64_formula(H, b, S):
    """sampler_solve_k<v> == solver_step(prediction="v") in fp64 with the same
    fp32 row and counter noise: the case list of
    test_sampler_solve_matches_fp64_formula (NaN-history cases included) plus
    step 0 of each solver, for v and -- at that test's steps -- for eps."""
    from distributed_3d_diffusion_pytorch_amd.diffusion import solver_step
    from distributed_3d_diffusion_pytorch_amd.engine import DiffusionSampler
    c0 = 4
    y, z, w, yc, yu = _heads(b, S)
    hist = torch.rand(b, 3, S, S, device=DEV) * 2 - 1
    lin = torch.nn.Linear(1, 1).to(DEV)
    mk = lambda **kw: DiffusionSampler(lin, timesteps=8, seed=3, chain_offset=c0, **kw)  # noqa: E731
    nan = torch.full_like(hist, float("nan"))
    cases = [("ddim eta 0", mk(solver="ddim"), 3, hist, False),
             ("ddim eta 0.7", mk(solver="ddim", eta=0.7), 3, hist, False),
             ("dpmpp2m mid", mk(solver="dpmpp2m"), 4, hist, False),
             ("dpmpp2m mid logsnr", mk(solver="dpmpp2m", spacing="logsnr"), 5, hist, False),
             ("dpmpp2m last (first order), NaN history", mk(solver="dpmpp2m"), 7, nan, True),
             ("ddim eta 0.7, NaN history", mk(solver="ddim", eta=0.7), 2, nan, True)]
    first_steps = [("ddim eta 0.7 step 0, NaN history", mk(solver="ddim", eta=0.7), 0, nan, True),
                   ("dpmpp2m step 0, NaN history", mk(solver="dpmpp2m"), 0, nan, True),
                   ("dpmpp2m logsnr step 0, NaN history", mk(solver="dpmpp2m", spacing="logsnr"), 0, nan, True)]
    for prediction, lst in (("v", cases + first_steps), ("eps", cases)):
        for name, smp, k, h0, first in lst:
            row = smp.solver_params(k)
            assert row[5] == 0.0 or not first
            prm = torch.tensor(row, dtype=torch.float32, device=DEV)
            zz, hh = z.clone(), h0.clone()
            H.sampler_solve(zz, hh, y, w, prm, None, smp.step_seed(k), c0, prediction=prediction)
            noise = smp._noise(T.K_NZ, k, (b, 3, S, S), torch.device(DEV)).to(F64)
            ref_z, ref_x0 = solver_step(z.to(F64), yc, yu, w.to(F64), None if first else h0.to(F64), prm.cpu(), noise,
                                        prediction=prediction)
            dz, dx = (zz - ref_z).abs().max().item(), (hh - ref_x0).abs().max().item()
            print(f"b={b} S={S} {prediction} {name}: max |dz'| {dz:.3e}  max |dx0| {dx:.3e}")
            assert torch.isfinite(zz).all() and torch.isfinite(hh).all(), name
            assert dz < 1e-4 and dx < 1e-4, (prediction, name, dz, dx)
    # at step 0 the v data prediction is not just what the clamp leaves
    smp = mk(solver="dpmpp2m")
    prm = torch.tensor(smp.solver_params(0), dtype=torch.float32, device=DEV)
    zz, hh = z.clone(), nan.clone()
    H.sampler_solve(zz, hh, y, w, prm, None, smp.step_seed(0), c0, prediction="v")
    assert (hh.abs() < 1.0).float().mean().item() > 0.1
    # the device seed word of the graphed step gives the same draw as the host seed
    smp = mk(solver="ddim", eta=0.7)
    prm = torch.tensor(smp.solver_params(3), dtype=torch.float32, device=DEV)
    za, ha, zb, hb = z.clone(), hist.clone(), z.clone(), hist.clone()
    H.sampler_solve(za, ha, y, w, prm, None, smp.step_seed(3), c0, prediction="v")
    H.sampler_solve(zb, hb, y, w, prm, torch.tensor([4, 0, 0], dtype=torch.int64, device=DEV), smp.seed_base, c0,
                    prediction="v")
    assert torch.equal(za, zb) and torch.equal(ha, hb)
    with pytest.raises(ValueError):
        H.sampler_solve(za, ha, y, w, prm, None, smp.step_seed(3), c0, prediction="x0")
    assert H.FALLBACKS == {}, H.FALLBACKS


# ------------------------------------------------- 10. graph replay, sampler
@pytest.mark.parametrize("solver", ["ancestral", "dpmpp2m"])
def test_v_sampler_graph_replay_matches_eager(model, solver):
    """sample and sample_groups with prediction="v", 5 steps: the HIP-graph
    replayed step == the eager step with the same kernels and seeds (the
    comparison and bound of test_solver_graph_replay_matches_eager), and the
    switch reaches the graph: the eps sampler's replayed result differs."""
    from distributed_3d_diffusion_pytorch_amd.engine import DiffusionSampler
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    from test_solver_gpu import _single_args, _group_args
    rec, tg1, K1, w = _single_args()
    recs, tgG, KG, wG, group = _group_args()
    outs = {}
    for graph in (False, True):
        kw = dict(timesteps=5, seed=9, device=torch.device(DEV), graph=graph, solver=solver, prediction="v")
        smp = DiffusionSampler(model, **kw)
        o = [smp.sample(rec, *tg1[0], K1, w)]
        captured = smp._g["graph"] if graph else None
        assert (smp._g is not None) == graph
        o.append(smp.sample(rec, *tg1[1], K1, w))
        if graph:
            assert smp._g["graph"] is captured and ("x0" in smp._g) == (solver != "ancestral")
        smp = DiffusionSampler(model, **kw)
        o.append(smp.sample_groups(recs, *tgG[0], KG, wG, group))
        captured = smp._gg["graph"] if graph else None
        assert (smp._gg is not None) == graph
        o.append(smp.sample_groups(recs, *tgG[1], KG, wG, group))
        if graph:
            assert smp._gg["graph"] is captured and ("x0" in smp._gg) == (solver != "ancestral")
        outs[graph] = o
    for i, name in enumerate(("sample", "sample (2nd call)", "sample_groups", "sample_groups (2nd call)")):
        assert torch.isfinite(outs[False][i]).all()
        d = (outs[False][i] - outs[True][i]).abs().max().item()
        print(f"v {solver} {name}: max |graph - eager| {d:.3e}")
        assert d < 1e-3, (name, d)
    assert (outs[True][0] - outs[True][1]).abs().max().item() > 1e-2     # the new target poses were used
    assert (outs[True][2] - outs[True][3]).abs().max().item() > 1e-2
    eps_smp = DiffusionSampler(model, timesteps=5, seed=9, device=torch.device(DEV), graph=True, solver=solver)
    assert (eps_smp.sample(rec, *tg1[0], K1, w) - outs[True][0]).abs().max().item() > 1e-2
    assert hip_impl.FALLBACKS == {}, hip_impl.FALLBACKS


# ------------------------------------------------ 11. graph replay, training
def _trainer(extra, **over):
    from distributed_3d_diffusion_pytorch_amd.config import make_config
    from distributed_3d_diffusion_pytorch_amd.engine import Trainer
    from distributed_3d_diffusion_pytorch_amd.parallel import DistContext
    ov = {"model.H": 32, "model.W": 32, "model.dropout": 0.1, "data.imgsize": 32, "global_batch": 4,
          "data.synthetic": True, "log_every": 0, "ckpt_every": 0, "optim.warmup_examples": 8}
    ov.update(over)
    ov.update(extra)
    return Trainer(make_config(None, ov), DistContext(device=torch.device("cuda", 0)))


@pytest.mark.parametrize("micro", [2, 0])
def test_v_minsnr_graph_train_step_matches_eager(micro):
    """The HIP-graph replayed training step with v-prediction and the min-SNR
    weight == the eager step: the four assertions and bounds of
    test_graph_train_step_matches_eager; and the objective reaches the graph:
    a default-config trainer's losses on the same batches are others."""
    from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    data = SyntheticBatches(4, 32, "cuda", seed=5)
    batches = [next(data) for _ in range(3)]
    try:
        te = _trainer(V_MINSNR, micro_batch=micro, graph=False)
        tg = _trainer(V_MINSNR, micro_batch=micro, graph=True)
        assert torch.equal(te.flat.data, tg.flat.data)
        le = [te.train_step(*b).item() for b in batches]
        lg = [tg.train_step(*b).item() for b in batches]
        assert tg._graphed is not None and tg._graphed.defer == (micro == 0)
        tg.sync()
        for a, b in zip(le, lg):
            assert abs(a - b) <= 2e-3 * abs(a) + 1e-4, (le, lg)
        d = (te.flat.data - tg.flat.data).abs().max().item()
        assert d < 5e-4, d
        dm = (te.optim.exp_avg_sq - tg.optim.exp_avg_sq).abs().max().item()
        assert dm <= 1e-3 * te.optim.exp_avg_sq.abs().max().item() + 1e-12, dm
        assert tg.flat.grad.abs().max().item() == 0.0
        td = _trainer({}, micro_batch=micro, graph=True)      # (made last: a new trainer takes over the gradient sink)
        ld = [td.train_step(*b).item() for b in batches]
        td.sync()
        print(f"micro={micro}: eager {le} graph {lg} default {ld}")
        for a, b in zip(lg, ld):
            assert abs(a - b) > 0.05 * abs(b), (lg, ld)
    finally:
        hip_impl.set_device_seed(None)
    assert hip_impl.FALLBACKS == {}, hip_impl.FALLBACKS


# ------------------------------------------------------ 12. validation loss
def test_v_minsnr_validation_loss_under_graph_step():
    """Trainer.validation_loss under the graph step with v + min_snr scores
    the configured (weighted) objective -- heldout_loss called directly with
    the same config gives the same value, the default config another -- and
    leaves the parameters bitwise unchanged."""
    from distributed_3d_diffusion_pytorch_amd.config import DiffusionConfig
    from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches
    from distributed_3d_diffusion_pytorch_amd.engine import heldout_loss
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    batch = next(SyntheticBatches(2, 32, "cuda", seed=5))
    try:
        tr = _trainer(V_MINSNR, global_batch=2, micro_batch=0, graph=True, val_batches=2)
        tr.train_step(*batch)
        assert tr._graphed is not None and tr._graphed.defer, "graph step with the deferred update expected"
        val = tr.make_val_data()
        a = tr.validation_loss(val)
        before = tr.flat.data.clone()
        b = tr.validation_loss(val)
        assert a == b and a > 0 and a == a, (a, b)
        assert torch.equal(tr.flat.data, before) and tr.model.training and tr.step == 1
        direct = float(heldout_loss(tr.model, (tr._to_dev(x) for x in val), tr.cfg.seed, tr.cfg.diffusion, tr.dtype))
        plain = float(heldout_loss(tr.model, (tr._to_dev(x) for x in val), tr.cfg.seed, DiffusionConfig(), tr.dtype))
        print(f"val_loss {a} direct {direct} default objective {plain}")
        assert direct == a
        assert abs(plain - a) > 0.05 * plain
        assert torch.equal(tr.flat.data, before)
    finally:
        hip_impl.set_device_seed(None)
    assert hip_impl.FALLBACKS == {}, hip_impl.FALLBACKS
