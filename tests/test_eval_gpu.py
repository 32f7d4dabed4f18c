"""Evaluation path on the GPU: the grouped sampler step (eager and
graph-replayed), the validation loss under the graph training step, and
engine.evaluate end to end -- at 32x32 with a handful of steps."""
import pytest
import torch

from metrics_oracle import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


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


def test_grouped_step_matches_per_chain_step(model):
    """HIP sampler step with the conditioning computed for the 2G classes
    (cond / uncond per group) == the per-chain step with the poses expanded,
    to bf16 accuracy; single mid-schedule steps of a 256-step schedule, for
    the reason test_sampler_shared_cond_matches_per_chain gives (a whole short
    run is ill-conditioned)."""
    from distributed_3d_diffusion_pytorch_amd.engine import DiffusionSampler
    from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    b = 5
    img, R, t, K = next(SyntheticBatches(b, 32, DEV, seed=2))
    group = torch.tensor([0, 1, 1, 0, 2], device=DEV)
    Rg, Tg = R[:3].float().contiguous(), t[:3].float().contiguous()
    Kg = (K[:3].float() * torch.tensor([1.0, 1.1, 0.9], device=DEV).view(3, 1, 1)).contiguous()
    w = torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0], device=DEV)
    smp = DiffusionSampler(model, timesteps=256, seed=9, device=torch.device(DEV))
    assert smp._hip(img)
    z = torch.randn(b, 3, 32, 32, device=DEV)
    for k in (100, 128, 200):
        za = smp.step(z, img[:, 0], Rg[group].contiguous(), Tg[group].contiguous(), Kg[group].contiguous(), w, k,
                      shared=False)
        zb = smp.step(z, img[:, 0], Rg, Tg, Kg, w, k, group=group)
        assert torch.isfinite(zb).all()
        print(f"k={k}: rel {rel(zb, za):.3e}")
        assert rel(zb, za) < 1e-2, (k, rel(zb, za))
        # the groups' poses are read: another map gives another step
        zc = smp.step(z, img[:, 0], Rg, Tg, Kg, w, k, group=torch.tensor([1, 0, 2, 1, 0], device=DEV))
        assert rel(zc, za) > rel(zb, za)
    assert hip_impl.FALLBACKS == {}, hip_impl.FALLBACKS


def test_sample_groups_graph_replay_matches_eager(model):
    """sample_groups: the HIP-graph replayed step == the eager grouped step
    (same kernels and seeds; 5 steps, G = 2, two record entries); a second call
    with new target poses reuses the captured graph and still matches."""
    from distributed_3d_diffusion_pytorch_amd.engine import DiffusionSampler, RecordEntry
    from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches
    img, R, t, K = next(SyntheticBatches(5, 32, DEV, seed=1))
    R, t = R.float(), t.float()
    group = torch.tensor([0, 0, 1, 1, 1])
    recs = [[RecordEntry(img[:2, 0].contiguous(), R[0, 0], t[0, 0]), RecordEntry(img[:2, 1].contiguous(), R[0, 1], t[0, 1])],
            [RecordEntry(img[2:, 0].contiguous(), R[1, 0], t[1, 0]), RecordEntry(img[2:, 1].contiguous(), R[1, 1], t[1, 1])]]
    w = torch.tensor([0.0, 1.0, 2.0, 3.0, 1.5])
    targets = [(torch.stack([R[2, 1], R[3, 1]]), torch.stack([t[2, 1], t[3, 1]])),
               (torch.stack([R[4, 0], R[4, 1]]), torch.stack([t[4, 0], t[4, 1]]))]
    outs = {}
    for graph in (False, True):
        smp = DiffusionSampler(model, timesteps=5, seed=9, device=torch.device(DEV), graph=graph)
        outs[graph] = [smp.sample_groups(recs, *targets[0], K[0].float(), w, group)]
        captured = smp._gg["graph"] if graph else None
        assert (smp._gg is not None) == graph
        outs[graph].append(smp.sample_groups(recs, *targets[1], K[0].float(), w, group))
        if graph:
            assert smp._gg["graph"] is captured            # cached on (b, G, H, W, group map, K, w)
    for i in range(2):
        assert torch.isfinite(outs[False][i]).all()
        d = (outs[False][i] - outs[True][i]).abs().max().item()
        print(f"call {i}: max |graph - eager| {d:.3e}")
        assert d < 1e-3, (i, d)
    assert (outs[True][0] - outs[True][1]).abs().max().item() > 1e-2     # the new target poses were used


def test_validation_loss_under_graph_step():
    """validation_loss between two graph-replayed training steps (deferred
    update on, batch 2 at 32x32): it applies the held update first, scores the
    same value twice, and the parameters after the second step equal a run
    without the validation call, bitwise."""
    from distributed_3d_diffusion_pytorch_amd.config import make_config
    from distributed_3d_diffusion_pytorch_amd.engine import Trainer
    from distributed_3d_diffusion_pytorch_amd.parallel import DistContext
    from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    ctx = DistContext(device=torch.device("cuda", 0))
    data = SyntheticBatches(2, 32, "cuda", seed=5)
    batches = [next(data) for _ in range(2)]
    runs = []
    try:
        for validate in (False, True):
            cfg = make_config(None, {"model.H": 32, "model.W": 32, "model.dropout": 0.1, "data.imgsize": 32,
                                     "global_batch": 2, "micro_batch": 0, "data.synthetic": True, "log_every": 0,
                                     "ckpt_every": 0, "graph": True, "optim.warmup_examples": 8, "val_batches": 2})
            tr = Trainer(cfg, ctx)
            tr.train_step(*batches[0])
            assert tr._graphed is not None and tr._graphed.defer, "graph step with the deferred update expected"
            if validate:
                val = tr.make_val_data()
                a, b = tr.validation_loss(val), tr.validation_loss(val)
                assert a == b and a > 0 and a == a, (a, b)
                assert tr.model.training and tr.step == 1
            tr.train_step(*batches[1])
            tr.sync()
            torch.cuda.synchronize()
            runs.append((tr.flat.data.clone(), tr.optim.exp_avg.clone(), tr.optim.exp_avg_sq.clone(),
                         tr.optim.step_count))
            del tr
    finally:
        hip_impl.set_device_seed(None)
    for x, y in zip(runs[0][:3], runs[1][:3]):
        assert torch.equal(x, y), (x - y).abs().max().item()
    assert runs[0][3] == runs[1][3]


def test_evaluate_objects_end_to_end(model):
    """engine.evaluate on synthetic objects (32x32 model, 4 steps, two sampler
    batches): every reported row equals the fp64 oracle on the returned images."""
    from distributed_3d_diffusion_pytorch_amd.engine import EvalObject, evaluate_objects, summarize
    from distributed_3d_diffusion_pytorch_amd.data import SyntheticBatches
    img, R, t, K = next(SyntheticBatches(3, 32, "cpu", seed=8))
    img2, R2, t2, _ = next(SyntheticBatches(3, 32, "cpu", seed=9))
    objs = []
    for i in range(3):
        imgs = {0: img[i, 0], 1: img[i, 1], 2: img2[i, 0]}
        Rs = {0: R[i, 0].float(), 1: R[i, 1].float(), 2: R2[i, 0].float()}
        Ts = {0: t[i, 0].float(), 1: t[i, 1].float(), 2: t2[i, 0].float()}
        objs.append(EvalObject(f"obj{i}", imgs, Rs, Ts, K[i].float()))
    w = (0.0, 3.0)
    rows, images = evaluate_objects(model, objs, input_view=0, views=(1, 2), w=w, timesteps=4, batch=2,
                                    autoregressive=True, seed=3, device=DEV, keep_images=True)
    assert len(rows) == 3 * 2 * 2 and sorted(r["chain"] for r in rows) == sorted(list(range(6)) * 2)
    for r in rows:
        o = objs[int(r["instance"][3:])]
        out = images[(r["instance"], r["view"])][w.index(r["w"])][None]
        rm, rs = oracle(out, o.imgs[r["view"]][None], True)
        assert abs(r["mse"] - float(rm)) <= 1e-6 * float(rm) + 1e-12, (r, float(rm))
        assert abs(r["ssim"] - float(rs)) <= 2e-6, (r, float(rs))
    s = summarize(rows)
    assert s["n_images"] == 12 and set(s["psnr_mean"]) == {"0", "3"}
