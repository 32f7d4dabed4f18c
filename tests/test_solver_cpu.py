"""Few-step solvers (DDIM, DPM-Solver++ 2M) on the CPU: the update rules
against the ancestral posterior and against an analytic probability-flow
solution, the sampler paths (sample, sample_groups, step) and the CLI."""
import json
import math
import os

import pytest
import torch

from distributed_3d_diffusion_pytorch_amd.config import make_config
from distributed_3d_diffusion_pytorch_amd.data import write_synthetic_srn
from distributed_3d_diffusion_pytorch_amd.diffusion import (cfg_posterior, sampler_logsnrs, solver_row, solver_step)
from distributed_3d_diffusion_pytorch_amd.engine import DiffusionSampler, RecordEntry, SolverState, Trainer
from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as TI
from distributed_3d_diffusion_pytorch_amd.parallel import DistContext
from test_eval_cpu import K, SPANS, TARGET_R, TARGET_T, TINY_OV, _records, _signal_model

F64 = torch.float64
LAM0 = 20.0


def _schedule(T, spacing):
    lam, lam_next = sampler_logsnrs(T, spacing=spacing)
    return lam.tolist(), lam_next.tolist()


# ------------------------------------------------------------------- math
def test_logsnr_spacing():
    a, b = sampler_logsnrs(8)
    a2, b2 = sampler_logsnrs(8, spacing="t")
    assert torch.equal(a, a2) and torch.equal(b, b2)
    lam, lam_next = sampler_logsnrs(8, -20.0, 20.0, spacing="logsnr")
    assert torch.equal(torch.cat([lam, lam_next[-1:]]), torch.linspace(-20.0, 20.0, 9))
    with pytest.raises(ValueError):
        sampler_logsnrs(8, spacing="karras")


@pytest.mark.parametrize("spacing", ["t", "logsnr"])
def test_ddim_eta1_is_the_ancestral_posterior(spacing):
    """fp64: the ddim row at eta = 1 gives cfg_posterior's mean + sqrt(var) *
    noise (an identity: only rounding remains); the last step adds no noise
    in either."""
    lam, lam_next = _schedule(8, spacing)
    g = torch.Generator().manual_seed(1)
    b = 3
    z, ec, eu, noise = (torch.randn(b, 3, 8, 8, generator=g, dtype=F64) for _ in range(4))
    w = torch.tensor([0.0, 2.0, 5.0], dtype=F64)
    for k in (2, 4, 6):
        row = solver_row(lam, lam_next, k, "ddim", 1.0, LAM0)
        out, x0 = solver_step(z, ec, eu, w, None, row, noise)
        mean, var = cfg_posterior(z, ec, eu, w, torch.tensor(lam[k], dtype=F64), torch.tensor(lam_next[k], dtype=F64))
        torch.testing.assert_close(out, mean + var.sqrt() * noise, rtol=0.0, atol=1e-10)
        assert x0.abs().max() <= 1.0 and row[0] == lam[k] and row[7] == LAM0 and row[5] == 0.0
    row = solver_row(lam, lam_next, 7, "ddim", 1.0, LAM0)
    assert row[6] == 0.0
    out, _ = solver_step(z, ec, eu, w, None, row, None)              # the noise is not read
    assert torch.isfinite(out).all()
    smp = DiffusionSampler(torch.nn.Linear(1, 1), timesteps=8, spacing=spacing)
    assert not smp.add_noise(7) and smp.add_noise(6)


@pytest.mark.parametrize("spacing", ["t", "logsnr"])
def test_dpmpp2m_first_and_last_rows_are_first_order(spacing):
    for T in (2, 8, 64):
        lam, lam_next = _schedule(T, spacing)
        for k in (0, T - 1):
            a = solver_row(lam, lam_next, k, "dpmpp2m", 0.0, LAM0)
            d = solver_row(lam, lam_next, k, "ddim", 0.0, LAM0)
            assert a[5] == 0.0 and a[6] == 0.0
            for x, y in zip(a, d):
                assert abs(x - y) <= 1e-12 * abs(y), (T, k, a, d)
        if T > 2:                       # the steps between are second order: k0 + k1 = q, k1 = -q / (2 r)
            k = T // 2
            a = solver_row(lam, lam_next, k, "dpmpp2m", 0.0, LAM0)
            f = solver_row(lam, lam_next, k, "dpmpp2m", 0.0, LAM0, first_order=True)
            h, hp = 0.5 * (lam_next[k] - lam[k]), 0.5 * (lam[k] - lam[k - 1])
            assert a[5] != 0.0 and f[5] == 0.0
            assert abs(a[4] + a[5] - f[4]) <= 1e-12 * abs(f[4])
            assert abs(a[5] + f[4] * h / (2 * hp)) <= 1e-12 * abs(a[5])


def _sample_args(b=2):
    g = torch.Generator().manual_seed(11)
    img = torch.rand(b, 3, 16, 16, generator=g) * 2 - 1
    rec = [RecordEntry(img, *p) for p in ((TARGET_R[1], TARGET_T[1]),)]
    return rec, TARGET_R[0], TARGET_T[0], K, torch.tensor([0.0, 2.0])[:b]


def test_two_step_dpmpp2m_equals_ddim():
    """T = 2: both dpmpp2m steps (first, last) are first order = ddim eta 0."""
    m = _signal_model()
    outs = [DiffusionSampler(m, timesteps=2, seed=5, solver=s).sample(*_sample_args()) for s in ("ddim", "dpmpp2m")]
    assert torch.isfinite(outs[0]).all()
    torch.testing.assert_close(outs[1], outs[0], rtol=1e-4, atol=1e-5)


# ------------------------------------------------------ order of accuracy
S_DATA = 0.25


class _GaussianEps(torch.nn.Module):
    """The exact eps-predictor of per-pixel data N(0, S_DATA^2):
    eps = sigma z / (alpha^2 S^2 + sigma^2); conditioning is ignored."""

    def __init__(self):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))

    def forward(self, batch, cond_mask=None, **kw):
        z = batch["z"].double()
        lam = batch["logsnr"][:, 1].double().view(-1, 1, 1, 1)
        a2, s2 = torch.sigmoid(lam), torch.sigmoid(-lam)
        return (s2.sqrt() * z / (a2 * S_DATA ** 2 + s2)).to(batch["z"].dtype)


def _sig(x):
    return 1.0 / (1.0 + math.exp(-x))


def _exact(smp, z0):
    ls, le = smp.lam[0], smp.lam_next[-1]
    return z0.double() * math.sqrt((_sig(le) * S_DATA ** 2 + _sig(-le)) / (_sig(ls) * S_DATA ** 2 + _sig(-ls)))


def _rms_error(T, spacing, solver):
    m = _GaussianEps()
    b = 4
    smp = DiffusionSampler(m, timesteps=T, seed=2, share_cond=False, solver=solver, spacing=spacing)
    img = torch.zeros(b, 3, 16, 16)
    rec = [RecordEntry(img, TARGET_R[1], TARGET_T[1])]
    out = smp.sample(rec, TARGET_R[0], TARGET_T[0], K, torch.tensor([0.0, 1.0, 2.0, 3.0]))
    z0 = smp._noise(TI.K_Z0, None, (b, 3, 16, 16), torch.device("cpu"))
    assert z0.abs().max() < 4.0          # x0 = alpha S^2 z / var stays inside the clamp all along
    return (out.double() - _exact(smp, z0)).square().mean().sqrt().item()


def _rms_2m_without_lower_order_final(T, spacing):
    """A local fp64 copy of the dpmpp2m recursion that keeps the LAST step
    second order (the library has no such switch)."""
    smp = DiffusionSampler(_GaussianEps(), timesteps=T, seed=2, share_cond=False, spacing=spacing)
    z0 = smp._noise(TI.K_Z0, None, (4, 3, 16, 16), torch.device("cpu")).double()
    z, x0_prev = z0.clone(), None
    for k in range(T):
        l, ln = smp.lam[k], smp.lam_next[k]
        alpha, sigma, alpha_n, sigma_n = (math.sqrt(v) for v in (_sig(l), _sig(-l), _sig(ln), _sig(-ln)))
        eps = sigma * z / (alpha ** 2 * S_DATA ** 2 + sigma ** 2)
        x0 = ((z - sigma * eps) / alpha).clamp(-1.0, 1.0)
        h = 0.5 * (ln - l)
        q = -alpha_n * math.expm1(-h)
        if k == 0:
            d = x0
        else:
            r = 0.5 * (l - smp.lam[k - 1]) / h
            d = (1.0 + 0.5 / r) * x0 - (0.5 / r) * x0_prev
        z, x0_prev = sigma_n / sigma * z + q * d, x0
    return (z - _exact(smp, z0)).square().mean().sqrt().item()


@pytest.fixture(scope="module")
def rms():
    return {(T, sp, s): _rms_error(T, sp, s) for T in (16, 32, 64) for sp in ("t", "logsnr") for s in ("ddim", "dpmpp2m")}


def test_order_of_accuracy_on_gaussian_data(rms):
    """Against the exact probability-flow solution of Gaussian data: dpmpp2m
    at most half the ddim (eta 0) error at T = 16, 32, 64 in both spacings, and
    ddim first order (doubling T cuts its error to <= 0.65)."""
    for (T, sp, s), v in sorted(rms.items()):
        print(f"T={T} spacing={sp} {s}: rms {v:.4e}")
    for T in (16, 32, 64):
        for sp in ("t", "logsnr"):
            assert rms[T, sp, "dpmpp2m"] <= 0.5 * rms[T, sp, "ddim"], (T, sp)
    for T in (16, 32):
        for sp in ("t", "logsnr"):
            assert rms[2 * T, sp, "ddim"] <= 0.65 * rms[T, sp, "ddim"], (T, sp)


def test_second_order_last_step_would_lose(rms):
    """Why the last dpmpp2m step is first order: with the final (big) logSNR
    step extrapolated, the 2M error is no longer half of ddim's."""
    ratios = {(T, sp): _rms_2m_without_lower_order_final(T, sp) / rms[T, sp, "ddim"]
              for T in (16, 32, 64) for sp in ("t", "logsnr")}
    print({k: round(v, 3) for k, v in ratios.items()})
    assert not all(v <= 0.5 for v in ratios.values()), ratios


# ---------------------------------------------------------- sampler paths
@pytest.fixture
def one_thread():
    """Runs of one chain in batches of different sizes are compared below.  The
    first step sits at logSNR -20, where x0 = (z - sigma eps) / alpha divides
    by alpha = 4.5e-5: the last-bit differences of a multi-threaded CPU forward
    between batch sizes (its work split depends on the batch) come out at
    2.6e-5 in the result with 8 threads -- for the ancestral chain at 4 steps
    just as for the solvers -- and at exactly 0 with one thread.  One thread
    takes that host-dependent term out; the tolerances stay the sampler's."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("solver,eta", [("dpmpp2m", 0.0), ("ddim", 0.5)])
def test_sample_groups_equals_per_object_sample(solver, eta, one_thread):
    m = _signal_model()
    g = torch.Generator().manual_seed(11)
    img = torch.rand(5, 3, 16, 16, generator=g) * 2 - 1
    w = torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0])
    group = torch.tensor([0, 0, 1, 1, 1])
    kw = {"timesteps": 4, "seed": 7, "solver": solver, "eta": eta}
    ref = []
    for gi, (lo, hi) in enumerate(SPANS):
        smp = DiffusionSampler(m, chain_offset=lo, **kw)
        ref.append(smp.sample(_records(img, gi), TARGET_R[gi], TARGET_T[gi], K, w[lo:hi]))
    ref = torch.cat(ref)
    assert torch.isfinite(ref).all()
    smp = DiffusionSampler(m, **kw)
    out = smp.sample_groups([_records(img, 0), _records(img, 1)], TARGET_R, TARGET_T, K, w, group)
    torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-5)
    smp = DiffusionSampler(m, share_cond=False, **kw)
    out2 = smp.sample_groups([_records(img, 0), _records(img, 1)], TARGET_R, TARGET_T, K[None].expand(2, 3, 3), w,
                             group)
    torch.testing.assert_close(out2, ref, rtol=1e-4, atol=1e-5)
    # another solver is another chain
    other = DiffusionSampler(m, timesteps=4, seed=7).sample_groups([_records(img, 0), _records(img, 1)], TARGET_R,
                                                                   TARGET_T, K, w, group)
    assert (other - ref).abs().max() > 1e-3


@pytest.mark.parametrize("solver,eta", [("dpmpp2m", 0.0), ("ddim", 0.5)])
def test_history_restarts_with_every_sample(solver, eta, one_thread):
    """A second `sample` on the same sampler == a fresh sampler's whose
    choice_rng is at the same state."""
    m = _signal_model()
    g = torch.Generator().manual_seed(11)
    img = torch.rand(2, 3, 16, 16, generator=g) * 2 - 1
    w = torch.tensor([0.0, 3.0])
    kw = {"timesteps": 4, "seed": 7, "solver": solver, "eta": eta}
    smp = DiffusionSampler(m, **kw)
    first = smp.sample(_records(img, 0), TARGET_R[0], TARGET_T[0], K, w)
    rng_state = smp.choice_rng.getstate()
    second = smp.sample(_records(img, 0), TARGET_R[1], TARGET_T[1], K, w)
    fresh = DiffusionSampler(m, **kw)
    fresh.choice_rng.setstate(rng_state)
    ref = fresh.sample(_records(img, 0), TARGET_R[1], TARGET_T[1], K, w)
    torch.testing.assert_close(second, ref, rtol=1e-4, atol=1e-5)
    assert (second - first).abs().max() > 1e-3


def test_step_with_and_without_state():
    m = _signal_model()
    g = torch.Generator().manual_seed(5)
    b = 2
    x = torch.rand(b, 3, 16, 16, generator=g) * 2 - 1
    z = torch.randn(b, 3, 16, 16, generator=g)
    w = torch.tensor([0.0, 2.0])
    R = torch.stack([TARGET_R[1], TARGET_R[0]])[None].expand(b, 2, 3, 3).contiguous()
    T = torch.stack([TARGET_T[1], TARGET_T[0]])[None].expand(b, 2, 3).contiguous()
    Kb = K[None].expand(b, 3, 3).contiguous()
    smp = DiffusionSampler(m, timesteps=8, seed=3, solver="dpmpp2m")
    k = 4
    # no state, or a state before its first step: first order (= the ddim eta 0 step)
    a = smp.step(z, x, R, T, Kb, w, k, shared=True)
    st = SolverState()
    a2 = smp.step(z, x, R, T, Kb, w, k, shared=True, state=st)
    d = DiffusionSampler(m, timesteps=8, seed=3, solver="ddim").step(z, x, R, T, Kb, w, k, shared=True)
    torch.testing.assert_close(a, d, rtol=1e-4, atol=1e-5)
    assert torch.equal(a, a2) and st.x0_prev is not None and st.x0_prev.abs().max() <= 1.0
    # with history: z' = first-order z' + k1 (x0_prev - x0)
    x0 = st.x0_prev.clone()
    hist = torch.rand(b, 3, 16, 16, generator=g) * 2 - 1
    st.x0_prev = hist.clone()
    c = smp.step(z, x, R, T, Kb, w, k, shared=True, state=st)
    k1 = smp.solver_params(k)[5]
    torch.testing.assert_close(c, a + k1 * (hist - x0), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(st.x0_prev, x0, rtol=0.0, atol=0.0)
    # the ancestral solver ignores the state
    anc = DiffusionSampler(m, timesteps=8, seed=3)
    st = SolverState()
    assert torch.equal(anc.step(z, x, R, T, Kb, w, k, shared=True, state=st), anc.step(z, x, R, T, Kb, w, k, shared=True))
    assert st.x0_prev is None


def test_argument_validation():
    m = torch.nn.Linear(1, 1)
    for kw in ({"solver": "euler"}, {"spacing": "karras"}, {"solver": "ddim", "eta": 1.5},
               {"solver": "ddim", "eta": -0.1}, {"solver": "dpmpp2m", "eta": 0.5},
               {"solver": "ddim", "ref_quirk": True}, {"solver": "dpmpp2m", "ref_quirk": True}):
        with pytest.raises(ValueError):
            DiffusionSampler(m, 4, **kw)
    DiffusionSampler(m, 4, solver="ddim", eta=1.0, spacing="logsnr")
    DiffusionSampler(m, 4, ref_quirk=True, spacing="logsnr")
    lam, lam_next = _schedule(4, "t")
    for solver, eta in (("ancestral", 0.0), ("ddim", 2.0), ("dpmpp2m", 0.1)):
        with pytest.raises(ValueError):
            solver_row(lam, lam_next, 1, solver, eta, LAM0)


def test_ancestral_path_unchanged():
    m = _signal_model()
    outs = [smp.sample(*_sample_args()) for smp in (DiffusionSampler(m, 3, seed=7),
                                                    DiffusionSampler(m, 3, seed=7, solver="ancestral", spacing="t"))]
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    smp = DiffusionSampler(m, 3, seed=7)
    assert (smp.solver, smp.eta, smp.spacing) == ("ancestral", 0.0, "t")


# -------------------------------------------------------------------- CLI
@pytest.fixture(scope="module")
def srn_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("srn_solver"))
    write_synthetic_srn(root, num_instances=20, num_views=4, size=16, seed=2)
    return root


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ckpt_solver"))
    cfg = make_config(None, dict(TINY_OV, **{"data.synthetic": True, "out_dir": out}))
    tr = Trainer(cfg, DistContext())
    with torch.no_grad():
        for p in tr.model.parameters():
            if p.abs().sum() == 0:
                p.normal_(0, 0.05)
    tr.save("latest.pt", epoch=0)
    tr.logger.close()
    return os.path.join(out, "latest.pt")


def test_evaluate_cli_sampler_flags(srn_root, checkpoint, tmp_path):
    import evaluate as evaluate_cli
    common = ["--model", checkpoint, "--data", srn_root, "--split", "val", "--instances", "2", "--views", "1",
              "--w", "0,2", "--timesteps", "4", "--imgsize", "16", "--backend", "torch", "--seed", "4", "--batch", "2"]
    res = {}
    for name, extra in (("2m", ["--sampler", "dpmpp2m"]), ("ddim", ["--sampler", "ddim", "--eta", "0.5", "--spacing", "logsnr"]),
                        ("default", [])):
        out = str(tmp_path / name)
        evaluate_cli.main(common + extra + ["--out", out])
        res[name] = json.load(open(os.path.join(out, "metrics.json")))
    a = res["2m"]["args"]
    assert (a["sampler"], a["eta"], a["spacing"], a["timesteps"]) == ("dpmpp2m", 0.0, "t", 4)
    a = res["ddim"]["args"]
    assert (a["sampler"], a["eta"], a["spacing"]) == ("ddim", 0.5, "logsnr")
    a = res["default"]["args"]
    assert (a["sampler"], a["eta"], a["spacing"]) == ("ancestral", 0.0, "t")
    assert res["2m"]["n_images"] == 4 and all(math.isfinite(r["mse"]) for r in res["2m"]["per_image"])
    assert [r["mse"] for r in res["2m"]["per_image"]] != [r["mse"] for r in res["default"]["per_image"]]
    with pytest.raises(SystemExit):
        evaluate_cli.parse(["--sampler", "euler"])
