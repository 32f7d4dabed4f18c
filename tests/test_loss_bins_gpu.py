"""Loss by noise level on the GPU: diff_loss_rows_k and loss_bins_k against
the torch forms and fp64, under guard bands, and through the validation
loss."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T  # noqa: E402

import guarded as G  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64
LOSS_TYPES = ["l2", "l1", "huber"]


@pytest.fixture(scope="module")
def H():
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    return hip_impl


def _head(B, S, seed=4):
    torch.manual_seed(seed)
    y = (torch.randn(B, S, S, 8, device=DEV) * 1.5).to(BF)
    target = torch.randn(B, 3, S, S, device=DEV)
    return y, target


def _rows64(y, target, loss_type):
    d = y[..., :3].permute(0, 3, 1, 2).double() - target.double()
    ad = d.abs()
    el = {"l2": d * d, "l1": ad, "huber": torch.where(ad < 1, 0.5 * d * d, ad - 0.5)}[loss_type]
    return torch.stack([el.flatten(1).mean(1), (d * d).flatten(1).mean(1)], 1)


def _logsnr(B, seed=7):
    """[B,2] with lambda = +-20 first (when there is room), the rest spread over +-12."""
    g = torch.Generator().manual_seed(seed)
    lam = (torch.rand(B, generator=g) * 2 - 1) * 12
    if B >= 3:
        lam[0], lam[1] = 20.0, -20.0
    return torch.stack([torch.full_like(lam, 20.0), lam], 1).contiguous().to(DEV)


def _rel(a, b):
    return ((a - b).abs() / b.abs().clamp_min(1e-300)).max().item()


# ---------------------------------------------------------------- 1. rows
@pytest.mark.parametrize("loss_type", LOSS_TYPES)
@pytest.mark.parametrize("B,S", [(1, 8), (5, 12), (6, 32), (33, 16)])
def test_diff_loss_rows_kernel(H, B, S, loss_type):
    """diff_loss_rows_k against fp64 on the same bf16 y: 1e-5 relative per row
    (fewer than 100 fp32 roundings enter any partial sum at these sizes, 100 x
    2^-24 ~ 6e-6); the torch form agrees likewise; NaN in channels 3..7 does
    not reach the result; a repeat call is bitwise equal; an example's row is
    bitwise the row of the example run alone."""
    y, target = _head(B, S)
    rows = H.diff_loss_rows(y, target, loss_type)
    assert rows.shape == (B, 2) and rows.dtype == torch.float32
    ref = _rows64(y, target, loss_type)
    err = _rel(rows.double(), ref)
    et = _rel(T.diff_loss_rows(y.float(), target, loss_type).double(), ref)
    print(f"B={B} S={S} {loss_type}: max rel vs fp64 {err:.2e} (torch form {et:.2e})")
    assert err < 1e-5 and et < 1e-5
    if loss_type == "l2":
        assert torch.equal(rows[:, 0], rows[:, 1])
    else:
        assert not torch.equal(rows[:, 0], rows[:, 1])
    yn = y.clone()
    yn[..., 3:] = float("nan")
    assert torch.equal(H.diff_loss_rows(yn, target, loss_type), rows)
    assert torch.equal(H.diff_loss_rows(y, target, loss_type), rows)
    for i in sorted({0, B // 2, B - 1}):
        alone = H.diff_loss_rows(y[i:i + 1].contiguous(), target[i:i + 1].contiguous(), loss_type)
        assert torch.equal(alone[0], rows[i]), i
    with pytest.raises(ValueError):
        H.diff_loss_rows(y, target, "l3")
    with pytest.raises(ValueError):
        H.diff_loss_rows(y.float(), target, loss_type)
    assert H.FALLBACKS == {}, H.FALLBACKS


# ---------------------------------------------------------------- 2. bins
@pytest.mark.parametrize("loss_weight", ["none", "min_snr"])
@pytest.mark.parametrize("prediction", ["eps", "v"])
@pytest.mark.parametrize("B,NB", [(5, 8), (33, 16), (300, 7)])
def test_loss_bins_kernel(H, B, NB, prediction, loss_weight):
    """loss_bins_k fed the same rows and logsnr tensors as the torch form:
    equal counts, the other columns to 1e-12 relative; three calls accumulate;
    bitwise reproducible.  (B = 300: more than one staging chunk of 256.)"""
    g = torch.Generator().manual_seed(B)
    rows = (torch.rand(B, 2, generator=g) * 3 + 0.01).to(DEV)
    logsnr = _logsnr(B)
    kw = dict(prediction=prediction, loss_weight=loss_weight, gamma=5.0, logsnr_min=-20.0, logsnr_max=20.0)
    want = T.loss_bins_add(torch.zeros(NB, 5, dtype=F64), rows.cpu(), logsnr.cpu(), **kw)
    table = torch.zeros(NB, 5, dtype=F64, device=DEV)
    assert H.loss_bins_add(table, rows, logsnr, **kw) is table
    assert torch.equal(table[:, 0].cpu(), want[:, 0]) and table[:, 0].sum().item() == B
    if B >= 3:
        assert table[0, 0].item() >= 1 and table[NB - 1, 0].item() >= 1      # lambda = +20 / -20
    err = _rel(table.cpu(), want)
    print(f"B={B} NB={NB} {prediction} {loss_weight}: max rel {err:.2e}")
    assert err < 1e-12
    rows2 = (rows * 0.5).contiguous()
    H.loss_bins_add(table, rows2, logsnr, **kw)
    H.loss_bins_add(table, rows, logsnr, **kw)
    T.loss_bins_add(want, rows2.cpu(), logsnr.cpu(), **kw)
    T.loss_bins_add(want, rows.cpu(), logsnr.cpu(), **kw)
    assert torch.equal(table[:, 0].cpu(), want[:, 0]) and _rel(table.cpu(), want) < 1e-12
    again = torch.zeros(NB, 5, dtype=F64, device=DEV)
    for r in (rows, rows2, rows):
        H.loss_bins_add(again, r, logsnr, **kw)
    assert torch.equal(again, table)
    with pytest.raises(ValueError):
        H.loss_bins_add(torch.zeros(NB, 5, device=DEV), rows, logsnr, **kw)
    with pytest.raises(ValueError):
        H.loss_bins_add(table, rows, logsnr, prediction="x0")
    assert H.FALLBACKS == {}, H.FALLBACKS


# ------------------------------------------------------------- 3. guards
@pytest.mark.parametrize("loss_type", LOSS_TYPES)
def test_guarded_rows_and_bins(H, loss_type):
    """Both ops at (5, 12) under guard bands and both poisons: guards intact,
    inputs unchanged (the table is the declared in-place output), results
    finite and bit-identical between the poison runs."""
    NB = 8

    def make():
        y, target = _head(5, 12)
        return {"y": y, "target": target, "logsnr": _logsnr(5), "table": torch.ones(NB, 5, dtype=F64, device=DEV)}

    def run(M):
        def fn(y, target, logsnr, table):
            rows = M.diff_loss_rows(y, target, loss_type)
            M.loss_bins_add(table, rows, logsnr, prediction="v", loss_weight="min_snr", gamma=5.0)
            return rows, table
        return fn

    rows, table = G.run_guarded(make, run(H), mutated=("table",))
    src = make()
    rr, rt = run(T)(src["y"].float().cpu(), src["target"].cpu(), src["logsnr"].cpu(), src["table"].cpu())
    assert _rel(rows.double().cpu(), _rows64(src["y"], src["target"], loss_type).cpu()) < 1e-5
    assert torch.equal(table[:, 0].cpu(), rt[:, 0]) and table[:, 0].sum().item() == NB + 5
    # (the rows of the two backends differ in their last fp32 bits, and the table sums them)
    assert _rel(table.cpu(), rt) < 1e-5
    assert H.FALLBACKS == {}, H.FALLBACKS


# --------------------------------------------------------- 4. validation
def test_validation_loss_bins():
    """Trainer.validation_loss(bins=8) at 32 x 32, batch 4, v + min_snr: the
    mean of the plain call, a report over val_batches x batch examples whose
    weighted column sums to it, equal to heldout_loss fed its own table; the
    parameters stay bitwise unchanged."""
    from distributed_3d_diffusion_pytorch_amd.config import make_config
    from distributed_3d_diffusion_pytorch_amd.diffusion import loss_bins_report
    from distributed_3d_diffusion_pytorch_amd.engine import Trainer, heldout_loss
    from distributed_3d_diffusion_pytorch_amd.ops import hip_impl
    from distributed_3d_diffusion_pytorch_amd.parallel import DistContext
    ov = {"model.H": 32, "model.W": 32, "data.imgsize": 32, "global_batch": 4, "data.synthetic": True, "log_every": 0,
          "ckpt_every": 0, "val_batches": 2, "diffusion.prediction": "v", "diffusion.loss_weight": "min_snr"}
    tr = Trainer(make_config(None, ov), DistContext(device=torch.device("cuda", 0)))
    val = tr.make_val_data()
    before = tr.flat.data.clone()
    a = tr.validation_loss(val)
    b, rep = tr.validation_loss(val, bins=8)
    assert a == b and a > 0 and sum(rep["count"]) == 2 * 4
    wsum = sum(c * m for c, m in zip(rep["count"], rep["weighted"]) if c) / 8
    print(f"val_loss {a} from the report {wsum}")
    assert abs(wsum - a) < 1e-5 * a
    table = torch.zeros(8, 5, dtype=F64, device=DEV)
    heldout_loss(tr.model, (tr._to_dev(x) for x in val), tr.cfg.seed, tr.cfg.diffusion, tr.dtype, bins=table)
    assert loss_bins_report(table) == rep
    assert torch.equal(tr.flat.data, before) and tr.model.training
    assert hip_impl.FALLBACKS == {}, hip_impl.FALLBACKS
