"""ops.sliced_wasserstein on the CPU (the float64 torch form, the oracle of
csrc/swd.hip): the properties a distribution metric must have on procedural
renders, the argument rules, and the ``--swd`` path of evaluate.py."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from distributed_3d_diffusion_pytorch_amd import ops
from distributed_3d_diffusion_pytorch_amd.data import procedural as P
from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T

KW = dict(levels=3, patches=32, dirs=64, seed=7)


def render(view, n=24, size=32):
    objs = list(range(1, n + 1))
    K = P.srn_intrinsics()[None].expand(n, 3, 3).contiguous()
    return T.scene_render(P.procedural_scene(1234, objs), *P.procedural_pose(1234, objs, [view] * n), K, size, size,
                          aa=2).contiguous()


def blur(x):
    g = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    k = (g[:, None] * g[None, :])[None, None].expand(3, 1, 5, 5)
    return F.conv2d(F.pad(x, (2, 2, 2, 2), mode="reflect"), k, groups=3).contiguous()


@pytest.fixture(scope="module")
def real():
    return render(0)


def test_metric_properties(real):
    """The issue's table: identical sets score exactly 0; a blur costs most at the finest level; two blurs cost more
    than one at every level (the fp64 prototype of the rule: 0.105 0.040 0.018 and 0.149 0.062 0.030)."""
    one, two = blur(real), blur(blur(real))
    noise = (real + 0.1 * torch.randn(real.shape, generator=torch.Generator().manual_seed(0))).clamp(-1, 1)
    res = {name: ops.sliced_wasserstein(x, real, **KW) for name, x in
           (("self", real.clone()), ("view 1", render(1)), ("blur", one), ("two blurs", two), ("noise", noise))}
    for name, v in res.items():
        print(name, [f"{x:.4f}" for x in v.tolist()])
        assert v.dtype == torch.float64 and v.shape == (3,) and torch.isfinite(v).all() and (v >= 0).all()
    assert torch.equal(res["self"], torch.zeros(3, dtype=torch.float64))
    assert res["blur"][0] > res["blur"][2] and res["two blurs"][0] > res["two blurs"][2]
    assert (res["two blurs"] > res["blur"]).all()
    assert torch.equal(ops.sliced_wasserstein(one, real, **KW), res["blur"])
    # a ready direction tensor is what the int builds; levels=None is the most with a coarsest side >= 16
    dirs = T.swd_directions(7, 2, 64)
    assert torch.allclose(dirs.norm(dim=-1), torch.ones(2, 64, dtype=torch.float64), atol=1e-14)
    assert torch.equal(ops.sliced_wasserstein(one, real, patches=32, dirs=dirs, seed=7),
                       ops.sliced_wasserstein(one, real, levels=2, patches=32, dirs=64, seed=7))


BAD = {"shape mismatch": dict(b=torch.zeros(4, 3, 32, 16)), "not 3 channels": dict(a=torch.zeros(4, 2, 32, 32)),
       "dtype": dict(a=torch.zeros(4, 3, 32, 32, dtype=torch.float64)),
       "device": dict(b=torch.zeros(4, 3, 32, 32).to("meta")),
       "contiguity": dict(a=torch.zeros(4, 3, 32, 32).transpose(-1, -2)), "not a tensor": dict(b=[1.0]),
       "levels 0": dict(levels=0), "levels not an int": dict(levels=1.5), "not divisible": dict(levels=7),
       "coarsest below 7": dict(levels=4),
       "side above 128": dict(a=torch.zeros(1, 3, 256, 256), b=torch.zeros(1, 3, 256, 256)),
       "patches 0": dict(patches=0), "too many descriptors": dict(patches=4097), "dirs 0": dict(dirs=0),
       "dirs shape": dict(dirs=torch.zeros(2, 8, 146, dtype=torch.float64)),
       "dirs levels": dict(dirs=torch.zeros(3, 8, 147, dtype=torch.float64)),
       "dirs dtype": dict(dirs=torch.zeros(2, 8, 147))}


@pytest.mark.parametrize("name", BAD)
def test_bad_arguments_raise(name):
    x = torch.zeros(4, 3, 32, 32)
    assert "sliced_wasserstein" in ops.__all__
    with pytest.raises(ValueError):
        ops.sliced_wasserstein(**dict(dict(a=x, b=x, levels=2, patches=4096, dirs=8, seed=0), **BAD[name]))


def test_cli(tmp_path):
    """evaluate.py --swd writes the block with finite values; without the flag metrics.json has no such key."""
    import evaluate as evaluate_cli
    from distributed_3d_diffusion_pytorch_amd.config import make_config
    from distributed_3d_diffusion_pytorch_amd.engine import Trainer
    from distributed_3d_diffusion_pytorch_amd.parallel import DistContext
    run = str(tmp_path / "run")
    tr = Trainer(make_config(None, {"model.ch": 32, "model.emb_ch": 64, "model.H": 16, "model.W": 16,
                                    "data.imgsize": 16, "global_batch": 2, "dtype": "fp32", "backend": "torch",
                                    "log_every": 1, "ckpt_every": 0, "data.num_workers": 0, "data.procedural": True,
                                    "out_dir": run}), DistContext())
    tr.save("latest.pt", epoch=0)
    tr.logger.close()
    common = ["--model", os.path.join(run, "latest.pt"), "--procedural", "--proc_seed", "4", "--proc_objects", "40",
              "--instances", "2", "--views", "1,2", "--w", "0,2", "--timesteps", "2", "--imgsize", "16", "--backend",
              "torch"]
    ev = str(tmp_path / "eval")
    res = evaluate_cli.run(evaluate_cli.parse(common + ["--swd", "--swd_patches", "9", "--swd_dirs", "16", "--samples",
                                                        "2", "--out", ev]))
    with open(os.path.join(ev, "metrics.json")) as f:
        block = json.load(f)["swd"]
    assert block == res["swd"]
    assert set(block) == {"levels", "patches", "dirs", "seed", "n_images", "per_w", "split_floor"}
    assert (block["levels"], block["patches"], block["dirs"], block["seed"], block["n_images"]) == (1, 9, 16, 0, 4)
    for d in list(block["per_w"].values()) + [block["split_floor"]]:
        assert len(d["levels"]) == 1 and all(v == v and 0 < v < float("inf") for v in d["levels"] + [d["mean"]])
    assert set(block["per_w"]) == {"0", "2"}
    ev0 = str(tmp_path / "eval0")
    res0 = evaluate_cli.run(evaluate_cli.parse(common + ["--out", ev0]))
    with open(os.path.join(ev0, "metrics.json")) as f:
        assert "swd" not in json.load(f) and "swd" not in res0
    with pytest.raises(SystemExit):
        evaluate_cli.parse(["--swd_dirs", "0"])
