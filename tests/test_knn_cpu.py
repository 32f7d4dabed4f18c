"""ops.image_knn on the CPU (the exact torch form, the oracle of csrc/knn.hip)
against a brute-force loop over Python ints, the argument rules, closed forms of
engine.knn_block, engine.nearest_train, and the --knn / --knn_train path of
evaluate.py."""
import json
import os

import pytest
import torch

from distributed_3d_diffusion_pytorch_amd import ops
from distributed_3d_diffusion_pytorch_amd.data import procedural as P
from distributed_3d_diffusion_pytorch_amd.engine import knn_block, nearest_train
from distributed_3d_diffusion_pytorch_amd.ops import torch_impl as T


def test_torch_form_equals_brute_force():
    g = torch.Generator().manual_seed(0)
    a = torch.rand(4, 3, 3, 3, generator=g) * 2.4 - 1.2                        # fp32, some beyond the clamp
    b = torch.randint(0, 256, (6, 3, 3, 3), dtype=torch.uint8, generator=g)
    b[4] = b[1]                                                                # a tie: the lower index first
    ua, ub = T.image_map_u8(a).reshape(4, -1).tolist(), b.reshape(6, -1).tolist()
    full = [[sum((x - y) ** 2 for x, y in zip(ua[i], ub[j])) for j in range(6)] for i in range(4)]
    radius = torch.tensor([full[0][0], -1, full[1][2], full[2][3] - 1, 10 ** 9, 0])
    d2, idx, inside = ops.image_knn(a, b, k=2, radius=radius)
    for i in range(4):
        top = sorted((full[i][j], j) for j in range(6))[:2]
        assert d2[i].tolist() == [t[0] for t in top] and idx[i].tolist() == [t[1] for t in top]
        assert int(inside[i]) == sum(full[i][j] <= int(radius[j]) for j in range(6))
    assert torch.equal(T.image_knn(a, b, k=2, chunk=4)[1], idx)                # chunks of b do not change the order
    x = T.image_map_u8(a)
    d2s, idxs = ops.image_knn(x, x, k=3, exclude_self=True)
    assert (idxs != torch.arange(4)[:, None]).all() and (d2s[:, 1:] >= d2s[:, :-1]).all()


X = torch.zeros(4, 3, 8, 8)
BAD = {"k 0": dict(k=0), "k 9": dict(k=9), "k not an int": dict(k=2.0), "k above M": dict(k=5),
       "k above M - 1": dict(k=4, exclude_self=True), "shape mismatch": dict(b=torch.zeros(4, 3, 8, 4)),
       "not 3 channels": dict(a=torch.zeros(4, 1, 8, 8)), "dtype": dict(a=X.double()), "not a tensor": dict(b=[1.0]),
       "D above 131071": dict(a=torch.zeros(1, 3, 256, 256, dtype=torch.uint8),
                              b=torch.zeros(4, 3, 256, 256, dtype=torch.uint8)),
       "device": dict(b=X.to("meta")), "radius dtype": dict(radius=torch.zeros(4)),
       "radius shape": dict(radius=torch.zeros(3, dtype=torch.int64))}


@pytest.mark.parametrize("name", BAD)
def test_bad_arguments_raise(name):
    assert "image_knn" in ops.__all__
    with pytest.raises(ValueError):
        ops.image_knn(**dict(dict(a=X, b=X, k=2), **BAD[name]))


@pytest.fixture(scope="module")
def real():
    n, objs = 12, list(range(1, 13))
    K = P.srn_intrinsics()[None].expand(n, 3, 3).contiguous()
    return T.scene_render(P.procedural_scene(1234, objs), *P.procedural_pose(1234, objs, [0] * n), K, 16, 16,
                          aa=2).contiguous()


def test_knn_block_closed_forms(real):
    n = real.shape[0]
    assert int(ops.image_knn(real, real, k=1, exclude_self=True)[0].min()) > 0       # pairwise distinct
    blk = knn_block([real.clone(), -real, real[3:4].repeat(n, 1, 1, 1)], real, [0.0, 1.0, 2.0], k=3)
    assert (blk["k"], blk["n_images"]) == (3, n) and set(blk["split_floor"]) == set(blk["per_w"]["0"])
    same, neg, one = (blk["per_w"][w] for w in ("0", "1", "2"))
    assert (same["precision"], same["recall"], same["coverage"]) == (1.0, 1.0, 1.0)
    assert (neg["precision"], neg["recall"], neg["coverage"], neg["density"]) == (0.0, 0.0, 0.0, 0.0)
    assert one["precision"] == 1.0 and one["recall"] == 1.0 / n
    with pytest.raises(ValueError):
        knn_block([real[:3]], real[:3], [0.0], k=3)


def test_nearest_train_chunking(real):
    g = torch.Generator().manual_seed(1)
    train = torch.randint(0, 256, (10, 3, 16, 16), dtype=torch.uint8, generator=g)
    train[7] = train[2]                                                              # a tie across the two chunks
    labels = [(f"obj{j // 2}", j % 2) for j in range(10)]
    d2, near = nearest_train(real, [(train[:4], labels[:4]), (train[4:], labels[4:])], k=4)
    ref_d2, ref_idx = ops.image_knn(real, train, k=4)
    assert torch.equal(d2, ref_d2) and near == [[labels[j] for j in row] for row in ref_idx.tolist()]


def test_cli(tmp_path):
    """evaluate.py --knn --knn_train writes both blocks; without the flags metrics.json has neither."""
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
    res = evaluate_cli.run(evaluate_cli.parse(common + ["--knn", "--knn_k", "1", "--knn_train", "3", "--knn_train_top",
                                                        "2", "--out", ev]))
    with open(os.path.join(ev, "metrics.json")) as f:
        saved = json.load(f)
    knn, mem = saved["knn"], saved["memorisation"]
    assert knn == res["knn"] and mem == res["memorisation"]
    assert (knn["k"], knn["n_images"]) == (1, 4) and set(knn["per_w"]) == {"0", "2"} == set(mem["per_w"])
    for d in list(knn["per_w"].values()) + [knn["split_floor"]]:
        assert set(d) == {"precision", "recall", "density", "coverage"} and all(0.0 <= v for v in d.values())
    assert len(mem["rows"]) == 8 and mem["gt_mse_nn_mean"] > 0
    for r in mem["rows"]:
        assert len(r["neighbours"]) == 2 and r["neighbours"][0]["mse"] <= r["neighbours"][1]["mse"]
        assert all(nb["view"] in (0, 1, 2) and nb["instance"].startswith("proc-4-") for nb in r["neighbours"])
    assert all(0.0 <= d["frac_closer_to_train"] <= 1.0 and d["mse_nn_mean"] > 0 for d in mem["per_w"].values())
    ev0 = str(tmp_path / "eval0")
    res0 = evaluate_cli.run(evaluate_cli.parse(common + ["--out", ev0]))
    with open(os.path.join(ev0, "metrics.json")) as f:
        assert not {"knn", "memorisation"} & (set(json.load(f)) | set(res0))
    with pytest.raises(SystemExit):
        evaluate_cli.parse(["--knn_k", "9"])
