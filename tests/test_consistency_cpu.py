"""Geometry-aware evaluation on the CPU (ops.view_consistency, the float64
torch form; engine.evaluate's consistency path): the op against a scalar
fp64 loop written from the rule, the ground truth's own reprojection error,
the sensitivity to a known offset, the exact cases, bad arguments, and the
evaluation path and CLI on a tiny model."""
import json
import math
import os

import pytest
import torch

from distributed_3d_diffusion_pytorch_amd import ops
from distributed_3d_diffusion_pytorch_amd.data import procedural_objects, procedural_scene
from distributed_3d_diffusion_pytorch_amd.data import procedural as P
from helpers import tiny_model

SEED = 1234
INF = float("inf")


def pairs(objs, size, src_view=0, tgt_view=1):
    """Ground-truth pairs of the objects: view 0 -> view 1, aa 3."""
    n = len(objs)
    src, Rs, ts, K = P.render_views(SEED, objs, [src_view] * n, size)
    tgt, Rt, tt, _ = P.render_views(SEED, objs, [tgt_view] * n, size)
    return {"table": procedural_scene(SEED, objs), "K": K, "R_src": Rs, "t_src": ts, "img_src": src, "R_tgt": Rt,
            "t_tgt": tt, "img_tgt": tgt}


def noise(shape, amp, seed=0):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * amp


# ------------------------------------------------- the scalar fp64 reference
def _inv3(m):
    (a, b, c), (d, e, f), (g, h, i) = m
    A, B, C = e * i - f * h, f * g - d * i, d * h - e * g
    det = a * A + b * B + c * C
    adj = [[A, c * h - b * i, b * f - c * e], [B, a * i - c * g, c * d - a * f], [C, b * g - a * h, a * e - b * d]]
    return [[x / det for x in row] for row in adj]


def _mv(m, x):
    return [m[r][0] * x[0] + m[r][1] * x[1] + m[r][2] * x[2] for r in range(3)]


def _trace(tab, o, d):
    """(t, surface id) of the nearest hit of o + t d; (inf, -1) on a miss."""
    best, sid = INF, -1
    for p, s in enumerate(tab):
        kind = int(s[15])
        if kind == 0:
            continue
        A = [s[0:3], s[3:6], s[6:9]]
        oo = _mv(A, [o[k] - s[9 + k] for k in range(3)])
        q = _mv(A, d)
        if kind == 1:
            a = sum(x * x for x in q)
            b = sum(x * y for x, y in zip(oo, q))
            c = sum(x * x for x in oo) - 1.0
            disc = b * b - a * c
            if not disc > 0.0:
                continue
            t, face = (-b - math.sqrt(disc)) / a, 0
        else:
            tmin, tmax, ax = -INF, INF, 0
            for k in range(3):
                inv = 1.0 / q[k] if q[k] != 0.0 else math.copysign(INF, q[k])
                t1, t2 = (-1.0 - oo[k]) * inv, (1.0 - oo[k]) * inv
                if min(t1, t2) > tmin:
                    tmin, ax = min(t1, t2), k
                tmax = min(tmax, max(t1, t2))
            if not tmin < tmax:
                continue
            sg = -1.0 if q[ax] > 0.0 else 1.0
            t, face = tmin, 1 + 2 * ax + (1 if sg > 0 else 0)
        if t > 0.0 and t < best:
            best, sid = t, 8 * p + face
    return best, sid


def scalar_reference(table, K, R_src, t_src, img_src, R_tgt, t_tgt, img_tgt, ref=None):
    """stats [N][8] and classes [N][H][W], one pixel at a time in Python floats."""
    N, _, H, W = img_tgt.shape
    stats, classes = [], []
    for n in range(N):
        tab = table[n].tolist()
        Ks = [[x * W / 128 for x in K[n, 0].tolist()], [x * H / 128 for x in K[n, 1].tolist()], K[n, 2].tolist()]
        Ki = _inv3(Ks)
        Rs, Rt, ts, tt = R_src[n].tolist(), R_tgt[n].tolist(), t_src[n].tolist(), t_tgt[n].tolist()
        RsT = [[Rs[c][r] for c in range(3)] for r in range(3)]
        src, tgt = img_src[n].double().tolist(), img_tgt[n].double().tolist()
        rf = ref[n].double().tolist() if ref is not None else None

        def ray(R, u, v):
            c = _mv(Ki, [u, v, 1.0])
            nrm = math.sqrt(sum(x * x for x in c))
            return _mv(R, [x / nrm for x in c])

        st, cl = [0.0] * 8, [[0] * W for _ in range(H)]
        for py in range(H):
            for px in range(W):
                d = ray(Rt, px + 0.5, py + 0.5)
                tau, s0 = _trace(tab, tt, d)
                k = 0
                if s0 >= 0:
                    k = 1
                    X = [tt[i] + tau * d[i] for i in range(3)]
                    e = [X[i] - ts[i] for i in range(3)]
                    dist = math.sqrt(sum(x * x for x in e))
                    c = _mv(RsT, e)
                    kc = _mv(Ks, c)
                    u, v = kc[0] / kc[2], kc[1] / kc[2]
                    x0, y0 = math.floor(u - 0.5), math.floor(v - 0.5)
                    tau1, s1 = _trace(tab, ts, [x / dist for x in e])
                    if (c[2] > 0 and 0 <= x0 and x0 + 1 <= W - 1 and 0 <= y0 and y0 + 1 <= H - 1
                            and abs(tau1 - dist) < 1e-9 and s1 == s0):
                        k = 2
                        corners = [_trace(tab, tt, ray(Rt, px + i, py + j))[1] for j in (0, 1) for i in (0, 1)]
                        lattice = [_trace(tab, ts, ray(Rs, x0 + i, y0 + j))[1] for j in (0, 1, 2) for i in (0, 1, 2)]
                        if all(s == s0 for s in corners + lattice):
                            k = 3
                            fx, fy = (u - 0.5) - x0, (v - 0.5) - y0
                            for ch in range(3):
                                a = src[ch]
                                warp = ((1 - fx) * (1 - fy) * a[y0][x0] + fx * (1 - fy) * a[y0][x0 + 1]
                                        + (1 - fx) * fy * a[y0 + 1][x0] + fx * fy * a[y0 + 1][x0 + 1])
                                st[7] += ((tgt[ch][py][px] - warp) / 2) ** 2
                            st[3] += 1
                cl[py][px] = k
                st[min(k, 2)] += 1
                if rf is not None:
                    st[4 + min(k, 2)] += sum(((tgt[ch][py][px] - rf[ch][py][px]) / 2) ** 2 for ch in range(3))
        stats.append(st)
        classes.append(cl)
    return stats, classes


def test_op_matches_the_scalar_loop():
    """(2,12,12), objects 1 and 3 (six primitives, both kinds): class planes
    and counts equal, sums to 1e-9 relative."""
    a = pairs([1, 3], 12)
    ref = a["img_tgt"]
    a["img_tgt"] = (ref + noise(ref.shape, 0.1)).contiguous()
    stats, cls = ops.view_consistency(**a, ref=ref, return_class=True)
    want, wcls = scalar_reference(**a, ref=ref)
    assert stats.shape == (2, 8) and stats.dtype == torch.float64
    assert cls.shape == (2, 12, 12) and cls.dtype == torch.int32
    assert torch.equal(cls, torch.tensor(wcls, dtype=torch.int32))
    assert set(cls.flatten().tolist()) == {0, 1, 2, 3}
    want = torch.tensor(want, dtype=torch.float64)
    assert torch.equal(stats[:, :4], want[:, :4])
    rel = ((stats[:, 4:] - want[:, 4:]).abs() / want[:, 4:]).max().item()
    print(f"sums against the scalar loop: relative {rel:.3e}")
    assert (want[:, 4:] > 0).all() and rel <= 1e-9
    # without ref: columns 4..6 are 0, the rest is the same; without the class plane: the same stats
    plain = ops.view_consistency(**a)
    assert torch.equal(plain[:, :4], stats[:, :4]) and torch.equal(plain[:, 7], stats[:, 7])
    assert (plain[:, 4:7] == 0).all()


# ------------------------------------------------------- 24 objects, 24 x 24
@pytest.fixture(scope="module")
def gt24():
    """Ground truth on both sides, ref = ground truth + noise; computed once."""
    a = pairs(list(range(24)), 24)
    ref = (a["img_tgt"] + noise(a["img_tgt"].shape, 0.1, 1)).contiguous()
    stats, cls = ops.view_consistency(**a, ref=ref, return_class=True)
    return a, ref, stats, cls


def test_ground_truth_is_consistent(gt24):
    a, ref, st, cls = gt24
    n_clean, total = st[:, 3].sum().item(), st[:, 7].sum().item()
    psnr = 10 * math.log10(3 * n_clean / total)
    hit = st[:, 1] + st[:, 2]
    print(f"clean / co-visible / hit {int(n_clean)} / {int(st[:, 2].sum())} / {int(hit.sum())}, pooled clean "
          f"reprojection PSNR {psnr:.2f} dB; (hit, co-visible, clean) of objects 0..4: "
          f"{[(int(hit[i]), int(st[i, 2]), int(st[i, 3])) for i in range(5)]}")
    assert psnr >= 50.0
    assert n_clean >= 300
    assert torch.equal(st[:, :3].sum(1), torch.full((24,), 24.0 * 24.0, dtype=torch.float64))
    assert (st[:, 3] <= st[:, 2]).all()
    for k in range(4):                                                 # the class plane is what was counted
        counted = st[:, k] if k < 2 else (st[:, 2] - st[:, 3] if k == 2 else st[:, 3])
        assert torch.equal((cls == k).flatten(1).sum(1).double(), counted)
    whole = ((a["img_tgt"].double() - ref.double()) / 2).square().flatten(1).sum(1)
    assert ((st[:, 4:7].sum(1) - whole).abs() / whole).max() <= 1e-12
    assert (st[:, 4:7] > 0).all()


def test_offset_is_measured(gt24):
    """tgt = ground truth + 0.4: the rms on the clean pixels is 0.2 within the
    ground truth's own worst element, sqrt(1.85e-4) = 0.0137."""
    a, _, st0, _ = gt24
    st = ops.view_consistency(**dict(a, img_tgt=a["img_tgt"] + 0.4))
    assert torch.equal(st[:, :4], st0[:, :4])                          # the classes do not read the images
    rms = math.sqrt(st[:, 7].sum().item() / (3 * st[:, 3].sum().item()))
    print(f"rms on the clean pixels: {rms:.5f}")
    assert abs(rms - 0.2) <= 0.0137
    for i in (1, 2, 3):                                                # ... and per pair, where there are clean pixels
        assert abs(math.sqrt(st[i, 7].item() / (3 * st[i, 3].item())) - 0.2) <= 0.0137


def test_exact_cases(gt24):
    a = {k: v[:3].clone() for k, v in gt24[0].items()}
    away = lambda R: R * torch.tensor([-1.0, 1.0, -1.0], dtype=R.dtype)  # noqa: E731  (columns 0 and 2 negated)
    st = ops.view_consistency(**dict(a, R_src=away(a["R_src"])))
    assert (st[:, 2] == 0).all() and (st[:, 3] == 0).all() and (st[:, 7] == 0).all()
    assert torch.equal(st[:, 1], gt24[2][:3, 1] + gt24[2][:3, 2]) and (st[:, 1] > 0).all()
    st, cls = ops.view_consistency(**dict(a, R_tgt=away(a["R_tgt"])), return_class=True)
    assert (st[:, 0] == 24 * 24).all() and (st[:, 1:4] == 0).all() and (st[:, 7] == 0).all() and (cls == 0).all()
    st, cls = ops.view_consistency(**dict(a, table=torch.zeros_like(a["table"])), ref=a["img_src"], return_class=True)
    assert (st[:, 0] == 24 * 24).all() and (st[:, 1:4] == 0).all() and (cls == 0).all()
    assert (st[:, 5:] == 0).all() and (st[:, 4] > 0).all()


def test_bad_arguments_raise(gt24):
    a = {k: v[:2] for k, v in gt24[0].items()}
    assert "view_consistency" in ops.__all__
    assert ops.view_consistency(**a).shape == (2, 8)
    bad = [dict(table=a["table"][:, :5]), dict(table=a["table"].float()), dict(table=a["table"][0]),
           dict(K=a["K"][:1]), dict(K=a["K"].float()), dict(R_src=a["R_src"][:, :2]), dict(R_tgt=a["R_tgt"].float()),
           dict(t_src=a["t_src"][:, :2]), dict(t_tgt=a["t_tgt"].float()), dict(img_src=a["img_src"][..., :23]),
           dict(img_src=a["img_src"].double()), dict(img_tgt=a["img_tgt"][:, :2]), dict(img_tgt=a["img_tgt"][0]),
           dict(img_tgt=a["img_tgt"].transpose(-1, -2)), dict(ref=a["img_tgt"].double()),
           dict(ref=a["img_tgt"][:1]), dict(img_src=a["img_src"].to("meta")), dict(K=[1.0])]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.view_consistency(**dict(a, **kw))
    empty = {k: v[:0] for k, v in a.items()}
    st, cls = ops.view_consistency(**empty, return_class=True)
    assert st.shape == (0, 8) and st.dtype == torch.float64 and cls.shape == (0, 24, 24) and cls.dtype == torch.int32
    assert ops.view_consistency(**empty, ref=empty["img_tgt"]).shape == (0, 8)


# ------------------------------------------------------ the evaluation path
FIELDS = ["n_background", "n_disoccluded", "n_covisible", "n_clean", "mse_background", "psnr_background",
          "mse_disoccluded", "psnr_disoccluded", "mse_covisible", "psnr_covisible", "reproj_mse", "reproj_psnr"]


@pytest.fixture(scope="module")
def model():
    return tiny_model().eval()


@pytest.fixture(scope="module")
def objects():
    objs = procedural_objects(SEED, 2, [0, 1, 2], 16, objects=100, device="cpu")
    assert all(o.scene.shape == (6, 16) and o.scene.dtype == torch.float64 for o in objs)
    assert torch.equal(objs[1].scene, procedural_scene(SEED, [19])[0])
    return objs


def test_evaluate_objects_with_consistency(model, objects):
    from distributed_3d_diffusion_pytorch_amd.engine import evaluate_objects
    kw = dict(input_view=0, views=(1, 2), w=(0.0, 2.0), timesteps=2, batch=2, seed=3, keep_images=True)
    rows, images, pair_rows = evaluate_objects(model, objects, consistency=True, **kw)
    assert len(rows) == 2 * 2 * 2 and all(set(FIELDS) <= set(r) for r in rows)
    json.dumps([rows, pair_rows], allow_nan=False)
    for r in rows:
        o = objects[[x.name for x in objects].index(r["instance"])]
        assert r["n_background"] + r["n_disoccluded"] + r["n_covisible"] == 16 * 16
        assert r["n_clean"] <= r["n_covisible"]
        out = images[(r["instance"], r["view"])][[0.0, 2.0].index(r["w"])][None].contiguous()
        st = ops.view_consistency(o.scene[None], o.K[None].double(), o.R[0][None].double(), o.T[0][None].double(),
                                  o.imgs[0][None], o.R[r["view"]][None].double(), o.T[r["view"]][None].double(), out,
                                  o.imgs[r["view"]][None])[0].tolist()
        assert [r["n_background"], r["n_disoccluded"], r["n_covisible"], r["n_clean"]] == [int(x) for x in st[:4]]
        for j, name in enumerate(("background", "disoccluded", "covisible")):
            if st[j] > 0 and st[4 + j] > 0:
                assert abs(r[f"mse_{name}"] - st[4 + j] / (3 * st[j])) <= 1e-12 * r[f"mse_{name}"]
                assert abs(r[f"psnr_{name}"] - 10 * math.log10(1 / r[f"mse_{name}"])) < 1e-9
            else:
                assert r[f"mse_{name}"] is None and r[f"psnr_{name}"] is None
        if st[3] > 0:
            assert abs(r["reproj_mse"] - st[7] / (3 * st[3])) <= 1e-12 * r["reproj_mse"]
        else:
            assert r["reproj_mse"] is None and r["reproj_psnr"] is None
    # one row per ordered pair of generated views of a chain
    assert len(pair_rows) == 4 * 2
    assert {(p["chain"], p["src_view"], p["tgt_view"]) for p in pair_rows} == \
        {(c, a, b) for c in range(4) for a, b in ((1, 2), (2, 1))}
    assert all(set(p) == {"instance", "w", "chain", "src_view", "tgt_view", "n_clean", "mse", "psnr"}
               for p in pair_rows)
    p = pair_rows[0]
    o = objects[0]
    d64 = lambda x: x[None].double()  # noqa: E731
    st = ops.view_consistency(o.scene[None], d64(o.K), d64(o.R[p["src_view"]]), d64(o.T[p["src_view"]]),
                              images[(o.name, p["src_view"])][:1].contiguous(), d64(o.R[p["tgt_view"]]),
                              d64(o.T[p["tgt_view"]]), images[(o.name, p["tgt_view"])][:1].contiguous())[0].tolist()
    assert p["instance"] == o.name and p["chain"] == 0 and p["n_clean"] == int(st[3])
    assert (p["mse"] is None) if st[3] == 0 else abs(p["mse"] - st[7] / (3 * st[3])) <= 1e-12 * p["mse"]
    # one view: no pairs; without the flag: the old two values and the old rows
    assert evaluate_objects(model, objects, consistency=True, **dict(kw, views=(1,)))[2] == []
    old = evaluate_objects(model, objects, **kw)
    assert isinstance(old, tuple) and len(old) == 2
    base = ["instance", "view", "w", "chain", "mse", "psnr", "ssim"]
    assert [list(r) for r in old[0]] == [base] * 8
    assert old[0] == [{k: r[k] for k in base} for r in rows]
    # objects without geometry are refused
    from distributed_3d_diffusion_pytorch_amd.engine import EvalObject
    bare = [EvalObject(o.name, o.imgs, o.R, o.T, o.K) for o in objects]
    assert bare[0].scene is None
    with pytest.raises(ValueError, match="scene"):
        evaluate_objects(model, bare, consistency=True, **kw)
    assert len(evaluate_objects(model, bare, **kw)) == 2


def test_summarize_consistency_pools():
    from distributed_3d_diffusion_pytorch_amd.engine import summarize_consistency
    row = lambda w, nb, nd, nc, ncl, mb, md, mc, mr: {  # noqa: E731
        "w": w, "n_background": nb, "n_disoccluded": nd, "n_covisible": nc, "n_clean": ncl, "mse_background": mb,
        "mse_disoccluded": md, "mse_covisible": mc, "reproj_mse": mr}
    rows = [row(1.0, 10, 4, 6, 2, 0.01, 0.04, 0.02, 0.001), row(1.0, 30, 0, 2, 0, 0.03, None, 0.06, None),
            row(2.0, 5, 5, 0, 0, None, 0.5, None, None)]
    prs = [{"w": 1.0, "n_clean": 3, "mse": 0.002}, {"w": 1.0, "n_clean": 0, "mse": None},
           {"w": 1.0, "n_clean": 1, "mse": 0.006}]
    s = summarize_consistency(rows, prs)
    assert set(s) == {"1", "2"} and set(s["1"]) == {"covisible", "disoccluded", "background", "reproj", "pairs"}
    near = lambda got, n, mse: (got["n"] == n and abs(got["mse"] - mse) < 1e-15  # noqa: E731
                                and abs(got["psnr"] - 10 * math.log10(1 / mse)) < 1e-9)
    assert near(s["1"]["covisible"], 8, (0.02 * 6 + 0.06 * 2) / 8)
    assert near(s["1"]["background"], 40, (0.01 * 10 + 0.03 * 30) / 40)
    assert near(s["1"]["disoccluded"], 4, 0.04)
    assert near(s["1"]["reproj"], 2, 0.001)
    assert near(s["1"]["pairs"], 4, (0.002 * 3 + 0.006) / 4)
    assert s["2"]["covisible"] == {"n": 0, "mse": None, "psnr": None} and near(s["2"]["disoccluded"], 5, 0.5)
    assert s["2"]["background"] == {"n": 5, "mse": None, "psnr": None}
    assert s["2"]["pairs"] == {"n": 0, "mse": None, "psnr": None}
    json.dumps(s, allow_nan=False)


def test_gt_ceiling_is_the_direct_call():
    from distributed_3d_diffusion_pytorch_amd.engine import gt_ceiling
    objects = procedural_objects(SEED, 4, [0, 1, 2], 24, objects=100, device="cpu")    # (at 16 x 16 no pair is clean)
    c = gt_ceiling(objects, 0, (1, 2))
    table = torch.stack([o.scene for o in objects])
    K = torch.stack([o.K for o in objects]).double()
    pose = lambda v: (torch.stack([o.R[v] for o in objects]).double(),  # noqa: E731
                      torch.stack([o.T[v] for o in objects]).double())
    img = lambda v: torch.stack([o.imgs[v] for o in objects])  # noqa: E731

    def direct(ps):
        st = sum(ops.view_consistency(table, K, *pose(a), img(a), *pose(b), img(b)) for a, b in ps)
        return int(st[:, 3].sum()), st[:, 7].sum().item() / (3 * st[:, 3].sum().item())

    for name, ps in (("reproj", [(0, 1), (0, 2)]), ("pairs", [(1, 2), (2, 1)])):
        n, mse = direct(ps)
        print(f"gt_ceiling {name}: {c[name]}")
        assert c[name]["n"] == n and n > 0 and abs(c[name]["mse"] - mse) <= 1e-12 * mse
        assert abs(c[name]["psnr"] - 10 * math.log10(1 / mse)) < 1e-9 and c[name]["psnr"] > 35


def test_cli(tmp_path):
    """evaluate.py --consistency: refused without --procedural; with it,
    metrics.json carries the row fields and the consistency block."""
    import evaluate as evaluate_cli
    from distributed_3d_diffusion_pytorch_amd.config import make_config
    from distributed_3d_diffusion_pytorch_amd.engine import Trainer
    from distributed_3d_diffusion_pytorch_amd.parallel import DistContext
    with pytest.raises(ValueError, match="geometry"):
        evaluate_cli.run(evaluate_cli.parse(["--consistency", "--model", str(tmp_path / "none.pt"), "--out",
                                             str(tmp_path / "refused")]))
    assert not os.path.exists(tmp_path / "refused")
    run = str(tmp_path / "run")
    tr = Trainer(make_config(None, {"model.ch": 32, "model.emb_ch": 64, "model.H": 16, "model.W": 16,
                                    "data.imgsize": 16, "global_batch": 2, "dtype": "fp32", "backend": "torch",
                                    "log_every": 1, "ckpt_every": 0, "data.num_workers": 0, "data.procedural": True,
                                    "out_dir": run}), DistContext())
    tr.save("latest.pt", epoch=0)
    tr.logger.close()
    ev = str(tmp_path / "eval")
    res = evaluate_cli.run(evaluate_cli.parse(
        ["--model", os.path.join(run, "latest.pt"), "--procedural", "--proc_seed", "4", "--proc_objects", "40",
         "--instances", "2", "--views", "1,3", "--w", "0,2", "--timesteps", "2", "--imgsize", "16", "--backend",
         "torch", "--consistency", "--out", ev]))
    with open(os.path.join(ev, "metrics.json")) as f:
        saved = json.load(f)
    assert saved["args"]["consistency"] is True and len(saved["per_image"]) == 8
    assert all(set(FIELDS) <= set(r) for r in saved["per_image"])
    block = saved["consistency"]
    assert set(block) == {"per_w", "pairs", "gt_ceiling"} and set(block["per_w"]) == {"0", "2"}
    assert len(block["pairs"]) == 4 * 2 and set(block["gt_ceiling"]) == {"reproj", "pairs"}
    assert block["per_w"]["0"]["background"]["n"] == sum(r["n_background"] for r in res["per_image"] if r["w"] == 0.0)
    # without the flag the file is what it was
    ev0 = str(tmp_path / "eval0")
    res0 = evaluate_cli.run(evaluate_cli.parse(
        ["--model", os.path.join(run, "latest.pt"), "--procedural", "--proc_seed", "4", "--proc_objects", "40",
         "--instances", "2", "--views", "1,3", "--w", "0,2", "--timesteps", "2", "--imgsize", "16", "--backend",
         "torch", "--out", ev0]))
    assert "consistency" not in res0 and not (set(FIELDS) & set(res0["per_image"][0]))
    assert [r["mse"] for r in res0["per_image"]] == [r["mse"] for r in res["per_image"]]
