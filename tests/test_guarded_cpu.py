"""Self-test of the guard-band instrument (tests/guarded.py) on CPU tensors:
a fake op module whose Python ops misbehave on purpose must be reported, with
the allocation site, and a well-behaved op must pass."""
import re
import types

import pytest
import torch

import guarded as G

FAKE_SRC = '''\
import torch

BF16 = torch.bfloat16


def good(x):
    ws = torch.empty(x.numel() + 3, dtype=torch.float32, device=x.device)      # site: good_ws
    ws[:x.numel()] = x.reshape(-1) * 2
    out = torch.empty_like(x)                                                  # site: good_out
    out.copy_(ws[:x.numel()].view(x.shape))
    acc = torch.zeros(x.shape[-1], dtype=torch.float32, device=x.device)       # site: good_acc
    acc += x.float().sum(0)
    return out, acc


def write_before(x):
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)                 # site: before
    out.copy_(x)
    torch.as_strided(out, (1,), (1,), out.storage_offset() - 1).fill_(1.0)
    return out


def write_after(x):
    out = torch.empty_like(x)                                                  # site: after
    out.copy_(x)
    torch.as_strided(out, (1,), (1,), out.storage_offset() + out.numel()).fill_(1.0)
    return out


def skip_one(x):
    out = torch.empty_like(x)                                                  # site: skip
    out.view(-1)[:-1] = x.reshape(-1)[:-1]
    return out


def read_unwritten(x):
    ws = torch.empty(x.numel(), dtype=torch.float32, device=x.device)          # site: ws
    ws[:-1] = x.reshape(-1)[:-1]
    out = torch.empty((), dtype=torch.float32, device=x.device)                # site: ws_out
    out.copy_(ws.sum())
    return out


def scribble(x):
    out = torch.empty_like(x)                                                  # site: scribble
    out.copy_(x)
    x.view(-1)[2] = 5.0
    return out


class _Twice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = torch.empty_like(x)                                                # site: fwd
        y.copy_(x * 2)
        return y

    @staticmethod
    def backward(ctx, dy):
        dx = torch.empty(dy.shape, dtype=dy.dtype, device=dy.device)           # site: bwd
        dx.copy_(dy * 2)
        torch.as_strided(dx, (1,), (1,), dx.storage_offset() + dx.numel()).fill_(3.0)
        return dx


def twice(x):
    return _Twice.apply(x)


def forms():
    return [torch.empty(2, 3), torch.empty((2, 3)), torch.empty([2, 3]), torch.empty(torch.Size([2, 3])),
            torch.empty(5), torch.empty(()), torch.empty(size=(4,)), torch.zeros(3, 2, dtype=torch.int32),
            torch.zeros((), dtype=torch.float32), torch.empty(7, dtype=torch.uint8),
            torch.empty(3, 5, dtype=BF16, device="cpu"), torch.zeros(torch.Size([2]), dtype=torch.float64),
            torch.empty(0, dtype=torch.float32), torch.empty(max(0, 1), dtype=torch.float32)]


def boom():
    torch.empty(3)
    raise ValueError("boom")
'''


def _line(tag):
    for i, ln in enumerate(FAKE_SRC.splitlines(), 1):
        if ln.rstrip().endswith(f"# site: {tag}"):
            return f"fake_impl.py:{i}"
    raise KeyError(tag)


@pytest.fixture
def fake():
    m = types.ModuleType("fake_impl")
    m.__file__ = "fake_impl.py"
    exec(compile(FAKE_SRC, "fake_impl.py", "exec"), m.__dict__)
    assert m.torch is torch
    yield m
    assert m.torch is torch, "guarded() left its proxy behind"


def _x(dtype=torch.float32):
    def make():
        torch.manual_seed(0)
        return {"x": torch.randn(6, 10).to(dtype)}
    return make


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_well_behaved_op_passes(fake, dtype):
    out, acc = G.run_guarded(_x(dtype), lambda x: fake.good(x), impl=fake)
    x = _x(dtype)()["x"]
    assert torch.equal(out, (x.float() * 2).to(dtype))
    assert torch.allclose(acc, x.float().sum(0))


@pytest.mark.parametrize("op,tag,what", [
    ("write_before", "before", r"front guard, first corrupted byte 4 bytes before the payload"),
    ("write_after", "after", r"back guard, first corrupted byte 0 bytes past the payload's end"),
    ("skip_one", "skip", r"not finite \(poison 0xFF\): 1 of 60 elements, first at 59"),
    ("read_unwritten", "ws", r"1 of 60 elements still poison, first at element 59"),
    ("scribble", "scribble", r"input 'x' modified"),
])
def test_misbehaving_op_is_reported_with_its_site(fake, op, tag, what):
    with pytest.raises(G.GuardError) as e:
        G.run_guarded(_x(), lambda x: getattr(fake, op)(x), impl=fake)
    msg = str(e.value)
    assert re.search(what, msg), msg
    if op == "scribble":
        assert "input 'x' shape=(6, 10) dtype=float32" in msg and "first at byte 8" in msg, msg
    else:
        assert _line(tag) in msg, msg
    assert "shape=" in msg


def test_finite_poison_alone_catches_a_used_uninitialised_value(fake):
    """0x4B is finite: the skipped element and the unwritten workspace word
    show only as a difference between the two runs."""
    for op, tag in (("skip_one", "skip"), ("read_unwritten", "ws_out")):
        src = _x()()
        res = []
        for byte in G.POISON[::-1]:
            with G.guarded(fake, byte) as arena:
                res.append(getattr(fake, op)(G.place(arena, src["x"], "x")))
            arena.check()
        assert torch.isfinite(res[0]).all() and not torch.equal(res[0], res[1]), op


def test_mutated_inputs_may_change_and_guard_of_input_is_checked(fake):
    G.run_guarded(_x(), lambda x: fake.scribble(x), mutated=("x",), impl=fake)

    def past_input(x):
        torch.as_strided(x, (1,), (1,), x.storage_offset() + x.numel()).fill_(0.0)
        return x.clone()

    with pytest.raises(G.GuardError, match=r"input 'x' shape=\(6, 10\).*back guard"):
        G.run_guarded(_x(), past_input, impl=fake)


def test_backward_thread_allocations_are_guarded(fake):
    def make():
        torch.manual_seed(1)
        return {"x": torch.randn(4, 4, requires_grad=True)}

    def fn(x):
        y = fake.twice(x)
        y.backward(torch.ones_like(y))
        return y, x.grad

    with pytest.raises(G.GuardError) as e:
        G.run_guarded(make, fn, impl=fake)
    assert _line("bwd") in str(e.value) and "back guard" in str(e.value), str(e.value)
    assert _line("fwd") not in str(e.value)


def test_proxy_argument_forms(fake):
    with G.guarded(fake, 0x4B) as arena:
        ts = fake.forms()
    arena.check()
    shapes = [(2, 3)] * 4 + [(5,), (), (4,), (3, 2), (), (7,), (3, 5), (2,), (0,), (1,)]
    dtypes = [torch.float32] * 7 + [torch.int32, torch.float32, torch.uint8, torch.bfloat16, torch.float64,
                                     torch.float32, torch.float32]
    assert [tuple(t.shape) for t in ts] == shapes
    assert [t.dtype for t in ts] == dtypes
    for t in ts:
        assert t.is_contiguous() and t.data_ptr() % G.ALIGN == 0
        b = arena.find(t)
        assert t.numel() == 0 or (b is not None and b.site.startswith("fake_impl.py:"))
    assert ts[7].eq(0).all() and ts[8].item() == 0.0 and ts[11].eq(0).all()        # zeros* zero the payload
    assert G._bits(ts[0]).eq(0x4B).all() and ts[9].eq(0x4B).all()                  # empty* stay poison
    assert ts[10].float().eq(13303808.0).all()                                     # bf16 0x4B4B: large, finite
    assert torch.isnan(G.Arena(0xFF).alloc((3,), torch.bfloat16, "cpu")).all()
    assert torch.isnan(G.Arena(0xFF).alloc((3,), torch.float32, "cpu")).all()
    # the tail guard starts at the first byte after the payload (no padding)
    b = arena.find(ts[9])
    assert b.nbytes == 7 and b.raw[b.off + 7].item() == 0x4B and len(arena.bufs) == len(ts)


def test_empty_like_keeps_dense_permuted_strides_and_packs_slices(fake):
    base = torch.randn(2, 3, 4, 5)
    with G.guarded(fake, 0xFF) as arena:
        a = fake.torch.empty_like(base.permute(0, 2, 3, 1))
        b = fake.torch.zeros_like(base[..., 1:3])
    arena.check()
    assert a.stride() == torch.empty_like(base.permute(0, 2, 3, 1)).stride()
    assert b.shape == (2, 3, 4, 2) and b.is_contiguous() and b.eq(0).all()


def test_real_torch_is_restored_on_exception(fake):
    with pytest.raises(ValueError, match="boom"):
        with G.guarded(fake, 0xFF):
            assert fake.torch is not torch
            fake.boom()
    assert fake.torch is torch
    with pytest.raises(TypeError, match="unsupported arguments"):
        with G.guarded(fake, 0xFF):
            fake.torch.empty(3, layout=torch.strided)
    assert fake.torch is torch


def test_guard_size_covers_the_widest_tile():
    assert G.GUARD >= 256 * 1024 * 4 and G.GUARD % G.ALIGN == 0
