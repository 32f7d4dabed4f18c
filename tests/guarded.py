"""Guard-band and poisoned-memory instrument for the HIP ops (a plain helper
module: no fixtures, no pytest settings).

Guard size: GUARD = 1 MiB on each side of every buffer.  Derived from the
widest output tiles of the kernels over the widest row the model has (1024
channels, the 8 x 8 level): 256 rows per tile stored as fp32 (wgrad_tn_k's
256 x 256 tiles in wgrad_gemm.hip, the split-K slabs of the 256-pixel conv
tiles) = 256 x 1024 x 4 B = 1 MiB, and conv_w8_k's 512-pixel tiles (128 x 512,
conv.hip) stored as bf16 = 512 x 1024 x 2 B = 1 MiB.  A kernel that stores
one whole tile of rows past either end of a buffer therefore still lands
inside the guard.

What the instrument sees, and what it does not:

* ``Arena.alloc`` lays every buffer out as ``[guard | payload | guard]`` in
  one uint8 allocation filled with a poison byte.  The payload stays 512-byte
  aligned (what the caching allocator gives the kernels anyway) and is NOT
  padded: the tail guard starts at the first byte after the payload, so a
  one-element overrun is seen.
* ``guarded(H, byte)`` swaps the ``torch`` global of an op module for a proxy
  whose ``empty`` / ``empty_like`` / ``zeros`` / ``zeros_like`` allocate from
  the arena, so every output and workspace of the module is guarded and
  starts out as poison instead of whatever the caching allocator last held
  there.  ``place`` copies a test input into the arena as well.
* Poison bytes: 0xFF (bf16 0xFFFF and fp32 0xFFFFFFFF are NaN) and 0x4B
  (about 1.3e7 in both formats: large, finite).  A kernel that skips part of
  its output, or reads a workspace tail or the bytes past an input and USES
  them, returns NaN in the first run or results that differ between the two.
* An overrun LONGER than the guard (a store more than GUARD bytes away from
  the buffer) is not detected.
* A pure out-of-bounds READ whose value is discarded (masked lanes, a
  prefetch that is never consumed) is invisible: the two runs are bit-equal
  by construction, and that is a pass.

The arena synchronises the device after each fill: the guarded runs are
eager, never graph-captured, and the sync keeps the fill from racing a
kernel on the weight-gradient or conditioning stream.
"""
from __future__ import annotations

import contextlib
import math
import os
import sys
import threading

import torch as _torch

GUARD = 1 << 20          # bytes on each side (see the module docstring)
ALIGN = 512              # payload alignment
POISON = (0xFF, 0x4B)

_SEQ = (tuple, list, _torch.Size)


def _sync(device) -> None:
    if _torch.device(device).type == "cuda":
        _torch.cuda.synchronize()


def _bits(t: _torch.Tensor) -> _torch.Tensor:
    """The tensor's bytes (NaN-safe bitwise comparisons)."""
    return t.detach().contiguous().reshape(-1).view(_torch.uint8)


class GuardError(AssertionError):
    pass


class _Buf:
    __slots__ = ("raw", "off", "nbytes", "site", "shape", "dtype", "payload", "is_input")

    def describe(self) -> str:
        return f"{self.site} shape={tuple(self.shape)} dtype={str(self.dtype).replace('torch.', '')}"


class Arena:
    """Allocator of guarded, poisoned buffers (see the module docstring)."""

    def __init__(self, byte: int):
        assert 0 <= int(byte) <= 255
        self.byte = int(byte)
        self.bufs = []
        self._lock = threading.Lock()       # autograd's backward thread allocates too

    def alloc(self, shape, dtype, device, site: str = "?", is_input: bool = False) -> _torch.Tensor:
        shape = tuple(int(s) for s in shape)
        item = _torch.empty((), dtype=dtype).element_size()
        n = math.prod(shape) * item
        raw = _torch.empty(GUARD + n + GUARD + ALIGN, dtype=_torch.uint8, device=device)
        off = GUARD + (-(raw.data_ptr() + GUARD)) % ALIGN
        raw.fill_(self.byte)
        _sync(raw.device)
        payload = raw[off:off + n].view(dtype).view(shape)
        assert payload.data_ptr() % ALIGN == 0 and payload.is_contiguous()
        b = _Buf()
        b.raw, b.off, b.nbytes, b.site, b.shape, b.dtype = raw, off, n, site, shape, dtype
        b.payload, b.is_input = payload, is_input
        with self._lock:
            self.bufs.append(b)
        return payload

    def find(self, t: _torch.Tensor):
        """The buffer a tensor lives in (None for a tensor from elsewhere)."""
        if not isinstance(t, _torch.Tensor) or t.numel() == 0:
            return None
        p = t.data_ptr()
        for b in self.bufs:
            lo = b.raw.data_ptr() + b.off
            if b.raw.device == t.device and lo <= p < lo + max(b.nbytes, 1):
                return b
        return None

    def failures(self) -> list:
        out = []
        for b in self.bufs:
            sides = (("front", b.raw[b.off - GUARD:b.off]),
                     ("back", b.raw[b.off + b.nbytes:b.off + b.nbytes + GUARD]))
            for side, g in sides:
                bad = g != self.byte
                if bool(bad.any()):
                    i = int(bad.nonzero()[0, 0])
                    nbad = int(bad.sum())
                    where = (f"{GUARD - i} bytes before the payload" if side == "front"
                             else f"{i} bytes past the payload's end")
                    out.append(f"guard overwritten: {b.describe()}: {side} guard, first corrupted byte {where} "
                               f"(guard offset {i}, {nbad} bytes changed, poison 0x{self.byte:02X})")
        return out

    def check(self) -> None:
        """Every guard byte still equals the poison byte (call after the work
        is done; synchronises the devices the arena holds buffers on)."""
        if any(b.raw.is_cuda for b in self.bufs):
            _torch.cuda.synchronize()
        f = self.failures()
        if f:
            raise GuardError("\n".join(f))

    def unwritten(self, limit: int = 6) -> list:
        """A hint for a failed run: non-input buffers that still hold whole
        elements of poison (never written by anybody)."""
        out = []
        for b in self.bufs:
            if b.is_input or b.nbytes == 0:
                continue
            item = b.payload.element_size()
            m = (_bits(b.payload) == self.byte).view(-1, item).all(1)
            k = int(m.sum())
            if k:
                out.append(f"{b.describe()}: {k} of {m.numel()} elements still poison, first at element "
                           f"{int(m.nonzero()[0, 0])}")
            if len(out) >= limit:
                break
        return out


def _site(module) -> str:
    """``file:line`` of the innermost frame that runs the module's code."""
    f = sys._getframe(2)
    first = f
    g = getattr(module, "__dict__", None)
    while f is not None and f.f_globals is not g:
        f = f.f_back
    f = f or first
    return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno}"


def _parse_size(args, kw):
    if "size" in kw:
        size = kw.pop("size")
    elif len(args) == 1 and isinstance(args[0], _SEQ):
        size = args[0]
    else:
        size = args
    return tuple(int(s) for s in size)


class _TorchProxy:
    """``torch`` with arena-backed ``empty`` / ``zeros`` (+ ``_like``)."""

    def __init__(self, arena: Arena, module):
        self.__dict__["_arena"] = arena
        self.__dict__["_module"] = module

    def __getattr__(self, name):
        return getattr(_torch, name)

    def _new(self, shape, kw, site, like=None, zero=False):
        dtype = kw.pop("dtype", None)
        device = kw.pop("device", None)
        rg = kw.pop("requires_grad", False)
        kw.pop("memory_format", None)
        if kw.pop("pin_memory", False) or kw.pop("out", None) is not None or kw:
            raise TypeError(f"guarded torch proxy: unsupported arguments {sorted(kw)} at {site}")
        if dtype is None:
            dtype = like.dtype if like is not None else _torch.get_default_dtype()
        if device is None:
            device = like.device if like is not None else "cpu"
        t = self._arena.alloc(shape, dtype, device, site)
        if like is not None and not like.is_contiguous():
            st = _torch.empty_like(like, device="meta").stride()     # preserve_format's strides
            if st != t.stride():
                t = t.as_strided(tuple(like.shape), st)
        if zero:
            t.zero_()
        return t.requires_grad_(True) if rg else t

    def empty(self, *args, **kw):
        return self._new(_parse_size(args, kw), kw, _site(self._module))

    def zeros(self, *args, **kw):
        return self._new(_parse_size(args, kw), kw, _site(self._module), zero=True)

    def empty_like(self, x, **kw):
        return self._new(tuple(x.shape), kw, _site(self._module), like=x)

    def zeros_like(self, x, **kw):
        return self._new(tuple(x.shape), kw, _site(self._module), like=x, zero=True)


@contextlib.contextmanager
def guarded(H, byte: int = POISON[0], arena: Arena = None):
    """Run ``H``'s ops with every ``torch.empty*`` / ``torch.zeros*`` of the
    module served from a poisoned arena; yields the arena.  The module's real
    ``torch`` is back on exit, also after an exception."""
    arena = arena if arena is not None else Arena(byte)
    real = H.torch
    assert real is _torch, "guarded() does not nest"
    H.torch = _TorchProxy(arena, H)
    try:
        yield arena
    finally:
        H.torch = real


def place(arena: Arena, t: _torch.Tensor, name: str = "") -> _torch.Tensor:
    """A copy of a test input inside the arena (same shape, dtype, device and
    requires_grad): the bytes around it are poison and its guards are checked."""
    p = arena.alloc(tuple(t.shape), t.dtype, t.device, f"input {name!r}" if name else "input", is_input=True)
    p.copy_(t.detach())
    _sync(p.device)
    return p.requires_grad_(True) if t.requires_grad else p


def _flat(res):
    """(name, tensor) pairs of a result: a tensor, a dict or a (nested) sequence."""
    if res is None:
        return []
    if isinstance(res, _torch.Tensor):
        return [("result", res)]
    if isinstance(res, dict):
        return [(f"{k}{'.' + n if n != 'result' else ''}", t) for k, v in res.items() for n, t in _flat(v)]
    return [(f"[{i}]{n if n != 'result' else ''}", t) for i, v in enumerate(res) for n, t in _flat(v)]


def run_guarded(make_inputs, fn, mutated=(), impl=None):
    """Run ``fn`` once per poison byte on identical inputs and check memory.

    ``make_inputs()`` returns a dict name -> tensor (other values pass
    through), the same every call; ``fn(**inputs)`` runs the op (and its
    backward) and returns its outputs and gradients (tensor, dict or
    sequence).  Asserts: every guard of every output, workspace and input is
    intact; every input not named in ``mutated`` is bitwise unchanged; every
    returned tensor is finite; the two runs agree bit for bit.  Returns the
    (second) result for the comparison with the reference."""
    if impl is None:
        from distributed_3d_diffusion_pytorch_amd.ops import hip_impl as impl
    runs = []
    for byte in POISON:
        src = make_inputs()
        arena = Arena(byte)
        placed = {k: place(arena, v, k) if isinstance(v, _torch.Tensor) else v for k, v in src.items()}
        with guarded(impl, byte, arena):
            res = fn(**placed)
        errs = []
        try:
            arena.check()
        except GuardError as e:
            errs.append(str(e))
        for k, v in src.items():
            if isinstance(v, _torch.Tensor) and k not in mutated and not _torch.equal(_bits(placed[k]), _bits(v)):
                d = (_bits(placed[k]) != _bits(v)).nonzero()
                errs.append(f"input {k!r} modified: {arena.find(placed[k]).describe()}: {d.numel()} bytes differ, "
                            f"first at byte {int(d[0, 0])}")
        named = _flat(res)
        for n, t in named:
            if t.is_floating_point() and not bool(_torch.isfinite(t).all()):
                bad = (~_torch.isfinite(t.detach())).reshape(-1).nonzero()
                b = arena.find(t)
                errs.append(f"{n} not finite (poison 0x{byte:02X}): {bad.numel()} of {t.numel()} elements, first at "
                            f"{int(bad[0, 0])}; allocated at {b.describe() if b else 'outside the arena'}")
        if runs and not errs:
            for (n, t), (_, t0) in zip(named, runs[0]):
                if t.shape != t0.shape or not _torch.equal(_bits(t), _bits(t0)):
                    d = (t.detach().reshape(-1) != t0.detach().reshape(-1)).nonzero()
                    b = arena.find(t)
                    errs.append(f"{n} differs between poison 0x{POISON[0]:02X} and 0x{byte:02X} (uninitialised "
                                f"memory used): {d.numel()} of {t.numel()} elements, first at "
                                f"{int(d[0, 0]) if d.numel() else -1}; allocated at "
                                f"{b.describe() if b else 'outside the arena'}")
        if errs:
            hint = arena.unwritten()
            if hint:
                errs.append("buffers with elements nobody wrote:\n  " + "\n  ".join(hint))
            raise GuardError(f"poison 0x{byte:02X}:\n" + "\n".join(errs))
        runs.append(named)
    return res
