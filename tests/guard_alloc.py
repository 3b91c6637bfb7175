"""Guard-band allocator for the kernel tests (test_guard_alloc.py, test_gpu_guard_bands.py).  Plain torch;
nothing here needs a GPU.

The csu modules allocate every output and workspace with torch.empty / empty_like / zeros / zeros_like.
PyTorch's caching allocator rounds those to 512 bytes and packs them into shared blocks, so a stray
store lands in slack or in a neighbour, a stray load reads some earlier test's finite data, and an output
element the kernel never writes may still hold the previous case's correct answer.  GuardedAlloc replaces
the four allocators, inside chosen modules only, with ones that lay every buffer out as

    [ front guard 4096 B | payload | back guard 4096 B ]

in one uint8 base buffer.  The back guard starts at the first byte after the payload, so padding to a
16-byte vector belongs to the guard.  Fills:
  * guards of allocations: 0xA5 bytes -- a tiny finite number as fp32 (-2.87e-16) and bf16, and a value
    no kernel can reproduce by copying a poisoned payload element out of bounds;
  * empty / empty_like payloads: 0xFF bytes -- NaN as fp32, bf16 and fp64, 255 as uint8, -1 as a signed
    integer -- so an element the kernel leaves unwritten fails the reference comparison;
  * zeros / zeros_like payloads: zero;
  * guards of guard_input() copies: NaN (0xFF bytes) for floating types, so an unmasked tail load that
    feeds a reduction shows in the result; a caller-given out-of-range value for label / mask types.

Use (see README.md, "Testing"):

    ga = GuardedAlloc()
    xd = ga.guard_input(x.to(dev)).requires_grad_(True)
    with patched(monkeypatch, ops, registry=ga):
        y = ops.some_op(xd)
        y.backward(ga.guard_input(dy.to(dev)))
        ops.flush_deferred(); ops.join_side_streams(); torch.cuda.synchronize()
    ga.check()                      # guards intact, inputs unchanged
    assert ga.contains(y)           # the case did not run unguarded
"""
import contextlib
import os
import sys
import threading
import types

import torch

GUARD = 4096            # bytes on each side; a multiple of every element size and of torch's 512-byte rounding
GUARD_BYTE = 0xA5       # guards of allocations
POISON_BYTE = 0xFF      # empty* payloads and the guards of floating-point inputs
ALLOCATORS = ("empty", "empty_like", "zeros", "zeros_like")

_THIS = os.path.abspath(__file__)


def _call_site():
    """file:line of the innermost frame outside this module (and outside the proxy's plumbing)."""
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _THIS:
        f = f.f_back
    if f is None:
        return "?"
    return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno}"


def _shape_of(size):
    """torch.empty's size forms: varargs of ints, or one tuple / list / torch.Size."""
    if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
        size = size[0]
    return tuple(int(s) for s in size)


def _esize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


class GuardError(AssertionError):
    pass


class _Span:
    """`nbytes` bytes at byte offset `off` of a uint8 buffer, exposed through __array_interface__ (host) or
    __cuda_array_interface__ (device); holds the buffer."""

    def __init__(self, base, off, nbytes):
        self.base = base
        iface = {"shape": (nbytes,), "typestr": "|u1", "data": (base.data_ptr() + off, False), "strides": None}
        if base.is_cuda:
            self.__cuda_array_interface__ = dict(iface, version=2)
        else:
            self.__array_interface__ = dict(iface, version=3)


class _Record:
    __slots__ = ("base", "nbytes", "shape", "dtype", "site", "kind", "name", "pattern", "snapshot", "inplace")

    def describe(self):
        return f"{self.kind} buffer {self.name or ''} allocated at {self.site}, shape {self.shape}, {self.dtype}, " \
               f"{self.nbytes} payload bytes"


class GuardedAlloc:
    """Registry of guarded buffers.  empty / empty_like / zeros / zeros_like take torch's call forms."""

    def __init__(self):
        self._lock = threading.Lock()     # autograd runs backward on another thread
        self.records = []
        self.fallthrough = []             # sites of *_like calls on non-contiguous tensors, left to torch

    def __len__(self):
        return len(self.records)

    # -- layout -------------------------------------------------------------------------------
    def _layout(self, shape, dtype, device, guard_byte, payload_byte, kind, pin_memory=False, name=None):
        dtype = dtype if dtype is not None else torch.get_default_dtype()
        n = 1
        for s in shape:
            n *= s
        nbytes = n * _esize(dtype)
        kw = {"pin_memory": True} if pin_memory else {}
        base = torch.empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device=device, **kw)
        base.fill_(guard_byte)
        if nbytes and payload_byte != guard_byte:
            base[GUARD:GUARD + nbytes].fill_(payload_byte)
        r = _Record()
        r.base, r.nbytes, r.shape, r.dtype, r.kind, r.name = base, nbytes, tuple(shape), dtype, kind, name
        r.site = _call_site()
        r.pattern = None      # None: every guard byte is guard_byte
        r.snapshot, r.inplace = None, False
        with self._lock:
            self.records.append(r)
        return r

    @staticmethod
    def _payload(r):
        """The payload as torch.empty would have returned it: a tensor of its own (no _base: the csu modules
        walk _base to find the parameter a gradient belongs to) at offset 0 of a storage of exactly the
        payload's bytes (they use storage_offset() and untyped_storage().nbytes() in their own address
        arithmetic).  The storage wraps the bytes between the guards through the array interface and keeps
        the base buffer alive."""
        if r.nbytes == 0:
            return torch.empty(r.shape, dtype=r.dtype, device=r.base.device)
        span = _Span(r.base, GUARD, r.nbytes)
        if r.base.is_cuda:
            u8 = torch.as_tensor(span, device=r.base.device)
        else:
            import numpy as np
            u8 = torch.from_numpy(np.asarray(span))
        assert u8.data_ptr() == r.base.data_ptr() + GUARD and u8.numel() == r.nbytes and u8.dtype == torch.uint8
        stride, n = [], 1
        for s in reversed(r.shape):
            stride.append(n)
            n *= max(s, 1)
        t = torch.empty(0, dtype=r.dtype, device=r.base.device)
        return t.set_(u8.untyped_storage(), 0, r.shape, tuple(reversed(stride)))

    # -- the four allocators ------------------------------------------------------------------
    def empty(self, *size, dtype=None, device=None, pin_memory=False):
        return self._payload(self._layout(_shape_of(size), dtype, device, GUARD_BYTE, POISON_BYTE, "empty", pin_memory))

    def zeros(self, *size, dtype=None, device=None, pin_memory=False):
        return self._payload(self._layout(_shape_of(size), dtype, device, GUARD_BYTE, 0, "zeros", pin_memory))

    def _like(self, t, dtype, device, memory_format, payload_byte, kind, fall):
        dense = memory_format in (None, torch.preserve_format) and not t.is_contiguous()
        if dense or memory_format not in (None, torch.preserve_format, torch.contiguous_format):
            with self._lock:
                self.fallthrough.append(_call_site())
            kw = {} if memory_format is None else {"memory_format": memory_format}
            return fall(t, dtype=dtype, device=device, **kw)
        return self._payload(self._layout(tuple(t.shape), dtype if dtype is not None else t.dtype,
                                          device if device is not None else t.device, GUARD_BYTE, payload_byte, kind))

    def empty_like(self, t, dtype=None, device=None, memory_format=None):
        return self._like(t, dtype, device, memory_format, POISON_BYTE, "empty", torch.empty_like)

    def zeros_like(self, t, dtype=None, device=None, memory_format=None):
        return self._like(t, dtype, device, memory_format, 0, "zeros", torch.zeros_like)

    # -- inputs -------------------------------------------------------------------------------
    def guard_input(self, t, fill=None, inplace=False, name=None, device=None):
        """Copy a test-made input into the guarded layout on `device` (its own if None); return the copy.

        Floating types get NaN guards (0xFF bytes).  Any other type needs `fill`, a value of that type
        outside the range the kernel accepts (a label that is no class, a mask that is neither 0 nor 1).
        The payload is snapshotted bit for bit; check() compares unless `inplace` (the op updates this
        input by contract)."""
        t = t.detach()
        dt = t.dtype
        if dt.is_floating_point:
            if fill is not None:
                raise ValueError("floating-point inputs take NaN guards; fill is for label / mask types")
        elif fill is None:
            raise ValueError(f"guard_input of a {dt} tensor needs an out-of-range fill value")
        r = self._layout(tuple(t.shape), dt, t.device if device is None else device, POISON_BYTE, POISON_BYTE, "input",
                         name=name)
        if not dt.is_floating_point:
            r.base[:GUARD].view(dt).fill_(fill)
            r.base[GUARD + r.nbytes:].view(dt).fill_(fill)
            r.pattern = r.base[:GUARD].cpu().clone()
        p = self._payload(r)
        p.copy_(t)
        r.inplace = inplace
        r.snapshot = r.base[GUARD:GUARD + r.nbytes].clone()
        return p

    # -- queries ------------------------------------------------------------------------------
    def contains(self, t):
        """Whether [data_ptr, data_ptr + nbytes) of `t` lies inside a registered payload."""
        lo = t.data_ptr()
        hi = lo + t.numel() * t.element_size()
        with self._lock:
            recs = list(self.records)
        for r in recs:
            if r.base.device != t.device:
                continue
            p0 = r.base.data_ptr() + GUARD
            if p0 <= lo and hi <= p0 + r.nbytes:
                return True
        return False

    def sizes(self, dtype=None, kinds=("empty", "zeros")):
        """Payload byte counts of the allocations seen (of one dtype, if given)."""
        with self._lock:
            return [r.nbytes for r in self.records if r.kind in kinds and (dtype is None or r.dtype == dtype)]

    def saw_workspace(self, nbytes):
        """Whether an allocation of exactly a workspace of `nbytes` was made: csu's workspaces are uint8
        buffers of max(n, 16) bytes or fp32 buffers of n // 4 elements."""
        n = int(nbytes)
        return n > 0 and any(b in (max(n, 16), n // 4 * 4) for b in self.sizes())

    # -- the check ----------------------------------------------------------------------------
    def problems(self):
        """One message per damaged guard or modified input.  The caller has synchronised the device."""
        out = []
        with self._lock:
            recs = list(self.records)
        for r in recs:
            host = torch.cat([r.base[:GUARD], r.base[GUARD + r.nbytes:]]).cpu()
            for side, got in (("front", host[:GUARD]), ("back", host[GUARD:])):
                want = r.pattern if r.pattern is not None else \
                    torch.full((GUARD,), GUARD_BYTE if r.kind != "input" else POISON_BYTE, dtype=torch.uint8)
                bad = (got != want).nonzero().flatten()
                if bad.numel():
                    off = -GUARD if side == "front" else r.nbytes
                    first, last = int(bad[0]) + off, int(bad[-1]) + off
                    out.append(f"{side} guard of {r.describe()} damaged: {bad.numel()} bytes, first at payload offset "
                               f"{first}, last at {last} (payload is [0, {r.nbytes}))")
            if r.snapshot is not None and not r.inplace:
                now = r.base[GUARD:GUARD + r.nbytes]
                if not torch.equal(now, r.snapshot):
                    bad = (now != r.snapshot).nonzero().flatten()
                    out.append(f"{r.describe()} was modified: {bad.numel()} bytes, first at payload offset {int(bad[0])}, "
                               f"last at {int(bad[-1])}")
        return out

    def check(self):
        """Assert every guard byte is intact and every guarded input equals its snapshot (unless in-place)."""
        bad = self.problems()
        if bad:
            raise GuardError("\n".join(bad))

    def release(self):
        with self._lock:
            self.records.clear()
            self.fallthrough.clear()


def make_proxy(registry):
    """A module object that is `torch` in every attribute but the four allocators."""

    class _TorchProxy(types.ModuleType):
        def __getattr__(self, name):          # only reached for names not set below
            return getattr(torch, name)

    proxy = _TorchProxy("torch")
    for name in ALLOCATORS:
        setattr(proxy, name, getattr(registry, name))
    proxy.__guard_registry__ = registry
    return proxy


@contextlib.contextmanager
def patched(monkeypatch, *modules, registry=None):
    """Replace the name `torch` in `modules` (csu.ops, csu.simam, ...) by a proxy whose allocators are
    guarded; yield the registry.  Scoped to those modules, so the test's own reference computations are
    untouched; autograd Function bodies look the name up when they run, so backward allocations are
    caught as long as backward runs inside the block.  Undone on exit."""
    ga = registry if registry is not None else GuardedAlloc()
    proxy = make_proxy(ga)
    with monkeypatch.context() as m:
        for mod in modules:
            if getattr(mod, "torch", None) is not torch:
                raise RuntimeError(f"{mod.__name__} has no global `torch` to patch (or is patched already)")
            m.setattr(mod, "torch", proxy)
        yield ga
