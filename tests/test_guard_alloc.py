"""The guard-band allocator itself (tests/guard_alloc.py), on the CPU: layout, fills, the call forms the
csu modules use, detection of stray writes and modified inputs, and the scoped torch proxy."""
import ast
import importlib
import os
import sys
import threading

import pytest
import torch

import guard_alloc as G
from guard_alloc import GUARD, GuardedAlloc, GuardError, patched

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cswin-simam-unet_amd", "csu")
GUARDED_MODULES = ("ops", "unet", "simam", "infer", "metrics", "optim", "ema")


def _base_of(ga, t):
    (r,) = [r for r in ga.records if r.base.data_ptr() + GUARD == t.data_ptr() and r.shape == tuple(t.shape)]
    return r


def _allocator_calls():
    """(module, lineno, name, n positional, positional is one sequence?, keyword names) for every
    torch.empty / empty_like / zeros / zeros_like call in the guarded csu modules."""
    out = []
    for mod in GUARDED_MODULES:
        with open(os.path.join(PKG, mod + ".py")) as f:
            tree = ast.parse(f.read())
        for node in ast.walk(tree):
            if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in G.ALLOCATORS
                    and isinstance(node.func.value, ast.Name) and node.func.value.id == "torch"):
                out.append((mod, node.lineno, node.func.attr, node.args, sorted(k.arg for k in node.keywords)))
    return out


def _size_form(args):
    """How a torch.empty / torch.zeros call spells its size."""
    if any(isinstance(a, ast.Starred) for a in args):
        return "starred"
    if len(args) == 1 and isinstance(args[0], (ast.Tuple, ast.List)):
        return "sequence"
    if len(args) == 1 and isinstance(args[0], ast.Attribute) and args[0].attr == "shape":
        return "shape"
    if len(args) == 1 and isinstance(args[0], ast.Name):
        return "name"                  # an int, or a shape held in a variable
    return "ints"


SIZE_FORMS = {
    "starred": lambda ga, x: ga.empty(*x.shape[:-1], x.shape[-1], dtype=x.dtype, device=x.device),
    "sequence": lambda ga, x: ga.empty((3, 5), dtype=x.dtype, device=x.device),
    "shape": lambda ga, x: ga.zeros(x.shape, dtype=torch.float64, device=x.device),
    "name": lambda ga, x: (ga.empty(x.numel(), dtype=torch.uint8), ga.empty(tuple(x.shape), dtype=x.dtype))[1],
    "ints": lambda ga, x: ga.empty(3, max(5, 1), dtype=x.dtype, device=x.device),
}


def test_every_call_form_under_csu_is_handled():
    calls = _allocator_calls()
    assert len(calls) > 150          # the grep found the sites at all
    assert {c[2] for c in calls} == set(G.ALLOCATORS)
    seen = set()
    for mod, line, name, args, kws in calls:
        where = f"csu/{mod}.py:{line}"
        assert not any(isinstance(a, ast.Starred) for a in args) or name in ("empty", "zeros"), where
        if name.endswith("_like"):
            assert len(args) == 1, where
            assert set(kws) <= {"dtype", "device", "memory_format"}, (where, kws)
        else:
            assert len(args) >= 1, where
            assert set(kws) <= {"dtype", "device", "pin_memory"}, (where, kws)
            seen.add(_size_form(args))
    # every way the size is spelt under csu/ is one the helper takes (each is run in test_call_forms)
    assert seen <= set(SIZE_FORMS), seen - set(SIZE_FORMS)
    ga = GuardedAlloc()
    x = torch.randn(3, 5)
    for form in seen:
        t = SIZE_FORMS[form](ga, x)
        assert ga.contains(t) and tuple(t.shape) == (3, 5), form


def test_call_forms():
    ga = GuardedAlloc()
    x = torch.randn(3, 5)
    forms = [
        (ga.empty(7, dtype=torch.float32, device="cpu"), (7,), torch.float32),
        (ga.empty(2, 3, 4, dtype=torch.bfloat16, device=x.device), (2, 3, 4), torch.bfloat16),
        (ga.empty((2, 3), dtype=torch.int32, device=x.device), (2, 3), torch.int32),
        (ga.empty([4, 1], dtype=torch.uint8), (4, 1), torch.uint8),
        (ga.empty(x.shape, dtype=torch.float64, device=x.device), (3, 5), torch.float64),
        (ga.empty(*x.shape, dtype=torch.float32), (3, 5), torch.float32),
        (ga.empty(max(0, 16), dtype=torch.uint8, device=x.device), (16,), torch.uint8),
        (ga.empty(5), (5,), torch.get_default_dtype()),
        (ga.empty(0, dtype=torch.float32), (0,), torch.float32),
        (ga.zeros(6, dtype=torch.int64, device=x.device), (6,), torch.int64),
        (ga.zeros((2, 2), dtype=torch.float32), (2, 2), torch.float32),
        (ga.zeros(x.shape, dtype=torch.float64, device=x.device), (3, 5), torch.float64),
        (ga.empty_like(x), (3, 5), torch.float32),
        (ga.empty_like(x, dtype=torch.bfloat16), (3, 5), torch.bfloat16),
        (ga.zeros_like(x), (3, 5), torch.float32),
        (ga.zeros_like(x, memory_format=torch.contiguous_format), (3, 5), torch.float32),
        (ga.zeros_like(x.t(), memory_format=torch.contiguous_format), (5, 3), torch.float32),
    ]
    for t, shape, dtype in forms:
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
        assert ga.contains(t) or t.numel() == 0     # an empty tensor has no address to place
    assert len(ga) == len(forms) and not ga.fallthrough
    ga.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8, torch.int32, torch.int64, torch.float64])
def test_payload_fill_alignment_contiguity(dtype):
    ga = GuardedAlloc()
    e, z = ga.empty(3, 5, dtype=dtype), ga.zeros(3, 5, dtype=dtype)
    el, zl = ga.empty_like(e), ga.zeros_like(e)
    for t in (e, z, el, zl):
        assert t.is_contiguous() and t.data_ptr() % 16 == 0 and t.dtype == dtype and t._base is None
        assert t.storage_offset() == 0 and t.untyped_storage().nbytes() == t.numel() * t.element_size()     # as torch.empty's
        r = _base_of(ga, t)
        assert r.base.data_ptr() % 16 == 0 and r.base.numel() == 2 * GUARD + t.numel() * t.element_size()
        # the back guard starts at the first byte after the payload, whatever 16-byte padding would add
        assert bool((r.base[:GUARD] == G.GUARD_BYTE).all()) and bool((r.base[GUARD + r.nbytes:] == G.GUARD_BYTE).all())
        assert r.base[GUARD + r.nbytes:].numel() == GUARD
    for t in (e, el):
        if dtype.is_floating_point:
            assert bool(torch.isnan(t).all())           # 0xFF bytes are NaN as fp32, bf16 and fp64
        elif dtype == torch.uint8:
            assert bool((t == 255).all())
        else:
            assert bool((t == -1).all())
    for t in (z, zl):
        assert bool((t == 0).all())


def test_guard_byte_is_a_tiny_finite_number():
    raw = torch.full((8,), G.GUARD_BYTE, dtype=torch.uint8)
    for dt in (torch.float32, torch.bfloat16):
        v = raw.view(dt).float()
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) < 1e-10 and float(v.abs().min()) > 0


def test_noncontiguous_like_falls_through_and_is_counted():
    ga = GuardedAlloc()
    xt = torch.randn(4, 6).t()
    a, b = ga.empty_like(xt), ga.zeros_like(xt)
    assert a.stride() == xt.stride() and b.stride() == xt.stride()
    assert not ga.contains(a) and not ga.contains(b)
    assert len(ga.fallthrough) == 2 and len(ga) == 0
    assert all(s.startswith("test_guard_alloc.py:") for s in ga.fallthrough)


@pytest.mark.parametrize("where", ["before", "after", "last"])
@pytest.mark.parametrize("numel,dtype", [(5, torch.float32), (13, torch.bfloat16), (3, torch.uint8)])
def test_stray_write_is_reported_with_side_and_offset(where, numel, dtype):
    ga = GuardedAlloc()
    clean = ga.empty(9, dtype=torch.float32)
    t, line = ga.empty(numel, dtype=dtype), sys._getframe().f_lineno     # the site the message must name
    t.fill_(1)
    ga.check()
    r = _base_of(ga, t)
    n = r.nbytes
    idx, side, off = {"before": (GUARD - 1, "front", -1), "after": (GUARD + n, "back", n),
                      "last": (2 * GUARD + n - 1, "back", n + GUARD - 1)}[where]
    r.base[idx] = 0
    with pytest.raises(GuardError) as ei:
        ga.check()
    msg = str(ei.value)
    assert msg.count("\n") == 0                                      # only the damaged buffer is named
    assert f"{side} guard" in msg and f"first at payload offset {off}, last at {off} " in msg
    assert f"test_guard_alloc.py:{line}" in msg
    assert f"shape ({numel},)" in msg and str(dtype) in msg
    del clean


def test_stray_write_span():
    ga = GuardedAlloc()
    t = ga.zeros(4, dtype=torch.float32)
    r = _base_of(ga, t)
    r.base[GUARD + 16:GUARD + 28] = 7          # a 16-byte vector store on a 1-element tail, 12 bytes long
    with pytest.raises(GuardError, match=r"back guard .* 12 bytes, first at payload offset 16, last at 27 "):
        ga.check()


def test_guard_input_snapshot_and_inplace():
    ga = GuardedAlloc()
    x = torch.randn(3, 7)
    xg = ga.guard_input(x, name="x")
    assert torch.equal(xg, x) and xg.data_ptr() != x.data_ptr() and ga.contains(xg) and xg.is_contiguous()
    assert xg._base is None                       # a tensor of its own, as a parameter is
    r = _base_of(ga, xg)
    assert bool(torch.isnan(r.base[:GUARD].view(torch.float32)).all())
    assert bool(torch.isnan(r.base[GUARD + r.nbytes:].view(torch.float32)).all())
    b = ga.guard_input(x.bfloat16())
    assert bool(torch.isnan(_base_of(ga, b).base[:GUARD].view(torch.bfloat16)).all())
    ga.check()
    assert xg.requires_grad_(True).is_leaf
    xg.detach()[1, 2] += 1.0
    with pytest.raises(GuardError, match=r"input buffer x .* was modified: .* first at payload offset 3[6-9]"):
        ga.check()
    ga2 = GuardedAlloc()
    stats = ga2.guard_input(x, inplace=True)
    stats.mul_(2.0)
    ga2.check()                                 # declared in-place: the payload may change ...
    _base_of(ga2, stats).base[GUARD - 4] = 0
    with pytest.raises(GuardError, match="front guard"):
        ga2.check()                             # ... its guards may not


def test_guard_input_labels_take_an_out_of_range_fill():
    ga = GuardedAlloc()
    lab = torch.randint(0, 3, (5, 6))
    with pytest.raises(ValueError):
        ga.guard_input(lab)
    with pytest.raises(ValueError):
        ga.guard_input(torch.randn(3), fill=1.0)
    lg = ga.guard_input(lab, fill=99)
    m8 = ga.guard_input(lab.to(torch.uint8), fill=77)
    assert torch.equal(lg, lab) and lg.dtype == torch.int64
    r = _base_of(ga, lg)
    assert bool((r.base[:GUARD].view(torch.int64) == 99).all())
    assert bool((r.base[GUARD + r.nbytes:].view(torch.int64) == 99).all())
    assert bool((_base_of(ga, m8).base[GUARD + 30:] == 77).all())
    ga.check()
    r.base[GUARD + r.nbytes] = 98
    with pytest.raises(GuardError, match=f"back guard .* first at payload offset {r.nbytes}, last at {r.nbytes} "):
        ga.check()


def test_contains():
    ga = GuardedAlloc()
    t = ga.empty(4, 6, dtype=torch.float32)
    assert ga.contains(t) and ga.contains(t[1:3]) and ga.contains(t.view(24)[5:6]) and ga.contains(t.view(6, 4))
    assert not ga.contains(torch.empty(4, 6))
    assert not ga.contains(t.clone())
    r = _base_of(ga, t)
    assert not ga.contains(r.base)                                    # guards are not payload
    assert not ga.contains(r.base[GUARD - 1:GUARD + 8]) and not ga.contains(r.base[GUARD + r.nbytes - 1:GUARD + r.nbytes + 1])
    assert ga.saw_workspace(0) is False
    ws = ga.empty(max(48, 16), dtype=torch.uint8)
    assert ga.saw_workspace(48) and ga.saw_workspace(50) and not ga.saw_workspace(52) and not ga.saw_workspace(1)
    del ws


def test_registry_keeps_bases_alive_and_is_thread_safe():
    ga = GuardedAlloc()

    def work():
        for _ in range(200):
            ga.empty(3, dtype=torch.float32)

    ts = [threading.Thread(target=work) for _ in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert len(ga) == 800
    assert len({r.base.data_ptr() for r in ga.records}) == 800       # none was recycled while registered
    ga.check()


def test_proxy_forwards_everything_but_the_allocators():
    ga = GuardedAlloc()
    proxy = G.make_proxy(ga)
    assert proxy.Tensor is torch.Tensor and proxy.autograd is torch.autograd
    assert proxy.autograd.Function is torch.autograd.Function
    for name in ("float32", "bfloat16", "uint8", "int32", "int64", "float64", "float8_e4m3fn"):
        assert getattr(proxy, name) is getattr(torch, name)
    assert proxy.cuda is torch.cuda and proxy.nn is torch.nn and proxy.no_grad is torch.no_grad
    assert proxy.ones is torch.ones and proxy.full is torch.full
    assert isinstance(torch.ones(2), proxy.Tensor)
    for name in G.ALLOCATORS:
        assert getattr(proxy, name) is not getattr(torch, name)
    assert ga.contains(proxy.empty(3, dtype=proxy.float32))
    with pytest.raises(AttributeError):
        proxy.no_such_attribute


def test_patched_is_scoped_and_undoes_itself(monkeypatch):
    ops, simam = importlib.import_module("csu.ops"), importlib.import_module("csu.simam")

    class F(torch.autograd.Function):     # a Function whose bodies allocate through the module's `torch`
        @staticmethod
        def forward(ctx, x):
            return ops.torch.empty_like(x).copy_(x * 2)

        @staticmethod
        def backward(ctx, g):
            return ops.torch.empty_like(g).copy_(g * 2)

    with patched(monkeypatch, ops, simam) as ga:
        assert ops.torch is not torch and simam.torch is ops.torch
        x = torch.randn(5, requires_grad=True)
        y = F.apply(x)
        assert ga.contains(y) and not ga.contains(torch.empty(5))     # the test's own torch is untouched
        y.backward(torch.ones(5))
        assert len(ga) == 2 and torch.equal(x.grad, torch.full((5,), 2.0))
        with pytest.raises(RuntimeError):
            with patched(monkeypatch, ops):
                pass
    assert ops.torch is torch and simam.torch is torch
    ga.check()
    with patched(monkeypatch, ops, registry=ga) as again:
        assert again is ga
    assert ops.torch is torch
