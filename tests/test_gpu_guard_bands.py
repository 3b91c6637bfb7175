"""Guard-band tests on the MI355X: every kernel stays inside its outputs and workspaces, writes all of
its output, and does not let bytes outside its inputs reach a result.

Every case: inputs from a seeded CPU generator -> fp64 reference (the one the op's own test uses) ->
inputs copied to the device between NaN guards (guard_alloc.guard_input) -> forward and backward with the
csu module's torch.empty / empty_like / zeros / zeros_like replaced by guarded ones (guard_alloc.patched:
0xA5 guards of 4096 bytes on both sides, NaN-filled payloads) -> flush, join, synchronise -> then
  (a) no guard byte changed and no input changed (unless in place by contract),
  (b) every returned tensor lies inside a guarded payload (the case did not run unguarded),
  (c) a workspace-sized uint8 allocation was seen where the op's *_workspace() is non-zero,
  (d) every output and gradient is NaN-free and meets the tolerance of the op's existing test
      (assert_close and friends are imported from those tests; no tolerance is introduced here).
(d) is what turns "left unwritten" and "read a NaN guard into a reduction" into failures.  Allocations
that fell through to plain torch (*_like of a non-contiguous tensor) are asserted to be none."""
import contextlib
import ctypes
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from guard_alloc import GUARD, GuardedAlloc, GuardError, patched
from oracle import cswin_ref as O
from test_gpu_kernels import (CONV_CASES, DMA_CONV_CASES, IGEMM_DMA_BN, _e4m3_rows, _frag8, _frag_ref, _gelu, assert_close,
                              dev)

F = torch.nn.functional
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]


def mod(name):
    return importlib.import_module("csu." + name)


@contextlib.contextmanager
def guarded(monkeypatch, *names, registry=None):
    """Run the body with the named csu modules' allocators guarded; on exit flush the deferred parameter
    gradients, join the side streams and synchronise.  Yields the registry."""
    ops = mod("ops")
    with patched(monkeypatch, *[mod(n) for n in names], registry=registry) as ga:
        yield ga
        ops.flush_deferred()
        ops.join_side_streams()
        torch.cuda.synchronize()


def verify(ga, outs=(), ws=0):
    """(a), (b), (c) and the fall-through count of one case."""
    ga.check()
    for i, t in enumerate(outs):
        assert ga.contains(t), f"returned tensor {i} {tuple(t.shape)} {t.dtype} is not in a guarded payload"
    assert ga.fallthrough == [], ga.fallthrough
    if ws:
        assert ga.saw_workspace(ws), (ws, ga.sizes(torch.uint8))


def finite(*ts):
    for i, t in enumerate(ts):
        assert not bool(torch.isnan(t.float()).any()), f"tensor {i}: NaN (unwritten output or a guard read)"


def close(got, ref, dtype):
    """(d): NaN-free and tests/test_gpu_kernels.py::assert_close."""
    finite(got)
    assert_close(got.detach(), ref.detach(), dtype)


def gin(ga, t, d, grad=False, **kw):
    x = ga.guard_input(t, device=d, **kw)
    return x.requires_grad_(True) if grad else x


# ---------------------------------------------------------------------------------------------
# the harness itself, on the device
# ---------------------------------------------------------------------------------------------
def test_harness_reports_a_damaged_back_guard_on_the_device(monkeypatch):
    """A write into memory the test owns (the first back-guard byte, through the base buffer with
    ordinary torch indexing) is reported with its side and offset; no kernel is involved."""
    ops = mod("ops")
    d = dev()
    with guarded(monkeypatch, "ops") as ga:
        t = ops.torch.empty(5, 3, dtype=BF16, device=d)
        z = ops.torch.zeros(7, dtype=F32, device=d)
        assert bool(torch.isnan(t).all()) and not bool(z.any()) and t.data_ptr() % 512 == 0
    ga.check()
    assert ga.contains(t) and ga.contains(z) and not ga.contains(torch.empty(5, 3, dtype=BF16, device=d))
    (r,) = [r for r in ga.records if r.shape == (5, 3)]
    r.base[GUARD + 30] = 0
    torch.cuda.synchronize()
    with pytest.raises(GuardError, match=r"back guard of empty buffer .*test_gpu_guard_bands.py:\d+, shape \(5, 3\), "
                                         r"torch.bfloat16.* 1 bytes, first at payload offset 30, last at 30 "):
        ga.check()


# ---------------------------------------------------------------------------------------------
# stripe attention
# ---------------------------------------------------------------------------------------------
GB_ATTN_CASES = [(7, -1, 7, 64, 2, 2), (16, 0, 1, 32, 1, 2), (14, 0, 7, 64, 2, 1), (20, -1, 20, 32, 1, 2),
                 (42, -1, 42, 64, 2, 1)]


def _attn_inputs(case):
    reso, idx, sw, cb, heads, B = case
    g = torch.Generator().manual_seed(hash(case) % 1000)
    L = reso * reso
    qkv = torch.randn(B, L, 3 * cb, generator=g)
    w = torch.randn(cb, 1, 3, 3, generator=g) * 0.3
    b = torch.randn(cb, generator=g) * 0.1
    gout = torch.randn(B, L, cb, generator=g)
    return qkv, w, b, gout


def _attn_ref(case, qkv, w, b, gout, attn_mask=None):
    reso, idx, sw, cb, heads, B = case
    hs, ws = O.stripe_geometry(reso, idx, sw)
    scale = (cb // heads) ** -0.5
    q64 = qkv.double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    kw = {} if attn_mask is None else {"attn_mask": attn_mask}
    ref = O.lepe_attention(q64[..., :cb], q64[..., cb:2 * cb], q64[..., 2 * cb:], reso, hs, ws, heads, w64, b64, scale, **kw)
    ref.backward(gout.double())
    return ref.detach(), q64.grad, w64.grad, b64.grad


def _attn_run(monkeypatch, case, dtype, qkv, w, b, gout, drop=None):
    ops = mod("ops")
    d = dev()
    reso, idx, sw, cb, heads, B = case
    hs, ws = O.stripe_geometry(reso, idx, sw)
    geom = ops.StripeGeometry(reso, cb, heads, [(hs, ws, 0)], (cb // heads) ** -0.5)
    ga = GuardedAlloc()
    qd = gin(ga, qkv.to(dtype), d, grad=True, name="qkv")
    wd, bd = gin(ga, w, d, grad=True, name="lepe_w"), gin(ga, b, d, grad=True, name="lepe_b")
    gd = gin(ga, gout.to(dtype), d, name="dout")
    with guarded(monkeypatch, "ops", registry=ga):
        out = ops.stripe_attention(qd, geom, [wd], [bd], drop(d) if drop else None)
        nfwd = len(ga)
        out.backward(gd)
        a = geom.args(B, [wd], [bd], [wd], [bd])
        nws = mod("_lib").lib().csu_stripe_attn_bwd_workspace(ctypes.byref(a))
    assert len(ga) > nfwd                       # the backward allocated through the guarded allocators
    verify(ga, [out], ws=nws)
    assert out.dtype == dtype
    return out, qd.grad, wd.grad, bd.grad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", GB_ATTN_CASES)
def test_stripe_attention(case, dtype, monkeypatch):
    qkv, w, b, gout = _attn_inputs(case)
    qkv, gout = qkv.to(dtype).float(), gout.to(dtype).float()       # the oracle sees the rounded inputs
    refs = _attn_ref(case, qkv, w, b, gout)
    for got, ref in zip(_attn_run(monkeypatch, case, dtype, qkv, w, b, gout), refs):
        close(got, ref, dtype)


@pytest.mark.parametrize("defer", [True, False], ids=["deferred", "immediate"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stripe_attention_lepe_reduction(dtype, defer, monkeypatch):
    """The LePE dW / db reduction at the end of backward (one batched launch over the partials left in
    the backward workspace) and inline, by the existing DEFER_WGRAD switch."""
    monkeypatch.setattr(mod("ops"), "DEFER_WGRAD", defer)
    case = (14, 0, 7, 64, 2, 1)
    qkv, w, b, gout = _attn_inputs(case)
    qkv, gout = qkv.to(dtype).float(), gout.to(dtype).float()
    refs = _attn_ref(case, qkv, w, b, gout)
    for got, ref in zip(_attn_run(monkeypatch, case, dtype, qkv, w, b, gout), refs):
        close(got, ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_stripe_attention_two_branch_launch(dtype, monkeypatch):
    """Both LePE branches of a CSWinBlock in one launch at reso 16, C 64 (test_two_branch_fused_launch)."""
    ops = mod("ops")
    d = dev()
    reso, C, heads, sw, B = 16, 64, 2, 2, 2
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B, reso * reso, 3 * C, generator=g).to(dtype)
    ws_ = [torch.randn(C // 2, 1, 3, 3, generator=g) * 0.3 for _ in range(2)]
    bs_ = [torch.randn(C // 2, generator=g) * 0.1 for _ in range(2)]
    gout = torch.randn(B, reso * reso, C, generator=g).to(dtype)
    scale = (C // heads) ** -0.5
    q = qkv.double().requires_grad_(True)
    w64 = [w.double().requires_grad_(True) for w in ws_]
    b64 = [b.double().requires_grad_(True) for b in bs_]
    outs = []
    for i, sl in enumerate((slice(0, C // 2), slice(C // 2, C))):
        hs, wsp = O.stripe_geometry(reso, i, sw)
        outs.append(O.lepe_attention(q[..., :C][..., sl], q[..., C:2 * C][..., sl], q[..., 2 * C:][..., sl], reso, hs,
                                     wsp, heads // 2, w64[i], b64[i], scale))
    ref = torch.cat(outs, -1)
    ref.backward(gout.double())
    geom = ops.StripeGeometry(reso, C, heads // 2, [(reso, sw, 0), (sw, reso, C // 2)], scale)
    ga = GuardedAlloc()
    qd = gin(ga, qkv, d, grad=True)
    wd = [gin(ga, w, d, grad=True) for w in ws_]
    bd = [gin(ga, b, d, grad=True) for b in bs_]
    gd = gin(ga, gout, d)
    with guarded(monkeypatch, "ops", registry=ga):
        out = ops.stripe_attention(qd, geom, wd, bd)
        out.backward(gd)
        nws = mod("_lib").lib().csu_stripe_attn_bwd_workspace(ctypes.byref(geom.args(B, wd, bd, wd, bd)))
    verify(ga, [out], ws=nws)
    close(out, ref, dtype)
    close(qd.grad, q.grad, dtype)
    for got, r in zip(wd + bd, w64 + b64):
        close(got.grad, r.grad, dtype)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
def test_stripe_attention_with_attn_drop(dt, monkeypatch):
    """Attention dropout inside the stripe kernels, ragged 49-token windows, vs the oracle under the same
    masks: the criteria of test_gpu_dropout.py::test_stripe_attention_dropout_vs_oracle."""
    from test_gpu_dropout import _attn_provider, _snap
    ops = mod("ops")
    case = (7, -1, 7, 64, 2, 2)
    qkv, w, b, gout = _attn_inputs(case)
    qkv = qkv.to(dt).float()
    p = 0.3
    snap = _snap(dev(), 77, 1)
    ref, dq, dw, db = _attn_ref(case, qkv, w, b, gout, attn_mask=_attn_provider(snap, 40, p, None))
    # the kernel's gradient arrives in the output dtype
    if dt == BF16:
        ref, dq, dw, db = _attn_ref(case, qkv, w, b, gout.to(dt).float(), attn_mask=_attn_provider(snap, 40, p, None))
    out, gq, gw, gb = _attn_run(monkeypatch, case, dt, qkv, w, b, gout, drop=lambda d: ops.AttnDrop(snap, 40, p))
    finite(out, gq, gw, gb)
    if dt == F32:
        torch.testing.assert_close(out.double().cpu(), ref, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(gq.double().cpu(), dq, rtol=1e-3, atol=1e-3)
        for a_, b_ in ((gw, dw), (gb, db)):
            torch.testing.assert_close(a_.double().cpu(), b_, rtol=1e-3, atol=1e-3 * max(1, float(b_.abs().max())))
    else:
        def rel(a_, b_):
            return float((a_.double().cpu() - b_).norm() / b_.norm())
        assert rel(out.detach(), ref) < 1e-2
        assert rel(gq, dq) < 2e-2 and rel(gw, dw) < 2e-2 and rel(gb, db) < 2e-2


# ---------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------
LN_PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16)]


def _ln_inputs(C, xdt, ydt, rows=517):
    g = torch.Generator().manual_seed(C)
    x = (torch.randn(1, rows, C, generator=g) * 2 + 0.5).to(xdt)
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dy = torch.randn(1, rows, C, generator=g).to(ydt)
    return x, w, b, dy


@pytest.mark.parametrize("C", [64, 128, 256, 512])
@pytest.mark.parametrize("xdt,ydt", LN_PAIRS)
def test_layer_norm(C, xdt, ydt, monkeypatch):
    ops = mod("ops")
    d = dev()
    x, w, b, dy = _ln_inputs(C, xdt, ydt)
    x64 = x.double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.layer_norm(x64, (C,), w64, b64, 1e-5)
    ref.backward(dy.double())
    ga = GuardedAlloc()
    xd = gin(ga, x, d, grad=True, name="x")
    wd, bd = gin(ga, w, d, grad=True, name="gamma"), gin(ga, b, d, grad=True, name="beta")
    dyd = gin(ga, dy, d, name="dy")
    with guarded(monkeypatch, "ops", registry=ga):
        y = ops.layer_norm(xd, wd, bd, 1e-5, ydt)
        y.backward(dyd)
    verify(ga, [y], ws=mod("_lib").lib().csu_layernorm_bwd_workspace(517, C))
    assert y.dtype == ydt
    tol_dt = F32 if (xdt, ydt) == (F32, F32) else BF16
    for got, r in ((y, ref), (xd.grad, x64.grad), (wd.grad, w64.grad), (bd.grad, b64.grad)):
        close(got, r, tol_dt)


@pytest.mark.parametrize("C", [64, 128, 256, 512])
@pytest.mark.parametrize("gdt", DTYPES)
def test_layer_norm_fork(C, gdt, monkeypatch):
    """x -> (x, LN(x)) with dx = dres + dLN in one kernel and its bf16 copy
    (test_layernorm_fork_residual_junction's criteria)."""
    ops = mod("ops")
    d = dev()
    g = torch.Generator().manual_seed(C + 7)
    x = torch.randn(1, 517, C, generator=g) * 2 + 0.5
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    gres = torch.randn(1, 517, C, generator=g)
    gln = torch.randn(1, 517, C, generator=g).to(gdt)
    x64 = x.double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y64 = F.layer_norm(x64, (C,), w64, b64, 1e-5)
    torch.autograd.backward([x64, y64], [gres.double(), gln.double()])
    seen = {}

    class Probe(torch.autograd.Function):   # upstream consumer: records the gradient object it receives
        @staticmethod
        def forward(ctx, t):
            return t.view_as(t)

        @staticmethod
        def backward(ctx, gt):
            seen["g"] = gt
            return gt

    ga = GuardedAlloc()
    x0, wd, bd = gin(ga, x, d, grad=True), gin(ga, w, d, grad=True), gin(ga, b, d, grad=True)
    gr, gl = gin(ga, gres, d), gin(ga, gln, d)
    with guarded(monkeypatch, "ops", registry=ga):
        xa, y = ops.layer_norm_fork(Probe.apply(x0), wd, bd, 1e-5, gdt)
        torch.autograd.backward([xa, y], [gr, gl])
    verify(ga, [xa, y, seen["g"], seen["g"]._csu_bf16], ws=mod("_lib").lib().csu_layernorm_bwd_workspace(517, C))
    assert y.dtype == gdt and xa.data_ptr() == x0.data_ptr()
    close(y, y64, gdt)
    close(x0.grad, x64.grad, gdt)
    close(wd.grad, w64.grad, BF16)
    close(bd.grad, b64.grad, BF16)
    gb = seen["g"]._csu_bf16
    finite(gb)
    assert torch.equal(gb, seen["g"].to(BF16))


# ---------------------------------------------------------------------------------------------
# SimAM
# ---------------------------------------------------------------------------------------------
SIMAM_SHAPES = [(3, 17, 200), (2, 64, 32), (2, 256, 256)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SIMAM_SHAPES)
def test_simam(shape, dtype, monkeypatch):
    simam = mod("simam")
    d = dev()
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.randn(*shape, generator=g) * 1.5 + 0.3).to(dtype)
    dy = torch.randn(*shape, generator=g).to(dtype)
    x64 = x.double().requires_grad_(True)
    ref = O.simam(x64)
    ref.backward(dy.double())
    nws = mod("_lib").lib().csu_simam_workspace(*shape)
    ga = GuardedAlloc()
    xd, dyd = gin(ga, x, d, grad=True), gin(ga, dy, d)
    xb, dyb = gin(ga, x, d, grad=True), gin(ga, dy.bfloat16(), d)
    with guarded(monkeypatch, "simam", registry=ga):
        y = simam.simam(xd)
        y.backward(dyd)
        yb = simam.simam(xb, out_dtype=BF16)      # bf16 output for the GEMM consumer, bf16 incoming gradient
        yb.backward(dyb)
    verify(ga, [y, yb], ws=nws)
    close(y, ref, dtype)
    close(xd.grad, x64.grad, dtype)
    assert yb.dtype == BF16 and xb.grad.dtype == dtype
    close(yb, ref, BF16)
    close(xb.grad, x64.grad, BF16)


@pytest.mark.parametrize("shape", SIMAM_SHAPES)
def test_simam_fork_join(shape, monkeypatch):
    """simam_fork (bf16 x and bf16 SimAM(x) in one pass; one joined backward pass writing dx and its bf16
    copy) vs the fp64 formula at the bf16 tolerance test_simam_vs_formula gives the bf16 output."""
    simam = mod("simam")
    d = dev()
    g = torch.Generator().manual_seed(sum(shape) + 1)
    x = torch.randn(*shape, generator=g) * 1.5 + 0.3
    g1 = torch.randn(*shape, generator=g).bfloat16()
    dy = torch.randn(*shape, generator=g).bfloat16()
    x64 = x.double().requires_grad_(True)
    ref = O.simam(x64)
    torch.autograd.backward([x64 * 1.0, ref], [g1.double(), dy.double()])
    captured = {}
    ga = GuardedAlloc()
    xd, g1d, dyd = gin(ga, x, d, grad=True), gin(ga, g1, d), gin(ga, dy, d)
    xd.register_hook(lambda gr: captured.update(g=gr, b=getattr(gr, "_csu_bf16", None)))
    with guarded(monkeypatch, "simam", registry=ga):
        xc, y = simam.simam_fork(xd)
        torch.autograd.backward([xc, y], [g1d, dyd])
    verify(ga, [xc, y, captured["g"], captured["b"]], ws=mod("_lib").lib().csu_simam_workspace(*shape))
    assert xc.dtype == y.dtype == BF16
    finite(xc)
    assert torch.equal(xc.cpu(), x.bfloat16())
    close(y, ref, BF16)
    close(xd.grad, x64.grad, BF16)
    finite(captured["b"])
    assert torch.equal(captured["b"], xd.grad.bfloat16())


# ---------------------------------------------------------------------------------------------
# CARAFE and the heads
# ---------------------------------------------------------------------------------------------
def _carafe_ref(x64, e64, B, H, C, s):
    xi = x64.transpose(1, 2).reshape(B, C, H, H)
    kern = e64.permute(0, 3, 1, 2).reshape(B, 9, s, s, H, H).softmax(dim=1)
    nb = F.unfold(xi, 3, padding=1).reshape(B, C, 9, H, H)
    return torch.einsum("btijhw,bcthw->bchiwj", kern, nb).reshape(B, C, H * s * H * s).transpose(1, 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,C,s", [(1, 5, 8, 2), (1, 7, 128, 2), (1, 5, 64, 4)])
def test_carafe_reassemble(B, H, C, s, dtype, monkeypatch):
    ops = mod("ops")
    d = dev()
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + C + s)
    x = torch.randn(B, H * H, C, generator=g).to(dtype)
    enc = (torch.randn(B, H, H, 9 * s * s, generator=g) * 2).to(dtype)
    gy = torch.randn(B, H * H * s * s, C, generator=g).to(dtype)
    x64, e64 = x.double().requires_grad_(True), enc.double().requires_grad_(True)
    ref = _carafe_ref(x64, e64, B, H, C, s)
    ref.backward(gy.double())
    ga = GuardedAlloc()
    xd, ed, gd = gin(ga, x, d, grad=True), gin(ga, enc, d, grad=True), gin(ga, gy, d)
    with guarded(monkeypatch, "ops", registry=ga):
        y = ops.carafe_reassemble(xd, ed, H, H, s)
        y.backward(gd)
    verify(ga, [y])
    close(y.float(), ref, dtype)
    close(xd.grad.float(), x64.grad, dtype)
    close(ed.grad.float(), e64.grad, dtype)


@pytest.mark.parametrize("folded", [False, True], ids=["head", "folded"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,C,s", [(2, 5, 64, 2), (1, 5, 32, 4)])
def test_carafe_head(B, H, C, s, dtype, folded, monkeypatch):
    """carafe_head / carafe_head_folded: sigmoid(output(CARAFE(x).out)) fused, vs the unfused fp64 chain
    (reassembly restated as in test_carafe_reassemble_lane_counts, then the two 1x1 convs)."""
    ops = mod("ops")
    d = dev()
    g = torch.Generator().manual_seed(B * 100 + H * 10 + s + C)
    x = torch.randn(B, H * H, C, generator=g).to(dtype)
    enc = (torch.randn(B, H, H, 9 * s * s, generator=g) * 2).to(dtype)
    w_out = torch.randn(C, C, 1, 1, generator=g) * C ** -0.5
    b_out = torch.randn(C, generator=g) * 0.3
    w_h = torch.randn(1, C, 1, 1, generator=g) * 0.3
    dp = torch.randn(B, 1, s * H, s * H, generator=g)
    x64, e64 = x.double().requires_grad_(True), enc.double().requires_grad_(True)
    wo64, bo64, wh64 = (t.double().requires_grad_(True) for t in (w_out, b_out, w_h))
    u64 = wo64.view(C, C).t() @ wh64.view(C)
    cb64 = wh64.view(C) @ bo64
    if not folded:       # the op takes u and cb as its leaves
        u64, cb64 = u64.detach().requires_grad_(True), cb64.detach().requires_grad_(True)
    ref = torch.sigmoid(_carafe_ref(x64, e64, B, H, C, s) @ u64 + cb64).view(B, 1, s * H, s * H)
    ref.backward(dp.double())
    ga = GuardedAlloc()
    xd, ed, dpd = gin(ga, x, d, grad=True), gin(ga, enc, d, grad=True), gin(ga, dp, d)
    if folded:
        ps = [gin(ga, t, d, grad=True) for t in (w_out, b_out, w_h)]
        prefs = [wo64.grad, bo64.grad, wh64.grad]
    else:
        ps = [gin(ga, u64.detach().float(), d, grad=True), gin(ga, cb64.detach().float().reshape(()), d, grad=True)]
        prefs = [u64.grad, cb64.grad]
    with guarded(monkeypatch, "ops", registry=ga):
        p = ops.carafe_head_folded(xd, ed, *ps, H, H, s) if folded else ops.carafe_head(xd, ed, *ps, H, H, s)
        p.backward(dpd)
    verify(ga, [p], ws=mod("_lib").lib().csu_carafe_head_bwd_workspace(B, H, H, C, s))
    assert p.dtype == F32 and p.shape == ref.shape
    close(p, ref, dtype)
    close(xd.grad, x64.grad, dtype)
    close(ed.grad, e64.grad, dtype)
    for t, r in zip(ps, prefs):
        close(t.grad, r.reshape(t.shape), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sigmoid_head_odd_rows(dtype, monkeypatch):
    ops = mod("ops")
    d = dev()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 333, 64, generator=g).to(dtype)
    w = torch.randn(1, 64, 1, 1, generator=g) * 0.2
    dp = torch.randn(3, 333, generator=g)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = torch.sigmoid(x64 @ w64.view(64))
    ref.backward(dp.double())
    ga = GuardedAlloc()
    xd, wd, dpd = gin(ga, x, d, grad=True), gin(ga, w, d, grad=True), gin(ga, dp, d)
    with guarded(monkeypatch, "ops", registry=ga):
        p = ops.sigmoid_head(xd, wd)
        p.backward(dpd)
    verify(ga, [p], ws=mod("_lib").lib().csu_head_bwd_workspace(3 * 333, 64))
    assert p.dtype == F32
    close(p, ref, dtype)
    close(xd.grad, x64.grad, dtype)
    close(wd.grad, w64.grad, dtype)


# ---------------------------------------------------------------------------------------------
# column sum, Linear weight gradient
# ---------------------------------------------------------------------------------------------
def _colsum_first_rows(cols, code):
    """The smallest row count for which csu_colsum_workspace is non-zero (the split path)."""
    L = mod("_lib").lib()
    hi = 1
    while not L.csu_colsum_workspace(hi, cols, code):
        hi *= 2
        assert hi < 1 << 24
    return next(r for r in range(hi // 2 + 1, hi + 1) if L.csu_colsum_workspace(r, cols, code))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 8), (7, 40), "split", "split-1"])
def test_colsum(shape, dtype, monkeypatch):
    ops, L = mod("ops"), mod("_lib")
    d = dev()
    if isinstance(shape, str):
        first = _colsum_first_rows(200, L.CSU_F32 if dtype == F32 else L.CSU_BF16)
        shape = (first if shape == "split" else first - 1, 200)
    rows, cols = shape
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + cols)).to(dtype)
    ref = x.double().sum(0)
    nws = L.lib().csu_colsum_workspace(rows, cols, L.CSU_F32 if dtype == F32 else L.CSU_BF16)
    ga = GuardedAlloc()
    xd = gin(ga, x, d)
    with guarded(monkeypatch, "ops", registry=ga):
        a = ops.colsum(xd)
    verify(ga, [a], ws=nws)
    finite(a)
    torch.testing.assert_close(a.double().cpu(), ref, rtol=1e-5, atol=1e-3 * max(1.0, rows ** 0.5) * 1e-2)


def _wgrad_check(dw, db, dy, x, dtype):
    """test_linear_wgrad_kernel's criterion."""
    M = dy.shape[0]
    ref_w, ref_b = dy.double().t() @ x.double(), dy.double().sum(0)
    tol = 1e-5 if dtype == F32 else 1e-2
    finite(dw, db)
    assert float((dw.double().cpu() - ref_w).abs().max()) <= tol * max(float(ref_w.abs().max()), M ** 0.5)
    assert float((db.double().cpu() - ref_b).abs().max()) <= tol * max(float(ref_b.abs().max()), M ** 0.5)


def _wgrad_inputs(M, N, K, dtype, seed=0):
    g = torch.Generator().manual_seed(M + N + K + seed)
    return torch.randn(M, N, generator=g).to(dtype), torch.randn(M, K, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(77, 64, 8), (1000, 16, 64)])
def test_linear_wgrad(M, N, K, dtype, monkeypatch):
    ops, L = mod("ops"), mod("_lib").lib()
    d = dev()
    dy, x = _wgrad_inputs(M, N, K, dtype)
    ga = GuardedAlloc()
    dyd, xd = gin(ga, dy, d), gin(ga, x, d)
    with guarded(monkeypatch, "ops", registry=ga):
        dw, db = ops.linear_wgrad(dyd, xd)
    verify(ga, [dw, db], ws=L.csu_gemm_f32_workspace(2, N, K, M) if dtype == F32 else L.csu_linear_wgrad_workspace(M, N, K))
    _wgrad_check(dw, db, dy, x, dtype)


def test_linear_wgrad_caller_buffers(monkeypatch):
    """The caller-provided out= / work= form, once: buffers of exactly the documented sizes."""
    ops, L = mod("ops"), mod("_lib").lib()
    d = dev()
    M, N, K = 1000, 16, 64
    dy, x = _wgrad_inputs(M, N, K, BF16, seed=1)
    ga = GuardedAlloc()
    dyd, xd = gin(ga, dy, d), gin(ga, x, d)
    out = ga.empty(N * K + N, dtype=F32, device=d)
    work = ga.empty(max(L.csu_linear_wgrad_workspace(M, N, K), 16), dtype=torch.uint8, device=d)
    with guarded(monkeypatch, "ops", registry=ga):
        dw, db = ops.linear_wgrad(dyd, xd, out=out, work=work)
    verify(ga, [dw, db])
    _wgrad_check(dw, db, dy, x, BF16)


@pytest.mark.parametrize("tn,tk,chunks", [(64, 64, 1), (128, 64, 5), (64, 128, 37)])
def test_linear_wgrad_tuned_plans(tn, tk, chunks):
    """csu_linear_wgrad_tuned at (700, 32, 128): the slab workspace is exactly what
    csu_linear_wgrad_tuned_workspace claims, between guards (test_linear_wgrad_plans' criterion)."""
    L_ = mod("_lib")
    L, ptr, d = L_.lib(), L_.ptr, dev()
    M, N, K = 700, 32, 128
    dy, x = _wgrad_inputs(M, N, K, BF16, seed=tn + chunks)
    ga = GuardedAlloc()
    dyd, xd = gin(ga, dy, d), gin(ga, x, d)
    n = L.csu_linear_wgrad_tuned_workspace(M, N, K, tn, tk, chunks)
    ws = ga.empty(max(n, 16), dtype=torch.uint8, device=d)
    out = ga.empty(N * K + N, dtype=F32, device=d)
    L_.check(L.csu_linear_wgrad_tuned(M, N, K, 1, ptr(dyd), ptr(xd), ptr(out), ptr(ws), n, tn, tk, chunks, L_.stream_ptr(d)),
             "linear_wgrad_tuned")
    torch.cuda.synchronize()
    verify(ga)
    dw, db = out[:N * K].view(N, K), out[N * K:]
    finite(dw, db)
    ref_w, ref_b = dy.double().t() @ x.double(), dy.double().sum(0)
    assert float((dw.double().cpu() - ref_w).abs().max()) <= 1e-2 * max(float(ref_w.abs().max()), M ** 0.5)
    assert float((db.double().cpu() - ref_b).abs().max()) <= 1e-2 * max(float(ref_b.abs().max()), M ** 0.5)


@pytest.mark.parametrize("group", [True, False], ids=["grouped", "deferred-slabs"])
def test_linear_wgrad_deferred(group, monkeypatch):
    """The grouped end-of-backward launch over Linears of mixed small shapes (rectangular group tiles,
    ragged token counts), and the deferred slab sums of the per-Linear kernel (GROUP_WGRAD off)."""
    ops = mod("ops")
    monkeypatch.setattr(ops, "GROUP_WGRAD", group)
    d = dev()
    shapes = [(100, 64, 64), (700, 256, 64), (1001, 64, 128), (77, 64, 8), (1000, 16, 64), (513, 256, 128)]
    ga = GuardedAlloc()
    ins = [_wgrad_inputs(M, N, K, BF16, seed=2) for M, N, K in shapes]
    dev_in = [(gin(ga, dy, d), gin(ga, x, d)) for dy, x in ins]
    with guarded(monkeypatch, "ops", registry=ga):
        res = [ops.linear_wgrad(dyd, xd, defer=True) for dyd, xd in dev_in]
        assert (len(ops._WG_DEFER) == len(shapes)) if group else not ops._WG_DEFER
        ops._wgrad_flush()
    assert not ops._WG_DEFER and not ops._WG_PENDING
    verify(ga, [t for r in res for t in r])
    for (dw, db), (dy, x) in zip(res, ins):
        _wgrad_check(dw, db, dy, x, BF16)


# ---------------------------------------------------------------------------------------------
# token GEMMs
# ---------------------------------------------------------------------------------------------
def _gemm_case(M, N, K, b_trans, mode, seed=0):
    g = torch.Generator().manual_seed(M + N + K + seed)
    a = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.1).bfloat16()
    b = torch.randn(K, N, generator=g).bfloat16() * 0.1 if b_trans else w
    bias = torch.randn(N, generator=g) if mode in ("bias_gelu_a", "gelu_out") else None
    aux = torch.randn(M, N, generator=g).bfloat16() if mode == "gelu_aux" else None
    res = torch.randn(M, N, generator=g) if mode == "resid" else None
    A = _gelu(a.float()).bfloat16().double() if mode == "bias_gelu_a" else a.double()
    ref = A @ (b.double() if b_trans else b.double().t())
    if bias is not None:
        ref = ref + bias.double()
    if aux is not None:
        x = aux.double()
        ref = ref * (0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5)
    if res is not None:
        ref = ref + res.double()
    return a, b, bias, aux, res, ref


@pytest.mark.parametrize("M,N,K", [(77, 64, 8), (513, 256, 32), (4099, 192, 64)])
@pytest.mark.parametrize("b_trans,mode", [(t, m) for t in (False, True) for m in ("plain", "bias_gelu_a", "gelu_aux", "resid")]
                         + [(False, "gelu_out")])   # the dual (h, gelu(h)) epilogue belongs to the b[n][k] kernel
def test_gemm(M, N, K, b_trans, mode, monkeypatch):
    ops = mod("ops")
    d = dev()
    a, b, bias, aux, res, ref = _gemm_case(M, N, K, b_trans, mode)
    odt = F32 if mode == "resid" else BF16
    ga = GuardedAlloc()
    ad, bd = gin(ga, a, d), gin(ga, b, d)
    biasd, auxd, resd = (None if t is None else gin(ga, t, d) for t in (bias, aux, res))
    with guarded(monkeypatch, "ops", registry=ga):
        out = ops.gemm(ad, bd, b_trans, odt, bias=biasd, a_gelu=mode == "bias_gelu_a", gelu_aux=auxd, resid=resd,
                       gelu_out=mode == "gelu_out")
    outs = list(out) if mode == "gelu_out" else [out]
    verify(ga, outs)
    assert outs[0].dtype == odt
    close(outs[0], ref, BF16)
    if mode == "gelu_out":
        close(outs[1], _gelu(ref), BF16)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19])
def test_gemm_tile_configs(cfg, monkeypatch):
    """Every tile configuration of the b[n][k] kernel with the dual epilogue at (1000, 64, 64)."""
    ops = mod("ops")
    d = dev()
    M, N, K = 1000, 64, 64
    a, w, bias, _, _, ref = _gemm_case(M, N, K, False, "gelu_out", seed=cfg)
    ga = GuardedAlloc()
    ad, wd, biasd = gin(ga, a, d), gin(ga, w, d), gin(ga, bias, d)
    with guarded(monkeypatch, "ops", registry=ga):
        h, gh = ops.gemm(ad, wd, False, BF16, bias=biasd, cfg=cfg, gelu_out=True)
    verify(ga, [h, gh])
    close(h, ref, BF16)
    close(gh, _gelu(ref), BF16)
    assert float((gh.float() - _gelu(h.float())).abs().max()) < 2e-2 * float(ref.abs().max())


@pytest.mark.parametrize("layout,M,N,K", [(0, 37, 64, 128), (1, 37, 64, 128), (2, 37, 64, 128), (2, 64, 16, 100)])
def test_gemm_f32(layout, M, N, K, monkeypatch):
    """csu_gemm_f32, all three layouts at (37, 64, 128); layout 2 with the A column sum.  Layout 2 reads
    A as (K, M) rows and refuses M = 37 (row lengths must be multiples of 4): the refusal is an error
    that leaves every guard intact; (64, 16, 100) of test_gemm_f32_layouts is the layout-2 case that runs."""
    ops = mod("ops")
    d = dev()
    g = torch.Generator().manual_seed(M + N + K + layout)
    ga = GuardedAlloc()
    if layout == 0:
        a, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
        bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
        ref = a.double() @ b.double().T + bias.double() + res.double()
        kw = dict(bias=gin(ga, bias, d), resid=gin(ga, res, d))
    elif layout == 1:
        a, b = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)
        ref, kw = a.double() @ b.double(), {}
    else:
        a, b = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g)
        ref, kw = a.double().T @ b.double(), dict(with_asum=True)
    ad, bd = gin(ga, a, d), gin(ga, b, d)
    if layout == 2 and M % 4:
        with guarded(monkeypatch, "ops", registry=ga):
            with pytest.raises(mod("_lib").CsuError):
                ops.gemm_f32(layout, ad, bd, M, N, K, **kw)
        verify(ga)
        return
    with guarded(monkeypatch, "ops", registry=ga):
        out = ops.gemm_f32(layout, ad, bd, M, N, K, **kw)
    outs = list(out) if layout == 2 else [out]
    verify(ga, outs, ws=mod("_lib").lib().csu_gemm_f32_workspace(layout, M, N, K))
    close(outs[0], ref, F32)
    if layout == 2:
        close(outs[1], a.double().sum(0), F32)


def test_gemm_f32_caller_buffers_and_token_splits(monkeypatch):
    """Layout 2 over enough tokens to take the ordered token splits (a non-zero workspace), into
    caller-provided out= / asum= buffers of exactly M*N and M elements."""
    ops, L = mod("ops"), mod("_lib").lib()
    d = dev()
    M, N = 64, 16
    K = 100
    while not L.csu_gemm_f32_workspace(2, M, N, K):
        K = K * 2 + 1
        assert K < 1 << 20
    g = torch.Generator().manual_seed(K)
    a, b = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g)
    ga = GuardedAlloc()
    ad, bd = gin(ga, a, d), gin(ga, b, d)
    out, asum = ga.empty(M, N, dtype=F32, device=d), ga.empty(M, dtype=F32, device=d)
    with guarded(monkeypatch, "ops", registry=ga):
        o2, s2 = ops.gemm_f32(2, ad, bd, M, N, K, with_asum=True, out=out, asum=asum)
    verify(ga, [o2, s2], ws=L.csu_gemm_f32_workspace(2, M, N, K))
    close(o2, a.double().T @ b.double(), F32)
    close(s2, a.double().sum(0), F32)


# ---------------------------------------------------------------------------------------------
# weight-streaming GEMMs
# ---------------------------------------------------------------------------------------------
def _first(pred, stop=1 << 14):
    return next(m for m in range(1, stop) if pred(m))


@pytest.mark.parametrize("N,K", [(64, 64), (192, 64), (128, 128), (768, 256)])
@pytest.mark.parametrize("mode", ["bf16_bias", "f32", "resid"])
@pytest.mark.parametrize("e4m3", [False, True], ids=["bf16w", "e4m3w"])
def test_gemm_ws(N, K, mode, e4m3, monkeypatch):
    """csu_gemm_ws / csu_gemm_ws_e4m3 at the smallest M csu_gemm_ws_supported accepts, at three times it
    with a strided token operand, and at M + 8 (no multiple of the token tile), which must be refused
    without touching a guard.  Criteria of test_gemm_ws_vs_fp64; the e4m3 form is bitwise the bf16 form
    on the dequantised weight (test_gemm_ws_e4m3_bitwise_vs_dequantised)."""
    ops, L = mod("ops"), mod("_lib")
    d = dev()
    odt = BF16 if mode == "bf16_bias" else F32
    code = L.CSU_BF16 if odt == BF16 else L.CSU_F32
    m0 = _first(lambda m: L.lib().csu_gemm_ws_supported(m, N, K, int(mode == "resid"), code))
    assert not L.lib().csu_gemm_ws_supported(m0 + 8, N, K, int(mode == "resid"), code)
    for M, ldx in ((m0, K), (3 * m0, K + 64)):
        g = torch.Generator().manual_seed(M + N + K)
        xfull = torch.randn(M + 8, ldx, generator=g).bfloat16()
        w = torch.randn(N, K, generator=g) / K ** 0.5
        bias = torch.randn(N, generator=g) if mode != "f32" else None
        resid = torch.randn(M, N, generator=g) if mode == "resid" else None
        ga = GuardedAlloc()
        xd = gin(ga, xfull, d)
        if e4m3:
            q, sc, wdq = _e4m3_rows(w.to(d))
            wq = (gin(ga, _frag8(q, False), d, fill=0), gin(ga, sc, d), 1)
            wb = wdq.cpu()
        else:
            wb = w.bfloat16()
            wq = gin(ga, _frag_ref(wb).contiguous(), d)
        biasd, residd = (None if t is None else gin(ga, t, d) for t in (bias, resid))
        x = xd[:M, :K]
        with guarded(monkeypatch, "ops", registry=ga):
            out = ops.gemm_ws(x, wq, N, odt, bias=biasd, resid=residd)
            with pytest.raises(Exception):
                ops.gemm_ws(xd[:M + 8, :K], wq, N, odt, bias=biasd)      # refused: M % tile != 0
        verify(ga, [out])
        finite(out)
        ref = xfull[:M, :K].double() @ wb.double().t()
        if bias is not None:
            ref = ref + bias.double()
        if resid is not None:
            ref = ref + resid.double()
        err, scale = float((out.double().cpu() - ref).abs().max()), float(ref.abs().max())
        if odt == F32:
            assert err <= 1e-5 * scale, (err, scale)
        else:
            assert err <= 2 ** -8 * scale + 1e-6, (err, scale)


@pytest.mark.parametrize("C", [64, 128, 256])
@pytest.mark.parametrize("e4m3", [False, True], ids=["bf16w", "e4m3w"])
def test_gemm_ws_ln(C, e4m3, monkeypatch):
    """csu_gemm_ws_ln / _ln_e4m3 (proj + residual with norm2 in the epilogue) at the smallest M it
    supports and three times it; M - 32 is refused with the guards intact.  test_gemm_ws_ln_vs_fp64's
    criteria: y bitwise csu_gemm_ws's residual epilogue, h / mean / rstd vs an fp64 LayerNorm of y."""
    ops, L_ = mod("ops"), mod("_lib")
    L, ptr, d = L_.lib(), L_.ptr, dev()
    m0 = _first(lambda m: L.csu_gemm_ws_ln_supported(m, C, C))
    for M in (m0, 3 * m0):
        g = torch.Generator().manual_seed(M + C)
        x = torch.randn(M, C, generator=g).bfloat16()
        w = torch.randn(C, C, generator=g) / C ** 0.5
        bias = torch.randn(C, generator=g)
        res = torch.randn(M, C, generator=g) * 2 + 0.5
        gam, bet = torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g) * 0.1
        ga = GuardedAlloc()
        xd, biasd, resd, gamd, betd = (gin(ga, t, d) for t in (x, bias, res, gam, bet))
        if e4m3:
            q, sc, wdq = _e4m3_rows(w.to(d))
            f8, scd = gin(ga, _frag8(q, False), d, fill=0), gin(ga, sc, d)
            wf = gin(ga, _frag_ref(wdq).contiguous(), d)
        else:
            wf = gin(ga, _frag_ref(w.bfloat16()).contiguous(), d)
        y, h = ga.empty(M, C, dtype=F32, device=d), ga.empty(M, C, dtype=BF16, device=d)
        mean, rstd = ga.empty(M, dtype=F32, device=d), ga.empty(M, dtype=F32, device=d)
        st = L_.stream_ptr(d)
        with guarded(monkeypatch, "ops", registry=ga):
            ref_y = ops.gemm_ws(xd, wf, C, F32, bias=biasd, resid=resd)
            if e4m3:
                rc = L.csu_gemm_ws_ln_e4m3(M, C, ptr(xd), C, ptr(f8), ptr(scd), ptr(biasd), ptr(resd), ptr(y), ptr(gamd),
                                           ptr(betd), 1e-5, ptr(h), ptr(mean), ptr(rstd), st)
                bad = L.csu_gemm_ws_ln_e4m3(M - 32, C, ptr(xd), C, ptr(f8), ptr(scd), ptr(biasd), ptr(resd), ptr(y), ptr(gamd),
                                            ptr(betd), 1e-5, ptr(h), ptr(mean), ptr(rstd), st)
            else:
                rc = L.csu_gemm_ws_ln(M, C, ptr(xd), C, ptr(wf), ptr(biasd), ptr(resd), ptr(y), ptr(gamd), ptr(betd), 1e-5,
                                      ptr(h), ptr(mean), ptr(rstd), st)
                bad = L.csu_gemm_ws_ln(M - 32, C, ptr(xd), C, ptr(wf), ptr(biasd), ptr(resd), ptr(y), ptr(gamd), ptr(betd),
                                       1e-5, ptr(h), ptr(mean), ptr(rstd), st)
        assert rc == 0 and bad != 0
        verify(ga, [ref_y])
        finite(y, h, mean, rstd)
        assert torch.equal(y, ref_y)
        y64 = y.double()
        mu, var = y64.mean(-1), y64.var(-1, unbiased=False)
        h64 = (y64 - mu[:, None]) / torch.sqrt(var[:, None] + 1e-5) * gamd.double() + betd.double()
        assert float((mean.double() - mu).abs().max()) <= 1e-6 * float(y64.abs().max())
        assert float((rstd.double() / torch.rsqrt(var + 1e-5) - 1).abs().max()) <= 1e-5
        assert float((h.double() - h64).abs().max()) <= 2 ** -8 * float(h64.abs().max())


@pytest.mark.parametrize("C", [128, 256])
def test_gemm_ws_lnbwd(C, monkeypatch):
    """_LnLinearWsFn (norm1 -> qkv with the LayerNorm backward in csu_gemm_ws_lnbwd's epilogue: dx, its
    bf16 copy and the dgamma / dbeta block partials) at the smallest M csu_gemm_ws_lnbwd_supported
    accepts and three times it, against the unfused layer_norm_fork + linear, both under guards:
    test_ln_linear_ws_vs_unfused's criterion (rel 1e-2).  M + 32 is refused."""
    ops, L = mod("ops"), mod("_lib")
    d = dev()
    m0 = _first(lambda m: L.lib().csu_gemm_ws_lnbwd_supported(m, C, 3 * C))
    assert not L.lib().csu_gemm_ws_lnbwd_supported(m0 + 32, C, 3 * C)
    for M in (m0, 3 * m0):
        g = torch.Generator().manual_seed(C + M)
        x0 = torch.randn(1, M, C, generator=g)
        gam, bet = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) * 0.4 - 0.2
        w, b = torch.randn(3 * C, C, generator=g) / C ** 0.5, torch.rand(3 * C, generator=g) * 0.2 - 0.1
        G, R = torch.randn(1, M, 3 * C, generator=g), torch.randn(1, M, C, generator=g)
        res = {}
        for fused in (True, False):
            ga = GuardedAlloc()
            x, gd, bd, wd, bb = (gin(ga, t, d, grad=True) for t in (x0, gam, bet, w, b))
            Gd, Rd = gin(ga, G, d), gin(ga, R, d)
            wc = w.bfloat16()
            wf, wtf = gin(ga, _frag_ref(wc).contiguous(), d), gin(ga, _frag_ref(wc.t().contiguous()).contiguous(), d)
            with guarded(monkeypatch, "ops", registry=ga):
                if fused:
                    xa, y = ops._LnLinearWsFn.apply(x, gd, bd, wd, bb, 1e-5, wf, wtf, None)
                else:
                    with torch.autocast("cuda", dtype=BF16):
                        xa, h = ops.layer_norm_fork(x, gd, bd, 1e-5, BF16)
                        y = ops.linear(h, wd, bb)
                torch.autograd.backward([y, xa], [Gd.to(y.dtype), Rd])
            verify(ga, [y])
            res[fused] = [y.detach().float(), x.grad, gd.grad, bd.grad, wd.grad, bb.grad]
            finite(*res[fused])
        for name, u, v in zip(["y", "dx", "dgamma", "dbeta", "dW", "db"], res[True], res[False]):
            rel = float((u - v).norm() / v.norm())
            assert rel < 1e-2, (M, name, rel)


# ---------------------------------------------------------------------------------------------
# fused Mlp
# ---------------------------------------------------------------------------------------------
MLP_SHAPES = [(64, 37), (128, 1000), (256, 100)]


def _mlp_setup(C, M, g):
    fc1, fc2 = torch.nn.Linear(C, 4 * C), torch.nn.Linear(4 * C, C)
    with torch.no_grad():
        fc1.weight.copy_(torch.randn(4 * C, C, generator=g) * C ** -0.5)
        fc2.weight.copy_(torch.randn(C, 4 * C, generator=g) * (4 * C) ** -0.5)
        fc1.bias.copy_(torch.randn(4 * C, generator=g) * 0.1)
        fc2.bias.copy_(torch.randn(C, generator=g) * 0.1)
    return fc1, fc2


def _guard_params(ga, module, d):
    """Move a module to the device with every parameter in a guarded buffer."""
    module.to(d)
    for name, p in list(module.named_parameters(recurse=False)):
        setattr(module, name, torch.nn.Parameter(ga.guard_input(p.detach(), name=name)))
    return module


@pytest.mark.parametrize("ln_next", [False, True], ids=["", "ln_next"])
@pytest.mark.parametrize("drop", [False, True], ids=["", "drop"])
@pytest.mark.parametrize("C,M", MLP_SHAPES)
def test_mlp_residual(C, M, drop, ln_next, monkeypatch):
    """mlp_residual (one fused forward launch, the fused backward -- with in-kernel weight gradients at
    C = 64 -- and the LayerNorm of the output for the next block) vs the fp64 Mlp + residual under the
    same dropout masks: y and every gradient at test_fused_mlp_residual_matches_unfused's tolerance, the
    attached LayerNorm at test_mlp_fwd_ln_next's."""
    ops, rng = mod("ops"), mod("rng")
    d = dev()
    g = torch.Generator().manual_seed(C + M)
    fc1, fc2 = _mlp_setup(C, M, g)
    res = torch.randn(1, M, C, generator=g)
    x = torch.randn(1, M, C, generator=g).bfloat16()
    gy = torch.randn(1, M, C, generator=g)
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) * 0.4 - 0.2
    p = 0.3
    snap = torch.tensor([5, 2], dtype=torch.int64, device=d)
    mh = mo = 1.0
    if drop:
        mh = rng.dropout_mask(snap, 21, p, M * 4 * C).view(1, M, 4 * C).double().cpu() / (1 - p)
        mo = rng.dropout_mask(snap, 22, p, M * C).view(1, M, C).double().cpu() / (1 - p)
    r64, x64 = res.double().requires_grad_(True), x.double().requires_grad_(True)
    ps = [t.detach().double().requires_grad_(True) for t in (fc1.weight, fc1.bias, fc2.weight, fc2.bias)]
    ref = r64 + mo * F.linear(F.gelu(F.linear(x64, ps[0], ps[1])) * mh, ps[2], ps[3])
    ref.backward(gy.double())
    ga = GuardedAlloc()
    _guard_params(ga, fc1, d), _guard_params(ga, fc2, d)
    resd, xd, gyd = gin(ga, res, d, grad=True), gin(ga, x, d, grad=True), gin(ga, gy, d)
    gamd, betd = gin(ga, gam, d), gin(ga, bet, d)
    md = ops.MlpDrop(snap, 21, 22, p, None, M) if drop else None
    with guarded(monkeypatch, "ops", registry=ga):
        with torch.autocast("cuda", dtype=BF16):
            y = ops.mlp_residual(resd, xd, fc1, fc2, md, ln_next=(gamd, betd, 1e-5) if ln_next else None)
        y.backward(gyd)
    pre = getattr(y, "_csu_ln", None)
    verify(ga, [y] + ([pre[3], pre[4], pre[5]] if ln_next else []))
    assert (pre is not None) == ln_next
    close(y, ref, BF16)
    for got, r in zip([resd.grad, xd.grad, fc1.weight.grad, fc1.bias.grad, fc2.weight.grad, fc2.bias.grad],
                      [r64.grad, x64.grad] + [q.grad for q in ps]):
        close(got, r, BF16)
    if ln_next:
        finite(pre[3], pre[4], pre[5])
        yd = y.detach().double().view(-1, C)
        mu = yd.mean(-1)
        var = ((yd - mu[:, None]) ** 2).mean(-1)
        lref = (yd - mu[:, None]) / torch.sqrt(var[:, None] + 1e-5) * gamd.double() + betd.double()
        torch.testing.assert_close(pre[4].double(), mu, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(pre[5].double(), 1 / torch.sqrt(var + 1e-5), rtol=1e-4, atol=0)
        assert float((pre[3].double().view(-1, C) - lref).abs().max()) <= 2 ** -7 * float(lref.abs().max())


@pytest.mark.parametrize("C,M", MLP_SHAPES + [(128, 64), (128, 192), (256, 64), (256, 192)])
def test_ln_mlp_residual(C, M, monkeypatch):
    """ln_mlp_residual (norm2 -> Mlp with the LayerNorm backward in csu_mlp_bwd_ln's row phase: dx, its
    bf16 copy and the dgamma / dbeta partials written over the dead LDS ring).  The three Mlp shapes of
    this file have no csu_mlp_bwd_ln (C = 64, or M no multiple of 64): the op declines with None and
    allocates nothing.  M = 64 (one workgroup) and 192 (three panels) run, against the switch-off path
    (layer_norm_fork + mlp_residual) under guards too and an fp64 reference of the junction, by
    test_ln_mlp_residual_block's criterion: the fused error at most twice the unfused plus 1e-6 max|ref|."""
    ops = mod("ops")
    d = dev()
    g = torch.Generator().manual_seed(11 + C + M)
    fc1, fc2 = _mlp_setup(C, M, g)
    ln = torch.nn.LayerNorm(C)
    with torch.no_grad():
        ln.weight.copy_(torch.rand(C, generator=g) + 0.5)
        ln.bias.copy_(torch.rand(C, generator=g) * 0.4 - 0.2)
    x0 = torch.randn(1, M, C, generator=g) + 2.0 * torch.randn(1, M, 1, generator=g)
    G = torch.randn(1, M, C, generator=g)
    ga = GuardedAlloc()
    for m_ in (ln, fc1, fc2):
        _guard_params(ga, m_, d)
    params = [ln.weight, ln.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias]
    supported = bool(mod("_lib").lib().csu_mlp_bwd_ln_supported(M, C))
    if not supported:
        n0 = len(ga)
        xd = gin(ga, x0, d, grad=True)
        with guarded(monkeypatch, "ops", registry=ga):
            with torch.autocast("cuda", dtype=BF16):
                assert ops.ln_mlp_residual(xd, ln, fc1, fc2, None, None) is None
        assert len(ga) == n0 + 1
        verify(ga)
        return
    outs = {}
    gamn, betn = gin(ga, torch.rand(C, generator=g) + 0.5, d), gin(ga, torch.rand(C, generator=g) * 0.4 - 0.2, d)
    for fused in (False, True):
        for q in params:
            q.grad = None
        xd, Gd = gin(ga, x0, d, grad=True), gin(ga, G, d)
        with guarded(monkeypatch, "ops", registry=ga):
            with torch.autocast("cuda", dtype=BF16):
                if fused:
                    snap = torch.tensor([5, 2], dtype=torch.int64, device=d)
                    assert ops.ln_mlp_residual(xd, ln, fc1, fc2, ops.MlpDrop(snap, 21, 22, 0.3, None, M), None) is None
                    y = ops.ln_mlp_residual(xd, ln, fc1, fc2, None, (gamn, betn, 1e-5))     # + the next block's norm1
                    assert y is not None
                    pre = y._csu_ln
                else:
                    xb, h2 = ops.layer_norm_fork(xd, ln.weight, ln.bias, ln.eps, BF16)
                    y = ops.mlp_residual(xb, h2, fc1, fc2, None, ln_next=None)
            y.backward(Gd)
        verify(ga, [y])
        outs[fused] = (y.detach().clone(), [xd.grad.clone()] + [q.grad.detach().clone() for q in params])
        finite(*outs[fused][1], y)
    assert torch.equal(outs[False][0], outs[True][0])
    # the LayerNorm of y for the next block, written by the fused forward (test_mlp_fwd_ln_next's criteria)
    assert ga.contains(pre[3]) and ga.contains(pre[4]) and ga.contains(pre[5])
    finite(pre[3], pre[4], pre[5])
    yd = outs[True][0].double().view(-1, C)
    mu = yd.mean(-1)
    var = ((yd - mu[:, None]) ** 2).mean(-1)
    lref = (yd - mu[:, None]) / torch.sqrt(var[:, None] + 1e-5) * gamn.double() + betn.double()
    torch.testing.assert_close(pre[4].double(), mu, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(pre[5].double(), 1 / torch.sqrt(var + 1e-5), rtol=1e-4, atol=0)
    assert float((pre[3].double().view(-1, C) - lref).abs().max()) <= 2 ** -7 * float(lref.abs().max())
    xr = x0.double().requires_grad_(True)
    pr = [q.detach().double().cpu().requires_grad_(True) for q in params]
    hr = F.layer_norm(xr, (C,), pr[0], pr[1], ln.eps)
    yr = xr + F.gelu(hr @ pr[2].t() + pr[3]) @ pr[4].t() + pr[5]
    (yr * G.double()).sum().backward()
    for name, a, b, r in zip(["dx", "dgamma", "dbeta", "dW1", "db1", "dW2", "db2"], outs[True][1], outs[False][1],
                             [xr.grad] + [q.grad for q in pr]):
        ef, eu, mx = float((a.double().cpu() - r).abs().max()), float((b.double().cpu() - r).abs().max()), float(r.abs().max())
        assert ef <= 2 * eu + 1e-6 * mx, (name, ef, eu, mx)


def _mlp_raw(C, M, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g).bfloat16()
    w1 = (torch.randn(4 * C, C, generator=g) * C ** -0.5).bfloat16()
    w2 = (torch.randn(C, 4 * C, generator=g) * (4 * C) ** -0.5).bfloat16()
    b1, b2 = torch.randn(4 * C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    res = torch.randn(M, C, generator=g)
    dy = torch.randn(M, C, generator=g).bfloat16()
    return x, w1, w2, b1, b2, res, dy


@pytest.mark.parametrize("C,M", [(128, 1000)])
def test_mlp_deep_ring(C, M, monkeypatch):
    """The C = 128 product Mlp through the C ABI, csu_mlp_fwd_dp and csu_mlp_bwd_dp (the deep-ring backward), and the
    per-panel backward csu_mlp_bwd_per_panel, with and without dropout + DropPath into guarded y, dh, g, dx: the fp64
    criteria of test_mlp_bwd_deep_ring_vs_fp64, and the same for y against the fp64 Mlp + residual."""
    L_, rng, ops = mod("_lib"), mod("rng"), mod("ops")
    L, ptr, d = L_.lib(), L_.ptr, dev()
    x, w1, w2, b1, b2, res, dy = _mlp_raw(C, M, C + M + 1)
    X, W1, W2, B1, B2, R, DY = (t.double() for t in (x, w1, w2, b1, b2, res, dy))
    st = L_.stream_ptr(d)
    for drop in (False, True):
        ga = GuardedAlloc()
        xd, w1d, w2d, b1d, b2d, resd, dyd = (gin(ga, t, d) for t in (x, w1, w2, b1, b2, res, dy))
        if drop:
            snap = torch.tensor([5, 2], dtype=torch.int64, device=d)
            rps = max(1, M // 3)
            rs = gin(ga, rng.droppath_scale(snap, 30, 0.3, -(-M // rps)), d)
            md = ops.MlpDrop(snap, 21, 22, 0.3, rs, rps).c_struct()
            mh = rng.dropout_mask(snap, 21, 0.3, M * 4 * C).view(M, 4 * C).double().cpu() / 0.7
            mo = rng.dropout_mask(snap, 22, 0.3, M * C).view(M, C).double().cpu() / 0.7
            outm = mo * rs.double().cpu()[torch.arange(M) // rps].view(M, 1)
        else:
            md = ops.MlpDrop(None, 0, 0, 0.0).c_struct()
            md.rows_per_sample = M
            mh, outm = torch.ones(M, 4 * C, dtype=torch.float64), 1.0
        y = ga.empty(M, C, dtype=F32, device=d)
        dh, gg = ga.empty(M, 4 * C, dtype=BF16, device=d), ga.empty(M, 4 * C, dtype=BF16, device=d)
        dx = ga.empty(M, C, dtype=BF16, device=d)
        dh2, gg2 = ga.empty(M, 4 * C, dtype=BF16, device=d), ga.empty(M, 4 * C, dtype=BF16, device=d)
        dx2 = ga.empty(M, C, dtype=BF16, device=d)
        L_.check(L.csu_mlp_fwd_dp(M, C, ptr(xd), ptr(w1d), ptr(b1d), ptr(w2d), ptr(b2d), ptr(resd), ptr(y), ctypes.byref(md),
                                  st), "mlp_fwd_dp")
        L_.check(L.csu_mlp_bwd_dp(M, C, ptr(xd), ptr(dyd), ptr(w1d), ptr(b1d), ptr(w2d), ptr(dh), ptr(gg), ptr(dx),
                                  ctypes.byref(md), st), "mlp_bwd_dp")
        L_.check(L.csu_mlp_bwd_per_panel(M, C, ptr(xd), ptr(dyd), ptr(w1d), ptr(b1d), ptr(w2d), ptr(dh2), ptr(gg2), ptr(dx2),
                                         ctypes.byref(md), st), "mlp_bwd_per_panel")
        torch.cuda.synchronize()
        verify(ga)
        finite(y, dh, gg, dx, dh2, gg2, dx2)
        ref = R + outm * ((F.gelu(X @ W1.T + B1) * mh) @ W2.T + B2)
        assert float((y.double().cpu() - ref).norm() / (ref - R).norm()) < 1e-2
        h = (X @ W1.T + B1).requires_grad_(True)
        gr = F.gelu(h)
        gr.backward((DY @ W2) * mh)
        for outs in ((dh, gg, dx), (dh2, gg2, dx2)):
            for name, got, r in zip(("dh", "g", "dx"), outs, (h.grad, gr.detach() * mh, h.grad @ W1)):
                assert float((got.double().cpu() - r).norm() / r.norm()) < 1e-2, (drop, name)


def test_mlp_bwd_wgrad_c64(monkeypatch):
    """csu_mlp_bwd_wgrad at C = 64 through mlp_residual (M = 37 and a three-panel M = 165): the per-workgroup
    weight-gradient slabs are exactly csu_mlp_bwd_wgrad_workspace's two sizes, between guards."""
    ops, L = mod("ops"), mod("_lib").lib()
    assert L.csu_mlp_bwd_wgrad_supported(64)
    monkeypatch.setattr(ops, "SIDE_WGRAD", False)      # as in the captured step: the weight gradients stay on the main stream
    d = dev()
    for M in (37, 165):
        g = torch.Generator().manual_seed(M)
        fc1, fc2 = _mlp_setup(64, M, g)
        res, x = torch.randn(1, M, 64, generator=g), torch.randn(1, M, 64, generator=g).bfloat16()
        gy = torch.randn(1, M, 64, generator=g)
        r64, x64 = res.double().requires_grad_(True), x.double().requires_grad_(True)
        ps = [t.detach().double().requires_grad_(True) for t in (fc1.weight, fc1.bias, fc2.weight, fc2.bias)]
        (r64 + F.linear(F.gelu(F.linear(x64, ps[0], ps[1])), ps[2], ps[3])).backward(gy.double())
        ga = GuardedAlloc()
        _guard_params(ga, fc1, d), _guard_params(ga, fc2, d)
        resd, xd, gyd = gin(ga, res, d, grad=True), gin(ga, x, d, grad=True), gin(ga, gy, d)
        launched = []
        real = ops._launch
        monkeypatch.setattr(ops, "_launch", lambda name, fn, *a, **k: (launched.append(name), real(name, fn, *a, **k))[1])
        with guarded(monkeypatch, "ops", registry=ga):
            with torch.autocast("cuda", dtype=BF16):
                y = ops.mlp_residual(resd, xd, fc1, fc2)
            y.backward(gyd)
        monkeypatch.setattr(ops, "_launch", real)
        n1, n2 = ctypes.c_size_t(), ctypes.c_size_t()
        assert L.csu_mlp_bwd_wgrad_workspace(M, 64, ctypes.byref(n1), ctypes.byref(n2)) == 0
        verify(ga, [y], ws=n1.value)
        assert ga.saw_workspace(n2.value)
        assert launched.count("mlp_bwd") == 1 and "gemm" not in launched      # the one fused backward launch
        for got, r in zip([resd.grad, xd.grad, fc1.weight.grad, fc1.bias.grad, fc2.weight.grad, fc2.bias.grad],
                          [r64.grad, x64.grad] + [q.grad for q in ps]):
            close(got, r, BF16)


@pytest.mark.parametrize("drop", [False, True], ids=["", "drop"])
@pytest.mark.parametrize("C,M", MLP_SHAPES)
def test_mlp_fp8(C, M, drop, monkeypatch):
    """csu_mlp_fp8_fwd / csu_mlp_fp8_bwd (e4m3 weights, MX-quantised activations) on operands quantised and
    laid out under guards (Fp8Weights), into guarded y, dh, g_q, dx: the relative-L2 gates of
    test_gpu_fp8.py::test_mlp_fp8_fused_vs_oracle against the fp64 restatement of the same roundings."""
    from oracle import fp8_ref as Q
    L_, rng, ops = mod("_lib"), mod("rng"), mod("ops")
    L, ptr, d = L_.lib(), L_.ptr, dev()
    assert L.csu_mlp_fp8_supported(C)
    g = torch.Generator().manual_seed(C + M)
    x = torch.randn(M, C, generator=g).bfloat16()
    w1, w2 = torch.randn(4 * C, C, generator=g) * C ** -0.5, torch.randn(C, 4 * C, generator=g) * (4 * C) ** -0.5
    b1, b2 = torch.randn(4 * C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    res = torch.randn(M, C, generator=g)
    dz = (torch.randn(M, C, generator=g) * 1e-3).bfloat16()
    ga = GuardedAlloc()
    xd, w1d, w2d, b1d, b2d, resd, dzd = (gin(ga, t, d) for t in (x, w1, w2, b1, b2, res, dz))
    snap = torch.tensor([5, 2], dtype=torch.int64, device=d)
    if drop:
        rps = max(1, M // 3)
        rs = gin(ga, rng.droppath_scale(snap, 30, 0.3, -(-M // rps)), d)
        md = ops.MlpDrop(snap, 21, 22, 0.3, rs, rps).c_struct()
        mh = rng.dropout_mask(snap, 21, 0.3, M * 4 * C).view(M, 4 * C).double().cpu() / 0.7
        mo = rng.dropout_mask(snap, 22, 0.3, M * C).view(M, C).double().cpu() / 0.7
        outm = mo * rs.double().cpu()[torch.arange(M) // rps].view(M, 1)
    else:
        md = ops.MlpDrop(None, 0, 0, 0.0).c_struct()
        md.rows_per_sample = M
        mh, outm = None, torch.ones(M, 1, dtype=torch.float64)
    st = L_.stream_ptr(d)
    with guarded(monkeypatch, "ops", registry=ga):
        fp8 = ops.Fp8Weights([w1d, w2d], mlp_pairs=[(w1d, w2d)])
        fp8.quantize()
        w1q, sw1, w2p, sw2, w2t, w1tp = fp8.mlp_operands(w1d, w2d)
        y = ops.torch.empty(M, C, dtype=F32, device=d)
        dh, gq = ops.torch.empty(M, 4 * C, dtype=BF16, device=d), ops.torch.empty(M, 4 * C, dtype=BF16, device=d)
        dx = ops.torch.empty(M, C, dtype=BF16, device=d)
        L_.check(L.csu_mlp_fp8_fwd(M, C, ptr(xd), ptr(w1q), ptr(sw1), ptr(b1d), ptr(w2p), ptr(sw2), ptr(b2d), ptr(resd), ptr(y),
                                   ctypes.byref(md), st), "mlp_fp8_fwd")
        L_.check(L.csu_mlp_fp8_bwd(M, C, ptr(xd), ptr(dzd), ptr(w1q), ptr(sw1), ptr(b1d), ptr(w2t), ptr(sw2), ptr(w1tp),
                                   ptr(dh), ptr(gq), ptr(dx), ctypes.byref(md), st), "mlp_fp8_bwd")
    verify(ga, [y, dh, gq, dx, w1q, sw1, w2p, sw2, w2t, w1tp])
    finite(y, dh, gq, dx)
    W1d, _, S1 = Q.quant_rows(w1)
    W2d, _, S2 = Q.quant_rows(w2)
    assert torch.equal(S1.float(), sw1.cpu()) and torch.equal(S2.float(), sw2.cpu())
    X, B1, B2, R, DZ = (t.double() for t in (x, b1, b2, res, dz))
    yref = R + outm * Q.fp8_mlp(X, W1d, B1, W2d, B2, S1, S2, mh)

    def rel(a, b):
        return float((a.double().cpu() - b).norm() / b.norm())

    assert rel(y.cpu() - res, yref - R) < 1e-2
    h = Q.mx_quant(X) @ W1d.T + B1
    gqr = Q.mx_quant(F.gelu(h) * (mh if mh is not None else 1))
    assert rel(gq, gqr) < 1e-2
    assert float((gq.double().cpu() != gqr).double().mean()) < 2e-3
    q1, q2 = W1d / S1[:, None], W2d / S2[:, None]
    dgelu = 0.5 * (1 + torch.erf(h / 2 ** 0.5)) + h * torch.exp(-0.5 * h * h) / (2 * torch.pi) ** 0.5
    dhr = (Q.mx_quant(DZ * S2) @ q2) * dgelu * (mh if mh is not None else 1)
    assert rel(dh, dhr) < 5e-3
    assert rel(dx, Q.mx_quant(dhr * S1) @ q1) < 1e-2


# ---------------------------------------------------------------------------------------------
# convolution
# ---------------------------------------------------------------------------------------------
GB_CONV_CASES = [(2, 32, 3, 64, 7, 4, 2), (2, 9, 32, 36, 3, 1, 1), (1, 10, 32, 68, 3, 1, 1), (2, 6, 40, 16, 1, 1, 0),
                 (2, 11, 64, 128, 3, 2, 1), (1, 13, 12, 20, 5, 3, 2), (1, 12, 8, 24, 3, 1, 1)]
assert set(GB_CONV_CASES) <= set(CONV_CASES)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", GB_CONV_CASES)
def test_conv2d(case, dtype, monkeypatch):
    ops, L = mod("ops"), mod("_lib")
    d = dev()
    B, H, C, N, k, s, p = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, H, H, C, generator=g).to(dtype)
    w = torch.randn(N, C, k, k, generator=g) * (1.0 / (C * k * k) ** 0.5)
    b = torch.randn(N, generator=g) * 0.1
    x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.conv2d(x64.permute(0, 3, 1, 2), w64, b64, stride=s, padding=p).permute(0, 2, 3, 1)
    gy = torch.randn(ref.shape, generator=g).to(dtype)
    ref.backward(gy.double())
    ga = GuardedAlloc()
    xd, wd, bd, gyd = gin(ga, x, d, grad=True), gin(ga, w, d, grad=True), gin(ga, b, d, grad=True), gin(ga, gy, d)
    with guarded(monkeypatch, "ops", registry=ga):
        with torch.autocast("cuda", dtype=BF16, enabled=dtype == BF16):
            y = ops.conv2d(xd, wd, bd, s, p)
        y.backward(gyd.to(y.dtype))
    gm = ops._conv_geom(B, H, H, ops._pad_channels(C), N, k, k, s, p)
    code = L.CSU_F32 if dtype == F32 else L.CSU_BF16
    verify(ga, [y], ws=L.lib().csu_conv2d_wgrad_workspace(ctypes.byref(gm)))
    for op in (0, 1):
        n = L.lib().csu_conv2d_workspace(op, ctypes.byref(gm), code)
        assert not n or ga.saw_workspace(n), (op, n)
    assert tuple(y.shape) == tuple(ref.shape)
    close(y.float(), ref, dtype)
    close(xd.grad, x64.grad, dtype)
    close(wd.grad, w64.grad, dtype)
    close(bd.grad, b64.grad, dtype)


def test_conv_igemm_dma_tile_configs():
    """Every tile configuration of the LDS-DMA implicit GEMM at DMA_CONV_CASES' (1, 20, 64, 256, 3, 1, 1)
    (M = 400: a partial 256-row tile), forward and input gradient into guarded outputs:
    test_conv_igemm_dma_cfgs' criterion."""
    ops, L = mod("ops"), mod("_lib")
    d = dev()
    case = (1, 20, 64, 256, 3, 1, 1)
    assert case in DMA_CONV_CASES
    B, H, C, N, k, s, p = case
    gm = ops._conv_geom(B, H, H, C, N, k, k, s, p)
    g = torch.Generator().manual_seed(sum(case) + 7)
    x = torch.randn(B, H, H, C, generator=g).bfloat16()
    w = (torch.randn(N, C, k, k, generator=g) / (C * k * k) ** 0.5).bfloat16()
    b = torch.randn(N, generator=g)
    dy = torch.randn(B, gm.OH, gm.OW, N, generator=g).bfloat16()
    ref_f = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), s, p).permute(0, 2, 3, 1)
    ref_d = F.conv_transpose2d(dy.double().permute(0, 3, 1, 2), w.double(), None, s, p).permute(0, 2, 3, 1)
    ga = GuardedAlloc()
    xd, dyd, bd = gin(ga, x, d), gin(ga, dy, d), gin(ga, b, d)
    w_ohwi, w_ihwo = gin(ga, w.permute(0, 2, 3, 1).contiguous(), d), gin(ga, w.permute(1, 2, 3, 0).contiguous(), d)
    st = torch.cuda.current_stream().cuda_stream
    ran = 0
    for op, src, wt, bias, ncols, cs, ref in ((0, xd, w_ohwi, bd, N, C, ref_f), (1, dyd, w_ihwo, None, C, N, ref_d)):
        for cfg, bn in IGEMM_DMA_BN.items():
            out = ga.empty(tuple(ref.shape), dtype=BF16, device=d)
            e = L.lib().csu_conv2d_ex(op, ctypes.byref(gm), L.CSU_BF16, src.data_ptr(), wt.data_ptr(),
                                      bias.data_ptr() if bias is not None else None, out.data_ptr(), cfg, st)
            torch.cuda.synchronize()
            if ncols % bn or cs % 64:
                assert e != 0, (op, cfg)
                continue
            assert e == 0, (op, cfg, L.lib().csu_last_error_string())
            ran += 1
            finite(out)
            err = float((out.double().cpu() - ref).norm() / ref.norm())
            assert err < 4e-3, (op, cfg, err)
    assert ran >= len(IGEMM_DMA_BN)
    verify(ga)


def test_conv2d_cat(monkeypatch):
    """conv2d_cat on the two-source kernels at (1, 32, 64, 64, 64) of test_conv2d_cat_two_source (not
    split-eligible: the materialised cat) and at the eligible (1, 64, 64, 64, 64)."""
    ops = mod("ops")
    d = dev()
    for B, H, Ca, Cb, N in ((1, 32, 64, 64, 64), (1, 64, 64, 64, 64)):
        g = torch.Generator().manual_seed(B + H + Ca + Cb + N)
        xa, xb = torch.randn(B, H, H, Ca, generator=g).bfloat16(), torch.randn(B, H, H, Cb, generator=g).bfloat16()
        w = torch.randn(N, Ca + Cb, 3, 3, generator=g) * (1.0 / (9 * (Ca + Cb)) ** 0.5)
        b = torch.randn(N, generator=g) * 0.1
        xa64, xb64 = xa.double().requires_grad_(True), xb.double().requires_grad_(True)
        w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
        ref = F.conv2d(torch.cat([xa64, xb64], -1).permute(0, 3, 1, 2), w64, b64, 1, 1).permute(0, 2, 3, 1)
        gy = torch.randn(ref.shape, generator=g).bfloat16()
        ref.backward(gy.double())
        gm = ops._conv_geom(B, H, H, Ca + Cb, N, 3, 3, 1, 1)
        assert bool(mod("_lib").lib().csu_conv2d_split_ok(ctypes.byref(gm), Ca)) == (H % 64 == 0)
        ga = GuardedAlloc()
        xad, xbd, wd, bd = (gin(ga, t, d, grad=True) for t in (xa, xb, w, b))
        gyd = gin(ga, gy, d)
        with guarded(monkeypatch, "ops", registry=ga):
            with torch.autocast("cuda", dtype=BF16):
                y = ops.conv2d_cat(xad, xbd, wd, bd, 1)
            y.backward(gyd)
        verify(ga, [y], ws=mod("_lib").lib().csu_conv2d_wgrad_workspace(ctypes.byref(gm)))
        for got, r in ((y.float(), ref), (xad.grad, xa64.grad), (xbd.grad, xb64.grad), (wd.grad, w64.grad),
                       (bd.grad, b64.grad)):
            close(got, r, BF16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_transpose2d(dtype, monkeypatch):
    ops = mod("ops")
    d = dev()
    B, H, Cin, Cout = 1, 5, 128, 64
    g = torch.Generator().manual_seed(B + H + Cin)
    x = torch.randn(B, H, H, Cin, generator=g).to(dtype)
    w, b = torch.randn(Cin, Cout, 2, 2, generator=g) * 0.1, torch.randn(Cout, generator=g) * 0.1
    x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.conv_transpose2d(x64.permute(0, 3, 1, 2), w64, b64, stride=2).permute(0, 2, 3, 1)
    gy = torch.randn(ref.shape, generator=g).to(dtype)
    ref.backward(gy.double())
    ga = GuardedAlloc()
    xd, wd, bd, gyd = gin(ga, x, d, grad=True), gin(ga, w, d, grad=True), gin(ga, b, d, grad=True), gin(ga, gy, d)
    with guarded(monkeypatch, "ops", registry=ga):
        with torch.autocast("cuda", dtype=BF16, enabled=dtype == BF16):
            y = ops.conv_transpose2d(xd, wd, bd, 2)
        y.backward(gyd.to(y.dtype))
    verify(ga, [y])
    for got, r in ((y.float(), ref), (xd.grad, x64.grad), (wd.grad, w64.grad), (bd.grad, b64.grad)):
        close(got, r, dtype)


def test_conv_c16_carafe4_encoder():
    """The CARAFE4 encoder Conv2d(16, 144, 3, 1, 1) at (1, 5, 64): the few-channel kernels (cfg 21) and the
    default dispatch, forward and input gradient into guarded outputs (test_conv_c16_carafe4_encoder)."""
    ops, L = mod("ops"), mod("_lib")
    d = dev()
    B, H, W = 1, 5, 64
    gm = ops._conv_geom(B, H, W, 16, 144, 3, 3, 1, 1)
    g = torch.Generator().manual_seed(B * 1000 + H + W)
    x = torch.randn(B, H, W, 16, generator=g).bfloat16()
    w = (torch.randn(144, 16, 3, 3, generator=g) / 12.0).bfloat16()
    b = torch.randn(144, generator=g)
    dy = torch.randn(B, H, W, 144, generator=g).bfloat16()
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), 1, 1).permute(0, 2, 3, 1)
    ref_d = F.conv_transpose2d(dy.double().permute(0, 3, 1, 2), w.double(), None, 1, 1).permute(0, 2, 3, 1)
    ga = GuardedAlloc()
    xd, bd, dyd = gin(ga, x, d), gin(ga, b, d), gin(ga, dy, d)
    w_ohwi, w_ihwo = gin(ga, w.permute(0, 2, 3, 1).contiguous(), d), gin(ga, w.permute(1, 2, 3, 0).contiguous(), d)
    st = torch.cuda.current_stream().cuda_stream
    for op, src, wt, bias, r in ((0, xd, w_ohwi, bd, ref), (1, dyd, w_ihwo, None, ref_d)):
        outs = []
        for cfg in (21, -1):
            out = ga.empty(tuple(r.shape), dtype=BF16, device=d)
            e = L.lib().csu_conv2d_ex(op, ctypes.byref(gm), L.CSU_BF16, src.data_ptr(), wt.data_ptr(),
                                      bias.data_ptr() if bias is not None else None, out.data_ptr(), cfg, st)
            assert e == 0, L.lib().csu_last_error_string()
            outs.append(out)
        torch.cuda.synchronize()
        finite(*outs)
        assert float((outs[0].double().cpu() - r).norm() / r.norm()) < 4e-3
        assert torch.equal(outs[0], outs[1])
    verify(ga)


# ---------------------------------------------------------------------------------------------
# plain UNet ops
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 5, 7, 64), (4, 9, 11, 72)])
def test_bn_relu_nhwc(shape, dtype, training, monkeypatch):
    """bn_relu_nhwc, training (the running statistics are an in-place input by contract) and eval (they
    are not): the criteria of test_bn_relu_train_vs_torch / test_bn_relu_eval_vs_torch."""
    from test_gpu_unet import _ref_bn, _rel
    unet = mod("unet")
    d = dev()
    g = torch.Generator().manual_seed(sum(shape))
    C = shape[-1]
    x = (torch.randn(shape, generator=g) * 3 + 5).to(dtype)
    dy = torch.randn(shape, generator=g).to(dtype)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    ref = {k: v.double().clone() for k, v in bn.state_dict().items() if v.is_floating_point()}
    x64 = x.double().requires_grad_(True)
    w64, b64 = ref["weight"].requires_grad_(True), ref["bias"].requires_grad_(True)
    rm0, rv0 = ref["running_mean"].clone(), ref["running_var"].clone()
    yr = _ref_bn(x64, w64, b64, ref["running_mean"], ref["running_var"], training, True)
    yr.backward(dy.double())
    ga = GuardedAlloc()
    bnd = _guard_params(ga, bn, d)
    bnd.running_mean = ga.guard_input(bnd.running_mean, inplace=training, name="running_mean")
    bnd.running_var = ga.guard_input(bnd.running_var, inplace=training, name="running_var")
    bnd.train(training)
    xd, dyd = gin(ga, x, d, grad=True), gin(ga, dy, d)
    with guarded(monkeypatch, "unet", registry=ga):
        y = unet.bn_relu_nhwc(xd, bnd, True)
        y.backward(dyd)
    verify(ga, [y], ws=mod("_lib").lib().csu_bn_workspace(x.numel() // C, C))
    assert y.dtype == dtype and y.shape == x.shape
    finite(y, xd.grad, bnd.weight.grad, bnd.bias.grad, bnd.running_mean, bnd.running_var)
    if not training:
        tol = 1e-4 if dtype == F32 else 2e-2
        assert _rel(y.cpu(), yr.detach()) < tol and _rel(xd.grad.cpu(), x64.grad) < tol
        assert _rel(bnd.weight.grad.cpu(), w64.grad) < tol and _rel(bnd.bias.grad.cpu(), b64.grad) < tol
        assert torch.equal(bnd.running_mean.cpu().double(), rm0) and torch.equal(bnd.running_var.cpu().double(), rv0)
        return
    if dtype == F32:
        torch.testing.assert_close(y.cpu().double(), yr.detach(), rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(xd.grad.cpu().double(), x64.grad, rtol=1e-4, atol=1e-5 * float(x64.grad.abs().max()))
        torch.testing.assert_close(bnd.weight.grad.cpu().double(), w64.grad, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(bnd.bias.grad.cpu().double(), b64.grad, rtol=1e-4, atol=1e-4)
    else:
        assert _rel(y.cpu(), yr.detach()) < 2e-2 and _rel(xd.grad.cpu(), x64.grad) < 2e-2
        assert _rel(bnd.weight.grad.cpu(), w64.grad) < 2e-2 and _rel(bnd.bias.grad.cpu(), b64.grad) < 2e-2
    torch.testing.assert_close(bnd.running_mean.cpu().double(), ref["running_mean"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(bnd.running_var.cpu().double(), ref["running_var"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(3, 7, 9, 16), (1, 5, 6, 8), (2, 4, 3, 24)])
def test_maxpool2_odd_sizes(shape, dtype, monkeypatch):
    """max_pool2_nhwc with odd H and / or W (the last row / column is in no window: dx must be zero
    there, not unwritten): bit-equal to torch (test_maxpool2_vs_torch)."""
    unet = mod("unet")
    d = dev()
    g = torch.Generator().manual_seed(shape[1])
    x = torch.randint(-3, 4, shape, generator=g).to(dtype)
    dy = torch.randn(shape[0], shape[1] // 2, shape[2] // 2, shape[3], generator=g).to(dtype)
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(xr.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    yr.backward(dy)
    ga = GuardedAlloc()
    xd, dyd = gin(ga, x, d, grad=True), gin(ga, dy, d)
    with guarded(monkeypatch, "unet", registry=ga):
        y = unet.max_pool2_nhwc(xd)
        y.backward(dyd)
    verify(ga, [y])
    finite(y, xd.grad)
    assert torch.equal(y.cpu(), yr.detach()) and torch.equal(xd.grad.cpu(), xr.grad)


# ---------------------------------------------------------------------------------------------
# dropout
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdt,odt", [(F32, F32), (BF16, BF16), (BF16, F32)])
def test_dropout_and_droppath(xdt, odt, monkeypatch):
    """dropout without and with residual + DropPath scale, and droppath_scale, at a ragged (3, 37, 72):
    bit-exact against the materialised masks (test_dropout_apply_and_droppath)."""
    ops, rng = mod("ops"), mod("rng")
    d = dev()
    snap = torch.tensor([11, 3], dtype=torch.int64, device=d)
    B, L, C = 3, 37, 72
    g = torch.Generator().manual_seed(5)
    x, res, gy = torch.randn(B, L, C, generator=g).to(xdt), torch.randn(B, L, C, generator=g), torch.randn(B, L, C, generator=g)
    m = rng.dropout_mask(snap, 9, 0.3, x.numel()).view(B, L, C).float() / 0.7
    ga = GuardedAlloc()
    xd, resd, gyd = gin(ga, x, d), gin(ga, res, d), gin(ga, gy, d)
    xr = gin(ga, x, d, grad=True)
    with guarded(monkeypatch, "ops", "rng", registry=ga):
        rs = ops.droppath_scale(B, 0.5, 17, d, snap)
        y = ops.dropout(xd, 0.3, 9, snap, out_dtype=odt)
        y2 = ops.dropout(xd, 0.3, 9, snap, row_scale=rs, rows_per_sample=L, residual=resd)
        y3 = ops.dropout(xr, 0.3, 9, snap, row_scale=rs, rows_per_sample=L)
        y3.float().backward(gyd)
    verify(ga, [rs, y, y2, y3])
    finite(rs, y, y2, y3, xr.grad)
    assert torch.equal(rs, rng.dropout_mask(snap, 17, 0.5, B).float() * 2)
    assert y.dtype == odt
    torch.testing.assert_close(y.float(), (xd.float() * m).to(odt).float(), rtol=0, atol=0)
    torch.testing.assert_close(y2, resd + rs.view(B, 1, 1) * m * xd.float(), rtol=1e-6, atol=1e-6)
    gx = gyd.to(xdt).float()
    torch.testing.assert_close(xr.grad.float(), (gx * rs.view(B, 1, 1) * m).to(xdt).float(), rtol=0, atol=0)


# ---------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 4 * 1024 + 3])
def test_bce_loss_and_stats(n, monkeypatch):
    """bce_loss / bce_loss_stats incl. exact 0 / 1 probabilities, vs torch's BCE on the same device values
    (test_bce_loss_vs_torch's reference and tolerances) and the exact thresholded sums."""
    ops = mod("ops")
    d = dev()
    g = torch.Generator().manual_seed(n)
    p = torch.rand(n, generator=g)
    p[:7] = torch.tensor([0.0, 1.0, 1e-30, 1 - 1e-7, 0.5, 1.0, 0.0])
    t = (torch.rand(n, generator=g) > 0.5).float()
    t[:7] = torch.tensor([1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0])
    pb = p.to(d).requires_grad_(True)
    lb = F.binary_cross_entropy(pb, t.to(d))
    lb.backward()
    ga = GuardedAlloc()
    pa, pc, td = gin(ga, p, d, grad=True), gin(ga, p, d, grad=True), gin(ga, t, d)
    with guarded(monkeypatch, "ops", registry=ga):
        la = ops.bce_loss(pa, td)
        la.backward()
        lc, stats = ops.bce_loss_stats(pc, td)
        lc.backward()
    verify(ga, [la, lc, stats], ws=mod("_lib").lib().csu_bce_loss_workspace(n))
    finite(la, lc, stats, pa.grad, pc.grad)
    for loss, leaf in ((la, pa), (lc, pc)):
        torch.testing.assert_close(loss.detach(), lb.detach(), rtol=1e-5, atol=0)
        torch.testing.assert_close(leaf.grad, pb.grad, rtol=1e-6, atol=0)
    pred = (p > 0.5).double()
    assert torch.equal(stats.double().cpu(), torch.stack([(pred * t).sum(), pred.sum(), t.double().sum()]))


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 5, 3), (3, 1, 37, 41)])
def test_seg_loss(shape, per_sample, monkeypatch):
    """seg_loss (fused BCE + Tversky with pos_weight) at test_gpu_seg_loss.py's two smallest ragged
    shapes: its reference, tolerances and exact sums."""
    from test_gpu_seg_loss import case
    from test_seg_loss import LOSS_RTOL, PARAM_SETS, UPSTREAM, check_grad, make_criterion, ref_loss_grad
    d = dev()
    p, t = case(shape)
    ps = PARAM_SETS[2]
    ref, gref = ref_loss_grad(p, t, ps, per_sample)
    crit = make_criterion(ps, per_sample)
    ga = GuardedAlloc()
    pa, td = gin(ga, p, d, grad=True), gin(ga, t, d)
    with guarded(monkeypatch, "ops", registry=ga):
        loss, stats = crit.loss_stats(pa, td)
        (loss * UPSTREAM).backward()
    rows = shape[0] if per_sample else 1
    verify(ga, [loss, stats], ws=mod("_lib").lib().csu_seg_loss_workspace(p.numel(), rows))
    finite(loss, stats, pa.grad)
    torch.testing.assert_close(loss.detach().double().cpu(), ref, rtol=LOSS_RTOL, atol=0)
    pd = p.double()
    check_grad(pa.grad, gref, pd * (1 - pd) >= 1e-12)
    pred = (p > 0.5).double()
    assert torch.equal(stats.double().cpu(), torch.stack([(pred * t).sum(), pred.sum(), t.double().sum()]))


def _place_guarded(ga, z, layout, d):
    """test_gpu_seg_ce.py::place with the logits' buffer between NaN guards (and NaN in the padding)."""
    B, K, H, W = z.shape
    if layout == "nchw":
        return gin(ga, z, d, grad=True)
    pitch = (K + 7) // 8 * 8 if layout == "class_last_padded" else K
    buf = torch.full((B, H * W, pitch), float("nan"), dtype=z.dtype)
    buf[..., :K] = z.reshape(B, K, H * W).transpose(1, 2)
    bd = gin(ga, buf, d)
    v = bd[..., :K].transpose(1, 2).reshape(B, K, H, W)
    assert v.data_ptr() == bd.data_ptr() and v.stride()[1:] == (1, W * pitch, pitch)
    return v.detach().requires_grad_(True)


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["nchw", "class_last_padded", "class_last_dense"])
@pytest.mark.parametrize("shape", [(1, 2, 3, 5), (2, 3, 7, 9), (3, 5, 37, 41)])
def test_seg_ce(shape, layout, dtype, per_sample, monkeypatch):
    """seg_ce (softmax CE + per-class Tversky) with class weights, ignore_index and background excluded
    (PARAM_SETS[2]) at test_gpu_seg_ce.py's three smallest ragged shapes, every logit layout, int64 and
    uint8 labels whose guards hold a label that is neither a class nor ignore_index."""
    from test_seg_ce import IGNORE, PARAM_SETS, UPSTREAM, check_grad, check_loss, make_case, make_criterion, ref_ce_loss_grad
    d = dev()
    ps = PARAM_SETS[2]
    z, t = make_case(shape, dtype=dtype)
    lref, gref, sref = ref_ce_loss_grad(z, t, ps, per_sample)
    crit = make_criterion(shape[1], ps, per_sample)
    B, K = shape[0], shape[1]
    for lab in (torch.int64, torch.uint8):
        ga = GuardedAlloc()
        za = _place_guarded(ga, z, layout, d)
        td = gin(ga, t.to(lab), d, fill=IGNORE - 1)
        with guarded(monkeypatch, "ops", registry=ga):
            loss, stats = crit.loss_stats(za, td)
            (loss * UPSTREAM).backward()
        verify(ga, [loss, stats], ws=mod("_lib").lib().csu_seg_ce_workspace(B, K, shape[2] * shape[3]))
        finite(loss, stats, za.grad)
        assert za.grad.dtype == dtype
        check_loss(loss, lref)
        check_grad(za.grad, gref, bf16=dtype == BF16)
        assert stats.dtype == torch.float64 and torch.equal(stats.cpu(), sref)


# ---------------------------------------------------------------------------------------------
# small utility ops
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,adt,bdt", [(64 * 64, BF16, BF16), (1000 * 8, F32, BF16), (4096, BF16, None), (8 * 13, F32, F32)])
def test_grad_join(n, adt, bdt, monkeypatch):
    ops = mod("ops")
    d = dev()
    g = torch.Generator().manual_seed(n)
    a = torch.randn(n // 8, 8, generator=g).to(adt)
    b = torch.randn(n // 8, 8, generator=g).to(bdt) if bdt is not None else None
    ga = GuardedAlloc()
    ad, bd = gin(ga, a, d), (None if b is None else gin(ga, b, d))
    with guarded(monkeypatch, "ops", registry=ga):
        out = ops.grad_join(ad, bd, F32)
        outb = ops.grad_join(ad, bd, BF16) if b is not None else None
    verify(ga, [out, out._csu_bf16] + ([outb] if outb is not None else []))
    ref = a.float() + (b.float() if b is not None else 0)
    finite(out, out._csu_bf16)
    assert out.dtype == F32 and torch.equal(out.cpu(), ref) and torch.equal(out._csu_bf16.cpu(), ref.bfloat16())
    if outb is not None:
        finite(outb)
        assert torch.equal(outb.cpu(), ref.bfloat16())


def test_shared_cast_and_concat_linear(monkeypatch):
    """shared_cast (one bf16 copy, its two gradients summed by one pass) and concat_linear (two GEMMs on
    the weight halves) at (1, 100, 64, 64): test_concat_linear_and_shared_cast_vs_fp64's criterion."""
    ops = mod("ops")
    d = dev()
    B, L, C, N = 1, 100, 64, 64
    g = torch.Generator().manual_seed(B * L + C)
    skip, up = torch.randn(B, L, C, generator=g), torch.randn(B, L, C, generator=g).bfloat16()
    w, b = torch.randn(N, 2 * C, generator=g) * 0.05, torch.randn(N, generator=g)
    gy, gm = torch.randn(B, L, N, generator=g), torch.randn(B, L, C, generator=g)
    s2, u2, w2, b2 = (t.double().requires_grad_(True) for t in (skip, up, w, b))
    sb = s2.bfloat16().double()
    y2 = F.linear(torch.cat([sb, u2], -1), w2.bfloat16().double(), b2)
    (y2 * gy.double()).sum().backward()
    gskip_ref = s2.grad + gm.double()
    ga = GuardedAlloc()
    skipd, upd, wd, bd = (gin(ga, t, d, grad=True) for t in (skip, up, w, b))
    gyd, gmd = gin(ga, gy, d), gin(ga, gm.bfloat16(), d)
    with guarded(monkeypatch, "ops", registry=ga):
        with torch.autocast("cuda", dtype=BF16):
            sm, sk = ops.shared_cast(skipd, BF16)
            y = ops.concat_linear(sk, upd, wd, bd)
        torch.autograd.backward([y, sm], [gyd, gmd])
    verify(ga, [y, sm])
    assert y.dtype == F32 and sm.dtype == BF16 and sm.data_ptr() == sk.data_ptr()
    finite(sm)
    assert torch.equal(sm.cpu(), skip.bfloat16())
    gskip_ref = s2.grad + gm.bfloat16().double()
    for got, ref, name in ((y, y2, "y"), (skipd.grad, gskip_ref, "dskip"), (upd.grad, u2.grad, "dup"), (wd.grad, w2.grad, "dw"),
                           (bd.grad, b2.grad, "db")):
        finite(got)
        ref = ref.detach()
        err = float((got.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-30))
        assert err <= 2e-2, (name, err)


def test_pack_nhwc_image():
    """csu_pack_nhwc_bf16: fp32 NCHW image -> bf16 NHWC, channels zero-padded to 8 (bit-exact), odd sizes."""
    L_ = mod("_lib")
    d = dev()
    x = torch.randn(3, 3, 37, 41, generator=torch.Generator().manual_seed(1))
    ga = GuardedAlloc()
    xd = gin(ga, x, d)
    y = ga.empty(3, 37, 41, 8, dtype=BF16, device=d)
    L_.check(L_.lib().csu_pack_nhwc_bf16(3, 3, 37, 41, 8, L_.ptr(xd), L_.ptr(y), L_.stream_ptr(d)), "pack")
    torch.cuda.synchronize()
    verify(ga)
    finite(y)
    assert torch.equal(y[..., :3].cpu(), x.permute(0, 2, 3, 1).bfloat16()) and not y[..., 3:].any()


def test_augment_batch(monkeypatch):
    """csu_augment_batch on odd 23-pixel images (flips, quarter turns, crops + resize) vs the oracle:
    test_device_augment_vs_oracle's criterion."""
    import numpy as np
    from oracle import augment_ref as A
    ops = mod("ops")
    d = dev()
    rng = np.random.RandomState(3)
    S = 23
    prm = [(0, 0, 0, 0, 0, S, S), (1, 0, 1, 0, 0, S, S), (0, 1, 2, 3, 2, S - 7, S - 5), (1, 1, 3, 2, 3, S - 5, S - 7),
           (0, 0, 3, 0, 0, S, S)]
    B = len(prm)
    img = rng.randint(0, 256, (B, S, S, 3)).astype(np.uint8)
    msk = ((rng.rand(B, S, S) > 0.5) * 255).astype(np.uint8)
    ga = GuardedAlloc()
    imgd, mskd = gin(ga, torch.from_numpy(img), d, fill=93), gin(ga, torch.from_numpy(msk), d, fill=93)
    with guarded(monkeypatch, "ops", registry=ga):
        oi, om = ops.augment_batch(imgd, mskd, prm)
    verify(ga, [oi, om])
    finite(oi, om)
    oi, om = oi.cpu().numpy(), om.cpu().numpy()
    for b in range(B):
        ri, rm = A.augment(img[b], msk[b], prm[b])
        di, dm = np.abs(oi[b] - ri).max(), np.abs(om[b] - rm).max()
        assert di <= 1 / 255 + 1e-6 and dm <= 1 / 255 + 1e-6, (b, prm[b], di, dm)
        if prm[b][5] == S and prm[b][6] == S:             # no crop: a pure permutation, bit-exact
            np.testing.assert_array_equal(oi[b], ri)
            np.testing.assert_array_equal(om[b], rm)


# ---------------------------------------------------------------------------------------------
# optimiser side
# ---------------------------------------------------------------------------------------------
OPT_NUMELS = [1, 1000, 4 * 1024 + 3]


class _Holder(torch.nn.Module):
    def __init__(self, ps):
        super().__init__()
        self.ps = torch.nn.ParameterList(ps)


def _opt_params(ga, d, seed=0):
    """Guarded parameters (in place by contract) of the three element counts, and their plain twins."""
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(n, generator=g) for n in OPT_NUMELS]
    mine = [torch.nn.Parameter(ga.guard_input(v, device=d, inplace=True, name=f"param{v.numel()}")) for v in vals]
    ref = [v.to(d).clone().requires_grad_(True) for v in vals]
    return mine, ref


def _opt_grads(ga, d, mine, ref, g):
    """Fresh gradients in guarded buffers (not in place: the step must not write them); the last one starts
    4 bytes into its buffer, off a 16-byte boundary."""
    for p, q in zip(mine, ref):
        n = p.numel()
        v = torch.randn(n, generator=g)
        if n == OPT_NUMELS[-1]:
            buf = ga.guard_input(torch.cat([torch.full((1,), float("nan")), v]), device=d, name="grad, 4-byte offset")
            p.grad = buf[1:]
            assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
        else:
            p.grad = ga.guard_input(v, device=d, name=f"grad{n}")
        q.grad = v.to(d).clone()


@pytest.mark.parametrize("mode", ["plain", "clip", "ema"])
def test_fused_adamw_step(mode, monkeypatch):
    """FusedAdamW.step (plain, with global-norm clipping, with the fused EMA) over guarded parameters,
    gradients, moments and averages: vs torch.optim.AdamW (+ clip_grad_norm_) at
    test_fused_adamw_matches_torch's tolerances, the EMA vs the fp64 recurrence over the recorded
    parameter sequence at test_ema_against_fp64_recurrence's bound."""
    import numpy as np
    optim, ema_mod = mod("optim"), mod("ema")
    d = dev()
    ga = GuardedAlloc()
    mine, ref = _opt_params(ga, d)
    cval = 0.5 * float(sum(OPT_NUMELS)) ** 0.5
    o_ref = torch.optim.AdamW(ref, lr=1e-3, weight_decay=1e-2, foreach=False)
    g = torch.Generator().manual_seed(1)
    with guarded(monkeypatch, "optim", "ema", registry=ga):
        ema = None
        if mode == "ema":
            ema = ema_mod.WeightEMA(_Holder(mine), decay=0.9, warmup=False)
            ema.tensors = [ga.guard_input(e, inplace=True, name="ema") for e in ema.tensors]
            ema._of = {id(p): e for p, e in zip(ema.params, ema.tensors)}
            e64 = [p.detach().double().cpu().clone() for p in mine]
            big = [p.detach().abs().double().cpu() for p in mine]
        o_mine = optim.FusedAdamW(mine, lr=1e-3, weight_decay=1e-2, max_grad_norm=cval if mode == "clip" else None, ema=ema)
        for it in range(3):
            _opt_grads(ga, d, mine, ref, g)
            if mode == "clip":
                tn = torch.nn.utils.clip_grad_norm_(ref, cval)
                assert float(tn) > cval
            o_ref.step()
            o_mine.step()
            if mode == "clip":
                want = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in mine))
                torch.testing.assert_close(o_mine.grad_norm.double(), want, rtol=1e-6, atol=0)
            if mode == "ema":
                dd = float(np.float32(0.9))
                for r, b, p in zip(e64, big, mine):
                    pc = p.detach().double().cpu()
                    r.mul_(dd).add_(pc, alpha=1 - dd)
                    torch.maximum(b, torch.maximum(pc.abs(), r.abs()), out=b)
    verify(ga, [o_mine.state[p][k] for p in mine for k in ("exp_avg", "exp_avg_sq")])
    for p, q in zip(ref, mine):
        finite(q, o_mine.state[q]["exp_avg"], o_mine.state[q]["exp_avg_sq"])
        torch.testing.assert_close(q.detach(), p.detach(), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(o_mine.state[q]["exp_avg"], o_ref.state[p]["exp_avg"], rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(o_mine.state[q]["exp_avg_sq"], o_ref.state[p]["exp_avg_sq"], rtol=5e-5, atol=1e-9)
    assert float(o_mine.state[mine[0]]["step"]) == 3.0
    if mode == "ema":
        assert float(ema.num_updates) == 3.0
        for e, r, b in zip(ema.tensors, e64, big):
            finite(e)
            assert bool(((e.double().cpu() - r).abs() <= 4e-6 * b).all())


def test_grad_norm_and_clip_in_place(monkeypatch):
    """csu_grad_sumsq / _finish / _scale through csu.optim.grad_norm and clip_grad_norm_: the norm vs fp64,
    the gradients (scaled in place by contract) vs torch's clip at test_standalone_clip_grad_norm_matches_torch's
    rtol 1e-6; the element in front of the 4-byte-offset gradient keeps its bits."""
    optim = mod("optim")
    d = dev()
    ga = GuardedAlloc()
    g = torch.Generator().manual_seed(21)
    vals = [torch.randn(n, generator=g) for n in OPT_NUMELS]
    a, b = [], []
    for v in vals:
        p = torch.zeros(v.numel(), device=d).requires_grad_(True)
        if v.numel() == OPT_NUMELS[-1]:
            buf = ga.guard_input(torch.cat([torch.full((1,), 123.0), v]), device=d, inplace=True, name="grad, 4-byte offset")
            p.grad = buf[1:]
            assert p.grad.data_ptr() % 16 == 4
        else:
            p.grad = ga.guard_input(v, device=d, inplace=True)
        q = torch.zeros(v.numel(), device=d).requires_grad_(True)
        q.grad = v.to(d).clone()
        a.append(p), b.append(q)
    norm = float(torch.sqrt(sum((v.double() ** 2).sum() for v in vals)))
    with guarded(monkeypatch, "optim", registry=ga):
        n0 = optim.grad_norm(a)
        n1 = optim.clip_grad_norm_(a, 0.5 * norm)
    n2 = torch.nn.utils.clip_grad_norm_(b, 0.5 * norm)
    L = mod("_lib").lib()
    chunks = sum(max(1, -(-n // L.csu_adamw_chunk_elems())) for n in OPT_NUMELS)
    verify(ga, [n0, n1], ws=L.csu_grad_norm_workspace(chunks))      # the fp64 partial sums, one per chunk
    finite(n0, n1)
    assert abs(float(n0) - norm) < 1e-6 * norm and abs(float(n1) - norm) < 1e-6 * norm
    torch.testing.assert_close(n1, n2, rtol=1e-6, atol=0)
    for p, q, v in zip(a, b, vals):
        finite(p.grad)
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-6, atol=0)
        assert not torch.equal(p.grad.cpu(), v)
    assert float(buf[0]) == 123.0


def test_ema_update_and_swap(monkeypatch):
    """WeightEMA.update (csu_ema_update) vs the fp64 recurrence at test_ema_against_fp64_recurrence's bound,
    and swap (csu_ema_swap): parameters and averages exchange bit for bit, and back."""
    import numpy as np
    ema_mod = mod("ema")
    d = dev()
    ga = GuardedAlloc()
    mine, _ = _opt_params(ga, d, seed=3)
    g = torch.Generator().manual_seed(4)
    with guarded(monkeypatch, "ema", "optim", registry=ga):
        ema = ema_mod.WeightEMA(_Holder(mine), decay=0.9, warmup=False)
        ema.tensors = [ga.guard_input(e, inplace=True, name="ema") for e in ema.tensors]
        ema._of = {id(p): e for p, e in zip(ema.params, ema.tensors)}
        e64 = [p.detach().double().cpu().clone() for p in mine]
        big = [p.detach().abs().double().cpu() for p in mine]
        dd = float(np.float32(0.9))
        for it in range(3):
            with torch.no_grad():
                for p in mine:
                    p.add_(torch.randn(p.shape, generator=g).to(d))
            ema.update()
            for r, b, p in zip(e64, big, mine):
                pc = p.detach().double().cpu()
                r.mul_(dd).add_(pc, alpha=1 - dd)
                torch.maximum(b, torch.maximum(pc.abs(), r.abs()), out=b)
        torch.cuda.synchronize()
        p0, e0 = [p.detach().clone() for p in mine], [e.clone() for e in ema.tensors]
        ema.swap()
        torch.cuda.synchronize()
        swapped = [(p.detach().clone(), e.clone()) for p, e in zip(mine, ema.tensors)]
        ema.swap()
    verify(ga)
    assert float(ema.num_updates) == 3.0
    for e, r, b in zip(e0, e64, big):
        finite(e)
        assert bool(((e.double().cpu() - r).abs() <= 4e-6 * b).all())
    for (ps, es), p, e, pp, ee in zip(swapped, p0, e0, mine, ema.tensors):
        assert torch.equal(ps, e) and torch.equal(es, p)
        assert torch.equal(pp.detach(), p) and torch.equal(ee, e)


# ---------------------------------------------------------------------------------------------
# cast cache
# ---------------------------------------------------------------------------------------------
def test_cast_cache_batch_kernels(monkeypatch):
    """CastCache.refresh (csu_cast_bf16_batch: bf16 shadows, (K, N) transposes with ragged 64 x 64 edge
    tiles, channels-last conv layouts) into guarded shadows: bit-equal to torch's casts
    (test_cast_cache_batch_kernel)."""
    ops = mod("ops")
    d = dev()
    g = torch.Generator().manual_seed(3)
    ps_c = [torch.randn(192, 64, generator=g), torch.randn(70, generator=g), torch.randn(16, 64, 1, 1, generator=g),
            torch.randn(130, 333, generator=g), torch.randn(5, generator=g)]
    convs_c = [torch.randn(36, 16, 3, 3, generator=g), torch.randn(64, 3, 7, 7, generator=g)]
    ga = GuardedAlloc()
    ps, convs = [gin(ga, t, d) for t in ps_c], [gin(ga, t, d) for t in convs_c]
    with guarded(monkeypatch, "ops", registry=ga):
        c = ops.CastCache()
        c.refresh(ps, BF16, convs)
        got = [(c.get(p, BF16), c.get_t(p.reshape(p.shape[0], -1), BF16) if p.dim() > 1 else None) for p in ps]
        gconv = [c.get_conv(w, BF16) for w in convs]
    verify(ga)
    assert c.items is not None
    for p, (sh, sht) in zip(ps_c, got):
        finite(sh)
        assert ga.contains(sh) and torch.equal(sh.cpu(), p.bfloat16())
        if sht is not None:
            finite(sht)
            assert ga.contains(sht) and torch.equal(sht.cpu(), p.reshape(p.shape[0], -1).t().bfloat16())
    for w, (o, i) in zip(convs_c, gconv):
        C = w.shape[1]
        finite(o)
        if C % 8:
            assert o.shape[-1] == 8 and i is None and not o[..., C:].any()
            assert torch.equal(o[..., :C].cpu(), w.permute(0, 2, 3, 1).bfloat16())
        else:
            finite(i)
            assert torch.equal(o.cpu(), w.permute(0, 2, 3, 1).bfloat16())
            assert torch.equal(i.cpu(), w.permute(1, 2, 3, 0).bfloat16())


@pytest.mark.parametrize("rows,cols", [(32, 16), (768, 256), (128, 384), (256, 768)])
def test_frag_layout_batch(rows, cols):
    """csu_frag_layout_batch (bf16 fragment order) and csu_frag8_layout_batch (e4m3, both orientations) at
    test_frag_layout_batch's sizes into guarded outputs of exactly rows * cols elements."""
    import numpy as np
    L_ = mod("_lib")
    d = dev()
    g = torch.Generator().manual_seed(rows + cols)
    ws_c = [torch.randn(rows, cols, generator=g).bfloat16(), torch.randn(64, 128, generator=g).bfloat16()]
    ga = GuardedAlloc()
    ws = [gin(ga, w, d) for w in ws_c]
    outs = [ga.empty(w.numel(), dtype=BF16, device=d) for w in ws]
    rec = np.zeros(len(ws), dtype=[("src", "<u8"), ("dst", "<u8"), ("rows", "<i4"), ("cols", "<i4"), ("chunk0", "<i8")])
    c0 = 0
    for k, (w, o) in enumerate(zip(ws, outs)):
        rec[k] = (w.data_ptr(), o.data_ptr(), w.shape[0], w.shape[1], c0)
        c0 += w.numel() // 8
    items = torch.frombuffer(bytearray(rec.tobytes()), dtype=torch.uint8).to(d)
    assert L_.lib().csu_frag_layout_batch(ctypes.c_void_p(items.data_ptr()), len(ws), c0, None) == 0
    torch.cuda.synchronize()
    for w, o in zip(ws_c, outs):
        finite(o)
        assert torch.equal(o.cpu(), _frag_ref(w))
    if rows % 64 == 0 and cols % 64 == 0:
        q = torch.randint(0, 256, (rows, cols), dtype=torch.uint8, generator=g)
        q[(q & 0x7F) == 0x7F] = 0                        # no e4m3 NaN encodings: plain bytes to permute
        qd = gin(ga, q, d, fill=0)
        dt = np.dtype([("src", "<u8"), ("dst", "<u8"), ("N", "<i4"), ("K", "<i4"), ("transpose", "<i4"), ("pad", "<i4"),
                       ("block0", "<i8")])
        for tr in (False, True):
            out8 = ga.empty(rows * cols, dtype=torch.uint8, device=d)
            it = torch.frombuffer(bytearray(np.array([(qd.data_ptr(), out8.data_ptr(), rows, cols, int(tr), 0, 0)], dtype=dt)
                                            .tobytes()), dtype=torch.uint8).to(d)
            L_.check(L_.lib().csu_frag8_layout_batch(L_.ptr(it), 1, rows * cols // 64, L_.stream_ptr(d)), "frag8")
            torch.cuda.synchronize()
            assert torch.equal(out8.cpu(), _frag_ref(q.t().contiguous() if tr else q))
    verify(ga)


def test_e4m3_quantisers(monkeypatch):
    """Fp8Weights.quantize (per-row power-of-two e4m3: bytes, scales, dequantised values) into guarded
    buffers, ragged row counts: bit-equal to the torch restatement (test_quantizer_matches_torch_e4m3fn)."""
    from test_gpu_fp8 import _ref_quant
    ops = mod("ops")
    d = dev()
    g = torch.Generator().manual_seed(0)
    ws = [torch.randn(192, 64, generator=g) * 0.02, torch.randn(64, 256, generator=g) * 3.0,
          torch.randn(7, 1, 3, 3, generator=g), torch.zeros(8, 16), torch.randn(37, 48, generator=g)]
    ws[1][3, 5] = 447.9
    ga = GuardedAlloc()
    ps = [gin(ga, w, d) for w in ws]
    with guarded(monkeypatch, "ops", registry=ga):
        fp8 = ops.Fp8Weights(ps)
        deq = fp8.quantize()
    verify(ga)
    for w, dq, q, sc in zip(ws, deq, fp8.q, fp8.scales):
        rd, rq, rs = _ref_quant(w)
        finite(dq, sc)
        assert ga.contains(q) and ga.contains(sc) and ga.contains(dq)
        assert torch.equal(sc.cpu(), rs) and torch.equal(q.cpu(), rq) and torch.equal(dq.cpu(), rd)


# ---------------------------------------------------------------------------------------------
# tiled inference and surface metrics
# ---------------------------------------------------------------------------------------------
TTA = [(1, 0, 0), (0, 0, 1)]          # one flipped and one quarter-turn variant


@pytest.mark.parametrize("kind", [0, 1], ids=["u8_hwc", "f32_chw"])
def test_tile_gather(kind, monkeypatch):
    """csu_tile_gather for a 37 x 53 image, 16-pixel tiles with overlap (edge tiles pulled back, clamped
    reads), a flipped and a quarter-turn variant, an inactive slot: bitwise the torch restatement
    (test_gather_is_bitwise_the_torch_restatement)."""
    import numpy as np
    from test_gpu_infer import torch_gather
    infer = mod("infer")
    d = dev()
    H, W, S = 37, 53, 16
    g = torch.Generator().manual_seed(H + W + kind)
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g) if kind == 0 else torch.rand(3, H, W, generator=g)
    table = infer.plan_tiles(H, W, S, 0.5, TTA)
    table = np.concatenate([table, np.zeros((2, 6), dtype=np.int32)])
    table[-2] = (5, 7, 1, 1, 3, 0)
    want = torch_gather(img, kind, torch.from_numpy(table), S)
    ga = GuardedAlloc()
    imgd = gin(ga, img, d, **({"fill": 93} if kind == 0 else {}))
    tabd = gin(ga, torch.from_numpy(table), d, fill=-7)
    with guarded(monkeypatch, "infer", registry=ga):
        got = infer.tile_gather(imgd, tabd, S)
    verify(ga, [got])
    finite(got)
    assert got.dtype == F32 and tuple(got.shape) == (len(table), 3, S, S)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("K,dtype,layout", [(3, F32, "nchw"), (5, BF16, "class_last_padded"), (1, F32, "prob")])
def test_tile_blend_and_finish(K, dtype, layout, monkeypatch):
    """csu_tile_blend / csu_tile_finish for a 37 x 53 canvas, 16-pixel tiles with overlap, a flipped and a
    quarter-turn variant, ragged batches with inactive slots, vs reference_predict's fp64 arithmetic on
    the same synthetic model outputs: test_gpu_infer.py's bounds (check_against_reference)."""
    import numpy as np
    from test_gpu_infer import check_against_reference
    infer = mod("infer")
    d = dev()
    H, W, S, overlap, batch = 37, 53, 16, 0.5, 7
    table = infer.plan_tiles(H, W, S, overlap, TTA)
    N = len(table)
    g = torch.Generator().manual_seed(1000 + K)
    z = 2.0 * torch.randn(N, K, S, S, generator=g)
    if layout == "prob":
        z = torch.sigmoid(z)
    z = z.to(dtype)
    chunks = iter(torch.split(z.double(), batch))
    ref_labels, ref_prob = infer.reference_predict(lambda x: next(chunks), torch.zeros(3, H, W), S, overlap, "gaussian", TTA,
                                                   batch, "prob" if layout == "prob" else "logits", True)
    w1 = infer.window_1d(S, "gaussian")
    ga = GuardedAlloc()
    w1d = gin(ga, torch.from_numpy(w1.astype(np.float32)), d)
    ry = gin(ga, torch.from_numpy(infer.axis_weight(H, S, overlap, w1).astype(np.float32)), d)
    rx = gin(ga, torch.from_numpy(infer.axis_weight(W, S, overlap, w1).astype(np.float32)), d)
    nb = -(-N // batch)
    pad = np.zeros((nb * batch, 6), dtype=np.int32)
    pad[:N] = table
    tab = gin(ga, torch.from_numpy(pad), d, fill=-7)
    with guarded(monkeypatch, "infer", registry=ga):
        canvas = infer.torch.zeros(K, H, W, dtype=F32, device=d)
        for i in range(nb):
            zb = torch.full((batch, K, S, S), 7.0, dtype=z.dtype)          # padding slots: finite junk that must not count
            n = min(batch, N - i * batch)
            zb[:n] = z[i * batch:i * batch + n]
            if layout in ("nchw", "prob"):
                zd = gin(ga, zb, d)
            else:
                pitch = (K + 7) // 8 * 8
                buf = torch.full((batch, S * S, pitch), float("nan"), dtype=z.dtype)
                buf[..., :K] = zb.reshape(batch, K, S * S).transpose(1, 2)
                zd = gin(ga, buf, d)[..., :K].transpose(1, 2).reshape(batch, K, S, S)
            region = infer.tile_region(pad[i * batch:(i + 1) * batch], S, H, W) if i % 2 else None
            infer.tile_blend(zd, tab[i * batch:(i + 1) * batch], w1d, canvas, "prob" if layout == "prob" else "logits", region)
        labels, prob = infer.tile_finish(canvas, ry, rx, len(TTA), return_prob=True)
    verify(ga, [canvas, labels, prob])
    finite(canvas, prob)
    check_against_reference(labels, prob, ref_labels, ref_prob, f"K{K} {layout}")


@pytest.mark.parametrize("spacing", [(1.0, 1.0), (0.7, 1.3)], ids=["unit", "0.7x1.3"])
def test_surface_metrics_and_edt(spacing, monkeypatch):
    """surface_metrics (two foreground classes, 19 x 23 maps, uint8 prediction against an int64 target)
    and distance_transform_edt (uint16 column distances in a workspace of exactly csu_edt_workspace
    bytes) vs the fp64 brute force: test_gpu_surface_metrics.py's tolerances."""
    import numpy as np
    from test_gpu_surface_metrics import EXACT_RTOL, F32_RTOL, blobs
    metrics, L = mod("metrics"), mod("_lib").lib()
    d = dev()
    rng = np.random.default_rng(19 * 23)
    B, H, W, Kc = 2, 19, 23, 3
    p = torch.from_numpy(rng.integers(1, Kc, (B, H, W)).astype(np.uint8)) * blobs(rng, (B, H, W), 0.1)
    t = torch.from_numpy(rng.integers(1, Kc, (B, H, W))) * blobs(rng, (B, H, W), 0.1).long()
    tau = 1.5 if spacing == (1.0, 1.0) else 2.0
    want = metrics.reference_surface_metrics(p, t, Kc, spacing, tau, 95.0)
    assert want.shape == (B, 2, 6) and not torch.isnan(want).any()      # both classes present in every image
    m = blobs(rng, (B, H, W), 0.15)
    eref = metrics.reference_distance_transform_edt(m, spacing)
    ga = GuardedAlloc()
    pd, td, md = gin(ga, p, d, fill=200), gin(ga, t, d, fill=200), gin(ga, m, d, fill=0)
    with guarded(monkeypatch, "metrics", registry=ga):
        got = metrics.surface_metrics(pd, td, Kc, spacing, tau, 95.0)
        e = metrics.distance_transform_edt(md, spacing)
    verify(ga, [got, e], ws=L.csu_surface_workspace(B, 2, H, W))
    assert ga.saw_workspace(L.csu_edt_workspace(B, H, W))
    finite(got, e)
    got = got.cpu()
    assert got.dtype == torch.float64 and torch.equal(got[:, :, 4:], want[:, :, 4:])
    exact = spacing == (1.0, 1.0)
    rtol = EXACT_RTOL if exact else F32_RTOL
    for j in (0, 1, 2):
        torch.testing.assert_close(got[:, :, j], want[:, :, j], rtol=rtol, atol=0)
    if exact:
        torch.testing.assert_close(got[:, :, 3], want[:, :, 3], rtol=EXACT_RTOL, atol=0)
        assert torch.equal(e.cpu(), eref.float())
    else:
        dist = []
        for b in range(B):
            for v in (1, 2):
                bp = metrics._border(p[b] == v).nonzero().double()
                bt = metrics._border(t[b] == v).nonzero().double()
                dist += [metrics._nearest(bp, bt, *spacing), metrics._nearest(bt, bp, *spacing)]
        assert not ((torch.cat(dist) - tau).abs() <= 1e-5 * tau).any(), "a border distance ties with the tolerance"
        assert torch.equal(got[:, :, 3], want[:, :, 3])
        e64 = e.cpu().double()
        assert torch.equal(e64 == 0, eref == 0)
        torch.testing.assert_close(e64, eref, rtol=F32_RTOL, atol=0)
