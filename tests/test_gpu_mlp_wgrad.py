"""csu_mlp_bwd_wgrad (C = 64): the fused Mlp backward that forms dW1 / db1 / dW2 / db2 inside the
kernel instead of writing dh and g for two later weight-gradient launches.

Kernel level (C ABI), per shape: dx is bitwise csu_mlp_bwd_dp's; the four gradients against fp64 --
computed on the CPU from the unchanged kernel's own bf16 dh / g contracted with x / dy -- stay within
test_linear_wgrad_kernel's bf16 bound |err|_max <= 1e-2 max(|ref|_max, sqrt(M)) and within twice the
error of the two-step path (csu_mlp_bwd_dp + ops.linear_wgrad; both are fp32 sums of the same bf16
products and differ only in association); two calls are bitwise equal.

Op level: ops.mlp_residual at C = 64 with ops.MLP64_FUSED_WGRAD on and off, with a gradient bucket
registered, and with a parameter that already has a .grad (fallback to the two-step path)."""
import ctypes
import functools
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 64
# (M, dropout p): one ragged panel in one workgroup; fewer panels than 2 x CUs; more panels than
# 2 x CUs (several unequal persistent iterations, ragged last panel); dropout + DropPath row scales
CASES = [(37, 0.0), (4096, 0.0), (40037, 0.0), (4096, 0.3)]
NAMES = ("dW1", "db1", "dW2", "db2")


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _inputs(M, d, seed):
    g = torch.Generator(device=d).manual_seed(seed)
    x = torch.randn(M, C, device=d, generator=g).bfloat16()
    dy = torch.randn(M, C, device=d, generator=g).bfloat16()
    w1 = (torch.randn(4 * C, C, device=d, generator=g) * C ** -0.5).bfloat16()
    w2 = (torch.randn(C, 4 * C, device=d, generator=g) * (4 * C) ** -0.5).bfloat16()
    b1 = torch.randn(4 * C, device=d, generator=g) * 0.1
    return x, dy, w1, w2, b1


def _fp64_ref(dh, g, x, dy):
    DH, G, X, DY = (t.double().cpu() for t in (dh, g, x, dy))
    return DH.t() @ X, DH.sum(0), DY.t() @ G, DY.sum(0)


def _fused(M, x, dy, w1, b1, w2, dd):
    """One csu_mlp_bwd_wgrad call + the slab sums on poisoned buffers: (dx, dW1, db1, dW2, db2)."""
    from csu import _lib
    from csu._lib import check, lib, ptr, stream_ptr
    L, d = lib(), x.device
    n1, n2 = ctypes.c_size_t(), ctypes.c_size_t()
    check(L.csu_mlp_bwd_wgrad_workspace(M, C, ctypes.byref(n1), ctypes.byref(n2)), "workspace")
    assert n1.value % ((4 * C * C + 4 * C) * 4) == 0 and n2.value % ((4 * C * C + C) * 4) == 0
    s1 = torch.full((n1.value // 4,), float("nan"), device=d)
    s2 = torch.full((n2.value // 4,), float("nan"), device=d)
    o1 = torch.full((4 * C * C + 4 * C,), float("nan"), device=d)
    o2 = torch.full((4 * C * C + C,), float("nan"), device=d)
    dx = torch.empty(M, C, device=d, dtype=torch.bfloat16)
    items = (_lib.WslabItem * 2)()
    check(L.csu_mlp_bwd_wgrad(M, C, ptr(x), ptr(dy), ptr(w1), ptr(b1), ptr(w2), ptr(dx), dd, ptr(s1), ptr(s2),
                              ctypes.byref(items[0]), ctypes.byref(items[1]), ptr(o1), ptr(o2), stream_ptr(d)), "mlp_bwd_wgrad")
    assert items[0].chunks == n1.value // ((4 * C * C + 4 * C) * 4)
    check(L.csu_wslab_reduce_batch(items, 2, stream_ptr(d)), "wslab_reduce_batch")
    torch.cuda.synchronize()
    return dx, o1[:4 * C * C].view(4 * C, C), o1[4 * C * C:], o2[:4 * C * C].view(C, 4 * C), o2[4 * C * C:]


@functools.lru_cache(maxsize=None)
def _case(M, p):
    """Everything the checks of one shape need, computed once: both paths' results and the fp64 reference."""
    from csu import _lib, ops
    from csu._lib import check, lib, ptr, stream_ptr
    d = dev()
    x, dy, w1, w2, b1 = _inputs(M, d, 1000 + M + int(p * 10))
    keep = []
    if p > 0:
        rps = 1024
        scale = torch.tensor([1 / 0.7, 0.0, 1 / 0.7, 1 / 0.7], device=d)   # DropPath: sample 1 dropped
        dy = (dy.float().view(-1, rps, C) * scale.view(-1, 1, 1)).view(M, C).bfloat16()
        rng = torch.tensor([20240607, 3], dtype=torch.int64, device=d)
        dsc = _lib.MlpDropout()
        dsc.rng, dsc.site_hidden, dsc.site_out, dsc.p = rng.data_ptr(), 11, 12, p
        dsc.row_scale, dsc.rows_per_sample = scale.data_ptr(), rps
        keep += [scale, rng, dsc]
        dd = ctypes.byref(dsc)
    else:
        dd = None
    dh = torch.empty(M, 4 * C, device=d, dtype=torch.bfloat16)
    g = torch.empty_like(dh)
    dx0 = torch.empty(M, C, device=d, dtype=torch.bfloat16)
    check(lib().csu_mlp_bwd_dp(M, C, ptr(x), ptr(dy), ptr(w1), ptr(b1), ptr(w2), ptr(dh), ptr(g), ptr(dx0), dd, stream_ptr(d)),
          "mlp_bwd_dp")
    dw1, db1 = ops.linear_wgrad(dh, x)
    dw2, db2 = ops.linear_wgrad(dy, g)
    a = _fused(M, x, dy, w1, b1, w2, dd)
    b = _fused(M, x, dy, w1, b1, w2, dd)
    torch.cuda.synchronize()
    ref = _fp64_ref(dh, g, x, dy)
    err_new = [float((t.double().cpu() - r).abs().max()) for t, r in zip(a[1:], ref)]
    err_old = [float((t.double().cpu() - r).abs().max()) for t, r in zip((dw1, db1, dw2, db2), ref)]
    for n, en, eo, r in zip(NAMES, err_new, err_old, ref):
        print(f"M={M} p={p} {n}: fused err {en:.3e}, two-step err {eo:.3e}, |ref|max {float(r.abs().max()):.3e}")
    if p > 0:
        assert float((g == 0).float().mean()) > 0.2        # the hidden mask is really on
    return {"dx0": dx0, "a": a, "b": b, "ref": ref, "err_new": err_new, "err_old": err_old}


@pytest.mark.parametrize("M,p", CASES)
def test_dx_bitwise_equals_two_step_kernel(M, p):
    r = _case(M, p)
    assert torch.equal(r["a"][0], r["dx0"])


@pytest.mark.parametrize("M,p", CASES)
def test_gradients_within_bf16_wgrad_bound(M, p):
    r = _case(M, p)
    for n, e, ref in zip(NAMES, r["err_new"], r["ref"]):
        assert e <= 1e-2 * max(float(ref.abs().max()), M ** 0.5), (n, e)


@pytest.mark.parametrize("M,p", CASES)
def test_error_at_most_twice_the_two_step_path(M, p):
    r = _case(M, p)
    for n, en, eo in zip(NAMES, r["err_new"], r["err_old"]):
        assert en <= 2 * eo, (n, en, eo)


@pytest.mark.parametrize("M,p", CASES)
def test_two_calls_bitwise_equal(M, p):
    r = _case(M, p)
    for n, u, v in zip(("dx",) + NAMES, r["a"], r["b"]):
        assert torch.equal(u, v), n


# ---- op level ---------------------------------------------------------------------------------------

class _Mlp:
    """fc1 / fc2 of a CSWinBlock Mlp at C = 64 on B = 2 images of 32 x 32 tokens."""

    def __init__(self, d):
        torch.manual_seed(7)
        self.fc1 = torch.nn.Linear(C, 4 * C).to(d)
        self.fc2 = torch.nn.Linear(4 * C, C).to(d)
        self.x = torch.randn(2, 1024, C, device=d).bfloat16()
        self.res = torch.randn(2, 1024, C, device=d)
        self.gy = torch.randn(2, 1024, C, device=d)
        self.params = (self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias)

    def run(self, ops, fused, pregrad=None):
        """(dx, param grads, True if the fused call was taken) of one forward + backward."""
        took = []
        real = ops._mlp_bwd_wgrad

        def spy(*a, **k):
            r = real(*a, **k)
            took.append(r is not None)
            return r

        old = ops.MLP64_FUSED_WGRAD, ops.SIDE_WGRAD
        ops.MLP64_FUSED_WGRAD, ops.SIDE_WGRAD, ops._mlp_bwd_wgrad = fused, False, spy   # as in the captured step
        try:
            for q in self.params:
                q.grad = None
            if pregrad is not None:
                self.fc1.weight.grad = pregrad.clone()
            x = self.x.clone().requires_grad_(True)
            y = ops.mlp_residual(self.res, x, self.fc1, self.fc2)
            y.backward(self.gy)
            torch.cuda.synchronize()
        finally:
            ops.MLP64_FUSED_WGRAD, ops.SIDE_WGRAD = old
            ops._mlp_bwd_wgrad = real
        return x.grad, [q.grad for q in self.params], took == [True]


def test_op_fused_vs_two_step():
    from csu import ops
    from csu._lib import check, lib, ptr, stream_ptr
    d = dev()
    m = _Mlp(d)
    dx_new, g_new, took = m.run(ops, True)
    assert took
    g_new = [t.clone() for t in g_new]
    dx_old, g_old, took_old = m.run(ops, False)
    assert not took_old
    assert torch.equal(dx_new, dx_old)
    # fp64 reference from the kernel's own operands, as at kernel level
    M = 2048
    x2, dyb = m.x.view(M, C), m.gy.bfloat16().view(M, C)
    w1, w2, b1 = m.fc1.weight.detach().bfloat16(), m.fc2.weight.detach().bfloat16(), m.fc1.bias.detach().float()
    dh = torch.empty(M, 4 * C, device=d, dtype=torch.bfloat16)
    g = torch.empty_like(dh)
    dx = torch.empty(M, C, device=d, dtype=torch.bfloat16)
    check(lib().csu_mlp_bwd_dp(M, C, ptr(x2), ptr(dyb), ptr(w1), ptr(b1), ptr(w2), ptr(dh), ptr(g), ptr(dx), None, stream_ptr(d)),
          "mlp_bwd_dp")
    torch.cuda.synchronize()
    for n, a, b, r in zip(NAMES, g_new, g_old, _fp64_ref(dh, g, x2, dyb)):
        en, eo = float((a.double().cpu() - r).abs().max()), float((b.double().cpu() - r).abs().max())
        print(f"op {n}: fused err {en:.3e}, two-step err {eo:.3e}")
        assert en <= 1e-2 * max(float(r.abs().max()), M ** 0.5), (n, en)
        assert en <= 2 * eo, (n, en, eo)


def test_op_gradients_land_in_bucket_slice():
    from csu import ops
    d = dev()
    m = _Mlp(d)
    _, g_plain, took = m.run(ops, True)
    assert took
    g_plain = [t.clone() for t in g_plain]
    flat = torch.full((sum(q.numel() for q in m.params) + 8,), float("nan"), device=d)
    off, offs = 4, []
    for q in m.params:
        ops._GRAD_DEST[id(q)] = (weakref.ref(q), flat, off)
        offs.append(off)
        off += q.numel()
    n0 = ops.STATS["late_grad_fixups"]
    try:
        _, g_b, took = m.run(ops, True)
    finally:
        for q in m.params:
            ops._GRAD_DEST.pop(id(q), None)
    assert took
    assert ops.STATS["late_grad_fixups"] == n0
    for q, gb, gp, o in zip(m.params, g_b, g_plain, offs):
        assert gb.data_ptr() == flat[o:].data_ptr()
        assert torch.equal(gb, gp)
        assert torch.equal(flat[o:o + q.numel()].view_as(q), gp)
    assert torch.isnan(flat[:4]).all() and torch.isnan(flat[-4:]).all()


def test_op_existing_grad_falls_back_and_accumulates():
    """A parameter with a .grad is not deferrable: the two-step path runs (bitwise the switch-off result
    on the same state) and autograd accumulates into the existing gradient."""
    from csu import ops
    d = dev()
    m = _Mlp(d)
    _, g_plain, _ = m.run(ops, False)
    g_plain = [t.clone() for t in g_plain]
    pre = torch.full_like(m.fc1.weight, 0.5)
    _, g_off, _ = m.run(ops, False, pregrad=pre)
    g_off = [t.clone() for t in g_off]
    _, g_acc, took = m.run(ops, True, pregrad=pre)
    assert not took
    for a, b in zip(g_acc, g_off):
        assert torch.equal(a, b)
    # accumulated: grad - 0.5 is the weight gradient (another split of the same fp32 sums than g_plain's)
    M = 2048
    tol = 1e-2 * max(float(g_plain[0].abs().max()), M ** 0.5)
    assert float(((g_acc[0] - pre) - g_plain[0]).abs().max()) <= tol
    assert float((g_acc[0] - g_plain[0]).mean()) > 0.49
