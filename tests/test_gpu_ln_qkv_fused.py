"""csu_gemm_ws_lnbwd: the qkv input-gradient GEMM with norm1's LayerNorm backward in its epilogue
(CSWinBlock cswin:357 -> 337), against the launch pair it replaces.

The fused kernel rounds dh = dY W to bf16 exactly as the plain csu_gemm_ws stores it and then runs the
arithmetic of csu_layernorm_bwd on whole token rows, so the two paths are fp32 sums of the same terms
in a different association.  The bound follows from that: against an fp64 LayerNorm backward of the
plain kernel's bf16 dh, the fused kernel's max error may be at most twice the stand-alone kernel's,
plus 1e-6 of the reference's magnitude."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _frag(w):
    """csu_frag_layout_batch of one bf16 (rows, cols) matrix."""
    from csu._lib import check, lib, ptr, stream_ptr
    rows, cols = w.shape
    w = w.contiguous()
    out = torch.empty(rows * cols, dtype=torch.bfloat16, device=w.device)
    rec = np.zeros(1, dtype=[("src", "<u8"), ("dst", "<u8"), ("rows", "<i4"), ("cols", "<i4"), ("chunk0", "<i8")])
    rec[0] = (w.data_ptr(), out.data_ptr(), rows, cols, 0)
    items = torch.frombuffer(bytearray(rec.tobytes()), dtype=torch.uint8).to(w.device)
    check(lib().csu_frag_layout_batch(ptr(items), 1, rows * cols // 8, stream_ptr(w.device)), "frag_layout")
    torch.cuda.synchronize()
    return out


def _param_reduce(work, rows, C, nblocks):
    from csu import _lib
    from csu._lib import check, lib, stream_ptr
    dgb = torch.empty(2 * C, dtype=torch.float32, device=work.device)
    it = (_lib.LnParamItem * 1)()
    it[0].workspace, it[0].dgamma, it[0].dbeta = work.data_ptr(), dgb.data_ptr(), dgb.data_ptr() + C * 4
    it[0].rows, it[0].C, it[0].nblocks = rows, C, nblocks
    check(lib().csu_layernorm_param_reduce_batch(it, 1, stream_ptr(work.device)), "param_reduce")
    return dgb[:C].clone(), dgb[C:].clone()


def _fused(M, C, dy, wtf, x, gamma, mean, rstd, dres):
    from csu._lib import check, lib, ptr, stream_ptr
    dx = torch.empty(M, C, dtype=torch.float32, device=x.device)
    dxb = torch.empty(M, C, dtype=torch.bfloat16, device=x.device)
    part = torch.empty(M // 64 * 2 * C, dtype=torch.float32, device=x.device)
    check(lib().csu_gemm_ws_lnbwd(M, C, 3 * C, ptr(dy), ptr(wtf), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres),
                                  ptr(dx), ptr(dxb), ptr(part), stream_ptr(x.device)), "gemm_ws_lnbwd")
    dg, db = _param_reduce(part, M, C, M // 64)
    torch.cuda.synchronize()
    return dx, dxb, dg, db


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("M", [64, 1024])
@pytest.mark.parametrize("C", [128, 256])
def test_gemm_ws_lnbwd_kernel(C, M, with_dres):
    """The kernel called directly; M = 64 is one workgroup, M = 1024 reaches the rotated tile order.

    Measured max |error| against the fp64 reference, fused / stand-alone (MI355X): see
    profiles/lq01_ln_qkv_ab.txt."""
    from csu._lib import CSU_BF16, CSU_F32, check, lib, ptr, stream_ptr
    d = dev()
    assert lib().csu_gemm_ws_lnbwd_supported(M, C, 3 * C)
    g = torch.Generator(device=d).manual_seed(1000 * C + M + int(with_dres))
    K = 3 * C
    x = (torch.randn(M, C, device=d, generator=g) + 3.0 * torch.randn(M, 1, device=d, generator=g)).contiguous()
    gamma = torch.rand(C, device=d, generator=g) + 0.5
    dy = torch.randn(M, K, device=d, generator=g).bfloat16()
    dres = torch.randn(M, C, device=d, generator=g) if with_dres else None
    w = (torch.randn(K, C, device=d, generator=g) / C ** 0.5).bfloat16()      # the Linear's (3C, C) weight
    wtf = _frag(w.t().contiguous())                                             # W^T (C, 3C), fragment-ordered
    xd = x.double()
    mean = xd.mean(1).float()
    rstd = (1.0 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5)).float()

    # dh_b: the plain kernel's bf16 output on the same operands
    dh_b = torch.empty(M, C, dtype=torch.bfloat16, device=d)
    check(lib().csu_gemm_ws(M, C, K, ptr(dy), K, ptr(wtf), None, None, CSU_BF16, ptr(dh_b), stream_ptr(d)), "gemm_ws")
    torch.cuda.synchronize()
    # the kernel itself against an fp64 GEMM (bf16 output rounding)
    dh_ref = dy.double() @ w.double()
    assert float((dh_b.double() - dh_ref).abs().max()) <= 2 ** -7 * float(dh_ref.abs().max())

    # fp64 LayerNorm backward of dh_b with the fp32 mean / rstd the kernels get
    dh = dh_b.double()
    xh = (xd - mean.double()[:, None]) * rstd.double()[:, None]
    gg = dh * gamma.double()
    ref_dx = rstd.double()[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    if with_dres:
        ref_dx = ref_dx + dres.double()
    ref = {"dx": ref_dx, "dgamma": (dh * xh).sum(0), "dbeta": dh.sum(0)}

    # the stand-alone pair: csu_layernorm_bwd(_ex) + csu_layernorm_param_reduce_batch on dh_b
    sdx = torch.empty(M, C, dtype=torch.float32, device=d)
    sdxb = torch.empty(M, C, dtype=torch.bfloat16, device=d)
    nbytes = lib().csu_layernorm_bwd_workspace(M, C)
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=d)
    check(lib().csu_layernorm_bwd_ex(M, C, CSU_F32, ptr(x), ptr(gamma), ptr(mean), ptr(rstd), CSU_BF16, ptr(dh_b),
                                     ptr(dres), ptr(sdx), ptr(sdxb), None, None, ptr(work), nbytes, stream_ptr(d)),
          "layernorm_bwd")
    sdg, sdb = _param_reduce(work, M, C, 0)
    torch.cuda.synchronize()
    alone = {"dx": sdx, "dgamma": sdg, "dbeta": sdb}

    dx, dxb, dg, db = _fused(M, C, dy, wtf, x, gamma, mean, rstd, dres)
    fused = {"dx": dx, "dgamma": dg, "dbeta": db}
    figs = {}
    for k in ("dx", "dgamma", "dbeta"):
        ef = float((fused[k].double() - ref[k]).abs().max())
        ea = float((alone[k].double() - ref[k]).abs().max())
        figs[k] = (ef, ea, float(ref[k].abs().max()))
        print(f"lnbwd C={C} M={M} dres={int(with_dres)} {k}: fused {ef:.3e} stand-alone {ea:.3e} max|ref| {figs[k][2]:.3e}")
    for k, (ef, ea, mx) in figs.items():
        assert ef <= 2 * ea + 1e-6 * mx, (k, ef, ea, mx)
    assert torch.equal(dxb, dx.bfloat16())
    # fixed summation order, no atomics: a second launch gives the same bits
    dx2, dxb2, dg2, db2 = _fused(M, C, dy, wtf, x, gamma, mean, rstd, dres)
    assert torch.equal(dx, dx2) and torch.equal(dxb, dxb2) and torch.equal(dg, dg2) and torch.equal(db, db2)


def test_ln_linear_ws_block(monkeypatch):
    """ops.ln_linear_ws inside an active weight cache (B = 2, L = 1024, C = 256): the fused path and the
    switch-off path (layer_norm_fork + linear, what CSWinBlock runs then) give the same y bit for bit, and
    every gradient within the kernel test's bound against an fp64 reference of the block."""
    from csu import ops
    d = dev()
    g = torch.Generator(device=d).manual_seed(7)
    B, L, C = 2, 1024, 256
    x0 = torch.randn(B, L, C, device=d, generator=g) + 2.0 * torch.randn(B, L, 1, device=d, generator=g)
    ln = torch.nn.LayerNorm(C).to(d)
    lin = torch.nn.Linear(C, 3 * C).to(d)
    with torch.no_grad():
        ln.weight.copy_(torch.rand(C, device=d, generator=g) + 0.5)
        ln.bias.copy_(torch.rand(C, device=d, generator=g) * 0.4 - 0.2)
        lin.bias.copy_(torch.rand(3 * C, device=d, generator=g) * 0.2 - 0.1)
    G = torch.randn(B, L, 3 * C, device=d, generator=g)
    R = torch.randn(B, L, C, device=d, generator=g)
    params = [ln.weight, ln.bias, lin.weight, lin.bias]
    cache = ops.CastCache()
    cache.refresh([lin.weight], torch.bfloat16)
    cache.refresh_frag()
    assert cache.get_frag(lin.weight) is not None and cache.get_frag_t(lin.weight) is not None
    outs = {}
    try:
        ops.set_cast_cache(cache)
        for fused in (False, True):
            monkeypatch.setattr(ops, "FUSE_LN_QKV", fused)
            for p in params:
                p.grad = None
            x = x0.clone().requires_grad_(True)
            calls = []
            real = ops._launch
            monkeypatch.setattr(ops, "_launch", lambda name, *a, **k: (calls.append(k.get("tag", name)), real(name, *a, **k))[1])
            with torch.autocast("cuda", dtype=torch.bfloat16):
                got = ops.ln_linear_ws(x, ln, lin)
                assert (got is not None) == fused
                if got is None:
                    xa, h = ops.layer_norm_fork(x, ln.weight, ln.bias, ln.eps, torch.bfloat16)
                    y = ops.linear(h, lin.weight, lin.bias)
                else:
                    xa, y = got
            ((y.float() * G).sum() + (xa * R).sum()).backward()
            torch.cuda.synchronize()
            monkeypatch.setattr(ops, "_launch", real)
            assert any("lnbwd" in str(c) for c in calls) == fused
            outs[fused] = (y.detach().clone(), [x.grad.clone()] + [p.grad.detach().clone() for p in params])
    finally:
        ops.set_cast_cache(None)
    assert torch.equal(outs[False][0], outs[True][0])
    # fp64 reference of the block
    xr = x0.double().requires_grad_(True)
    pr = [p.detach().double().requires_grad_(True) for p in params]
    hr = torch.nn.functional.layer_norm(xr, (C,), pr[0], pr[1], ln.eps)
    yr = hr @ pr[2].t() + pr[3]
    ((yr * G.double()).sum() + (xr * R.double()).sum()).backward()
    refs = [xr.grad] + [p.grad for p in pr]
    for name, a, b, r in zip(["dx", "dgamma", "dbeta", "dW", "db"], outs[True][1], outs[False][1], refs):
        ef, eu, mx = float((a.double() - r).abs().max()), float((b.double() - r).abs().max()), float(r.abs().max())
        print(f"ln_linear_ws block {name}: fused {ef:.3e} unfused {eu:.3e} max|ref| {mx:.3e}")
        assert ef <= 2 * eu + 1e-6 * mx, (name, ef, eu, mx)
