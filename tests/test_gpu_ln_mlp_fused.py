"""csu_mlp_bwd_ln: the fused Mlp backward with norm2's LayerNorm backward in its row phase (CSWinBlock
x + Mlp(LN(x)), cswin:368), against the launch pair it replaces.

The fused kernel rounds the Mlp's input gradient dX to bf16 exactly as the plain csu_mlp_bwd_dp stores it
and then runs the arithmetic of csu_layernorm_bwd on whole token rows, so the two paths are fp32 sums of
the same bf16-rounded terms in a different association.  The bound follows from that (as in
tests/test_gpu_ln_qkv_fused.py): against an fp64 LayerNorm backward of the plain kernel's bf16 dX, the
fused kernel's max error may be at most twice the stand-alone pair's (csu_layernorm_bwd_ex +
csu_layernorm_param_reduce_batch), plus 1e-6 of the reference's magnitude."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _param_reduce(work, rows, C, nblocks):
    from csu import _lib
    from csu._lib import check, lib, stream_ptr
    dgb = torch.empty(2 * C, dtype=torch.float32, device=work.device)
    it = (_lib.LnParamItem * 1)()
    it[0].workspace, it[0].dgamma, it[0].dbeta = work.data_ptr(), dgb.data_ptr(), dgb.data_ptr() + C * 4
    it[0].rows, it[0].C, it[0].nblocks = rows, C, nblocks
    check(lib().csu_layernorm_param_reduce_batch(it, 1, stream_ptr(work.device)), "param_reduce")
    return dgb[:C].clone(), dgb[C:].clone()


def _fused(M, C, rpi, h, dy, w1, b1, w2, x, gamma, mean, rstd, dres):
    from csu._lib import check, lib, ptr, stream_ptr
    d = x.device
    dh = torch.empty(M, 4 * C, dtype=torch.bfloat16, device=d)
    gl = torch.empty_like(dh)
    dx = torch.empty(M, C, dtype=torch.float32, device=d)
    dxb = torch.empty(M, C, dtype=torch.bfloat16, device=d)
    part = torch.empty(M // 64 * 2 * C, dtype=torch.float32, device=d)
    check(lib().csu_mlp_bwd_ln(M, C, ptr(h), ptr(dy), ptr(w1), ptr(b1), ptr(w2), ptr(dh), ptr(gl), rpi, ptr(x), ptr(gamma),
                               ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(dxb), ptr(part), stream_ptr(d)), "mlp_bwd_ln")
    dg, db = _param_reduce(part, M, C, M // 64)
    torch.cuda.synchronize()
    return dh, gl, dx, dxb, dg, db


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("M", [64, 192])
@pytest.mark.parametrize("C", [128, 256])
def test_mlp_bwd_ln_kernel(C, M, with_dres):
    """The kernel called directly; M = 64 is one workgroup, M = 192 three panels with rows-per-image = 192,
    so each panel starts at a different hidden chunk of the rotation.

    Measured max |error| against the fp64 reference, fused / stand-alone (MI355X): see
    profiles/ln02_ln_mlp_ab.txt."""
    from csu import _lib
    from csu._lib import CSU_BF16, CSU_F32, check, lib, ptr, stream_ptr
    d = dev()
    assert lib().csu_mlp_bwd_ln_supported(M, C)
    g = torch.Generator(device=d).manual_seed(1000 * C + M + int(with_dres))
    x = (torch.randn(M, C, device=d, generator=g) + 3.0 * torch.randn(M, 1, device=d, generator=g)).contiguous()
    gamma = torch.rand(C, device=d, generator=g) + 0.5
    beta = torch.rand(C, device=d, generator=g) * 0.4 - 0.2
    dy = torch.randn(M, C, device=d, generator=g).bfloat16()
    dres = torch.randn(M, C, device=d, generator=g) if with_dres else None
    w1 = (torch.randn(4 * C, C, device=d, generator=g) / C ** 0.5).bfloat16()
    b1 = torch.rand(4 * C, device=d, generator=g) * 0.2 - 0.1
    w2 = (torch.randn(C, 4 * C, device=d, generator=g) / (4 * C) ** 0.5).bfloat16()
    xd = x.double()
    mean = xd.mean(1).float()
    rstd = (1.0 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5)).float()
    h = (((xd - mean.double()[:, None]) * rstd.double()[:, None]) * gamma.double() + beta.double()).float().bfloat16()
    rpi = M

    # the plain kernel on the same operands: dX_b (bf16), dH, G
    dd = _lib.MlpDropout()
    dd.p, dd.rows_per_sample = 0.0, rpi
    dx_b = torch.empty(M, C, dtype=torch.bfloat16, device=d)
    dh0 = torch.empty(M, 4 * C, dtype=torch.bfloat16, device=d)
    g0 = torch.empty_like(dh0)
    check(lib().csu_mlp_bwd_dp(M, C, ptr(h), ptr(dy), ptr(w1), ptr(b1), ptr(w2), ptr(dh0), ptr(g0), ptr(dx_b),
                               ctypes.byref(dd), stream_ptr(d)), "mlp_bwd_dp")
    torch.cuda.synchronize()

    # fp64 LayerNorm backward of dX_b with the fp32 mean / rstd the kernels get
    dX = dx_b.double()
    xh = (xd - mean.double()[:, None]) * rstd.double()[:, None]
    gg = dX * gamma.double()
    ref_dx = rstd.double()[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    if with_dres:
        ref_dx = ref_dx + dres.double()
    ref = {"dx": ref_dx, "dgamma": (dX * xh).sum(0), "dbeta": dX.sum(0)}

    # the stand-alone pair: csu_layernorm_bwd_ex + csu_layernorm_param_reduce_batch on dX_b
    sdx = torch.empty(M, C, dtype=torch.float32, device=d)
    sdxb = torch.empty(M, C, dtype=torch.bfloat16, device=d)
    nbytes = lib().csu_layernorm_bwd_workspace(M, C)
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=d)
    check(lib().csu_layernorm_bwd_ex(M, C, CSU_F32, ptr(x), ptr(gamma), ptr(mean), ptr(rstd), CSU_BF16, ptr(dx_b),
                                     ptr(dres), ptr(sdx), ptr(sdxb), None, None, ptr(work), nbytes, stream_ptr(d)),
          "layernorm_bwd")
    sdg, sdb = _param_reduce(work, M, C, 0)
    torch.cuda.synchronize()
    alone = {"dx": sdx, "dgamma": sdg, "dbeta": sdb}

    dh, gl, dx, dxb, dg, db = _fused(M, C, rpi, h, dy, w1, b1, w2, x, gamma, mean, rstd, dres)
    # the weight-gradient operands are the plain kernel's, bit for bit
    assert torch.equal(dh, dh0) and torch.equal(gl, g0)
    fused = {"dx": dx, "dgamma": dg, "dbeta": db}
    figs = {}
    for k in ("dx", "dgamma", "dbeta"):
        ef = float((fused[k].double() - ref[k]).abs().max())
        ea = float((alone[k].double() - ref[k]).abs().max())
        figs[k] = (ef, ea, float(ref[k].abs().max()))
        print(f"mlp lnbwd C={C} M={M} dres={int(with_dres)} {k}: fused {ef:.3e} stand-alone {ea:.3e} max|ref| {figs[k][2]:.3e}")
    for k, (ef, ea, mx) in figs.items():
        assert ef <= 2 * ea + 1e-6 * mx, (k, ef, ea, mx)
    assert torch.equal(dxb, dx.bfloat16())
    # fixed summation order, no atomics: a second launch gives the same bits
    second = _fused(M, C, rpi, h, dy, w1, b1, w2, x, gamma, mean, rstd, dres)
    for a, b in zip((dh, gl, dx, dxb, dg, db), second):
        assert torch.equal(a, b)


def test_mlp_bwd_ln_supported():
    """The predicate, and ops.ln_mlp_residual declining what the kernel does not have."""
    from csu import ops
    from csu._lib import lib
    d = dev()
    L = lib()
    assert L.csu_mlp_bwd_ln_supported(64, 128) and L.csu_mlp_bwd_ln_supported(192, 256)
    assert not L.csu_mlp_bwd_ln_supported(100, 128) and not L.csu_mlp_bwd_ln_supported(100, 256)
    assert not L.csu_mlp_bwd_ln_supported(128, 64) and not L.csu_mlp_bwd_ln_supported(128, 512)
    for M, C in ((100, 128), (128, 64), (128, 512)):
        ln = torch.nn.LayerNorm(C).to(d)
        fc1, fc2 = torch.nn.Linear(C, 4 * C).to(d), torch.nn.Linear(4 * C, C).to(d)
        x = torch.randn(1, M, C, device=d)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert ops.ln_mlp_residual(x, ln, fc1, fc2, None, None) is None


@pytest.mark.parametrize("C", [256, 128])
def test_ln_mlp_residual_block(C, monkeypatch):
    """ops.ln_mlp_residual after a proj + residual GEMM that computes norm2 in its epilogue (the _ln_pre
    path), inside an active weight cache (B = 2, L = 256): the fused path and the switch-off path
    (layer_norm_fork + mlp_residual, what CSWinBlock runs then) give the same y bit for bit, and every
    gradient within the kernel test's bound against an fp64 reference of the block."""
    from csu import ops
    d = dev()
    g = torch.Generator(device=d).manual_seed(11 + C)
    B, L = 2, 256
    x0 = torch.randn(B, L, C, device=d, generator=g) + 2.0 * torch.randn(B, L, 1, device=d, generator=g)
    a0 = torch.randn(B, L, C, device=d, generator=g).bfloat16()
    proj = torch.nn.Linear(C, C).to(d)
    ln = torch.nn.LayerNorm(C).to(d)
    fc1, fc2 = torch.nn.Linear(C, 4 * C).to(d), torch.nn.Linear(4 * C, C).to(d)
    with torch.no_grad():
        ln.weight.copy_(torch.rand(C, device=d, generator=g) + 0.5)
        ln.bias.copy_(torch.rand(C, device=d, generator=g) * 0.4 - 0.2)
        fc1.bias.copy_(torch.rand(4 * C, device=d, generator=g) * 0.2 - 0.1)
        fc2.bias.copy_(torch.rand(C, device=d, generator=g) * 0.2 - 0.1)
    G = torch.randn(B, L, C, device=d, generator=g)
    params = [ln.weight, ln.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias]
    cache = ops.CastCache()
    cache.refresh([proj.weight, fc1.weight, fc2.weight], torch.bfloat16)
    cache.refresh_frag()
    outs = {}
    try:
        ops.set_cast_cache(cache)
        for fused in (False, True):
            monkeypatch.setattr(ops, "FUSE_LN_MLP", fused)
            for p in params + [proj.weight, proj.bias]:
                p.grad = None
            x = x0.clone().requires_grad_(True)
            calls = []
            real = ops._launch
            # (name, tag, flops): the batched dgamma / dbeta reduction is charged to "layernorm_bwd" with 0 FLOPs
            monkeypatch.setattr(ops, "_launch", lambda name, fn, flops=0, *a, **k: (
                calls.append((name, str(k.get("tag", "")), flops)), real(name, fn, flops, *a, **k))[1])
            with torch.autocast("cuda", dtype=torch.bfloat16):
                x1 = ops.linear_residual(x, a0, proj.weight, proj.bias, ln_next=(ln.weight, ln.bias, ln.eps))
                assert getattr(x1, "_csu_ln", None) is not None      # norm2 came out of the proj epilogue
                y = ops.ln_mlp_residual(x1, ln, fc1, fc2, None, None)
                assert (y is not None) == fused
                if y is None:
                    xb, h2 = ops.layer_norm_fork(x1, ln.weight, ln.bias, ln.eps, torch.bfloat16)
                    y = ops.mlp_residual(xb, h2, fc1, fc2, None, ln_next=None)
            assert not any(c[0] == "layernorm_fwd" for c in calls)   # _ln_pre: no LayerNorm launch in either path
            (y * G).sum().backward()
            torch.cuda.synchronize()
            monkeypatch.setattr(ops, "_launch", real)
            # one Mlp backward launch, the lnbwd one when on; no stand-alone LayerNorm-backward kernel then
            assert [("lnbwd" in t) for n, t, _ in calls if n == "mlp_bwd"] == [fused]
            assert sum(1 for n, _, fl in calls if n == "layernorm_bwd" and fl > 0) == (0 if fused else 1)
            # the proj + residual backward hands x its gradient unchanged: x.grad is the junction's dx
            outs[fused] = (y.detach().clone(), x1.detach().clone(), [x.grad.clone()] + [p.grad.detach().clone() for p in params])
    finally:
        ops.set_cast_cache(None)
    assert torch.equal(outs[False][0], outs[True][0])
    # fp64 reference of the junction on the proj output x1 both paths saw
    xr = outs[True][1].double().requires_grad_(True)
    pr = [p.detach().double().requires_grad_(True) for p in params]
    hr = torch.nn.functional.layer_norm(xr, (C,), pr[0], pr[1], ln.eps)
    yr = xr + torch.nn.functional.gelu(hr @ pr[2].t() + pr[3]) @ pr[4].t() + pr[5]
    (yr * G.double()).sum().backward()
    refs = [xr.grad] + [p.grad for p in pr]
    for name, a, b, r in zip(["dx", "dgamma", "dbeta", "dW1", "db1", "dW2", "db2"], outs[True][2], outs[False][2], refs):
        ef, eu, mx = float((a.double() - r).abs().max()), float((b.double() - r).abs().max()), float(r.abs().max())
        print(f"ln_mlp_residual block C={C} {name}: fused {ef:.3e} unfused {eu:.3e} max|ref| {mx:.3e}")
        assert ef <= 2 * eu + 1e-6 * mx, (name, ef, eu, mx)
