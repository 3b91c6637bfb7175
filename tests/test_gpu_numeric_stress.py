"""Numeric stress parity on the MI355X: the model's kernels against the fp64 reference of the same
operation on inputs that make their numerical safeguards work -- softmax max subtraction and
running-max rescale (|logit| up to ~190), two-pass / pivot-shifted variances (mean / std up to 100,
variance 0 and far below eps), GELU tails out to |h| > 12, a sigmoid head that saturates to exactly
0 / 1, e4m3 scales on and next to their power-of-two boundaries, AdamW gradients over 30 decades.

The inputs come from stress_inputs.py, whose fp32-eager preconditions test_numeric_stress_inputs.py
checks on the CPU.  Criteria: tests/test_gpu_kernels.py::assert_close's (fp32: rtol 1e-4, atol 1e-5 *
max(1, max|ref|); bf16: rel-L2 < 2e-2 and max-abs < 3e-2 * max|ref|), applied per kind of row / channel /
token group, never over a whole tensor (stress_inputs.usage restates the helper as the used fraction of
its bound; the CPU tests check the two agree).  Every test prints the used fraction of its bound per kind
("numeric_stress ..." lines; a run's figures are kept in profiles/numeric_stress.txt)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import stress_inputs as S

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def judge(family, figs, limit=1.0):
    """Print every figure (used fraction of the bound), then require each to be within the bound."""
    for k, v in figs.items():
        print(f"numeric_stress {family} {k}: {v:.3f} of the bound")
    bad = {k: v for k, v in figs.items() if not v <= limit}
    assert not bad, (family, bad)


def kinds_figs(figs, name, got, ref, kinds, dim, dtype, names=None):
    for k, v in S.by_kind(got, ref, kinds, dim, dtype).items():
        figs[f"{name}[{names[k] if names else k}]"] = v


def dname(dt):
    return {F32: "fp32", BF16: "bf16"}[dt]


# ---------------------------------------------------------------------------------------------
# 1. stripe attention
# ---------------------------------------------------------------------------------------------
def _attn_gpu(case, inp, drop=None):
    from csu import ops
    d = dev()
    reso, idx, sw, cb, heads, B = case
    qd = inp["qkv"].to(d).requires_grad_(True)
    wd, bd = inp["w"].to(d).requires_grad_(True), inp["b"].to(d).requires_grad_(True)
    geom = ops.StripeGeometry(reso, cb, heads, [(inp["hs"], inp["ws"], 0)], inp["scale"])
    out = ops.stripe_attention(qd, geom, [wd], [bd]) if drop is None else ops.stripe_attention(qd, geom, [wd], [bd], drop)
    out.backward(inp["gout"].to(d))
    torch.cuda.synchronize()
    assert out.dtype == inp["qkv"].dtype
    return out.detach().cpu(), qd.grad.cpu(), wd.grad.cpu(), bd.grad.cpu()


def _emulation_rule(family, got, emu, ref, inp, only=None, tag=""):
    """Gradients under the sharp gains in bf16: the kernel's error against fp64 (max-abs and L2) may be
    at most twice the error of the bf16 emulation (stress_inputs.lepe_attention_plain: fp32 arithmetic,
    bf16 rounding only at P, O, dS and the outputs, delta from the rounded O -- the factor 2 is for a
    different summation order of the same terms) plus 1e-3 of the reference's magnitude."""
    ek, ee = S.attn_errors(got, ref, inp), S.attn_errors(emu, ref, inp)
    figs = {}
    for name in ek:
        if only is not None and name not in only:
            continue
        (ka, kl, mx), (ea, el, _) = ek[name], ee[name]
        name = name + tag
        print(f"numeric_stress {family} {name}: kernel max-abs {ka:.3e} rel-L2 {kl:.3e} | emulation max-abs {ea:.3e} "
              f"rel-L2 {el:.3e} | max|ref| {mx:.3e}")
        figs[name + " max-abs"] = S.ratio(ka, 2 * ea + 1e-3 * mx)
        figs[name + " rel-L2"] = S.ratio(kl, 2 * el + 1e-3)
    return figs


@pytest.mark.parametrize("case", S.STRESS_ATTN_CASES, ids=str)
def test_stripe_attention_fp32_sharp(case):
    inp, ref = S.attn_reference(case, S.GAINS_SHARP, F32)
    judge(f"attention fp32 sharp {case}", S.attn_usages(_attn_gpu(case, inp), ref, inp, F32))


@pytest.mark.parametrize("case", S.STRESS_ATTN_CASES, ids=str)
def test_stripe_attention_bf16_mild(case):
    inp, ref = S.attn_reference(case, S.GAINS_MILD, BF16)
    judge(f"attention bf16 mild {case}", S.attn_usages(_attn_gpu(case, inp), ref, inp, BF16))


@pytest.mark.parametrize("case", S.STRESS_ATTN_CASES, ids=str)
def test_stripe_attention_bf16_sharp(case):
    """Forward: the file's bf16 bound.  Gradients: _emulation_rule."""
    inp, ref = S.attn_reference(case, S.GAINS_SHARP, BF16)
    got = _attn_gpu(case, inp)
    emu = S.attn_eval(inp, case, F32, emulate_bf16=True)
    fam = f"attention bf16 sharp {case}"
    figs = {k: v for k, v in S.attn_usages(got, ref, inp, BF16).items() if k.startswith("out")}
    figs.update(_emulation_rule(fam, got, emu, ref, inp))
    judge(fam, figs)


def _two_branch_gpu(inp):
    from csu import ops
    d = dev()
    reso, C, heads, sw = (S.TWO_BRANCH[k] for k in ("reso", "C", "heads", "sw"))
    geom = ops.StripeGeometry(reso, C, heads // 2, [(reso, sw, 0), (sw, reso, C // 2)], inp["scale"])
    qd = inp["qkv"].to(d).requires_grad_(True)
    ws_ = [w.to(d).requires_grad_(True) for w in inp["ws"]]
    bs_ = [b.to(d).requires_grad_(True) for b in inp["bs"]]
    out = ops.stripe_attention(qd, geom, ws_, bs_)
    out.backward(inp["gout"].to(d))
    torch.cuda.synchronize()
    return out.detach().cpu(), qd.grad.cpu(), [w.grad.cpu() for w in ws_], [b.grad.cpu() for b in bs_]


@pytest.mark.parametrize("dtype,gains", [(F32, S.GAINS_SHARP), (BF16, S.GAINS_MILD), (BF16, S.GAINS_SHARP)],
                         ids=["fp32-sharp", "bf16-mild", "bf16-sharp"])
def test_two_branch_launch(dtype, gains):
    """The two-branch launch of test_two_branch_fused_launch, forward and backward.  Under the sharp
    gains in bf16 the forward is held to the file's bound and every gradient (dq, dk, dv per kind, both
    branches' LePE dW and db) to _emulation_rule, as the single-branch cases."""
    inp = S.two_branch_inputs(gains, dtype)
    ref, got = S.two_branch_eval(inp, F64), _two_branch_gpu(inp)
    fam = f"attention two-branch {dname(dtype)} gains {gains}"
    figs = S.attn_usages(S.two_branch_pack(got, 0), S.two_branch_pack(ref, 0), inp, dtype)
    figs["dW_lepe1"], figs["db_lepe1"] = S.usage(got[2][1], ref[2][1], dtype), S.usage(got[3][1], ref[3][1], dtype)
    if dtype == BF16 and gains == S.GAINS_SHARP:
        emu = S.two_branch_eval(inp, F32, emulate_bf16=True)
        figs = {k: v for k, v in figs.items() if k.startswith("out")}
        figs.update(_emulation_rule(fam, S.two_branch_pack(got, 0), S.two_branch_pack(emu, 0), S.two_branch_pack(ref, 0), inp))
        figs.update(_emulation_rule(fam, S.two_branch_pack(got, 1), S.two_branch_pack(emu, 1), S.two_branch_pack(ref, 1), inp,
                                    only=("dW_lepe", "db_lepe"), tag="1"))
    judge(fam, figs)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
def test_stripe_attention_dropout_sharp(dtype):
    """Attention dropout on the sharp P (ops.AttnDrop), the device's masks fed to the reference the
    way test_stripe_attention_dropout_vs_oracle does."""
    from csu import ops, rng
    d = dev()
    case = (14, 0, 7, 64, 2, 1)
    inp, _ = S.attn_reference(case, S.GAINS_SHARP, dtype)
    snap = torch.tensor([77, 1], dtype=torch.int64, device=d)
    p = 0.3

    def mask(shape):
        Bw, H, N, _ = shape
        npad = -(-N // 32) * 32
        m = rng.dropout_mask(snap, 40, p, Bw * H * N * npad).view(Bw, H, N, npad)[..., :N]
        return m.double().cpu() / (1 - p)

    ref = S.attn_eval(inp, case, F64, attn_mask=mask)
    got = _attn_gpu(case, inp, ops.AttnDrop(snap, 40, p))
    fam = f"attention dropout {dname(dtype)} sharp {case}"
    if dtype == F32:
        figs = S.attn_usages(got, ref, inp, F32)
    else:
        emu = S.attn_eval(inp, case, F32, emulate_bf16=True, attn_mask=mask)
        figs = {k: v for k, v in S.attn_usages(got, ref, inp, BF16).items() if k.startswith("out")}
        figs.update(_emulation_rule(fam, got, emu, ref, inp))
    judge(fam, figs)
    nodrop = _attn_gpu(case, inp)[0]
    assert float((nodrop.float() - got[0].float()).abs().max()) > 1e-2      # the mask is really applied


# ---------------------------------------------------------------------------------------------
# 2. LayerNorm: every kernel that computes or differentiates it
# ---------------------------------------------------------------------------------------------
LN_ROWS = 70


@functools.lru_cache(maxsize=None)
def _ln_case(rows, C, xdt, ydt):
    x, kinds = S.ln_rows(rows, C, dtype=xdt)
    w, b = S.ln_params(C)
    dy = torch.randn(rows, C, generator=torch.Generator().manual_seed(C)).to(ydt)
    return x, kinds, w, b, dy, S.ln_eval(x, w, b, dy, F64)


@pytest.mark.parametrize("C", [64, 128, 256, 512])
@pytest.mark.parametrize("xdt,ydt", [(F32, F32), (F32, BF16), (BF16, BF16)], ids=["f32-f32", "f32-bf16", "bf16-bf16"])
def test_layer_norm_rows(C, xdt, ydt):
    from csu import ops
    d = dev()
    x, kinds, w, b, dy, ref = _ln_case(LN_ROWS, C, xdt, ydt)
    xd = x.view(1, LN_ROWS, C).to(d).requires_grad_(True)
    wd, bd = w.to(d).requires_grad_(True), b.to(d).requires_grad_(True)
    y = ops.layer_norm(xd, wd, bd, 1e-5, ydt)
    y.backward(dy.view(1, LN_ROWS, C).to(d))
    assert y.dtype == ydt
    tol = F32 if (xdt, ydt) == (F32, F32) else BF16
    figs = {}
    kinds_figs(figs, "y", y.view(LN_ROWS, C), ref[0], kinds, 0, tol, S.LN_KINDS)
    kinds_figs(figs, "dx", xd.grad.view(LN_ROWS, C), ref[1], kinds, 0, tol, S.LN_KINDS)
    figs["dgamma"], figs["dbeta"] = S.usage(wd.grad, ref[2], tol), S.usage(bd.grad, ref[3], tol)
    judge(f"layer_norm C={C} {dname(xdt)}->{dname(ydt)}", figs)


@pytest.mark.parametrize("C", [64, 128, 256, 512])
@pytest.mark.parametrize("gdt", [F32, BF16], ids=dname)
def test_layer_norm_fork_rows(C, gdt):
    """x -> (x, LN(x)) with gradients through both (test_layernorm_fork_residual_junction's form and
    tolerance classes) on the stress rows."""
    from csu import ops
    d = dev()
    x, kinds = S.ln_rows(LN_ROWS, C)
    w, b = S.ln_params(C)
    g = torch.Generator().manual_seed(C + 7)
    gres = torch.randn(LN_ROWS, C, generator=g)
    gln = torch.randn(LN_ROWS, C, generator=g).to(gdt)
    x64 = x.double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y64 = torch.nn.functional.layer_norm(x64, (C,), w64, b64, 1e-5)
    ((x64 * gres.double()).sum() + (y64 * gln.double()).sum()).backward()
    x0 = x.view(1, LN_ROWS, C).to(d).requires_grad_(True)
    wd, bd = w.to(d).requires_grad_(True), b.to(d).requires_grad_(True)
    xa, y = ops.layer_norm_fork(x0.view_as(x0), wd, bd, 1e-5, gdt)
    ((xa * gres.view(1, LN_ROWS, C).to(d)).sum() + (y.float() * gln.view(1, LN_ROWS, C).to(d).float()).sum()).backward()
    figs = {}
    kinds_figs(figs, "y", y.view(LN_ROWS, C), y64.detach(), kinds, 0, gdt, S.LN_KINDS)
    kinds_figs(figs, "dx", x0.grad.view(LN_ROWS, C), x64.grad, kinds, 0, gdt, S.LN_KINDS)
    figs["dgamma"], figs["dbeta"] = S.usage(wd.grad, w64.grad, BF16), S.usage(bd.grad, b64.grad, BF16)
    judge(f"layer_norm_fork C={C} grad {dname(gdt)}", figs)


def _frag(w):
    """csu_frag_layout_batch of one bf16 (rows, cols) matrix (as tests/test_gpu_ln_qkv_fused.py)."""
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


WS_M = 128      # two 64-token panels; kind = row % 7, so each panel holds every kind


def _row_scale(res, kinds):
    """Per-row magnitude of the token operand of a fused epilogue: half the row's own spread, 0 on the
    constant rows, so that the GEMM / Mlp term keeps every row in its kind."""
    s = res.double().std(1, keepdim=True).float() * 0.5
    s[kinds == 5] = 0.5          # the one-outlier rows: the spread of their other features
    return s


def _epilogue_ln_figs(figs, y, h, mean, rstd, gam, bet, kinds, eps=1e-5):
    """LayerNorm output / mean / rstd of a fused epilogue against an fp64 LayerNorm of the kernel's own
    fp32 output y: h (bf16) by the bf16 bound, mean and rstd (fp32) by the fp32 criterion, per kind."""
    y64 = y.double().cpu()
    mu = y64.mean(-1)
    var = y64.var(-1, unbiased=False)
    h64 = (y64 - mu[:, None]) / torch.sqrt(var[:, None] + eps) * gam.double().cpu() + bet.double().cpu()
    kinds_figs(figs, "ln_out", h, h64, kinds, 0, BF16, S.LN_KINDS)
    kinds_figs(figs, "mean", mean.view(-1, 1), mu.view(-1, 1), kinds, 0, F32, S.LN_KINDS)
    kinds_figs(figs, "rstd", rstd.view(-1, 1), torch.rsqrt(var + eps).view(-1, 1), kinds, 0, F32, S.LN_KINDS)


@pytest.mark.parametrize("C", [64, 128, 256])
def test_gemm_ws_ln_residual_rows(C):
    """csu_gemm_ws_ln (proj + residual, norm2 in the epilogue): the residual operand carries the stress
    rows.  y against the fp64 GEMM + residual (fp32 criterion per kind), the LayerNorm against an fp64
    LayerNorm of y."""
    from csu._lib import lib, ptr, stream_ptr
    d = dev()
    M = WS_M
    res, kinds = S.ln_rows(M, C, seed=3)
    g = torch.Generator().manual_seed(C)
    x = (torch.randn(M, C, generator=g) * _row_scale(res, kinds)).bfloat16()
    w = (torch.randn(C, C, generator=g) / C ** 0.5).bfloat16()
    gam, bet = S.ln_params(C)
    bias = torch.zeros(C)
    xd, wd, resd, gd, bd, biasd = (t.to(d) for t in (x, w, res, gam, bet, bias))
    wf = _frag(wd)
    assert lib().csu_gemm_ws_ln_supported(M, C, C)
    y = torch.empty(M, C, device=d)
    h = torch.empty(M, C, device=d, dtype=BF16)
    mean, rstd = torch.empty(M, device=d), torch.empty(M, device=d)
    rc = lib().csu_gemm_ws_ln(M, C, ptr(xd), C, ptr(wf), ptr(biasd), ptr(resd), ptr(y), ptr(gd), ptr(bd), 1e-5, ptr(h),
                              ptr(mean), ptr(rstd), stream_ptr(d))
    torch.cuda.synchronize()
    assert rc == 0
    figs = {}
    kinds_figs(figs, "y", y, x.double() @ w.double().t() + res.double(), kinds, 0, F32, S.LN_KINDS)
    _epilogue_ln_figs(figs, y, h, mean, rstd, gam, bet, kinds)
    judge(f"gemm_ws_ln C={C}", figs)


@pytest.mark.parametrize("C", [64, 128, 256])
def test_mlp_fwd_ln_residual_rows(C):
    """csu_mlp_fwd_ln (the fused Mlp with the next block's norm1 in its epilogue) through
    ops.mlp_residual(ln_next=...): stress rows in the residual operand.  y against the fp64 Mlp + residual
    (bf16 bound per kind: the hidden layer is bf16), the LayerNorm against an fp64 LayerNorm of y."""
    from csu import ops
    d = dev()
    M = WS_M
    res, kinds = S.ln_rows(M, C, seed=5)
    g = torch.Generator().manual_seed(C + 1)
    x = (torch.randn(M, C, generator=g) * _row_scale(res, kinds)).bfloat16()
    fc1, fc2 = torch.nn.Linear(C, 4 * C), torch.nn.Linear(4 * C, C)
    with torch.no_grad():
        fc1.weight.copy_((torch.randn(4 * C, C, generator=g) * C ** -0.5).bfloat16())
        fc2.weight.copy_((torch.randn(C, 4 * C, generator=g) * (4 * C) ** -0.5).bfloat16())
        fc1.bias.zero_()
        fc2.bias.zero_()
    gam, bet = S.ln_params(C)
    W1, W2 = fc1.weight.detach().double(), fc2.weight.detach().double()
    ref_y = res.double() + S.gelu_exact(x.double() @ W1.t()) @ W2.t()
    fc1, fc2 = fc1.to(d), fc2.to(d)
    gd, bd = gam.to(d), bet.to(d)
    with torch.no_grad():
        y = ops.mlp_residual(res.view(1, M, C).to(d), x.view(1, M, C).to(d), fc1, fc2, None, ln_next=(gd, bd, 1e-5))
    torch.cuda.synchronize()
    pre = y._csu_ln
    figs = {}
    kinds_figs(figs, "y", y.view(M, C), ref_y, kinds, 0, BF16, S.LN_KINDS)
    _epilogue_ln_figs(figs, y.view(M, C), pre[3].view(M, C), pre[4].view(-1), pre[5].view(-1), gam, bet, kinds)
    judge(f"mlp_fwd_ln C={C}", figs)


def _param_reduce(work, rows, C, nblocks):
    from csu import _lib
    from csu._lib import check, lib, stream_ptr
    dgb = torch.empty(2 * C, dtype=torch.float32, device=work.device)
    it = (_lib.LnParamItem * 1)()
    it[0].workspace, it[0].dgamma, it[0].dbeta = work.data_ptr(), dgb.data_ptr(), dgb.data_ptr() + C * 4
    it[0].rows, it[0].C, it[0].nblocks = rows, C, nblocks
    check(lib().csu_layernorm_param_reduce_batch(it, 1, stream_ptr(work.device)), "param_reduce")
    return dgb[:C].clone(), dgb[C:].clone()


@pytest.mark.parametrize("C", [128, 256])
def test_gemm_ws_lnbwd_rows(C):
    """csu_gemm_ws_lnbwd (norm1's backward in the qkv input-gradient GEMM) with the stress rows as the
    LayerNorm's input, under the kernel's own rule (tests/test_gpu_ln_qkv_fused.py): error <= 2 x the
    stand-alone csu_layernorm_bwd's + 1e-6 max|ref|, here per kind of row; and the stand-alone kernel's dx
    against the same fp64 reference by the fp32 criterion per kind."""
    from csu._lib import CSU_BF16, CSU_F32, check, lib, ptr, stream_ptr
    d = dev()
    M, K = WS_M, 3 * C
    assert lib().csu_gemm_ws_lnbwd_supported(M, C, K)
    xc, kinds = S.ln_rows(M, C, seed=9)
    g = torch.Generator().manual_seed(1000 * C)
    gamma = (torch.rand(C, generator=g) + 0.5).to(d)
    dy = torch.randn(M, K, generator=g).bfloat16().to(d)
    dres = torch.randn(M, C, generator=g).to(d)
    w = (torch.randn(K, C, generator=g) / C ** 0.5).bfloat16().to(d)
    wtf = _frag(w.t().contiguous())
    x = xc.to(d)
    xd = xc.double()
    mean = xd.mean(1).float().to(d)
    rstd = (1.0 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5)).float().to(d)
    dh_b = torch.empty(M, C, dtype=BF16, device=d)
    check(lib().csu_gemm_ws(M, C, K, ptr(dy), K, ptr(wtf), None, None, CSU_BF16, ptr(dh_b), stream_ptr(d)), "gemm_ws")
    torch.cuda.synchronize()
    # fp64 LayerNorm backward of dh_b with the fp32 mean / rstd the kernels get
    dh = dh_b.double().cpu()
    m64, r64 = mean.double().cpu(), rstd.double().cpu()
    xh = (xd - m64[:, None]) * r64[:, None]
    gg = dh * gamma.double().cpu()
    ref_dx = r64[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True)) + dres.double().cpu()
    ref = {"dgamma": (dh * xh).sum(0), "dbeta": dh.sum(0)}
    # stand-alone pair
    sdx = torch.empty(M, C, dtype=F32, device=d)
    sdxb = torch.empty(M, C, dtype=BF16, device=d)
    nbytes = lib().csu_layernorm_bwd_workspace(M, C)
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=d)
    check(lib().csu_layernorm_bwd_ex(M, C, CSU_F32, ptr(x), ptr(gamma), ptr(mean), ptr(rstd), CSU_BF16, ptr(dh_b),
                                     ptr(dres), ptr(sdx), ptr(sdxb), None, None, ptr(work), nbytes, stream_ptr(d)),
          "layernorm_bwd")
    sdg, sdb = _param_reduce(work, M, C, 0)
    # fused
    dx = torch.empty(M, C, dtype=F32, device=d)
    dxb = torch.empty(M, C, dtype=BF16, device=d)
    part = torch.empty(M // 64 * 2 * C, dtype=F32, device=d)
    check(lib().csu_gemm_ws_lnbwd(M, C, K, ptr(dy), ptr(wtf), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres),
                                  ptr(dx), ptr(dxb), ptr(part), stream_ptr(d)), "gemm_ws_lnbwd")
    dg, db = _param_reduce(part, M, C, M // 64)
    torch.cuda.synchronize()
    figs = {}
    fam = f"gemm_ws_lnbwd C={C}"

    def rule(name, fused, alone, r):
        ef, ea = float((fused.double().cpu() - r).abs().max()), float((alone.double().cpu() - r).abs().max())
        mx = float(r.abs().max())
        print(f"numeric_stress {fam} {name}: fused {ef:.3e} stand-alone {ea:.3e} max|ref| {mx:.3e}")
        figs[name + " (<= 2 x stand-alone + 1e-6 max|ref|)"] = S.ratio(ef, 2 * ea + 1e-6 * mx)

    for k in sorted(set(kinds.tolist())):
        rows = kinds == k
        rule(f"dx[{S.LN_KINDS[k]}]", dx[rows.to(d)], sdx[rows.to(d)], ref_dx[rows])
    rule("dgamma", dg, sdg, ref["dgamma"])
    rule("dbeta", db, sdb, ref["dbeta"])
    kinds_figs(figs, "stand-alone dx", sdx, ref_dx, kinds, 0, F32, S.LN_KINDS)
    judge(fam, figs)
    assert torch.equal(dxb, dx.bfloat16())


# ---------------------------------------------------------------------------------------------
# 3. SimAM, BatchNorm + ReLU
# ---------------------------------------------------------------------------------------------
SIMAM_SHAPES = [(2, 64, 32), (3, 17, 200), (2, 1000, 256)]


@functools.lru_cache(maxsize=None)
def _simam_case(shape, dtype):
    x, kinds = S.channel_kinds(shape, True, dtype=dtype)
    dy = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(dtype)
    return x, kinds, dy, S.simam_eval(x, dy, F64)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
@pytest.mark.parametrize("shape", SIMAM_SHAPES, ids=str)
def test_simam_channels(shape, dtype):
    from csu.simam import simam
    d = dev()
    x, kinds, dy, ref = _simam_case(shape, dtype)
    xd = x.to(d).requires_grad_(True)
    y = simam(xd)
    y.backward(dy.to(d))
    figs = {}
    kinds_figs(figs, "y", y, ref[0], kinds, 2, dtype, S.CH_KINDS)
    kinds_figs(figs, "dx", xd.grad, ref[1], kinds, 2, dtype, S.CH_KINDS)
    # bf16 output for the GEMM consumer, bf16 incoming gradient
    xb = x.to(d).requires_grad_(True)
    yb = simam(xb, out_dtype=BF16)
    dyb = dy.bfloat16()
    yb.backward(dyb.to(d))
    refb = S.simam_eval(x, dyb, F64)
    kinds_figs(figs, "y->bf16", yb, refb[0], kinds, 2, BF16, S.CH_KINDS)
    kinds_figs(figs, "dx(bf16 dy)", xb.grad, refb[1], kinds, 2, BF16, S.CH_KINDS)
    judge(f"simam {shape} {dname(dtype)}", figs)


@pytest.mark.parametrize("shape", SIMAM_SHAPES, ids=str)
def test_simam_fork_channels(shape):
    """simam_fork: (bf16 x, bf16 SimAM(x)) and the joined gradient against fp64, bf16 bound per kind."""
    from csu.simam import simam_fork
    d = dev()
    x, kinds = S.channel_kinds(shape, True)
    g = torch.Generator().manual_seed(2)
    g1, dy = torch.randn(shape, generator=g).bfloat16(), torch.randn(shape, generator=g).bfloat16()
    x64 = x.double().requires_grad_(True)
    y64 = S.simam_ref(x64)
    torch.autograd.backward([x64 * 1.0, y64], [g1.double(), dy.double()])
    xd = x.to(d).requires_grad_(True)
    xc, y = simam_fork(xd)
    torch.autograd.backward([xc, y], [g1.to(d), dy.to(d)])
    assert torch.equal(xc.cpu(), x.bfloat16())
    figs = {}
    kinds_figs(figs, "y", y, y64.detach(), kinds, 2, BF16, S.CH_KINDS)
    kinds_figs(figs, "dx", xd.grad, x64.grad, kinds, 2, BF16, S.CH_KINDS)
    judge(f"simam_fork {shape}", figs)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
@pytest.mark.parametrize("shape", [(2, 5, 7, 64), (4, 9, 11, 72)], ids=str)
def test_bn_relu_channels(shape, dtype):
    """csu_bn_relu in training mode through csu.unet.bn_relu_nhwc: y, dx, dgamma, dbeta and the
    running-stat update per channel kind (fp32 statistics: the running stats take the fp32 criterion
    in both dtypes)."""
    from csu.unet import bn_relu_nhwc
    d = dev()
    C = shape[-1]
    x, kinds = S.channel_kinds(shape, False, dtype=dtype)
    dy = torch.randn(shape, generator=torch.Generator().manual_seed(2)).to(dtype)
    w, b, rm, rv = S.bn_params(C)
    ref = S.bn_eval(x, w, b, rm, rv, dy, F64)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(w), bn.bias.copy_(b), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    bnd = bn.to(d).train()
    xd = x.to(d).requires_grad_(True)
    y = bn_relu_nhwc(xd, bnd, True)
    y.backward(dy.to(d))
    assert y.dtype == dtype
    got = (y, xd.grad, bnd.weight.grad, bnd.bias.grad, bnd.running_mean, bnd.running_var)
    figs = {}
    for i, name in enumerate(S.BN_OUT):
        kinds_figs(figs, name, got[i], ref[i], kinds, got[i].dim() - 1, F32 if i >= 4 else dtype, S.CH_KINDS)
    judge(f"bn_relu {shape} {dname(dtype)}", figs)


# ---------------------------------------------------------------------------------------------
# 4. CARAFE tap softmax, sigmoid heads
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
@pytest.mark.parametrize("B,H,C,s", S.CARAFE_SHAPES)
def test_carafe_reassemble_sharp_shifted_logits(B, H, C, s, dtype):
    from csu import ops
    d = dev()
    enc, kinds = S.carafe_logits(B, H, s, dtype=dtype)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, H * H, C, generator=g).to(dtype)
    gy = torch.randn(B, H * H * s * s, C, generator=g)
    ref = S.carafe_eval(x, enc, gy, H, s, F64)
    xd, ed = x.to(d).requires_grad_(True), enc.to(d).requires_grad_(True)
    y = ops.carafe_reassemble(xd, ed, H, H, s)
    y.float().backward(gy.to(d))
    figs = {}
    kinds_figs(figs, "out", y.float().reshape(-1, C), ref[0].reshape(-1, C), S.carafe_out_kinds(kinds, B, H, s), 0, dtype)
    kinds_figs(figs, "dx", xd.grad.float().reshape(-1, C), ref[1].reshape(-1, C), kinds, 0, dtype)
    kinds_figs(figs, "denc", ed.grad.float().reshape(B * H * H, -1), ref[2].reshape(B * H * H, -1), kinds, 0, dtype)
    judge(f"carafe_reassemble {(B, H, C, s)} {dname(dtype)}", figs)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
def test_sigmoid_head_saturated_into_bce(dtype):
    """ops.sigmoid_head chained into ops.bce_loss with the pre-activation spanning +-100 (kinds: |z| < 6,
    < 17, beyond: the fp32 probability is exactly 0 or 1).  The probability and dx per kind; in bf16 the
    saturated kind of dx is judged together with the others over all pixels instead of alone: the bf16
    criterion has no absolute term, and dx = (p - t) w / n from an fp32 probability cannot resolve p - t
    below 2^-24, the whole value on a saturated pixel."""
    from csu import ops
    d = dev()
    P, C = 515, 64
    x, w, t = S.head_inputs(P, C, dtype=dtype)
    ref = S.head_eval(x, w, t, F64)
    kinds = S.head_kinds(x.double() @ w.double().view(C))
    xd, wd = x.to(d).requires_grad_(True), w.to(d).requires_grad_(True)
    p = ops.sigmoid_head(xd, wd)
    loss = ops.bce_loss(p, t.to(d))
    loss.backward()
    assert p.dtype == F32
    assert int(((p == 0) | (p == 1)).sum()) > 10
    figs = {"loss": S.usage(loss, ref[1], dtype), "dw": S.usage(wd.grad, ref[3], dtype)}
    kinds_figs(figs, "prob", p, ref[0], kinds, 0, dtype)
    if dtype == F32:
        kinds_figs(figs, "dx", xd.grad.float(), ref[2], kinds, 0, dtype)
    else:
        unsat = (kinds < 2).nonzero().flatten()
        kinds_figs(figs, "dx", xd.grad.float().cpu()[unsat], ref[2][unsat], kinds[unsat], 0, dtype)
        figs["dx[all pixels]"] = S.usage(xd.grad.float(), ref[2], dtype)
    judge(f"sigmoid_head+bce {dname(dtype)}", figs)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dname)
@pytest.mark.parametrize("folded", [False, True], ids=["carafe_head", "carafe_head_folded"])
@pytest.mark.parametrize("B,H,C,s", [(2, 5, 64, 2), (1, 5, 32, 4)])
def test_carafe_head_saturated_into_bce(B, H, C, s, folded, dtype):
    """ops.carafe_head (u = W_out^T w_h, cb = w_h . b_out given) and ops.carafe_head_folded (raw head
    weights) with sharp / shifted tap logits and a pre-activation spanning +-100, chained into
    ops.bce_loss: probabilities, loss and every gradient against fp64."""
    from csu import ops
    d = dev()
    x, enc, w_out, b_out, w_h, t, kinds = S.carafe_head_inputs(B, H, C, s, dtype=dtype)
    xd, ed = x.to(d).requires_grad_(True), enc.to(d).requires_grad_(True)
    if folded:
        ref = S.carafe_head_eval(x, enc, w_out, b_out, w_h, t, H, s, F64)
        ps = [v.to(d).requires_grad_(True) for v in (w_out, b_out, w_h.view(1, -1))]
        p = ops.carafe_head_folded(xd, ed, ps[0], ps[1], ps[2], H, H, s)
        names = S.CARAFE_HEAD_OUT
    else:
        u, cb = w_out.t() @ w_h, (w_h @ b_out).reshape(())
        x64, e64 = x.double().requires_grad_(True), enc.double().requires_grad_(True)
        u64, c64 = u.double().requires_grad_(True), cb.double().requires_grad_(True)
        p64 = torch.sigmoid(S.carafe_reassemble_ref(x64, e64, H, s) @ u64 + c64).view(B, 1, s * H, s * H)
        l64 = S.bce_clamped(p64, t.double())
        l64.backward()
        ref = (p64.detach(), l64.detach(), x64.grad, e64.grad, u64.grad, c64.grad)
        ps = [u.to(d).requires_grad_(True), cb.to(d).requires_grad_(True)]
        p = ops.carafe_head(xd, ed, ps[0], ps[1], H, H, s)
        names = ("prob", "loss", "dx", "denc", "du", "dcb")
    loss = ops.bce_loss(p, t.to(d))
    loss.backward()
    assert p.dtype == F32 and int(((p == 0) | (p == 1)).sum()) > 0
    got = (p, loss, xd.grad.float(), ed.grad.float()) + tuple(q.grad.reshape(r.shape) for q, r in zip(ps, ref[4:]))
    judge(f"{'carafe_head_folded' if folded else 'carafe_head'}+bce {(B, H, C, s)} {dname(dtype)}",
          S.carafe_head_usages(names, got, ref, kinds, B, H, s, dtype))


# ---------------------------------------------------------------------------------------------
# 5. fused Mlp and the GELU epilogues
# ---------------------------------------------------------------------------------------------
MLP_SHAPES = [(64, 37), (128, 100), (256, 100)]


@pytest.mark.parametrize("C,M", MLP_SHAPES)
def test_mlp_fused_gelu_tails(C, M):
    """csu_mlp_fwd / csu_mlp_bwd (and at C = 64 csu_mlp_bwd_wgrad) with h out to |h| > 12 against the
    exact-erf fp64 Mlp on the same bf16 operands: bf16 bound; g, dh, dW1 and db1 per gain group of hidden
    features.  Where the kernel does not form them (C != 64) dW / db come from ops.linear_wgrad on the
    kernel's dh and g, as in the two-step path."""
    from csu import _lib, ops
    from csu._lib import check, lib, ptr, stream_ptr
    d = dev()
    inp = S.mlp_inputs(C, M)
    ref = S.mlp_eval(inp, F64)
    x, w1, b1, w2, b2, res, dy = (inp[k].to(d) for k in ("x", "w1", "b1", "w2", "b2", "res", "dy"))
    st = stream_ptr(d)
    y = torch.empty(M, C, device=d)
    check(lib().csu_mlp_fwd(M, C, ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(res), ptr(y), st), "mlp_fwd")
    dh = torch.empty(M, 4 * C, device=d, dtype=BF16)
    gl = torch.empty_like(dh)
    dx = torch.empty(M, C, device=d, dtype=BF16)
    check(lib().csu_mlp_bwd(M, C, ptr(x), ptr(dy), ptr(w1), ptr(b1), ptr(w2), ptr(dh), ptr(gl), ptr(dx), st), "mlp_bwd")
    torch.cuda.synchronize()
    got = {"y": y, "g": gl, "dh": dh, "dx": dx}
    dw1, db1 = ops.linear_wgrad(dh, x)
    dw2, db2 = ops.linear_wgrad(dy, gl)
    got.update({"dW1": dw1, "db1": db1, "dW2": dw2, "db2": db2})
    if lib().csu_mlp_bwd_wgrad_supported(C):
        n1, n2 = ctypes.c_size_t(), ctypes.c_size_t()
        check(lib().csu_mlp_bwd_wgrad_workspace(M, C, ctypes.byref(n1), ctypes.byref(n2)), "workspace")
        s1 = torch.full((n1.value // 4,), float("nan"), device=d)
        s2 = torch.full((n2.value // 4,), float("nan"), device=d)
        o1 = torch.full((4 * C * C + 4 * C,), float("nan"), device=d)
        o2 = torch.full((4 * C * C + C,), float("nan"), device=d)
        dxw = torch.empty(M, C, device=d, dtype=BF16)
        items = (_lib.WslabItem * 2)()
        check(lib().csu_mlp_bwd_wgrad(M, C, ptr(x), ptr(dy), ptr(w1), ptr(b1), ptr(w2), ptr(dxw), None, ptr(s1), ptr(s2),
                                      ctypes.byref(items[0]), ctypes.byref(items[1]), ptr(o1), ptr(o2), st), "mlp_bwd_wgrad")
        check(lib().csu_wslab_reduce_batch(items, 2, st), "wslab_reduce_batch")
        torch.cuda.synchronize()
        assert torch.equal(dxw, dx)
        got.update({"wgrad dW1": o1[:4 * C * C].view(4 * C, C), "wgrad db1": o1[4 * C * C:],
                    "wgrad dW2": o2[:4 * C * C].view(C, 4 * C), "wgrad db2": o2[4 * C * C:]})
    h = inp["x"].double() @ inp["w1"].double().t() + inp["b1"].double()
    assert float(h.abs().max()) > 12.0
    figs = {}
    for name, t in got.items():
        key = name.replace("wgrad ", "")
        if key in ("g", "dh", "dW1", "db1"):
            kinds_figs(figs, name, t, ref[key], inp["kinds"], 1 if key in ("g", "dh") else 0, BF16,
                       [f"gain {v:g}" for v in S.MLP_GAINS])
        else:
            figs[name] = S.usage(t, ref[key], BF16)
    judge(f"mlp C={C} M={M}", figs)


@pytest.mark.parametrize("M,N,K", [(77, 64, 8), (513, 256, 32)])
@pytest.mark.parametrize("mode", ["bias_gelu_a", "gelu_aux"])
def test_gemm_gelu_epilogue_tails(M, N, K, mode):
    """csu_gemm with GELU on its A operand (bias_gelu_a) and with the GELU derivative of an auxiliary
    tensor in its epilogue (gelu_aux), the GELU argument spanning the tails (gain {1, 4, 12} per feature,
    offsets {0, +-6}): exact-erf fp64 on the same bf16 operands, bf16 bound (gelu_aux: per gain group
    of output features)."""
    from csu import ops
    d = dev()
    g = torch.Generator().manual_seed(M + N + K)

    def tails(rows, cols):
        kinds = torch.arange(cols) % 3
        v = torch.randn(rows, cols, generator=g) * torch.tensor(S.MLP_GAINS)[kinds]
        return (v + torch.tensor([0.0, 6.0, -6.0])[(torch.arange(cols) // 3) % 3]).bfloat16(), kinds

    w = (torch.randn(N, K, generator=g) * 0.1).bfloat16()
    figs = {}
    if mode == "bias_gelu_a":
        a, _ = tails(M, K)
        bias = torch.randn(N, generator=g)
        out = ops.gemm(a.to(d), w.to(d), False, BF16, bias=bias.to(d), a_gelu=True)
        ref = S.gelu_exact(a.double()) @ w.double().t() + bias.double()
        figs["out"] = S.usage(out, ref, BF16)
    else:
        a = torch.randn(M, K, generator=g).bfloat16()
        aux, kinds = tails(M, N)
        out = ops.gemm(a.to(d), w.to(d), False, BF16, gelu_aux=aux.to(d))
        ref = (a.double() @ w.double().t()) * S.gelu_grad_exact(aux.double())
        kinds_figs(figs, "out", out, ref, kinds, 1, BF16, [f"gain {v:g}" for v in S.MLP_GAINS])
    assert out.dtype == BF16
    judge(f"gemm {mode} {(M, N, K)}", figs)


def test_mlp_fp8_gelu_tails():
    """The fp8 fused Mlp (csu_mlp_fp8_fwd / _bwd) at (C, M) = (128, 100) with the tail-reaching fc1
    against the fp64 restatement of its roundings (oracle/fp8_ref.py), bf16 bound.  g is itself
    e4m3-valued (3 mantissa bits): the device's fast GELU can move a value across a rounding tie, one
    e4m3 step, up to 2^-3 of the value, which no max-abs bound of 3e-2 max|ref| can hold -- so g is judged
    by the rel-L2 half of the bound alone; the share of differing codes is printed, not asserted."""
    from csu import ops
    from csu._lib import check, lib, ptr, stream_ptr
    from oracle import fp8_ref as Q
    d = dev()
    C, M = 128, 100
    inp = S.mlp_inputs(C, M)
    x, b1, b2, res = (inp[k].to(d) for k in ("x", "b1", "b2", "res"))
    w1, w2 = inp["w1"].float().to(d), inp["w2"].float().to(d)
    dz = (inp["dy"].float() * 1e-3).bfloat16().to(d)
    fp8 = ops.Fp8Weights([w1, w2], mlp_pairs=[(w1, w2)])
    fp8.quantize()
    w1q, sw1, w2p, sw2, w2t, w1tp = fp8.mlp_operands(w1, w2)
    md = ops.MlpDrop(None, 0, 0, 0.0).c_struct()
    md.rows_per_sample = M
    st = stream_ptr(d)
    y = torch.empty(M, C, device=d)
    check(lib().csu_mlp_fp8_fwd(M, C, ptr(x), ptr(w1q), ptr(sw1), ptr(b1), ptr(w2p), ptr(sw2), ptr(b2), ptr(res), ptr(y),
                                ctypes.byref(md), st), "mlp_fp8_fwd")
    dh = torch.empty(M, 4 * C, device=d, dtype=BF16)
    gq = torch.empty_like(dh)
    dx = torch.empty(M, C, device=d, dtype=BF16)
    check(lib().csu_mlp_fp8_bwd(M, C, ptr(x), ptr(dz), ptr(w1q), ptr(sw1), ptr(b1), ptr(w2t), ptr(sw2), ptr(w1tp),
                                ptr(dh), ptr(gq), ptr(dx), ctypes.byref(md), st), "mlp_fp8_bwd")
    torch.cuda.synchronize()
    W1d, _, S1 = Q.quant_rows(w1.cpu())
    W2d, _, S2 = Q.quant_rows(w2.cpu())
    X, B1, B2, R, DZ = (t.double().cpu() for t in (x, b1, b2, res, dz))
    z = Q.fp8_mlp(X, W1d, B1, W2d, B2, S1, S2, None)
    h = Q.mx_quant(X) @ W1d.T + B1
    assert float(h.abs().max()) > 12.0
    gqr = Q.mx_quant(S.gelu_exact(h))
    q1, q2 = W1d / S1[:, None], W2d / S2[:, None]
    dhr = (Q.mx_quant(DZ * S2) @ q2) * S.gelu_grad_exact(h)
    dxr = Q.mx_quant(dhr * S1) @ q1
    figs = {"y - res": S.usage(y.cpu().double() - R, z, BF16), "dx": S.usage(dx, dxr, BF16)}
    kinds_figs(figs, "dh", dh, dhr, inp["kinds"], 1, BF16, [f"gain {v:g}" for v in S.MLP_GAINS])
    figs["g rel-L2"] = float((gq.double().cpu() - gqr).norm() / gqr.norm()) / 2e-2
    print(f"numeric_stress mlp_fp8 C=128 M=100 g: {float((gq.double().cpu() != gqr).double().mean()):.2e} of the codes differ")
    judge("mlp_fp8 C=128 M=100", figs)


# ---------------------------------------------------------------------------------------------
# 6. e4m3 quantisers on the power-of-two boundaries
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [64, 200])
def test_e4m3_quantisers_on_scale_boundaries(cols):
    """csu_quant_e4m3_batch and csu_quant_e4m3_shadow_batch: rows whose amax is 0, exactly 448 * 2^k
    (k = -20 .. 10), one fp32 ulp either side, 1e-30, 1e30, or a single non-zero element.  Scale: the
    smallest power of two s with amax / s <= 448, computed exactly; codes: torch.float8_e4m3fn of w / s,
    bit for bit."""
    from csu import ops
    d = dev()
    w, am = S.e4m3_rows(cols)
    rs, rq, rd = S.e4m3_expected(w, am)
    p = w.to(d)
    fp8 = ops.Fp8Weights([p])
    deq = fp8.quantize()
    torch.cuda.synchronize()

    def mismatches(tag, sc, q, dq):
        ws = (sc.cpu() != rs).nonzero().flatten().tolist()
        wq = (q.cpu() != rq).any(1).nonzero().flatten().tolist()
        print(f"numeric_stress e4m3 {tag} cols={cols}: {len(ws)} of {len(am)} scales, {len(wq)} rows of codes differ")
        assert not ws, [(am[i], float(sc[i]), float(rs[i])) for i in ws[:8]]
        assert not wq, [am[i] for i in wq[:8]]
        assert torch.equal(dq.float().cpu(), rd)

    mismatches("quant_e4m3_batch", fp8.scales[0], fp8.q[0], deq[0])
    if cols % 16:
        # the shadow quantiser takes whole 16-column runs only: it must refuse, and runs on the next multiple
        bad = ops.Fp8Weights([p])
        cache = ops.CastCache()
        cache.refresh([p], BF16, (), sources=bad.sources())
        with pytest.raises(ValueError):
            bad.quantize(cache)
        cols = -(-cols // 16) * 16
        w, am = S.e4m3_rows(cols)
        rs, rq, rd = S.e4m3_expected(w, am)
        p = w.to(d)
    fp8b = ops.Fp8Weights([p])
    cache = ops.CastCache()
    cache.refresh([p], BF16, (), sources=fp8b.sources())
    fp8b.quantize(cache)
    torch.cuda.synchronize()
    mismatches("quant_e4m3_shadow_batch", fp8b.scales[0], fp8b.q[0], cache.shadow[0])
    assert torch.equal(cache.shadow_t[0].float().cpu(), rd.t())


# ---------------------------------------------------------------------------------------------
# 7. FusedAdamW
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 5])
@pytest.mark.parametrize("capturable", [False, True])
def test_fused_adamw_gradients_over_thirty_decades(capturable, steps):
    """csu_adamw_step against torch.optim.AdamW in fp32 on the same device, gradients spanning
    {0, 1e-15, 1e-4, 1, 1e4, 1e15} per element group; test_fused_adamw_matches_torch's tolerance."""
    from csu.optim import FusedAdamW
    d = dev()
    g = torch.Generator().manual_seed(0)
    ps = [torch.randn(s, generator=g).to(d) for s in S.ADAMW_SHAPES]
    ref = [p.clone().requires_grad_(True) for p in ps]
    mine = [p.clone().requires_grad_(True) for p in ps]
    o_ref = torch.optim.AdamW(ref, lr=1e-3, weight_decay=1e-2, foreach=False)
    o_mine = FusedAdamW(mine, lr=1e-3, weight_decay=1e-2, capturable=capturable)
    for it in range(steps):
        for p, q, s in zip(ref, mine, S.ADAMW_SHAPES):
            gr = S.adamw_grad(s, it).to(d)
            p.grad, q.grad = gr.clone(), gr.clone()
        o_ref.step()
        o_mine.step()
    torch.cuda.synchronize()
    figs = {}
    for i, (p, q) in enumerate(zip(ref, mine)):
        figs[f"param{i}"] = S.tol_usage(q, p, 1e-5, 1e-6)
        figs[f"exp_avg{i}"] = S.tol_usage(o_mine.state[q]["exp_avg"], o_ref.state[p]["exp_avg"], 1e-5, 1e-7)
        figs[f"exp_avg_sq{i}"] = S.tol_usage(o_mine.state[q]["exp_avg_sq"], o_ref.state[p]["exp_avg_sq"], 5e-5, 1e-9)
        assert torch.isfinite(q).all() and torch.isfinite(o_mine.state[q]["exp_avg_sq"]).all()
    judge(f"adamw capturable={capturable} steps={steps}", figs)
