"""Preconditions of the numeric stress tests (test_gpu_numeric_stress.py), checked on the CPU.

For every generator of stress_inputs.py at the shapes the GPU tests use, the operation evaluated in
torch fp32 eager meets the fp32 criterion against the fp64 reference per kind, using at most half of
it; for attention the bf16 emulation under the mild gains meets the bf16 bound using at most 0.6 of
it (and under the sharp gains its forward does).  This keeps the GPU tests honest: a failure there is the kernel's, not the input's."""
import math

import pytest
import torch

import stress_inputs as S

F32, F64 = torch.float32, torch.float64
HALF = 0.5


def _check(figs, limit=HALF):
    for k, v in figs.items():
        print(f"  {k}: {v:.3f} of the bound")
    bad = {k: v for k, v in figs.items() if not v <= limit}
    assert not bad, bad


@pytest.mark.parametrize("dtype", [F32, torch.bfloat16])
def test_usage_restates_assert_close(dtype):
    """usage(a, ref) <= 1 exactly when the copied assert_close passes."""
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(64, 33, generator=g).double() * 7
    noise = torch.randn(64, 33, generator=g).double()
    seen = set()
    for amp in (1e-7, 3e-5, 7e-5, 2e-4, 1e-3, 1e-2, 3e-2, 1e-1, 1.0):
        a = ref + amp * noise * (ref.abs() if dtype == F32 else 1.0)
        try:
            S.assert_close(a, ref, dtype)
            ok = True
        except AssertionError:
            ok = False
        assert ok == (S.usage(a, ref, dtype) <= 1.0), amp
        seen.add(ok)
    assert seen == {True, False}


# ---- the restated references equal the oracle's functions in fp64 ------------------------------------
@pytest.mark.parametrize("case", S.STRESS_ATTN_CASES[:4], ids=str)
def test_attention_restatement_equals_the_oracle(case):
    from oracle import cswin_ref as O
    reso, idx, sw, cb, heads, B = case
    inp, _ = S.attn_reference(case, S.GAINS_SHARP, F32)
    q = inp["qkv"].double()
    assert (inp["hs"], inp["ws"]) == O.stripe_geometry(reso, idx, sw)
    assert torch.equal(S.window_tokens(reso, inp["hs"], inp["ws"]),
                       O.stripe_partition(torch.arange(reso * reso).view(1, -1, 1), reso, inp["hs"], inp["ws"])[..., 0])

    def mask(shape):
        return (torch.rand(shape, generator=torch.Generator().manual_seed(5)) > 0.3).double() / 0.7

    for m in (None, mask):
        args = (q[..., :cb], q[..., cb:2 * cb], q[..., 2 * cb:], reso, inp["hs"], inp["ws"], heads, inp["w"].double(),
                inp["b"].double(), inp["scale"])
        assert torch.equal(S.lepe_attention_plain(*args, attn_mask=m), O.lepe_attention(*args, attn_mask=m))


def test_simam_and_carafe_restatements_equal_the_oracle():
    from oracle import cswin_ref as O
    x, _ = S.channel_kinds((3, 17, 200), True)
    assert torch.equal(S.simam_ref(x.double()), O.simam(x.double()))
    # O.carafe with identity `down` / `out` convs: its encoder's logits fed to the restated reassembly
    B, H, C, s = 2, 5, 8, 2
    g = torch.Generator().manual_seed(6)
    xt = torch.randn(B, H * H, C, generator=g).double()
    eye = torch.eye(C, dtype=F64).view(C, C, 1, 1)
    p = {".down.weight": eye, ".down.bias": torch.zeros(C, dtype=F64),
         ".encoder.weight": torch.randn(9 * s * s, C, 3, 3, generator=g).double() * 3, ".encoder.bias": torch.randn(9 * s * s, generator=g).double(),
         ".out.weight": eye, ".out.bias": torch.zeros(C, dtype=F64)}
    enc = torch.nn.functional.conv2d(xt.transpose(1, 2).reshape(B, C, H, H), p[".encoder.weight"], p[".encoder.bias"], padding=1)
    assert torch.equal(S.carafe_reassemble_ref(xt, enc.permute(0, 2, 3, 1), H, s), O.carafe(xt, p, "", s))


# ---- attention ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("gains", [S.GAINS_SHARP, S.GAINS_MILD], ids=["sharp", "mild"])
@pytest.mark.parametrize("case", S.STRESS_ATTN_CASES, ids=str)
def test_attention_fp32_eager_within_half_the_bound(case, gains):
    inp, ref = S.attn_reference(case, gains, F32)
    assert float(inp["gain"].max()) == max(gains) and float(inp["gain"].min()) == 0.0
    _check(S.attn_usages(S.attn_eval(inp, case, F32), ref, inp, F32))


@pytest.mark.parametrize("case", S.STRESS_ATTN_CASES, ids=str)
def test_attention_logits_need_the_shift(case):
    """The sharp regime really overflows an unshifted exp (|logit| > 88.7), the degenerate rows are
    exactly uniform, and two keys tie."""
    reso, idx, sw, cb, heads, B = case
    inp, _ = S.attn_reference(case, S.GAINS_SHARP, F32)
    q, k = inp["qkv"][..., :cb].double(), inp["qkv"][..., cb:2 * cb].double()
    wt = S.window_tokens(reso, inp["hs"], inp["ws"])
    hd = cb // heads
    top = 0.0
    for h in range(heads):
        qs, ks = q[:, wt][..., h * hd:(h + 1) * hd], k[:, wt][..., h * hd:(h + 1) * hd]
        s = qs @ ks.transpose(-1, -2) * inp["scale"]
        top = max(top, float(s.abs().max()))
        assert torch.equal(s[..., 0], s[..., 1])
    assert top > 100.0, top
    assert int((inp["gain"] == 0).sum()) >= B


@pytest.mark.parametrize("case", S.STRESS_ATTN_CASES, ids=str)
def test_attention_bf16_emulation_within_0p6_of_the_bound_mild(case):
    inp, ref = S.attn_reference(case, S.GAINS_MILD, torch.bfloat16)
    emu = S.attn_eval(inp, case, F32, emulate_bf16=True)
    _check(S.attn_usages(emu, ref, inp, torch.bfloat16), 0.6)


@pytest.mark.parametrize("case", S.STRESS_ATTN_CASES, ids=str)
def test_attention_bf16_emulation_forward_sharp(case):
    """Under the sharp gains the forward of the emulation stays within 0.6 of the bf16 bound."""
    inp, ref = S.attn_reference(case, S.GAINS_SHARP, torch.bfloat16)
    emu = S.attn_eval(inp, case, F32, emulate_bf16=True)
    figs = S.attn_usages(emu, ref, inp, torch.bfloat16)
    _check({k: v for k, v in figs.items() if k.startswith("out")}, 0.6)


def test_two_branch_bf16_emulation_preconditions():
    """The two-branch emulation: within 0.6 of the bf16 bound under the mild gains, its forward under the sharp."""
    for gains in (S.GAINS_MILD, S.GAINS_SHARP):
        inp = S.two_branch_inputs(gains, torch.bfloat16)
        ref, emu = S.two_branch_eval(inp, F64), S.two_branch_eval(inp, F32, emulate_bf16=True)
        figs = S.attn_usages(S.two_branch_pack(emu, 0), S.two_branch_pack(ref, 0), inp, torch.bfloat16)
        figs["dW_lepe1"] = S.usage(emu[2][1], ref[2][1], torch.bfloat16)
        figs["db_lepe1"] = S.usage(emu[3][1], ref[3][1], torch.bfloat16)
        if gains == S.GAINS_SHARP:
            figs = {k: v for k, v in figs.items() if k.startswith("out")}
        _check(figs, 0.6)


@pytest.mark.parametrize("gains", [S.GAINS_SHARP, S.GAINS_MILD], ids=["sharp", "mild"])
def test_two_branch_fp32_eager_within_half_the_bound(gains):
    inp = S.two_branch_inputs(gains, F32)
    ref, got = S.two_branch_eval(inp, F64), S.two_branch_eval(inp, F32)
    C = S.TWO_BRANCH["C"]
    figs = S.attn_usages((got[0], got[1], got[2][0], got[3][0]), (ref[0], ref[1], ref[2][0], ref[3][0]), inp, F32)
    figs["dW_lepe1"], figs["db_lepe1"] = S.usage(got[2][1], ref[2][1], F32), S.usage(got[3][1], ref[3][1], F32)
    assert got[1].shape[-1] == 3 * C
    _check(figs)


# ---- LayerNorm ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [70, 128])
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_layernorm_rows_fp32_eager_within_half_the_bound(C, rows):
    x, kinds = S.ln_rows(rows, C)
    assert set(kinds[:7].tolist()) == set(range(7)) and len(S.LN_KINDS) == 7
    assert float(x[kinds == 3].var(1, unbiased=False).max()) == 0.0
    assert float(x[kinds == 2].double().var(1).max()) < 1e-5 / 5 and abs(float(x[kinds == 2].mean()) - 0.1) < 1e-3
    w, b = S.ln_params(C)
    dy = torch.randn(rows, C, generator=torch.Generator().manual_seed(C))
    ref, got = S.ln_eval(x, w, b, dy, F64), S.ln_eval(x, w, b, dy, F32)
    figs = {}
    for name, i in (("y", 0), ("dx", 1)):
        for k, v in S.by_kind(got[i], ref[i], kinds, 0, F32).items():
            figs[f"{name}[{S.LN_KINDS[k]}]"] = v
    figs["dgamma"], figs["dbeta"] = S.usage(got[2], ref[2], F32), S.usage(got[3], ref[3], F32)
    _check(figs)


# ---- SimAM / BatchNorm -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 64, 32), (3, 17, 200), (2, 1000, 256)])
def test_simam_channels_fp32_eager_within_half_the_bound(shape):
    x, kinds = S.channel_kinds(shape, True)
    assert float(x[..., kinds == 2].var(1, unbiased=False).max()) == 0.0
    dy = torch.randn(shape, generator=torch.Generator().manual_seed(1))
    ref, got = S.simam_eval(x, dy, F64), S.simam_eval(x, dy, F32)
    figs = {}
    for name, i in (("y", 0), ("dx", 1)):
        for k, v in S.by_kind(got[i], ref[i], kinds, 2, F32).items():
            figs[f"{name}[{S.CH_KINDS[k]}]"] = v
    _check(figs)


@pytest.mark.parametrize("shape", [(2, 5, 7, 64), (4, 9, 11, 72)])
def test_batchnorm_channels_fp32_eager_within_half_the_bound(shape):
    x, kinds = S.channel_kinds(shape, False)
    assert float(x[..., kinds == 2].reshape(-1, int((kinds == 2).sum())).var(0, unbiased=False).max()) == 0.0
    dy = torch.randn(shape, generator=torch.Generator().manual_seed(2))
    w, b, rm, rv = S.bn_params(shape[-1])
    ref, got = S.bn_eval(x, w, b, rm, rv, dy, F64), S.bn_eval(x, w, b, rm, rv, dy, F32)
    figs = {}
    for i, name in enumerate(S.BN_OUT):
        for k, v in S.by_kind(got[i], ref[i], kinds, got[i].dim() - 1, F32).items():
            figs[f"{name}[{S.CH_KINDS[k]}]"] = v
    _check(figs)


# ---- CARAFE / heads ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,C,s", S.CARAFE_SHAPES)
def test_carafe_logits_fp32_eager_within_half_the_bound(B, H, C, s):
    enc, kinds = S.carafe_logits(B, H, s)
    assert float(enc.abs().max()) > 9e3 and set(kinds.tolist()) >= {0, 1, 2}
    g = torch.Generator().manual_seed(3)
    x, gy = torch.randn(B, H * H, C, generator=g), torch.randn(B, H * H * s * s, C, generator=g)
    ref, got = S.carafe_eval(x, enc, gy, H, s, F64), S.carafe_eval(x, enc, gy, H, s, F32)
    figs = {}
    for k, v in S.by_kind(got[0].reshape(-1, C), ref[0].reshape(-1, C), S.carafe_out_kinds(kinds, B, H, s), 0, F32).items():
        figs[f"out[{k}]"] = v
    for k, v in S.by_kind(got[1].reshape(-1, C), ref[1].reshape(-1, C), kinds, 0, F32).items():
        figs[f"dx[{k}]"] = v
    for k, v in S.by_kind(got[2].reshape(B * H * H, -1), ref[2].reshape(B * H * H, -1), kinds, 0, F32).items():
        figs[f"denc[{k}]"] = v
    _check(figs)


def test_sigmoid_head_fp32_eager_within_half_the_bound():
    P, C = 515, 64
    x, w, t = S.head_inputs(P, C)
    ref, got = S.head_eval(x, w, t, F64), S.head_eval(x, w, t, F32)
    z = x.double() @ w.double().view(C)
    kinds = S.head_kinds(z)
    assert set(kinds.tolist()) == {0, 1, 2} and float(z.abs().max()) > 99.0
    assert int(((got[0] == 0) | (got[0] == 1)).sum()) > 10          # exactly 0 or 1 in fp32
    figs = {"loss": S.usage(got[1], ref[1], F32), "dw": S.usage(got[3], ref[3], F32)}
    for k, v in S.by_kind(got[0], ref[0], kinds, 0, F32).items():
        figs[f"prob[{k}]"] = v
    for k, v in S.by_kind(got[2], ref[2], kinds, 0, F32).items():
        figs[f"dx[{k}]"] = v
    _check(figs)


@pytest.mark.parametrize("B,H,C,s", [(2, 5, 64, 2), (1, 5, 32, 4)])
def test_carafe_head_fp32_eager_within_half_the_bound(B, H, C, s):
    x, enc, w_out, b_out, w_h, t, kinds = S.carafe_head_inputs(B, H, C, s)
    ref = S.carafe_head_eval(x, enc, w_out, b_out, w_h, t, H, s, F64)
    got = S.carafe_head_eval(x, enc, w_out, b_out, w_h, t, H, s, F32)
    assert int(((got[0] == 0) | (got[0] == 1)).sum()) > 0
    _check(S.carafe_head_usages(S.CARAFE_HEAD_OUT, got, ref, kinds, B, H, s, F32))


# ---- Mlp ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,M", [(64, 37), (128, 100), (256, 100)])
def test_mlp_gelu_tails_fp32_eager_within_half_the_bound(C, M):
    inp = S.mlp_inputs(C, M)
    ref, got = S.mlp_eval(inp, F64), S.mlp_eval(inp, F32)
    h = inp["x"].double() @ inp["w1"].double().t() + inp["b1"].double()
    assert float(h.abs().max()) > 12.0
    assert (h < -12).any() and (h > 12).any()
    assert (S.gelu_exact(h[h < -12]) == 0).all() and torch.equal(S.gelu_exact(h[h > 12]), h[h > 12])   # 1 - Phi underflows
    figs = {k: S.usage(got[k], ref[k], F32) for k in ("y", "dx", "dW2", "db2")}
    for name, dim in (("g", 1), ("dh", 1), ("dW1", 0), ("db1", 0)):
        for k, v in S.by_kind(got[name], ref[name], inp["kinds"], dim, F32).items():
            figs[f"{name}[gain {S.MLP_GAINS[k]:g}]"] = v
    _check(figs)


# ---- e4m3 rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [64, 200, 208])
def test_e4m3_rows_sit_on_the_power_of_two_boundaries(cols):
    w, am = S.e4m3_rows(cols)
    s, q, deq = S.e4m3_expected(w, am)
    assert len(am) == 1 + 3 * 31 + 2 + 3
    for a, sc in zip(am, s.tolist()):
        if a == 0:
            assert sc == 1.0
            continue
        assert math.frexp(sc)[0] == 0.5                     # a power of two
        assert a / sc <= 448.0 < a / (sc / 2)                # the smallest one (exact: power-of-two division)
    # the rule restated with fp64 logarithms agrees on every row
    a64 = torch.tensor(am, dtype=F64)
    s64 = torch.where(a64 > 0, torch.exp2(torch.ceil(torch.log2(a64 / 448.0))), torch.ones_like(a64))
    assert torch.equal(s64.float(), s)
    # boundary rows: exactly 448 * 2^k keeps scale 2^k (code 0x7e = 448), one ulp above doubles it
    for k in range(-20, 11):
        i = 1 + 3 * (k + 20)
        assert s[i - 0].item() == 2.0 ** k and s[i + 1].item() == 2.0 ** k and s[i + 2].item() == 2.0 ** (k + 1)
        assert int((q[i + 1] & 0x7F).max()) == 0x7E
    assert not bool(((q & 0x7F) == 0x7F).any())              # no NaN code
    assert torch.isfinite(deq).all()


# ---- AdamW -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 5])
def test_adamw_gradients_fp32_eager_within_half_the_tolerance(steps):
    """torch.optim.AdamW in fp32 against fp64 on the stress gradients: half of
    test_fused_adamw_matches_torch's tolerance."""
    res = {}
    for dt in (F32, F64):
        g = torch.Generator().manual_seed(0)
        ps = [torch.randn(s, generator=g).to(dt).requires_grad_(True) for s in S.ADAMW_SHAPES]
        opt = torch.optim.AdamW(ps, lr=1e-3, weight_decay=1e-2, foreach=False)
        for it in range(steps):
            for p, s in zip(ps, S.ADAMW_SHAPES):
                p.grad = S.adamw_grad(s, it).to(dt)
            opt.step()
        res[dt] = (ps, [opt.state[p]["exp_avg"] for p in ps], [opt.state[p]["exp_avg_sq"] for p in ps])
    figs = {}
    for i in range(len(S.ADAMW_SHAPES)):
        figs[f"param{i}"] = S.tol_usage(res[F32][0][i], res[F64][0][i], 1e-5, 1e-6)
        figs[f"exp_avg{i}"] = S.tol_usage(res[F32][1][i], res[F64][1][i], 1e-5, 1e-7)
        figs[f"exp_avg_sq{i}"] = S.tol_usage(res[F32][2][i], res[F64][2][i], 5e-5, 1e-9)
    assert all(torch.isfinite(t).all() for t in res[F32][2])
    _check(figs)
