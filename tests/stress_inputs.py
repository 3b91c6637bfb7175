"""Input generators and criteria for the numeric stress parity tests (test_gpu_numeric_stress.py,
test_numeric_stress_inputs.py).  Plain torch on the CPU; nothing here needs a GPU.

Every generator mixes several numeric regimes ("kinds") inside one tensor, laid out so that every
tile, panel and wave of a kernel holds all kinds, and returns the kind of each row / channel / token so
the criteria can be applied per kind: a x1e3 row must not loosen the absolute tolerance of the row
beside it, and a fault confined to one kind must not be diluted in an L2 norm over all of them.

All inputs are finite.  The criteria are those of tests/test_gpu_kernels.py::assert_close, expressed as
the used fraction of the bound (<= 1 passes):
  fp32: |a - ref| <= 1e-5 * max(1, max|ref|) + 1e-4 |ref| elementwise;
  bf16: rel-L2 < 2e-2 and max-abs < 3e-2 * max|ref|.

Kinds made milder than first planned, because the fp32 eager evaluation (or, for bf16 attention, the
emulation) did not meet the precondition of test_numeric_stress_inputs.py -- half of the fp32 criterion,
0.6 of the bf16 bound -- on the CPU.  Figures: used fraction of the bound before -> after.
  * attention, sharp gains {1, 8, 32} for {1, 8, 40}: out[gain 40] of the 128-token stripes 0.51 -> 0.34
    (one ulp of a logit near 240 is 1.5e-5 of P).
  * attention, mild gains {1, 4, 8} for {1, 4, 16}: the emulation, which like the kernels takes the
    backward's delta = rowsum(dO * (O - LePE)) from the bf16 output, used 0.77 on dq[gain 16] and 0.63 on dk;
    {1, 4, 8}: 0.46.  Logits beyond exp's range stay covered in bf16 by the sharp gains.
  * LayerNorm rows of variance 1e-6: mean 0.1 for 0.5.  The rounding of the mean (3e-8 at 0.5) times
    rstd = eps^-1/2 = 316 is the whole absolute tolerance: y 1.1 .. 1.8 -> 0.29.
  * LayerNorm constant rows: a bf16-exact constant of magnitude ~2^-4 for ~2.  torch's eager row mean of
    512 equal values is an ulp off, times 316: dgamma 0.89 -> 0.16.
  * SimAM / BatchNorm channels: mean 50 for 100 (SimAM dx 0.79 -> 0.45), std 1e-3 about 0.1 for 0.5 (SimAM
    dx 1.8, BatchNorm y 1.1 and dgamma 1.1 -> at most 0.29), constants of magnitude ~2^-5 (BatchNorm y 1.6 -> 0.01:
    the eager batch mean of 70 or 396 equal values is an ulp off).
  * sigmoid heads: a pixel with |z| >= 6 carries the target the sign of z predicts.  An fp32 probability
    that is exactly 0 or 1 with the opposite target costs the clamp's 100, not |z|.
  * AdamW: each element's gradient keeps its sign over the steps.  exp_avg of opposite-sign 1e15 terms
    cancels to 40 x the relative tolerance in eager fp32.
  * the shadow quantiser takes 208 columns for 200: it needs a multiple of 16 and must refuse 200."""
import functools
import math

import torch
import torch.nn.functional as F

# ---------------------------------------------------------------------------------------------
# criteria
# ---------------------------------------------------------------------------------------------


def assert_close(a, b, dtype):
    """tests/test_gpu_kernels.py::assert_close, copied: the criterion the usage functions restate."""
    a, b = a.double().cpu(), b.double().cpu()
    scale = float(b.abs().max().clamp_min(1e-30))
    if dtype == torch.float32:
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5 * max(1.0, scale))
    else:
        rel = float((a - b).norm() / b.norm().clamp_min(1e-30))
        assert rel < 2e-2, rel
        assert float((a - b).abs().max()) < 3e-2 * scale


def tol_usage(a, ref, rtol, atol):
    """max over elements of |a - ref| / (atol + rtol |ref|): torch.testing.assert_close's criterion."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    if ref.numel() == 0:
        return 0.0
    return float(((a - ref).abs() / (atol + rtol * ref.abs())).max())


def fp32_usage(a, ref):
    """max over elements of |a - ref| / (1e-5 max(1, max|ref|) + 1e-4 |ref|): the fp32 criterion."""
    if ref.numel() == 0:
        return 0.0
    scale = float(ref.detach().double().abs().max().clamp_min(1e-30))
    return tol_usage(a, ref, 1e-4, 1e-5 * max(1.0, scale))


def bf16_usage(a, ref):
    """max(rel-L2 / 2e-2, max-abs / (3e-2 max|ref|)): the bf16 criterion."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    if ref.numel() == 0:
        return 0.0
    scale = float(ref.abs().max().clamp_min(1e-30))
    l2 = float((a - ref).norm() / ref.norm().clamp_min(1e-30))
    return max(l2 / 2e-2, float((a - ref).abs().max()) / (3e-2 * scale))


def usage(a, ref, dtype):
    return fp32_usage(a, ref) if dtype == torch.float32 else bf16_usage(a, ref)


def by_kind(a, ref, kinds, dim, dtype):
    """{kind: used fraction of the `dtype` criterion} over the slices of `dim` whose kind is that kind.
    `kinds` is a 1-D integer tensor of length a.shape[dim]."""
    out = {}
    for k in sorted(set(kinds.tolist())):
        idx = (kinds == k).nonzero().flatten()
        out[int(k)] = usage(a.detach().cpu().index_select(dim, idx), ref.detach().cpu().index_select(dim, idx), dtype)
    return out


# ---------------------------------------------------------------------------------------------
# 1. stripe attention
# ---------------------------------------------------------------------------------------------
STRESS_ATTN_CASES = [
    (16, 0, 2, 64, 2, 2),     # N = 32
    (16, 1, 1, 32, 1, 2),     # width-1 stripes
    (7, -1, 7, 64, 2, 2),     # N = 49, masked tail
    (14, 0, 7, 64, 2, 1),     # N = 98, ragged
    (128, 0, 1, 32, 1, 1),    # the headline's 128-token stripes
    (20, -1, 20, 32, 1, 2),   # 400, ragged, LDS-resident
    (32, -1, 32, 32, 1, 1),   # 1024
    (42, -1, 42, 64, 2, 1),   # 1764, streamed
]
GAINS_SHARP = (1.0, 8.0, 32.0)     # |logit| up to ~190: exp overflows at 88.7 without the shift
GAINS_MILD = (1.0, 4.0, 8.0)       # bf16 gradients held to the unchanged bf16 bound
TWO_BRANCH = dict(reso=32, C=128, heads=4, sw=2, B=2)   # test_two_branch_fused_launch's launch


def stripe_geometry(reso, idx, split):
    return (reso, reso) if idx == -1 else ((reso, split) if idx == 0 else (split, reso))


def window_tokens(reso, hs, ws):
    """(nWin, N) token indices of each stripe window (the oracle's stripe_partition order)."""
    t = torch.arange(reso * reso).view(reso // hs, hs, reso // ws, ws)
    return t.permute(0, 2, 1, 3).reshape(-1, hs * ws)


def attn_token_gains(B, reso, windows, gains, g):
    """Per-token q gain (B, L): drawn from `gains`; 0 (the degenerate kind: uniform softmax, exactly
    1 / N) for a quarter of the tokens of one window per (batch item, window layout)."""
    L = reso * reso
    gain = torch.tensor(gains)[torch.randint(0, len(gains), (B, L), generator=g)]
    for hs, ws in windows:
        idx = window_tokens(reso, hs, ws)
        N = idx.shape[1]
        for b in range(B):
            w = (1 + 3 * b) % idx.shape[0]
            gain[b, idx[w, : max(1, N // 4)]] = 0.0
    return gain


def attn_inputs(case, gains, dtype, seed=0):
    """Inputs of one single-branch ATTN_CASES entry: q scaled per token by a gain from `gains`
    (sharp rows: |logit| up to ~6 gain), q = 0 on a quarter of one window per batch item (degenerate),
    and the k of the first two tokens of every window identical (duplicate maximum).
    Returns dict(qkv, w, b, gout, gain): gain (B, L) is the token kind."""
    reso, idx, sw, cb, heads, B = case
    g = torch.Generator().manual_seed(1000 + seed + sum(abs(c) for c in case))
    L = reso * reso
    hs, ws = stripe_geometry(reso, idx, sw)
    qkv = torch.randn(B, L, 3 * cb, generator=g)
    gain = attn_token_gains(B, reso, [(hs, ws)], gains, g)
    qkv[..., :cb] *= gain[..., None]
    wt = window_tokens(reso, hs, ws)
    qkv[:, wt[:, 1], cb:2 * cb] = qkv[:, wt[:, 0], cb:2 * cb]
    dup = torch.zeros(B, L, dtype=torch.bool)
    dup[:, wt[:, :2].flatten()] = True
    w = torch.randn(cb, 1, 3, 3, generator=g) * 0.3
    b = torch.randn(cb, generator=g) * 0.1
    gout = torch.randn(B, L, cb, generator=g)
    return dict(qkv=qkv.to(dtype), w=w, b=b, gout=gout.to(dtype), gain=gain, dup=dup, hs=hs, ws=ws,
                scale=(cb // heads) ** -0.5)


def two_branch_inputs(gains, dtype, seed=0):
    """The two-branch launch of test_two_branch_fused_launch under the same regimes (both window
    layouts get their degenerate quarter window and their duplicate keys)."""
    reso, C, heads, sw, B = (TWO_BRANCH[k] for k in ("reso", "C", "heads", "sw", "B"))
    g = torch.Generator().manual_seed(77 + seed)
    L = reso * reso
    qkv = torch.randn(B, L, 3 * C, generator=g)
    wins = [stripe_geometry(reso, i, sw) for i in range(2)]
    gain = attn_token_gains(B, reso, wins, gains, g)
    qkv[..., :C] *= gain[..., None]
    dup = torch.zeros(B, L, dtype=torch.bool)
    for i, (hs, ws) in enumerate(wins):
        wt = window_tokens(reso, hs, ws)
        sl = slice(C + i * C // 2, C + (i + 1) * C // 2)
        qkv[:, wt[:, 1], sl] = qkv[:, wt[:, 0], sl]
        dup[:, wt[:, :2].flatten()] = True
    ws_ = [torch.randn(C // 2, 1, 3, 3, generator=g) * 0.3 for _ in range(2)]
    bs_ = [torch.randn(C // 2, generator=g) * 0.1 for _ in range(2)]
    gout = torch.randn(B, L, C, generator=g)
    return dict(qkv=qkv.to(dtype), ws=ws_, bs=bs_, gout=gout.to(dtype), gain=gain, dup=dup, wins=wins,
                scale=(C // heads) ** -0.5)


class _RoundFwd(torch.autograd.Function):
    """bf16 rounding of a value; the gradient passes unchanged."""

    @staticmethod
    def forward(ctx, t):
        return t.bfloat16().to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


class _SoftmaxDelta(torch.autograd.Function):
    """softmax over the keys whose backward is the attention kernels': dS = P (dP - delta) with
    delta = rowsum(dO * O_attn) taken from the stored (bf16) output, dS rounded to bf16."""

    @staticmethod
    def forward(ctx, s, holder):
        p = torch.softmax(s, dim=-1)
        ctx.save_for_backward(p)
        ctx.holder = holder
        return p

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        ds = p * (g - ctx.holder["delta"][..., None])
        return ds.bfloat16().to(g.dtype), None


def lepe_attention_plain(q, k, v, reso, hs, ws, heads, w, b, scale, emulate_bf16=False, attn_mask=None, gout=None):
    """softmax(q scale k^T) v + dwconv3x3(v) per stripe window in q's dtype, restated in plain torch.
    emulate_bf16 (with the output gradient `gout`): the arithmetic of a kernel that keeps scores, softmax
    statistics and accumulators in fp32 and rounds to bf16 only P (the MFMA operand), O and dS; the
    backward's row constant delta = rowsum(dO * (O - LePE)) comes from the rounded O, as in the kernels
    (csrc/stripe_attn.hip).  The input gradients are rounded by the caller."""
    B, L, Cb = q.shape
    hd, N = Cb // heads, hs * ws

    def part(t):
        return t.reshape(B, reso // hs, hs, reso // ws, ws, Cb).permute(0, 1, 3, 2, 4, 5).reshape(-1, N, Cb)

    def hf(t):
        return t.reshape(t.shape[0], N, heads, hd).permute(0, 2, 1, 3)

    qw, kw, vwin = hf(part(q)), hf(part(k)), part(v)
    lepe = F.conv2d(vwin.transpose(1, 2).reshape(-1, Cb, hs, ws), w, b, stride=1, padding=1, groups=Cb)
    lepe = lepe.reshape(-1, heads, hd, N).permute(0, 1, 3, 2)
    s = torch.matmul(qw * scale, kw.transpose(-2, -1))
    holder = {}
    p = _SoftmaxDelta.apply(s, holder) if emulate_bf16 else torch.softmax(s, dim=-1)
    if attn_mask is not None:
        p = p * attn_mask(p.shape).to(p.dtype)
    if emulate_bf16:
        p = _RoundFwd.apply(p)
    o = torch.matmul(p, hf(vwin)) + lepe
    o = o.transpose(1, 2).reshape(-1, N, Cb)
    o = o.reshape(B, reso // hs, reso // ws, hs, ws, Cb).permute(0, 1, 3, 2, 4, 5).reshape(B, L, Cb)
    if not emulate_bf16:
        return o
    o = _RoundFwd.apply(o)
    holder["delta"] = (hf(part(gout)) * (hf(part(o.detach())) - lepe.detach())).sum(-1)
    return o


def attn_eval(inp, case, dtype, emulate_bf16=False, attn_mask=None):
    """(out, dqkv, dw, db) of one single-branch case evaluated in `dtype` on the CPU (fp64: the
    reference; fp32: the eager precondition; fp32 + emulate_bf16: the bf16 emulation)."""
    reso, idx, sw, cb, heads, B = case
    qkv = inp["qkv"].detach().to(dtype).clone().requires_grad_(True)
    w, b = inp["w"].detach().to(dtype).clone().requires_grad_(True), inp["b"].detach().to(dtype).clone().requires_grad_(True)
    out = lepe_attention_plain(qkv[..., :cb], qkv[..., cb:2 * cb], qkv[..., 2 * cb:], reso, inp["hs"], inp["ws"], heads,
                               w, b, inp["scale"], emulate_bf16, attn_mask, inp["gout"].to(dtype))
    out.backward(inp["gout"].to(dtype))
    dq = qkv.grad
    if emulate_bf16:
        dq = dq.bfloat16().to(dtype)
    return out.detach(), dq, w.grad, b.grad


def two_branch_eval(inp, dtype, emulate_bf16=False):
    """(out, dqkv, [dw], [db]) of the two-branch launch in `dtype` on the CPU (emulate_bf16: the bf16
    emulation of lepe_attention_plain per branch, dqkv rounded to bf16)."""
    reso, C, heads = TWO_BRANCH["reso"], TWO_BRANCH["C"], TWO_BRANCH["heads"]
    qkv = inp["qkv"].detach().to(dtype).clone().requires_grad_(True)
    ws_ = [w.detach().to(dtype).clone().requires_grad_(True) for w in inp["ws"]]
    bs_ = [b.detach().to(dtype).clone().requires_grad_(True) for b in inp["bs"]]
    outs = []
    gout = inp["gout"].to(dtype)
    for i, (hs, wsp) in enumerate(inp["wins"]):
        sl = slice(i * C // 2, (i + 1) * C // 2)
        outs.append(lepe_attention_plain(qkv[..., :C][..., sl], qkv[..., C:2 * C][..., sl], qkv[..., 2 * C:][..., sl],
                                         reso, hs, wsp, heads // 2, ws_[i], bs_[i], inp["scale"], emulate_bf16, None,
                                         gout[..., sl]))
    out = torch.cat(outs, -1)
    out.backward(gout)
    dq = qkv.grad.bfloat16().to(dtype) if emulate_bf16 else qkv.grad
    return out.detach(), dq, [w.grad for w in ws_], [b.grad for b in bs_]


def two_branch_pack(r, branch):
    """(out, dqkv, dw, db) of one branch's LePE parameters, the form attn_usages / attn_errors take."""
    return r[0], r[1], r[2][branch], r[3][branch]


def attn_groups(gain, cb, dup):
    """[(name, token mask (B, L), channel slice)] over which a (B, L, 3 cb) gradient is judged: dq per
    query kind (the token's q gain, 0 = degenerate); dk and dv per key kind (`dup` (B, L): the tokens
    whose keys are identical, against all others) -- a token's q gain says nothing about its key row."""
    out = []
    for gval in sorted(set(gain.flatten().tolist())):
        out.append((f"dq[gain {gval:g}]", gain == gval, slice(0, cb)))
    for sec, name in ((1, "dk"), (2, "dv")):
        out.append((f"{name}[duplicate keys]", dup, slice(sec * cb, (sec + 1) * cb)))
        out.append((f"{name}[other keys]", ~dup, slice(sec * cb, (sec + 1) * cb)))
    return out


def attn_usages(got, ref, inp, dtype):
    """{group: used fraction} of (out, dqkv, dw, db) against the reference, per token kind."""
    o, dq, dw, db = got
    ro, rdq, rdw, rdb = ref
    cb = o.shape[-1]
    gain = inp["gain"]
    res = {}
    for gval in sorted(set(gain.flatten().tolist())):
        m = gain == gval
        res[f"out[gain {gval:g}]"] = usage(o.cpu()[m], ro[m], dtype)
    for name, m, sl in attn_groups(gain, cb, inp["dup"]):
        res[name] = usage(dq.cpu()[..., sl][m], rdq[..., sl][m], dtype)
    res["dW_lepe"] = usage(dw, rdw, dtype)
    res["db_lepe"] = usage(db, rdb, dtype)
    return res


def attn_errors(got, ref, inp):
    """{group: (max-abs error, rel-L2 error, max|ref|)} of the gradients (dqkv per group, dw, db)."""
    _, dq, dw, db = got
    _, rdq, rdw, rdb = ref
    cb = dq.shape[-1] // 3

    def fig(a, r):
        a, r = a.detach().double().cpu(), r.detach().double().cpu()
        return (float((a - r).abs().max()), float((a - r).norm() / r.norm().clamp_min(1e-30)), float(r.abs().max()))

    res = {name: fig(dq.cpu()[..., sl][m], rdq[..., sl][m]) for name, m, sl in attn_groups(inp["gain"], cb, inp["dup"])}
    res["dW_lepe"] = fig(dw, rdw)
    res["db_lepe"] = fig(db, rdb)
    return res


@functools.lru_cache(maxsize=None)
def attn_reference(case, gains, dtype, seed=0):
    """(inputs, fp64 reference) of a case, computed once per process."""
    inp = attn_inputs(case, gains, dtype, seed)
    return inp, attn_eval(inp, case, torch.float64)


# ---------------------------------------------------------------------------------------------
# 2. LayerNorm rows
# ---------------------------------------------------------------------------------------------
LN_KINDS = ("randn", "mean 100 std 1", "mean 0.1 std 1e-3", "constant", "randn * 1e3", "randn + one 500", "randn * 1e-6")


def ln_rows(rows, C, seed=0, dtype=torch.float32):
    """(x (rows, C), kinds (rows,)): kind = row % 7, so every 64-token panel and every wave holds
    all kinds.  Constant rows hold a bf16-exact value, so their variance is exactly 0."""
    g = torch.Generator().manual_seed(31 * C + rows + seed)
    x = torch.randn(rows, C, generator=g)
    kinds = torch.arange(rows) % 7
    x[kinds == 1] += 100.0
    x[kinds == 2] = x[kinds == 2] * 1e-3 + 0.1
    n3 = int((kinds == 3).sum())
    x[kinds == 3] = (torch.randn(n3, 1, generator=g) * 2 ** -5).bfloat16().float().expand(n3, C)
    x[kinds == 4] *= 1e3
    r5 = (kinds == 5).nonzero().flatten()
    x[r5, torch.randint(0, C, (len(r5),), generator=g)] += 500.0
    x[kinds == 6] *= 1e-6
    return x.to(dtype), kinds


def ln_params(C, seed=0):
    g = torch.Generator().manual_seed(17 * C + seed)
    return torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.3


def ln_eval(x, w, b, dy, dtype, eps=1e-5):
    """(y, dx, dgamma, dbeta) of torch's LayerNorm in `dtype` on the CPU."""
    x_ = x.detach().to(dtype).clone().requires_grad_(True)
    w_, b_ = w.detach().to(dtype).clone().requires_grad_(True), b.detach().to(dtype).clone().requires_grad_(True)
    y = F.layer_norm(x_, (x.shape[-1],), w_, b_, eps)
    y.backward(dy.to(dtype))
    return y.detach(), x_.grad, w_.grad, b_.grad


# ---------------------------------------------------------------------------------------------
# 3. SimAM / BatchNorm channels
# ---------------------------------------------------------------------------------------------
CH_KINDS = ("plain", "mean 50 std 1", "constant", "std 1e-3 about 0.1", "randn * 100", "pivot outlier")


def channel_kinds(shape, per_sample, seed=0, dtype=torch.float32):
    """(x, kinds (C,)) for a channels-last tensor; kind = channel % 6.  per_sample: the statistics
    are per (batch item, channel) over dim 1 (SimAM on (B, L, C)); else per channel over all leading
    dims (BatchNorm on (B, H, W, C)).  The pivot outlier sits on element 0 of each reduction (token 0 /
    pixel (0, 0, 0)), which both kernels use as their shift."""
    g = torch.Generator().manual_seed(sum(shape) + seed)
    C = shape[-1]
    x = torch.randn(shape, generator=g)
    kinds = torch.arange(C) % 6
    x[..., kinds == 1] += 50.0
    n2 = int((kinds == 2).sum())
    cshape = (shape[0],) + (1,) * (len(shape) - 2) + (n2,) if per_sample else (1,) * (len(shape) - 1) + (n2,)
    x[..., kinds == 2] = (torch.randn(cshape, generator=g) * 2 ** -6).bfloat16().float().expand(shape[:-1] + (n2,))
    x[..., kinds == 3] = x[..., kinds == 3] * 1e-3 + 0.1
    x[..., kinds == 4] *= 100.0
    c5 = (kinds == 5).nonzero().flatten()
    if per_sample:
        x[:, 0, c5] += 30.0
    else:
        x[(0,) * (len(shape) - 1)][c5] += 30.0
    return x.to(dtype), kinds


def simam_ref(x, lam=1e-4):
    """SimAM on (B, L, C) tokens in x's dtype (oracle.cswin_ref.simam)."""
    n = x.shape[1] - 1
    d = (x - x.mean(dim=1, keepdim=True)).pow(2)
    v = d.sum(dim=1, keepdim=True) / n
    return x * torch.sigmoid(d / (4 * (v + lam)) + 0.5)


def simam_eval(x, dy, dtype):
    x_ = x.detach().to(dtype).clone().requires_grad_(True)
    y = simam_ref(x_)
    y.backward(dy.to(dtype))
    return y.detach(), x_.grad


def bn_eval(x, w, b, rm, rv, dy, dtype, momentum=0.1, eps=1e-5):
    """(y, dx, dgamma, dbeta, running_mean, running_var) of training-mode BatchNorm2d + ReLU on an
    NHWC tensor in `dtype` on the CPU."""
    x_ = x.detach().to(dtype).clone().requires_grad_(True)
    w_, b_ = w.detach().to(dtype).clone().requires_grad_(True), b.detach().to(dtype).clone().requires_grad_(True)
    rm_, rv_ = rm.to(dtype).clone(), rv.to(dtype).clone()
    y = torch.relu(F.batch_norm(x_.permute(0, 3, 1, 2), rm_, rv_, w_, b_, True, momentum, eps)).permute(0, 2, 3, 1)
    y.backward(dy.to(dtype))
    return y.detach(), x_.grad, w_.grad, b_.grad, rm_, rv_


def bn_params(C):
    """(gamma, beta, running_mean, running_var) of a BatchNorm2d before the step."""
    g = torch.Generator().manual_seed(C)
    return (torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g),
            torch.rand(C, generator=g) + 0.5)


BN_OUT = ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var")


# ---------------------------------------------------------------------------------------------
# 4. CARAFE tap softmax, sigmoid head
# ---------------------------------------------------------------------------------------------
CARAFE_SHAPES = [(1, 5, 8, 2), (2, 5, 64, 2), (1, 5, 32, 4)]     # (B, H, C, s)


def carafe_logits(B, H, s, seed=0, dtype=torch.float32):
    """(enc (B, H, H, 9 s^2), kinds (B H H,)): randn scaled per pixel by {1, 20, 80} (kind 0 / 1 / 2)
    plus a common shift of +-1e4 over all taps on a quarter of the pixels (kind + 3): a softmax
    without its max subtraction overflows; with it the shift cancels exactly."""
    g = torch.Generator().manual_seed(5 * B + H + s + seed)
    enc = torch.randn(B, H, H, 9 * s * s, generator=g)
    k = torch.randint(0, 3, (B, H, H), generator=g)
    enc *= torch.tensor([1.0, 20.0, 80.0])[k][..., None]
    sh = torch.rand(B, H, H, generator=g) < 0.25
    sh.view(-1)[:2] = True
    sign = torch.where(torch.rand(B, H, H, generator=g) < 0.5, -1.0, 1.0)
    enc = enc + (sh * sign * 1e4)[..., None]
    return enc.to(dtype), (k + 3 * sh).flatten()


def carafe_out_kinds(kinds, B, H, s):
    """Kind of each output pixel (that of the source pixel whose taps it reassembles)."""
    return kinds.view(B, H, H).repeat_interleave(s, 1).repeat_interleave(s, 2).flatten()


def carafe_head_usages(names, got, ref, kinds, B, H, s, dtype):
    """{name: used fraction}: prob per kind of output pixel, dx and denc per kind of source pixel, the
    loss and the weight gradients whole."""
    figs = {}
    for n, a, r in zip(names, got, ref):
        if n == "prob":
            ks, sh = carafe_out_kinds(kinds, B, H, s), (B * s * s * H * H, 1)
        elif n in ("dx", "denc"):
            ks, sh = kinds, (B * H * H, -1)
        else:
            figs[n] = usage(a, r, dtype)
            continue
        for k, v in by_kind(a.reshape(sh), r.reshape(sh), ks, 0, dtype).items():
            figs[f"{n}[{k}]"] = v
    return figs


def ratio(err, bound):
    """err / bound with 0 / 0 = 0."""
    return 0.0 if err == 0 else err / max(bound, 1e-300)


def carafe_eval(x, enc, gy, H, s, dtype):
    """(out, dx, denc) of the softmax reassembly (oracle.cswin_ref.carafe without its convs)."""
    B, _, C = x.shape
    x_, e_ = x.detach().to(dtype).clone().requires_grad_(True), enc.detach().to(dtype).clone().requires_grad_(True)
    out = carafe_reassemble_ref(x_, e_, H, s)
    out.backward(gy.to(dtype))
    return out.detach(), x_.grad, e_.grad


def carafe_reassemble_ref(x, enc, H, s):
    B, _, C = x.shape
    xi = x.transpose(1, 2).reshape(B, C, H, H)
    kern = enc.permute(0, 3, 1, 2).reshape(B, 9, s, s, H, H).softmax(dim=1)
    nb = F.unfold(xi, 3, padding=1).reshape(B, C, 9, H, H)
    return torch.einsum("btijhw,bcthw->bchiwj", kern, nb).reshape(B, C, H * s * H * s).transpose(1, 2)


def bce_clamped(prob, target):
    """nn.BCELoss (mean) with its log clamp at -100, in prob's dtype."""
    return F.binary_cross_entropy(prob, target)


HEAD_Z_EDGES = (6.0, 17.0)     # |z| < 6: unsaturated; < 17: 1 - p still resolved in fp32; beyond: p is 0 or 1


def head_target(z, g):
    """Random targets where |z| < 6; the target the sign of z predicts elsewhere (module docstring)."""
    t = (torch.rand(z.shape, generator=g) > 0.5)
    return torch.where(z.abs() < HEAD_Z_EDGES[0], t, z > 0).float()


def head_kinds(z):
    """0 / 1 / 2 by |z| against HEAD_Z_EDGES."""
    a = z.detach().abs().flatten()
    return (a >= HEAD_Z_EDGES[0]).long() + (a >= HEAD_Z_EDGES[1]).long()


def head_inputs(P, C, seed=0, dtype=torch.float32):
    """x (P, C), w (1, C, 1, 1), target (P,): w scaled so the pre-activation spans +-100 -- the fp32
    sigmoid is exactly 0 or 1 on part of the pixels."""
    g = torch.Generator().manual_seed(P + C + seed)
    x = torch.randn(P, C, generator=g).to(dtype)
    w = torch.randn(1, C, 1, 1, generator=g)
    z = x.double() @ w.double().view(C)
    w = w * (100.0 / float(z.abs().max()))
    t = head_target(z * (100.0 / float(z.abs().max())), g)
    return x, w, t


def head_eval(x, w, t, dtype):
    """(prob, loss, dx, dw) of sigmoid(x @ w) chained into the clamped BCE."""
    x_, w_ = x.detach().to(dtype).clone().requires_grad_(True), w.detach().to(dtype).clone().requires_grad_(True)
    p = torch.sigmoid(x_ @ w_.view(-1))
    loss = bce_clamped(p, t.to(dtype))
    loss.backward()
    return p.detach(), loss.detach(), x_.grad, w_.grad


def carafe_head_inputs(B, H, C, s, O=None, seed=0, dtype=torch.float32):
    """x (B, H H, C), enc logits (carafe_logits), w_out (O, C), b_out (O), w_h (O), target: the head
    weights scaled so the pre-activation spans +-100."""
    O = O or C
    g = torch.Generator().manual_seed(B * 100 + H * 10 + C + s + seed)
    x = torch.randn(B, H * H, C, generator=g).to(dtype)
    enc, kinds = carafe_logits(B, H, s, seed, dtype)
    w_out = torch.randn(O, C, generator=g) * C ** -0.5
    b_out = torch.randn(O, generator=g) * 0.3
    w_h = torch.randn(O, generator=g) * O ** -0.5
    y = carafe_reassemble_ref(x.double(), enc.double(), H, s)
    z = (y @ w_out.double().t() + b_out.double()) @ w_h.double()
    w_h = w_h * (100.0 / float(z.abs().max()))
    t = head_target(z * (100.0 / float(z.abs().max())), g).view(B, 1, s * H, s * H)
    return x, enc, w_out, b_out, w_h, t, kinds


def carafe_head_eval(x, enc, w_out, b_out, w_h, t, H, s, dtype):
    """(prob, loss, dx, denc, dw_out, db_out, dw_h) of the unfused chain reassembly -> out conv ->
    1-class output conv -> sigmoid -> clamped BCE."""
    B = x.shape[0]
    ts = [v.detach().to(dtype).clone().requires_grad_(True) for v in (x, enc, w_out, b_out, w_h)]
    y = carafe_reassemble_ref(ts[0], ts[1], H, s)
    p = torch.sigmoid((y @ ts[2].t() + ts[3]) @ ts[4]).view(B, 1, s * H, s * H)
    loss = bce_clamped(p, t.to(dtype))
    loss.backward()
    return (p.detach(), loss.detach()) + tuple(v.grad for v in ts)


CARAFE_HEAD_OUT = ("prob", "loss", "dx", "denc", "dw_out", "db_out", "dw_h")


# ---------------------------------------------------------------------------------------------
# 5. Mlp / GELU tails
# ---------------------------------------------------------------------------------------------
MLP_GAINS = (1.0, 4.0, 12.0)


def mlp_inputs(C, M, seed=0):
    """bf16 operands of the fused Mlp with fc1's rows scaled per hidden feature by {1, 4, 12}
    (kind = feature % 3) and b1 in {0, +6, -6}: h covers the GELU tails out to |h| ~ 12 and beyond,
    where 1 - Phi underflows.  Returns dict(x, w1, b1, w2, b2, res, dy, kinds (4C,))."""
    g = torch.Generator().manual_seed(C + M + seed)
    x = torch.randn(M, C, generator=g).bfloat16()
    kinds = torch.arange(4 * C) % 3
    w1 = torch.randn(4 * C, C, generator=g) * C ** -0.5 * torch.tensor(MLP_GAINS)[kinds][:, None]
    b1 = torch.tensor([0.0, 6.0, -6.0])[(torch.arange(4 * C) // 3) % 3] + torch.randn(4 * C, generator=g) * 0.1
    w2 = torch.randn(C, 4 * C, generator=g) * (4 * C) ** -0.5
    b2 = torch.randn(C, generator=g) * 0.1
    res = torch.randn(M, C, generator=g)
    dy = torch.randn(M, C, generator=g).bfloat16()
    return dict(x=x, w1=w1.bfloat16(), b1=b1, w2=w2.bfloat16(), b2=b2, res=res, dy=dy, kinds=kinds)


def gelu_exact(h):
    return 0.5 * h * (1 + torch.erf(h / 2 ** 0.5))


def gelu_grad_exact(h):
    return 0.5 * (1 + torch.erf(h / 2 ** 0.5)) + h * torch.exp(-0.5 * h * h) / (2 * math.pi) ** 0.5


def mlp_eval(inp, dtype):
    """dict(y, g, dh, dx, dW1, db1, dW2, db2) of res + fc2(gelu(fc1 x)) with the exact-erf GELU."""
    X, W1, B1, W2, B2, R, DY = (inp[k].to(dtype) for k in ("x", "w1", "b1", "w2", "b2", "res", "dy"))
    h = X @ W1.t() + B1
    gl = gelu_exact(h)
    dh = (DY @ W2) * gelu_grad_exact(h)
    return dict(y=R + gl @ W2.t() + B2, g=gl, dh=dh, dx=dh @ W1, dW1=dh.t() @ X, db1=dh.sum(0), dW2=DY.t() @ gl,
                db2=DY.sum(0))


# ---------------------------------------------------------------------------------------------
# 6. e4m3 quantiser rows
# ---------------------------------------------------------------------------------------------
def e4m3_amax_values():
    """amax of each stress row: 0; 448 * 2^k for k = -20 .. 10 with one fp32 ulp below and above;
    1e-30; 1e30."""
    vals = [0.0]
    for k in range(-20, 11):
        a = torch.tensor(448.0 * 2.0 ** k, dtype=torch.float32)
        vals += [float(torch.nextafter(a, torch.tensor(0.0))), float(a), float(torch.nextafter(a, torch.tensor(float("inf"))))]
    vals += [float(torch.tensor(1e-30, dtype=torch.float32)), float(torch.tensor(1e30, dtype=torch.float32))]
    return vals


def e4m3_rows(cols, seed=0):
    """(w (rows, cols) fp32, amax list): one row per e4m3_amax_values() entry whose largest magnitude
    is exactly that value (at a random column, random sign, the rest smaller), plus rows with a single
    non-zero element (the last three)."""
    g = torch.Generator().manual_seed(cols + seed)
    am = e4m3_amax_values()
    rows = len(am)
    w = (torch.rand(rows, cols, generator=g) * 2 - 1) * 0.999 * torch.tensor(am, dtype=torch.float32)[:, None]
    pos = torch.randint(0, cols, (rows,), generator=g)
    sgn = torch.where(torch.rand(rows, generator=g) < 0.5, -1.0, 1.0)
    w[torch.arange(rows), pos] = torch.tensor(am, dtype=torch.float32) * sgn
    single = torch.zeros(3, cols)
    single[0, 0], single[1, cols // 2], single[2, cols - 1] = 448.0, -3.0e-3, 449.0
    w = torch.cat([w, single])
    am = am + [448.0, float(torch.tensor(3.0e-3, dtype=torch.float32)), 449.0]
    assert torch.equal(w.abs().amax(1), torch.tensor(am, dtype=torch.float32))
    return w, am


def e4m3_scale_exact(amax):
    """The smallest power of two s with amax / s <= 448, exactly (1 for amax = 0)."""
    if amax == 0:
        return 1.0
    m, e = math.frexp(amax)            # amax = m 2^e, 0.5 <= m < 1;  448 = 0.875 * 2^9
    return math.ldexp(1.0, e - 9 if m <= 0.875 else e - 8)


def e4m3_expected(w, am):
    """(scales (rows,) fp32, codes (rows, cols) uint8, dequantised fp32) by the exact rule."""
    s = torch.tensor([e4m3_scale_exact(a) for a in am], dtype=torch.float64)
    q = (w.double() / s[:, None]).float().to(torch.float8_e4m3fn)
    return s.float(), q.view(torch.uint8), (q.float().double() * s[:, None]).float()


# ---------------------------------------------------------------------------------------------
# 7. AdamW gradients
# ---------------------------------------------------------------------------------------------
ADAMW_GRAD_MAGS = (0.0, 1e-15, 1e-4, 1.0, 1e4, 1e15)
ADAMW_SHAPES = [(256, 64), (64,), (3, 7, 11), (1,), (4099,)]


def adamw_grad(shape, step, seed=0):
    """A gradient whose element group e % 6 has magnitude ADAMW_GRAD_MAGS[e % 6] (fp32 squares stay
    finite), a random factor in [0.5, 1) per step and a random sign per element, the same at every step."""
    g = torch.Generator().manual_seed(sum(shape) + 100 * step + seed)
    n = int(torch.tensor(shape).prod())
    mag = torch.tensor(ADAMW_GRAD_MAGS, dtype=torch.float32)[torch.arange(n) % 6]
    sign = torch.where(torch.rand(n, generator=torch.Generator().manual_seed(sum(shape) + seed)) < 0.5, -1.0, 1.0)
    v = (torch.rand(n, generator=g) * 0.5 + 0.5) * sign
    return (v * mag).view(shape)

