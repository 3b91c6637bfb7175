"""Stripe attention under every launch plan that batch size can select, on the MI355X.

The whole-window bf16 kernels of csrc/stripe_attn.hip run `sp` workgroups per window-head, sp chosen from the
batch; the suite's other attention cases are small and only ever select the largest split, one 32-row pass per
wave.  Here every split of every LDS image size is forced through StripeGeometry.split (attn_plan_cases.PLAN_CASES),
and a few launches reach the multi-pass plans -- and several row tiles per block of lepe_wgrad_tiles -- through
B and heads alone (NATURAL_CASES).  tests/test_attn_plans.py shows on the CPU that these cases cover every plan
the models select at their production batch sizes, and that the inputs leave half of the bound.

Reference: oracle.cswin_ref.lepe_attention in fp64 on the same rounded inputs, forward and backward, as
test_gpu_kernels.test_stripe_attention_vs_oracle.  Criterion: that file's assert_close bounds (bf16: rel-L2 < 2e-2
and max-abs < 3e-2 max|ref|), applied per (image, window, head, 32-row block) group of out, dq, dk and dv -- the
rows one wave computes in one pass, so one wrong row block is not averaged away -- and to the LePE dW and db as
a whole.  Every test prints the used fraction of its bound ("attn_plans ..." lines; a run's figures are kept in
profiles/attn_plans.txt).

Bitwise equality between plans.  In stripe_fwd_w, stripe_bwd_dq_w and stripe_bwd_dkdv_w a row's result is
computed by one wave from that row's own fragment and the window's K / V (Q / dO, lse, delta) images in LDS, over
all keys (queries) in the same fixed order; the split, the wave count and the pass only decide WHICH workgroup
and wave does it, and every workgroup stages the same images.  So out and lse of the forward, and dq, dk, dv of
the split backward (from the bitwise equal out and lse), must not change by one bit between a forced split and
the heuristic's.  The one-pass backward (N <= 512) and both LePE weight-gradient kernels take no split at all;
fed the same out and lse they are the same launch.  Hence torch.equal is required of EVERY output: out, lse (read
through the C ABI), dqkv, dW and db; none is exempt."""
import ctypes
import functools

import pytest
import torch

import attn_plan_cases as P
import stress_inputs as S

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def judge(family, figs, limit=1.0):
    """Print every figure (used fraction of the bound), then require each to be within the bound."""
    for k, v in figs.items():
        print(f"attn_plans {family} {k}: {v:.3f} of the bound")
    bad = {k: v for k, v in figs.items() if not v <= limit}
    assert not bad, (family, bad)


def _run(geom, B, inp_qkv, ws, bs, gout, drop=None):
    """Forward and backward through ops.stripe_attention: (out, dqkv, [dw], [db]) on the CPU."""
    from csu import ops
    d = dev()
    qd = inp_qkv.to(d).requires_grad_(True)
    wd = [w.to(d).requires_grad_(True) for w in ws]
    bd = [b.to(d).requires_grad_(True) for b in bs]
    out = ops.stripe_attention(qd, geom, wd, bd, drop)
    out.backward(gout.to(d))
    torch.cuda.synchronize()
    assert out.dtype == inp_qkv.dtype
    return out.detach().cpu(), qd.grad.cpu(), [w.grad.cpu() for w in wd], [b.grad.cpu() for b in bd]


def _lse(geom, B, qkv, ws, bs, drop=None):
    """The forward's softmax statistics, which no autograd output shows: csu_stripe_attn_fwd called as
    ops.stripe_attention calls it."""
    from csu import _lib
    d = dev()
    qd = qkv.to(d)
    wd, bd = [w.float().to(d) for w in ws], [b.float().to(d) for b in bs]
    L = qd.shape[1]
    out = torch.empty(B, L, geom.C, dtype=qd.dtype, device=d)
    lse = torch.full((len(geom.branches), B, geom.heads, L), float("nan"), dtype=F32, device=d)
    a = geom.args(B, wd, bd, drop=drop)
    _lib.check(_lib.lib().csu_stripe_attn_fwd(ctypes.byref(a), _lib.dtype_code(qd), _lib.ptr(qd), _lib.ptr(out), _lib.ptr(lse),
                                              _lib.stream_ptr(d)), "stripe_attn_fwd")
    torch.cuda.synchronize()
    return out.cpu(), lse.cpu()


def _drop(snap):
    from csu import ops
    return None if snap is None else ops.AttnDrop(snap, P.DROP_SITE, P.DROP_P)


@functools.lru_cache(maxsize=None)
def _single(shape, split, dropped=False):
    """(out, dqkv, dw, db, lse) of a PLAN_SHAPES entry at a forced split (0: the heuristic), once per process."""
    inp, _ = P.plan_reference(shape)
    snap = torch.tensor([77, 1], dtype=torch.int64, device=dev()) if dropped else None
    geom = P.geometry(shape, split)
    o, dq, dw, db = _run(geom, shape[5], inp["qkv"], [inp["w"]], [inp["b"]], inp["gout"], _drop(snap))
    o2, lse = _lse(geom, shape[5], inp["qkv"], [inp["w"]], [inp["b"]], _drop(snap))
    assert torch.equal(o, o2)
    assert bool(torch.isfinite(lse).all())
    return o, dq, dw[0], db[0], lse


def _same_as_heuristic(got, base, what):
    for name, a, b in zip(("out", "dqkv", "dW_lepe", "db_lepe", "lse"), got, base):
        assert torch.equal(a, b), f"{what}: {name} differs from the heuristic plan's by " \
                                  f"{float((a.double() - b.double()).abs().max()):.3e}"


@pytest.mark.parametrize("shape,split", P.PLAN_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_forced_split_vs_oracle(shape, split):
    """Every split of every LDS image size (forward; split backward for N > 512, one-pass backward below)
    against the fp64 oracle per row block, and bitwise against the heuristic's plan (module docstring)."""
    dev()
    inp, ref = P.plan_reference(shape)
    p = P.plan(P.geometry(shape, split), shape[5], BF16)
    assert p.fwd.kernel == 1 and p.fwd.sp == split and (p.bwd.sp == split or p.bwd.kernel == 2)
    got = _single(shape, split)
    fam = f"{shape} split {split} [fwd {P.describe(p.fwd)}; bwd {P.describe(p.bwd)}]"
    judge(fam, P.case_figs(got[:4], ref, shape))
    _same_as_heuristic(got, _single(shape, 0), fam)


@pytest.mark.parametrize("shape,split", P.DROP_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_forced_split_dropout_vs_oracle(shape, split):
    """Attention dropout at a multi-pass split of each kernel family: the mask index of the later passes.  The
    device's masks are fed to the reference the way test_stripe_attention_dropout_sharp does."""
    dev()
    from csu import rng
    inp, _ = P.plan_reference(shape)
    snap = torch.tensor([77, 1], dtype=torch.int64, device=dev())
    p = P.plan(P.geometry(shape, split), shape[5], BF16)
    assert p.fwd.passes > 1 and p.bwd.passes > 1

    def mask(shp):
        Bw, H, N, _ = shp
        npad = -(-N // 32) * 32
        m = rng.dropout_mask(snap, P.DROP_SITE, P.DROP_P, Bw * H * N * npad).view(Bw, H, N, npad)[..., :N]
        return m.double().cpu() / (1 - P.DROP_P)

    ref = P.oracle_eval(inp, shape, attn_mask=mask)
    got = _single(shape, split, True)
    fam = f"dropout {shape} split {split} [fwd {P.describe(p.fwd)}; bwd {P.describe(p.bwd)}]"
    judge(fam, P.case_figs(got[:4], ref, shape))
    _same_as_heuristic(got, _single(shape, 0, True), fam)
    assert float((_single(shape, split)[0].float() - got[0].float()).abs().max()) > 1e-2      # the mask is really applied


@pytest.mark.parametrize("t", P.TWO_BRANCH_CASES, ids=lambda t: f"reso{t['reso']}-split{t['split']}")
def test_two_branch_multi_pass(t):
    """Both branches in one launch (grid y = branch) at a multi-pass split: 256-token windows (forward, one-pass
    backward) and 1024-token windows (forward and split backward)."""
    dev()
    inp = P.two_branch_inputs(t)
    ref = P.two_branch_eval(inp)
    geom, heur = P.two_branch_geometry(t), P.two_branch_geometry(t, 0)
    p = P.plan(geom, t["B"], BF16)
    assert p.fwd.sp == t["split"] and p.fwd.passes > 1 and p.bwd.passes > 1 and P.plan(heur, t["B"], BF16).fwd.sp != t["split"]
    got = _run(geom, t["B"], inp["qkv"], inp["ws"], inp["bs"], inp["gout"])
    judge(f"two-branch reso {t['reso']} split {t['split']} [fwd {P.describe(p.fwd)}; bwd {P.describe(p.bwd)}]",
          P.two_branch_figs(t, got, ref))
    base = _run(heur, t["B"], inp["qkv"], inp["ws"], inp["bs"], inp["gout"])
    lse = [_lse(g, t["B"], inp["qkv"], inp["ws"], inp["bs"])[1] for g in (geom, heur)]
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]) and torch.equal(lse[0], lse[1])
    for i in range(2):
        assert torch.equal(got[2][i], base[2][i]) and torch.equal(got[3][i], base[3][i])


@pytest.mark.parametrize("case", P.NATURAL_CASES, ids=lambda c: str(c).replace(" ", ""))
def test_heuristic_selects_multi_pass_plan(case):
    """B and heads alone select the plan (split 0), as in training: a batch of 4 distinct images in a fixed
    non-periodic order, every image against its own fp64 reference, the LePE gradients against the
    count-weighted fp64 sum.  bf16: per row block, dW and db whole; fp32 (lepe_wgrad_tiles<float> with several
    tiles per block; the attention kernels are the streamed ones): assert_close's fp32 bound."""
    dev()
    reso, cb, heads, B, dtype = case
    inp, ref, order = P.natural_reference(case)
    geom = P.natural_geometry(case)
    p = P.plan(geom, B, dtype)
    if dtype == BF16:
        assert p.fwd.passes > 1 and p.fwd.kernel == 1 and p.bwd.passes > 1
    else:
        assert p.lepe_kernel == 1 and p.tiles_blk > 1
    idx = torch.tensor(order)
    got = _run(geom, B, inp["qkv"][idx], [inp["w"]], [inp["b"]], inp["gout"][idx])
    full = (ref[0][idx], ref[1][idx])
    fam = f"natural {case[:4]} {'bf16' if dtype == BF16 else 'fp32'} [fwd {P.describe(p.fwd)}; bwd {P.describe(p.bwd)}; " \
          f"LePE {P.LEPE_NAMES[p.lepe_kernel]}, {p.tiles_blk} tiles per block, flags {p.wgrad_flags}]"
    if dtype == BF16:
        figs = P.block_figs(got, full, P.block_ids(B, reso, reso, reso, heads), cb, heads, use_by_kind=False)
    else:
        figs = {"out": S.usage(got[0], full[0], F32)}
        for i, n in enumerate(("dq", "dk", "dv")):
            figs[n] = S.usage(got[1][..., i * cb:(i + 1) * cb], full[1][..., i * cb:(i + 1) * cb], F32)
    figs["dW_lepe"], figs["db_lepe"] = S.usage(got[2][0], ref[2], dtype), S.usage(got[3][0], ref[3], dtype)
    judge(fam, figs)


def test_untiled_lepe_wgrad_vs_oracle():
    """lepe_wgrad_partial (images too wide for a row tile in 64 KiB of LDS: fp32 above 128 tokens), which no other
    kernel-level case reaches: fp32 forward and backward, assert_close's fp32 bound."""
    dev()
    shape = P.UNTILED_LEPE_CASE
    cb = shape[3]
    inp, ref = P.untiled_reference()
    p = P.plan(P.geometry(shape), shape[5], F32)
    assert p.lepe_kernel == 2
    got = _run(P.geometry(shape), shape[5], inp["qkv"], [inp["w"]], [inp["b"]], inp["gout"])
    figs = {"out": S.usage(got[0], ref[0], F32)}
    for i, n in enumerate(("dq", "dk", "dv")):
        figs[n] = S.usage(got[1][..., i * cb:(i + 1) * cb], ref[1][..., i * cb:(i + 1) * cb], F32)
    figs["dW_lepe"], figs["db_lepe"] = S.usage(got[2][0], ref[2], F32), S.usage(got[3][0], ref[3], F32)
    judge(f"untiled LePE {shape} fp32 [{p.wgrad_nblk} blocks]", figs)
