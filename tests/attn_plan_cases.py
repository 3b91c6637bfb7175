"""The launch plans of csrc/stripe_attn.hip and the cases that run each of them: the table behind
tests/test_attn_plans.py (CPU) and tests/test_gpu_attn_plans.py (MI355X).  Plain torch and the host-only
csu_stripe_attn_plan; nothing here needs a GPU.

The whole-window bf16 kernels (stripe_fwd_w, stripe_bwd_dq_w, stripe_bwd_dkdv_w) run `sp` workgroups per
window-head, chosen from the BATCH (about 1024 workgroups per launch), an even sp as 8-wave workgroups; a
workgroup walks its rows in passes of 32 * waves.  The suite's other attention cases are all small, so they
only ever select the largest split, one pass per wave.  ``PLAN_CASES`` forces every split of every LDS image
size through csu_stripe_args.split; ``NATURAL_CASES`` reach the multi-pass plans (and several row tiles per
block of lepe_wgrad_tiles) through B and heads alone, as training does.

A plan key is (direction, kernel, WM, sp, waves, passes > 1, flags): what selects code in the kernels.  The
streamed kernels' key leaves out the block count: there it is the grid size, not a path."""
import functools

import torch

import stress_inputs as S

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


def max_split(N):
    """csu_stripe_args.split's upper end: ceil(roundup32(N) / 128)."""
    return (-(-N // 32) * 32 + 127) // 128


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
# (reso, idx, sw, cb, heads, B): the smallest shapes that reach each path, B <= 2 and heads <= 2
PLAN_SHAPES = {
    256: [(12, -1, 12, 32, 1, 2),     # N = 144: sp 1 has a second pass with one valid wave
          (14, -1, 14, 64, 2, 1),     # N = 196: ragged key tail and a ragged second pass
          (16, -1, 16, 64, 2, 2)],    # N = 256
    512: [(20, -1, 20, 32, 1, 2),     # N = 400
          (32, 0, 16, 64, 2, 1)],     # N = 512, two windows per image: decode_w's id decomposition with a split
    1024: [(24, -1, 24, 64, 2, 1),    # N = 576
           (28, -1, 28, 32, 1, 2),    # N = 784
           (30, -1, 30, 32, 1, 2),    # N = 900: at sp 7 the workgroups own 160 rows, six cover the padded window
                                      # (928 rows) and the seventh owns none; its first row (960) is past the end
           (32, -1, 32, 64, 2, 2)],   # N = 1024
}
FOUR_WINDOWS = ((64, 1, 16, 64, 2, 1), 3)     # N = 1024, four windows per image, an odd split: one case


def shape_tokens(shape):
    hs, ws = S.stripe_geometry(*shape[:3])
    return hs * ws


# (shape, forced split): every split 1 .. max_split of every shape
PLAN_CASES = [(shape, sp) for wm in (256, 512, 1024) for shape in PLAN_SHAPES[wm]
              for sp in range(1, max_split(shape_tokens(shape)) + 1)] + [FOUR_WINDOWS]

# one attention-dropout case per kernel family at a multi-pass split: (shape, split), p = 0.3
DROP_P, DROP_SITE = 0.3, 40
DROP_CASES = [((16, -1, 16, 64, 2, 2), 1),    # forward WM 256, two passes; one-pass backward <256, 4>
              ((20, -1, 20, 32, 1, 2), 1),    # forward WM 512, four passes, the last ragged; one-pass backward <512, 8>
              ((24, -1, 24, 64, 2, 1), 1),    # forward WM 1024 and the split backward, 4 waves, five passes
              ((24, -1, 24, 64, 2, 1), 2)]    # ... as one 8-wave workgroup, three passes

# the two-branch launch of test_two_branch_fused_launch (reso 32, C 128, 2 heads per branch, B 2) with 8-wide
# stripes for its 2-wide ones: 64-token windows allow no split but 1 and no second pass; 256-token ones at
# split 1 make two passes in both branches (forward; one-pass backward).  The second launch has 1024-token
# windows, four per image and branch: the multi-pass split backward with grid y = branch
TWO_BRANCH_CASES = [dict(reso=32, C=128, heads=4, sw=8, B=2, split=1),
                    dict(reso=64, C=128, heads=4, sw=16, B=1, split=3)]

# the heuristic itself selecting the multi-pass plans: (reso, cb, heads, B, dtype), full window, a batch built
# from NATURAL_DISTINCT images in the order natural_order(B)
NATURAL_DISTINCT = 4
NATURAL_CASES = [
    (16, 256, 8, 128, BF16),    # 1024 window-heads: sp 1, two passes; one-pass backward
    (24, 256, 8, 64, BF16),     # 512 window-heads at N = 576: sp 2 as 8 waves, three passes, split backward;
                                # lepe_wgrad_tiles<bf16>, six tiles per block
    (16, 128, 4, 64, F32),      # lepe_wgrad_tiles<float>: two tiles per block
    (16, 128, 4, 128, F32),     # four tiles per block
    (14, 128, 4, 128, F32),     # four tiles per block, the last ragged
]


# lepe_wgrad_partial, the untiled pass 1: fp32 images wider than 128 tokens (bf16: 256), whose row tile with its
# halo does not fit 64 KiB of LDS -- stage 1 of the 1024 x 1024 model in fp32.  No other kernel-level case is
# that wide.  (reso, idx, sw, cb, heads, B), fp32
UNTILED_LEPE_CASE = (132, 0, 1, 64, 2, 2)


def natural_order(B):
    """Which of the NATURAL_DISTINCT images each batch item is: fixed, not periodic, every image present."""
    return [(i * i + i // 3) % NATURAL_DISTINCT for i in range(B)]


# ---------------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------------
def geometry(shape, split=0):
    from csu import ops
    reso, idx, sw, cb, heads, B = shape
    hs, ws = S.stripe_geometry(reso, idx, sw)
    return ops.StripeGeometry(reso, cb, heads, [(hs, ws, 0)], (cb // heads) ** -0.5, split=split)


def two_branch_geometry(t, split=None):
    from csu import ops
    return ops.StripeGeometry(t["reso"], t["C"], t["heads"] // 2, [(t["reso"], t["sw"], 0), (t["sw"], t["reso"], t["C"] // 2)],
                              (t["C"] // t["heads"]) ** -0.5, split=t["split"] if split is None else split)


def natural_geometry(case):
    from csu import ops
    reso, cb, heads, B, dtype = case
    return ops.StripeGeometry(reso, cb, heads, [(reso, reso, 0)], (cb // heads) ** -0.5)


def plan(geom, B, dtype):
    from csu import ops
    return ops.stripe_plan(geom, B, dtype)


KERNEL_NAMES = {0: "streamed", 1: "window", 2: "fused-bwd"}
LEPE_NAMES = {0: "in fused-bwd", 1: "tiles", 2: "partial"}


def kernel_key(direction, k):
    """(direction, kernel, WM, sp, waves, passes > 1, flags) of a csu_stripe_kernel_plan."""
    if k.kernel == 0:
        return (direction, "streamed", 0, 0, k.waves, False, 0)
    return (direction, KERNEL_NAMES[k.kernel], k.wm, k.sp, k.waves, k.passes > 1, k.flags)


def lepe_key(p):
    """(kernel of pass 1, several tiles per block, flags) of the LePE weight gradient of a backward."""
    return (LEPE_NAMES[p.lepe_kernel], p.lepe_kernel == 1 and p.tiles_blk > 1, p.wgrad_flags if p.lepe_kernel == 1 else 0)


def plan_keys(geom, B, dtype):
    p = plan(geom, B, dtype)
    return {kernel_key("fwd", p.fwd), kernel_key("bwd", p.bwd)}, {lepe_key(p)}


def describe(k):
    return (f"{KERNEL_NAMES[k.kernel]} WM {k.wm} sp {k.sp} ({k.split} x {k.waves} waves, {k.rows} rows, {k.passes} pass"
            f"{'es' if k.passes > 1 else ''}{', ragged' if k.flags & 1 else ''}{', empty partner' if k.flags & 2 else ''})")


def existing_cases():
    """[(name, geometry, B, dtype)] of the kernel-level attention cases the suite had before this table:
    ATTN_CASES and STRESS_ATTN_CASES in both dtypes, the two-branch launch."""
    import test_gpu_kernels as K
    from csu import ops
    out = []
    for name, cases in (("ATTN_CASES", K.ATTN_CASES), ("STRESS_ATTN_CASES", S.STRESS_ATTN_CASES)):
        for c in cases:
            for dt in (F32, BF16):
                out.append((f"{name} {c}", geometry(c), c[5], dt))
    t = S.TWO_BRANCH
    g2 = ops.StripeGeometry(t["reso"], t["C"], t["heads"] // 2, [(t["reso"], t["sw"], 0), (t["sw"], t["reso"], t["C"] // 2)],
                            (t["C"] // t["heads"]) ** -0.5)
    for dt in (F32, BF16):
        out.append(("two-branch", g2, t["B"], dt))
    return out


def tested_launches(plan_cases=None):
    """[(name, geometry, B, dtype)] of every launch a GPU test compares with a reference."""
    out = existing_cases()
    for shape, sp in (PLAN_CASES if plan_cases is None else plan_cases):
        out.append((f"plan {shape} split {sp}", geometry(shape, sp), shape[5], BF16))
    for shape, sp in DROP_CASES:
        out.append((f"dropout {shape} split {sp}", geometry(shape, sp), shape[5], BF16))
    for t in TWO_BRANCH_CASES:
        out.append((f"two-branch reso {t['reso']} split {t['split']}", two_branch_geometry(t), t["B"], BF16))
    for c in NATURAL_CASES:
        out.append((f"natural {c[:4]}", natural_geometry(c), c[3], c[4]))
    out.append((f"untiled LePE {UNTILED_LEPE_CASE}", geometry(UNTILED_LEPE_CASE), UNTILED_LEPE_CASE[5], F32))
    return out


def forced_keys(plan_cases=None):
    """The kernel plan keys of the forced-split launches of PLAN_CASES alone."""
    K = set()
    for shape, sp in (PLAN_CASES if plan_cases is None else plan_cases):
        K |= plan_keys(geometry(shape, sp), shape[5], BF16)[0]
    return K


def tested_keys(plan_cases=None):
    T, TL = set(), set()
    for _, geom, B, dt in tested_launches(plan_cases):
        k, l = plan_keys(geom, B, dt)
        T |= k
        TL |= l
    return T, TL


PRODUCTION_IMAGES = (256, 512, 1024)
PRODUCTION_SPLITS = ((1, 2, 8, 8), (1, 2, 7, 7))
PRODUCTION_BATCHES = (1, 2, 4, 8, 16, 32, 64)


def model_geometries(img, split):
    """The StripeGeometry of every distinct CSWinBlock of the model, or None where the geometry does not
    allow the split sizes (the reference's view fails, csu.model raises)."""
    from csu.model import CSWinBlock, CSWinTransformer
    try:
        m = CSWinTransformer(img_size=img, depth=[1, 1, 1, 1], split_size=list(split))
    except ValueError:
        return None
    seen, out = set(), []
    for mod in m.modules():
        if isinstance(mod, CSWinBlock):
            g = mod._geom
            key = (g.reso, g.C, g.heads, tuple(g.branches))
            if key not in seen:
                seen.add(key)
                out.append(g)
    return out


def production_launches():
    """[(name, geometry, B, dtype)]: every stage of the models at PRODUCTION_IMAGES x PRODUCTION_SPLITS x
    PRODUCTION_BATCHES and of test_gpu_train.FULL_CONFIGS, in both dtypes."""
    import test_gpu_train as T
    configs = [(img, split, B) for img in PRODUCTION_IMAGES for split in PRODUCTION_SPLITS for B in PRODUCTION_BATCHES]
    configs += [(c[0], tuple(c[3]), c[1]) for c in T.FULL_CONFIGS]
    out, geoms = [], {}
    for img, split, B in configs:
        if (img, split) not in geoms:
            geoms[img, split] = model_geometries(img, split)
        for g in geoms[img, split] or []:
            for dt in (F32, BF16):
                out.append((f"img {img} split {split} B {B} reso {g.reso} {dt}", g, B, dt))
    return out


# ---------------------------------------------------------------------------------------------
# inputs, references, criteria
# ---------------------------------------------------------------------------------------------
LEPE_W = 0.1


def plan_inputs(shape, seed=0, B=None, dtype=BF16):
    """Inputs of one single-branch case as test_stripe_attention_vs_oracle draws them (randn qkv and output
    gradient, LePE bias 0.1 randn), in the form stress_inputs.attn_eval takes.  LePE weights LEPE_W randn
    for that test's 0.3: with 0.3 the output is mostly LePE (|O| ~ 1 against an attention part of ~ N^-1/2), and
    the bf16 rounding of that O, through delta = rowsum(dO * (O - LePE)), alone uses up to 0.64 of the bound in
    a row block of dq at N = 1024 (test_attn_plans.py's precondition allows 0.5); with 0.1 at most 0.3."""
    reso, idx, sw, cb, heads, Bc = shape
    B = Bc if B is None else B
    g = torch.Generator().manual_seed(2000 + seed + sum(abs(c) for c in shape))
    L = reso * reso
    hs, ws = S.stripe_geometry(reso, idx, sw)
    qkv = torch.randn(B, L, 3 * cb, generator=g).to(dtype)
    w = torch.randn(cb, 1, 3, 3, generator=g) * LEPE_W
    b = torch.randn(cb, generator=g) * 0.1
    gout = torch.randn(B, L, cb, generator=g).to(dtype)
    return dict(qkv=qkv, w=w, b=b, gout=gout, hs=hs, ws=ws, scale=(cb // heads) ** -0.5)


def oracle_eval(inp, shape, attn_mask=None):
    """(out, dqkv, dw, db): oracle.cswin_ref.lepe_attention in fp64 on the same rounded inputs, forward and
    backward, as test_stripe_attention_vs_oracle."""
    from oracle import cswin_ref as O
    reso, idx, sw, cb, heads, _ = shape
    q = inp["qkv"].double().requires_grad_(True)
    w, b = inp["w"].double().requires_grad_(True), inp["b"].double().requires_grad_(True)
    ref = O.lepe_attention(q[..., :cb], q[..., cb:2 * cb], q[..., 2 * cb:], reso, inp["hs"], inp["ws"], heads, w, b,
                           inp["scale"], attn_mask=attn_mask)
    ref.backward(inp["gout"].double())
    return ref.detach(), q.grad, w.grad, b.grad


@functools.lru_cache(maxsize=None)
def plan_reference(shape):
    """(inputs, fp64 reference) of a PLAN_SHAPES entry, computed once per process and left unchanged."""
    inp = plan_inputs(shape)
    return inp, oracle_eval(inp, shape)


@functools.lru_cache(maxsize=None)
def untiled_reference():
    inp = plan_inputs(UNTILED_LEPE_CASE, dtype=F32)
    return inp, oracle_eval(inp, UNTILED_LEPE_CASE)


def two_branch_inputs(t):
    reso, C, B = t["reso"], t["C"], t["B"]
    g = torch.Generator().manual_seed(2003 + reso)
    qkv = torch.randn(B, reso * reso, 3 * C, generator=g).bfloat16()
    ws_ = [torch.randn(C // 2, 1, 3, 3, generator=g) * LEPE_W for _ in range(2)]
    bs_ = [torch.randn(C // 2, generator=g) * 0.1 for _ in range(2)]
    gout = torch.randn(B, reso * reso, C, generator=g).bfloat16()
    wins = [S.stripe_geometry(reso, i, t["sw"]) for i in range(2)]
    return dict(qkv=qkv, ws=ws_, bs=bs_, gout=gout, wins=wins, scale=(C // t["heads"]) ** -0.5, case=t)


def two_branch_eval(inp, dtype=F64, emulate_bf16=False):
    """(out, dqkv, [dw], [db]) of a TWO_BRANCH_CASES entry: the oracle per branch + cat in fp64 (test_two_branch_fused_launch's
    reference, with its backward), or stress_inputs' bf16 emulation per branch."""
    from oracle import cswin_ref as O
    t = inp["case"]
    reso, C, heads = t["reso"], t["C"], t["heads"]
    qkv = inp["qkv"].to(dtype).clone().requires_grad_(True)
    ws_ = [w.to(dtype).clone().requires_grad_(True) for w in inp["ws"]]
    bs_ = [b.to(dtype).clone().requires_grad_(True) for b in inp["bs"]]
    gout = inp["gout"].to(dtype)
    outs = []
    for i, (hs, wsp) in enumerate(inp["wins"]):
        sl = slice(i * C // 2, (i + 1) * C // 2)
        args = (qkv[..., :C][..., sl], qkv[..., C:2 * C][..., sl], qkv[..., 2 * C:][..., sl], reso, hs, wsp, heads // 2,
                ws_[i], bs_[i], inp["scale"])
        outs.append(S.lepe_attention_plain(*args, True, None, gout[..., sl]) if emulate_bf16 else O.lepe_attention(*args))
    out = torch.cat(outs, -1)
    out.backward(gout)
    dq = qkv.grad.bfloat16().to(dtype) if emulate_bf16 else qkv.grad
    return out.detach(), dq, [w.grad for w in ws_], [b.grad for b in bs_]


def natural_inputs(case):
    """The NATURAL_DISTINCT distinct images of a NATURAL_CASES entry (as a batch of that size)."""
    reso, cb, heads, B, dtype = case
    return plan_inputs((reso, -1, reso, cb, heads, NATURAL_DISTINCT), seed=7, dtype=dtype)


@functools.lru_cache(maxsize=None)
def natural_reference(case):
    """(distinct inputs, their fp64 reference (out, dqkv per distinct image; dw, db of the whole batch: the
    count-weighted sum over the distinct images), order)."""
    reso, cb, heads, B, dtype = case
    inp = natural_inputs(case)
    order = natural_order(B)
    count = torch.bincount(torch.tensor(order), minlength=NATURAL_DISTINCT).double()
    assert int(count.min()) > 0
    from oracle import cswin_ref as O
    outs, dqs = [], []
    dw, db = torch.zeros(cb, 1, 3, 3, dtype=F64), torch.zeros(cb, dtype=F64)
    for i in range(NATURAL_DISTINCT):
        one = dict(inp, qkv=inp["qkv"][i:i + 1], gout=inp["gout"][i:i + 1])
        o, dq, w_, b_ = oracle_eval(one, (reso, -1, reso, cb, heads, 1))
        outs.append(o)
        dqs.append(dq)
        dw += count[i] * w_
        db += count[i] * b_
    return inp, (torch.cat(outs), torch.cat(dqs), dw, db), order


def block_ids(B, reso, hs, ws, heads):
    """(B, L, heads) integer id of the (image, window, head, 32-row block) group of every (token, head): the
    rows one wave computes in one pass of any plan."""
    wt = S.window_tokens(reso, hs, ws)                    # (nwin, N)
    nwin, N = wt.shape
    nblk = -(-N // 32)
    tok_grp = torch.empty(reso * reso, dtype=torch.long)
    tok_grp[wt.flatten()] = (torch.arange(nwin)[:, None] * nblk + torch.arange(N)[None, :] // 32).flatten()
    per_img = nwin * nblk
    ids = (torch.arange(B)[:, None, None] * per_img + tok_grp[None, :, None]) * heads + torch.arange(heads)[None, None, :]
    return ids


def rows_of(t, heads):
    """(B, L, heads * hd) -> (B * L * heads, hd): one row per (token, head)."""
    B, L, Cb = t.shape
    return t.detach().cpu().reshape(B * L * heads, Cb // heads)


def block_usage_max(a, ref, ids, heads):
    """max over the groups of `ids` of the used fraction of the bf16 bound (rel-L2 < 2e-2, max-abs < 3e-2
    max|ref|, both taken inside the group): stress_inputs.by_kind's figures, all groups at once (the CPU file
    checks the two agree).  For the batches of NATURAL_CASES, where by_kind's loop over 10^4 groups is slow."""
    a, ref = rows_of(a, heads).double(), rows_of(ref, heads).double()
    g = ids.flatten()
    n = int(g.max()) + 1
    err = a - ref
    e2 = torch.zeros(n, dtype=F64).index_add_(0, g, (err * err).sum(1))
    r2 = torch.zeros(n, dtype=F64).index_add_(0, g, (ref * ref).sum(1))
    emax = torch.zeros(n, dtype=F64).scatter_reduce_(0, g, err.abs().amax(1), "amax", include_self=True)
    rmax = torch.zeros(n, dtype=F64).scatter_reduce_(0, g, ref.abs().amax(1), "amax", include_self=True)
    l2 = e2.sqrt() / r2.sqrt().clamp_min(1e-30)
    return float(torch.maximum(l2 / 2e-2, emax / (3e-2 * rmax.clamp_min(1e-30))).max())


def block_figs(got, ref, ids, cb, heads, use_by_kind=True):
    """{out, dq, dk, dv: the largest used fraction of the bf16 bound over the (image, window, head, 32-row
    block) groups} of (out, dqkv) against the reference."""
    figs = {}
    parts = [("out", got[0], ref[0])] + [(n, got[1][..., i * cb:(i + 1) * cb], ref[1][..., i * cb:(i + 1) * cb])
                                         for i, n in enumerate(("dq", "dk", "dv"))]
    for name, a, r in parts:
        if use_by_kind:
            figs[name] = max(S.by_kind(rows_of(a, heads), rows_of(r, heads), ids.flatten(), 0, BF16).values())
        else:
            figs[name] = block_usage_max(a, r, ids, heads)
    return figs


def case_figs(got, ref, shape, B=None, use_by_kind=True):
    """The figures one single-branch case is judged by: out, dq, dk, dv per block group, LePE dW and db whole."""
    reso, idx, sw, cb, heads, Bc = shape
    hs, ws = S.stripe_geometry(reso, idx, sw)
    ids = block_ids(Bc if B is None else B, reso, hs, ws, heads)
    figs = block_figs(got, ref, ids, cb, heads, use_by_kind)
    figs["dW_lepe"], figs["db_lepe"] = S.usage(got[2], ref[2], BF16), S.usage(got[3], ref[3], BF16)
    return figs


def two_branch_figs(t, got, ref):
    C, heads = t["C"], t["heads"] // 2
    figs = {}
    for i, (hs, ws) in enumerate(S.stripe_geometry(t["reso"], j, t["sw"]) for j in range(2)):
        ids = block_ids(t["B"], t["reso"], hs, ws, heads)
        sl = slice(i * C // 2, (i + 1) * C // 2)
        pick = lambda x: (x[0][..., sl], torch.cat([x[1][..., k * C:(k + 1) * C][..., sl] for k in range(3)], -1))
        for k, v in block_figs(pick(got), pick(ref), ids, C // 2, heads).items():
            figs[f"{k}{i}"] = v
        figs[f"dW_lepe{i}"], figs[f"db_lepe{i}"] = S.usage(got[2][i], ref[2][i], BF16), S.usage(got[3][i], ref[3][i], BF16)
    return figs
