"""The persistent convolution kernels in their steady state, and every conv launch plan, on the MI355X.

igemm_dma (12 tile configurations), conv3_halo64, conv3_c16 and conv3_c16d launch 1 or 2 workgroups per CU and
walk their tiles as one stream through a ring.  The suite's other conv cases never give a workgroup a second
tile, so the ring stage carried across tiles, the vmcnt accounting of the previous tile's stores, the gather
bases of the next tile, the clamped re-fetch of the last unit and the XCD ranges with their remainder never
decide a result there.  Here csu_conv2d_ex2's `wgs` runs the same kernels on 8 and 16 workgroups
(conv_plan_cases.py), each case asserting from csu_conv2d_plan -- the function the launch takes its decisions
from -- that a workgroup owns >= 3 tiles, that counts differ, that tiles % 8 != 0 and so on.

Reference: fp64 torch conv2d / conv_transpose2d on the CPU on the same bf16 operands.  Criterion: rel-L2 < 4e-3
(test_conv_igemm_dma_cfgs' bound: bf16 output rounding, 2^-9 relative, dominates) per block of BM consecutive
GEMM rows, so one wrong tile is not averaged away; outputs are pre-filled with NaN.  The autograd paths
(AUTO_CASES) use test_gpu_kernels.assert_close.  Every forced case prints the used fraction of its bound.

Bitwise equality between grids: a tile's arithmetic -- its K slices in order, one accumulator per output --
does not depend on the workgroup that computes it or on what that workgroup computed before, so the outputs
under 8, 16 and the default number of workgroups must be equal bit for bit.  A stale ring stage or gather base
breaks exactly this."""
import ctypes
import functools

import pytest
import torch

import conv_plan_cases as P
import stress_inputs as S

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def launch(op, g, src, w, bias, cfg, wgs, c_split=0, ws=False):
    """csu_conv2d_ex2 on NaN-filled outputs.  src / w / bias: CPU tensors (w in torch's (N, C, k, k) layout);
    c_split: the forward's src is split on channels, the input gradient's output comes back in two pieces.
    Returns the NHWC output on the CPU (the two pieces concatenated)."""
    from csu import _lib
    d = dev()
    L = _lib.lib()
    wl = P.weight_layout(op, w).to(d)
    bd = None if bias is None else bias.float().to(d)
    shape = (g.B, g.OH, g.OW, g.N) if op == 0 else (g.B, g.H, g.W, g.C)
    if c_split and op == 0:
        a, b = src[..., :c_split].contiguous().to(d), src[..., c_split:].contiguous().to(d)
        out = torch.full(shape, float("nan"), dtype=BF16, device=d)
        second, outs = b, [out]
    elif c_split:
        a = src.to(d)
        out = torch.full(shape[:3] + (c_split,), float("nan"), dtype=BF16, device=d)
        second = torch.full(shape[:3] + (shape[3] - c_split,), float("nan"), dtype=BF16, device=d)
        outs = [out, second]
    else:
        a, second = src.to(d), None
        out = torch.full(shape, float("nan"), dtype=BF16, device=d)
        outs = [out]
    nws = L.csu_conv2d_workspace(op, ctypes.byref(g), _lib.CSU_BF16) if ws else 0
    work = torch.empty(max(nws, 16), dtype=torch.uint8, device=d) if nws else None
    rc = L.csu_conv2d_ex2(op, ctypes.byref(g), _lib.CSU_BF16, a.data_ptr(), wl.data_ptr(), None if bd is None else bd.data_ptr(),
                          out.data_ptr(), None if second is None else second.data_ptr(), c_split, cfg, wgs,
                          None if work is None else work.data_ptr(), nws, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (op, cfg, wgs, L.csu_last_error_string())
    torch.cuda.synchronize()
    return torch.cat([o.cpu() for o in outs], -1)


def grids(name, op, g, r, cfg, bm, c_split=0, wgs=P.WGS):
    """The case under every grid: each against fp64 per BM-row block, all bitwise equal."""
    outs = {w: launch(op, g, r["src"], r["w"], r["bias"], cfg, w, c_split) for w in wgs}
    for w, o in outs.items():
        u = P.block_usage(o, r["ref"], bm)
        print(f"conv_plans {name} wgs {w}: {u:.3f} of the bound")
        assert u <= 1.0, (name, w, u)
    base = outs[wgs[-1]]
    for w, o in outs.items():
        assert torch.equal(o, base), f"{name}: grid {w} differs from grid {wgs[-1]} by " \
                                     f"{float((o.double() - base.double()).abs().max()):.3e}"
    return base


@pytest.mark.parametrize("kind,op,cfg", P.STEADY_CASES, ids=lambda v: str(v))
def test_steady_state(kind, op, cfg):
    """Every igemm_dma configuration with workgroups that own several tiles (module docstring)."""
    dev()
    ps = P.check_steady(kind, op, cfg)
    print(f"conv_plans steady {kind} op {op} cfg {cfg}: " + " | ".join(f"wgs {w}: {P.describe(p)}" for w, p in ps.items()))
    grids(f"steady {kind} op {op} cfg {cfg}", op, P.steady_geom(kind, op, cfg), P.steady_inputs(kind, op, cfg), cfg,
          P.IGEMM_DMA[cfg][0])


@pytest.mark.parametrize("name,cfg", P.STRIDE2_CASES, ids=lambda v: str(v))
def test_stride2_input_gradient(name, cfg):
    """Four phases per launch: different tap counts (nk 1, 2, 2, 4) and row counts, one with a tile or less; the
    ConvTranspose2d(2, 2) form with equal and ragged tile counts."""
    dev()
    ps = P.check_stride2(name, cfg)
    print(f"conv_plans stride2 {name} cfg {cfg}: " + " | ".join(f"wgs {w}: {P.describe(p)}" for w, p in ps.items()))
    grids(f"stride2 {name} cfg {cfg}", 1, P.stride2_geom(name), P.stride2_reference(name), cfg, P.IGEMM_DMA[cfg][0])


@pytest.mark.parametrize("op,cfg", P.SPLIT_CASES, ids=lambda v: str(v))
def test_two_source(op, cfg):
    """Two sources (forward) / two destinations (input gradient) under every choice the split entries can make."""
    dev()
    ps = P.check_split(op, cfg)
    print(f"conv_plans split op {op} cfg {cfg}: " + " | ".join(f"wgs {w}: {P.describe(p)}" for w, p in ps.items()))
    bm = P.IGEMM_DMA[cfg][0] if cfg > 0 else 128
    grids(f"split op {op} cfg {cfg}", op, P.split_geom(), P.split_reference(op), cfg, bm, P.SPLIT_AT)


@pytest.mark.parametrize("op,cfg", P.SPLIT_EQUAL_CASES, ids=lambda v: str(v))
def test_two_source_equal_counts(op, cfg):
    dev()
    p = P.check_split_equal(op, cfg)
    print(f"conv_plans split_equal op {op} cfg {cfg}: {P.describe(p)}")
    grids(f"split_equal op {op} cfg {cfg}", op, P.split_equal_geom(op), P.split_equal_reference(op), cfg, P.IGEMM_DMA[cfg][0],
          P.SPLIT_AT, wgs=(8, 0))


@pytest.mark.parametrize("cfg,op", P.ITEM_CASES, ids=lambda v: str(v))
def test_item_kernels(cfg, op):
    """conv3_halo64 / conv3_c16 / conv3_c16d: several row pairs and segments per image, workgroups of 2 to 6
    items whose range holds an image boundary."""
    dev()
    ps = P.check_item(cfg, op)
    print(f"conv_plans item cfg {cfg} op {op}: " + " | ".join(f"wgs {w}: {P.describe(p)}" for w, p in ps.items()))
    grids(f"item cfg {cfg} op {op}", op, P.item_geom(cfg), P.item_reference(cfg, op), cfg, ps[8].phase_bm[0])


@pytest.mark.parametrize("case", P.EQUAL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_equal_counts(case):
    """Every workgroup owns two tiles (the bucket the large production shapes fall into), against the default grid."""
    dev()
    p = P.check_equal(case)
    print(f"conv_plans equal {case}: {P.describe(p)}")
    grids(f"equal {case}", case[0], P.equal_geom(case), P.equal_reference(case), case[2], p.phase_bm[0], wgs=(case[3], 0))


FORCED_EQ = [("pick11", 0), ("pick2", 0), ("halo64", 0), ("halo64", 1), ("c16", 0), ("c16", 1), ("wd_3", 0), ("merge", 1)]


@pytest.mark.parametrize("name,op", FORCED_EQ, ids=lambda v: str(v))
def test_plan_choice_forced_is_the_same_launch(name, op):
    """cfg -1 and the cfg the plan reports for it: bitwise equal outputs (plan and launch share one decision)."""
    dev()
    _, _, (B, H, W, C, N, k, s, pd) = P.AUTO_CASES[name]
    g = P.geom(B, H, W, C, N, k, s, pd)
    p = P.plan(op, g, BF16, -1, 0, 0, 0)
    cfgs = {p.phase_cfg[i] for i in P.phases(p)}
    assert len(cfgs) == 1 and p.ksplit == 1, P.describe(p)
    cfg = cfgs.pop()
    pf = P.plan(op, g, BF16, cfg, 0, 0, 0)
    assert P.plan_class(op, pf, BF16) == P.plan_class(op, p, BF16)
    r = P.conv_reference(op, B, H, W, C, N, k, s, pd, "forced")
    bias = None if p.family == 5 else r["bias"]
    a = launch(op, g, r["src"], r["w"], bias, -1, 0)
    b = launch(op, g, r["src"], r["w"], bias, cfg, 0)
    assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all()), (name, op, cfg)
    ref = r["ref"] if bias is not None else r["ref"] - r["bias"].double()
    u = P.block_usage(a, ref, p.phase_bm[0])
    print(f"conv_plans forced {name} op {op} -> cfg {cfg} [{P.describe(p)}]: {u:.3f} of the bound")
    assert u <= 1.0


# what each AUTO case exists for: (form, field, value) read from the plan of the launch ops makes
AUTO_EXPECT = {
    "pick7": [("fwd", "cfg", 8)], "pick2": [("fwd", "cfg", 3)], "pick11": [("fwd", "cfg", 12)],
    "v2_phase": [("dgrad", "cfg", 0), ("dgrad", "np", 4)],
    "ksplit0": [("fwd", "ksplit", 6), ("dgrad", "ksplit", 3)], "ksplit1": [("fwd", "ksplit", 3), ("dgrad", "ksplit", 3)],
    "ksplit_dgrad": [("fwd", "ksplit", 3), ("dgrad", "ksplit", 8)],
    "wd_halo128": [("wgrad", "pick", 6), ("wgrad", "ragged", True)], "wd_halo64": [("wgrad", "pick", 5), ("wgrad", "ragged", True)],
    "wd_3": [("wgrad", "pick", 3), ("wgrad", "ragged", True)], "wd_2": [("wgrad", "pick", 2), ("wgrad", "ragged", True)],
    "wd_v2": [("wgrad", "pick", -1), ("wgrad", "ragged", True)],
    "halo64": [("fwd", "cfg", 20), ("dgrad", "cfg", 20)], "c16": [("fwd", "cfg", 21), ("dgrad", "cfg", 21)],
    "cat": [("fwd", "two", 64), ("dgrad", "two", 64), ("wgrad", "pick", 6)], "cat64": [("wgrad", "pick", 5)],
    "convT": [("fwd", "np", 4)],
}


def auto_plans(name):
    dt, ls = P.auto_launches(name)
    return {form: P.plan(op, g, dt, -1, 0, cs, ws) for form, op, g, cs, ws in ls}


def check_auto(name):
    plans = auto_plans(name)
    for form, field, want in AUTO_EXPECT.get(name, []):
        p = plans[form]
        got = {"cfg": p.phase_cfg[0], "np": p.n_problems, "ksplit": p.ksplit, "pick": p.wgrad_pick, "two": p.two_source,
               "ragged": p.wgrad_chunks > 1 and p.wgrad_last < p.wgrad_rpc}[field]
        assert got == want, (name, form, field, got, want, P.describe(p))
    if name == "v2_phase":     # phase (0, 0) alone would take igemm_dma; the tapless phases cannot, so all four run v2
        _, _, (B, H, W, C, N, k, s, pd) = P.AUTO_CASES[name]
        one = P.plan(0, P.geom(B, (H + 1) // 2, (W + 1) // 2, N, C, 1, 1, 0), BF16, 3, 0, 0, 0)
        assert one.phase_tiles[0] >= one.cus
    return plans


# conv entry -> (op, index of c_split among the arguments or None, index of ws_bytes or None)
CONV_ENTRIES = {"csu_conv2d_fwd": (0, None, None), "csu_conv2d_dgrad": (1, None, None), "csu_conv2d_fwd_ws": (0, None, 7),
                "csu_conv2d_dgrad_ws": (1, None, 7), "csu_conv2d_fwd_split": (0, 4, None), "csu_conv2d_dgrad_split": (1, 6, None),
                "csu_conv2d_wgrad": (2, None, None), "csu_conv2d_wgrad_oihw": (2, None, None),
                "csu_conv2d_wgrad_split_oihw": (2, 4, None), "csu_conv2d_ex": (None, None, None),
                "csu_conv2d_ex2": (None, None, None), "csu_conv2d_wgrad_ex": (None, None, None)}


def geom_key(g):
    return tuple(getattr(g, f) for f, _ in g._fields_)


class Recorder:
    """Stands in for csu.ops.lib(): passes every call on, noting (op, geometry, c_split, ws_bytes) of the conv launches."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name not in CONV_ENTRIES:
            return fn
        op, ics, iws = CONV_ENTRIES[name]
        assert op is not None, f"csu.ops launched {name}: a forced configuration"

        def call(*a):
            self.calls.append((op, geom_key(a[0]._obj), a[ics] if ics is not None else 0, a[iws] if iws is not None else 0))
            return fn(*a)
        return call


@pytest.mark.parametrize("name", list(P.AUTO_CASES), ids=str)
def test_heuristic_plan(name, monkeypatch):
    """The plans shape alone selects (cfg -1, default grid), through ops under autocast: the output and every
    gradient against fp64 autograd.  The conv launches csu.ops makes are recorded and must be the ones whose plans
    were checked (conv_plan_cases.ops_launches, which the CPU enumeration of the models relies on)."""
    import ctypes
    from csu import _lib, ops
    from test_gpu_kernels import assert_close
    d = dev()
    plans = check_auto(name)
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(ops, "lib", lambda: rec)
    for form, p in plans.items():
        print(f"conv_plans auto {name} {form}: {P.describe(p)}")
    entry, dtype, (B, H, W, C, N, k, s, pd) = P.AUTO_CASES[name]
    g = torch.Generator().manual_seed(len(name) * 131 + B + H + C + N)
    bias = torch.randn(C if entry == "conv_transpose2d" else N, generator=g) * 0.1
    if entry == "conv_transpose2d":    # (B, H, W, C) is the OUTPUT; weight (in = N, out = C, k, k)
        x = torch.randn(B, (H - k) // s + 1, (W - k) // s + 1, N, generator=g).to(dtype)
        w = torch.randn(N, C, k, k, generator=g) / (N * k * k) ** 0.5
    else:
        x = torch.randn(B, H, W, C, generator=g).to(dtype)
        w = torch.randn(N, C, k, k, generator=g) / (C * k * k) ** 0.5
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, bias))
    if entry == "conv_transpose2d":
        ref = torch.nn.functional.conv_transpose2d(x64.permute(0, 3, 1, 2), w64, b64, stride=s).permute(0, 2, 3, 1)
    else:
        ref = torch.nn.functional.conv2d(x64.permute(0, 3, 1, 2), w64, b64, stride=s, padding=pd).permute(0, 2, 3, 1)
    gy = torch.randn(ref.shape, generator=g).to(dtype)
    ref.backward(gy.double())
    xd, wd, bd = (t.to(d).requires_grad_(True) for t in (x, w, bias))
    with torch.autocast("cuda", dtype=BF16, enabled=dtype == BF16):
        if entry == "conv2d":
            y = ops.conv2d(xd, wd, bd, s, pd)
        elif entry == "conv_transpose2d":
            y = ops.conv_transpose2d(xd, wd, bd, s)
        else:
            ca = P.AUTO_SPLIT[name]
            xa, xb = xd[..., :ca].detach().contiguous().requires_grad_(True), xd[..., ca:].detach().contiguous().requires_grad_(True)
            y = ops.conv2d_cat(xa, xb, wd, bd, pd)
    y.backward(gy.to(d).to(y.dtype))
    torch.cuda.synchronize()
    dt, ls = P.auto_launches(name)
    want = sorted((op, geom_key(lg), cs, _lib.lib().csu_conv2d_workspace(op, ctypes.byref(lg), _lib.CSU_BF16) if ws is None and dt == BF16
                   else (ws or 0)) for _, op, lg, cs, ws in ls)
    assert sorted(rec.calls) == want, (name, rec.calls, want)
    dx = xd.grad if entry != "conv2d_cat" else torch.cat([xa.grad, xb.grad], -1)
    assert tuple(y.shape) == tuple(ref.shape)
    assert_close(y.float(), ref, dtype)
    assert_close(dx, x64.grad, dtype)
    assert_close(wd.grad, w64.grad, dtype)
    assert_close(bd.grad, b64.grad, dtype)
    if dtype == BF16:       # the kernels' own bounds on the same bf16 operands
        fw = S.bf16_usage(y, ref)
        print(f"conv_plans auto {name}: y {fw:.3f} of the bf16 bound")


WGRAD_CASES = ["wd_halo128", "wd_halo64", "wd_3", "wd_3_one", "wd_2", "wd_v2", "cat", "cat64"]


@pytest.mark.parametrize("name", WGRAD_CASES, ids=str)
def test_weight_gradient_picks(name):
    """Every weight-gradient pick (several chunks with a ragged last one, and one chunk), fp32 result on bf16
    operands against fp64 torch.nn.grad.conv2d_weight: rel-L2 < 1e-5 (fp32 accumulation of exact bf16 products)."""
    from csu import _lib, ops
    d = dev()
    entry, _, (B, H, W, C, N, k, s, pd) = P.AUTO_CASES[name]
    g = P.geom(B, H, W, C, N, k, s, pd)
    cs = P.AUTO_SPLIT.get(name, 0)
    p = P.plan(2, g, BF16, -1, 0, cs)
    print(f"conv_plans wgrad {name}: {P.describe(p)}")
    gen = torch.Generator().manual_seed(H * 7 + C + N)
    x = torch.randn(B, H, W, C, generator=gen).bfloat16()
    dy = torch.randn(B, g.OH, g.OW, N, generator=gen).bfloat16()
    ref_w = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (N, C, k, k), dy.double().permute(0, 3, 1, 2), s, pd)
    ref_b = dy.double().sum((0, 1, 2))
    L = _lib.lib()
    out = torch.full((N * k * k * C + N,), float("nan"), dtype=F32, device=d)
    work = torch.empty(max(int(p.wgrad_ws_bytes), 16), dtype=torch.uint8, device=d)
    xd, dyd = x.to(d), dy.to(d)
    st = torch.cuda.current_stream().cuda_stream
    if cs:
        xa, xb = xd[..., :cs].contiguous(), xd[..., cs:].contiguous()
        rc = L.csu_conv2d_wgrad_split_oihw(ctypes.byref(g), _lib.CSU_BF16, xa.data_ptr(), xb.data_ptr(), cs, dyd.data_ptr(),
                                           out.data_ptr(), work.data_ptr(), work.numel(), st)
    else:
        rc = L.csu_conv2d_wgrad_oihw(ctypes.byref(g), _lib.CSU_BF16, xd.data_ptr(), dyd.data_ptr(), C, out.data_ptr(),
                                     work.data_ptr(), work.numel(), st)
    assert rc == 0, L.csu_last_error_string()
    torch.cuda.synchronize()
    dw, db = out[:N * k * k * C].view(N, C, k, k).double().cpu(), out[N * k * k * C:].double().cpu()
    ew, eb = float((dw - ref_w).norm() / ref_w.norm()), float((db - ref_b).norm() / ref_b.norm())
    print(f"conv_plans wgrad {name}: dW {ew:.2e} db {eb:.2e} (bound 1e-5)")
    assert ew < 1e-5 and eb < 1e-5, (name, ew, eb)
