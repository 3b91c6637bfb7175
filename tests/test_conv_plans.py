"""CPU checks of the convolution launch plans (conv_plan_cases.py, csu_conv2d_plan): the GPU cases meet the
conditions they exist for, every plan class the two models select at image 256 / 512 / 1024 and batch 1 to 64 is
one tests/test_gpu_conv_plans.py runs against fp64, the heuristics' thresholds are pinned, bad arguments are
refused by the plan and the launch alike, and the inputs leave half of the bound.  Needs the built library, no GPU."""
import ctypes

import pytest
import torch

import conv_plan_cases as P

BF16, F32 = torch.bfloat16, torch.float32


def test_forced_cases_meet_their_conditions():
    for c in P.STEADY_CASES:
        P.check_steady(*c)
    for c in P.STRIDE2_CASES:
        P.check_stride2(*c)
    for c in P.SPLIT_CASES:
        P.check_split(*c)
    for c in P.SPLIT_EQUAL_CASES:
        P.check_split_equal(*c)
    for c in P.ITEM_CASES:
        P.check_item(*c)
    for c in P.EQUAL_CASES:
        P.check_equal(c)
    # every persistent kernel and configuration: >= 3 tiles on a workgroup, unequal counts, XCD remainder
    seen = set()
    for name, op, g, dt, cfg, w, cs in P.forced_launches():
        p = P.plan(op, g, dt, cfg, w, cs, 0)
        if p.family >= 2 and p.wg_tiles_max >= 3 and p.wg_tiles_max != p.wg_tiles_min and p.phase_xcd_rem[0]:
            seen.add((p.family, p.phase_cfg[0], op))
    want = {(2, cfg, op) for cfg in P.IGEMM_DMA for op in (0, 1)} | {(3, 20, 0), (3, 20, 1), (4, 21, 0), (5, 21, 1)}
    assert want <= seen, sorted(want - seen)


def test_auto_cases_select_their_plans():
    import test_gpu_conv_plans as G
    for name in P.AUTO_CASES:
        G.check_auto(name)
    assert set(G.AUTO_EXPECT) <= set(P.AUTO_CASES) and set(G.WGRAD_CASES) <= set(P.AUTO_CASES)
    import exact_inputs as E
    ks = [P.AUTO_CASES[n][2] for n in ("ksplit0", "ksplit1")]
    assert [(B, H, C, N, k, s, p) for B, H, W, C, N, k, s, p in ks] == list(E.CONV_KSPLIT_CASES)


def test_every_model_plan_class_is_tested():
    """A heuristic or model size that selects a plan class no GPU case has fails here, without a GPU."""
    from csu import _lib
    tested = P.tested_classes()
    missing, refused, seen, big = {}, 0, {}, 0
    for model in ("unet", "cswin"):
        for img in (256, 512, 1024):
            for B in range(1, 65):
                for dt in (BF16, F32):
                    for name, form, op, g, cs, ws in P.model_launches(model, img, B, dt):
                        if P.operand_bytes(g, dt) >= 2 ** 31:     # beyond 32-bit byte offsets: the bf16 kernels refuse or
                            big += 1                              # fall back to 64-bit ones; such operands are not tested
                            continue
                        try:
                            p = P.plan(op, g, dt, -1, 0, cs, ws)
                        except _lib.CsuError as e:       # the launch refuses the same way (operands above 2 GiB)
                            assert "2 GiB" in str(e) or "2^31" in str(e), (name, form, str(e))
                            refused += 1
                            continue
                        c = P.plan_class(op, p, dt)
                        seen.setdefault(c, f"{name} {form}")
                        if c not in tested:
                            missing.setdefault(c, f"{name} {form}: {P.describe(p)}")
    if missing:
        print("plan classes of the models (class: first launch / GPU case):")
        for c in sorted(seen, key=str):
            print(f"  {c}: {seen[c]} / {tested.get(c, 'UNTESTED')}")
    assert not missing, missing
    assert len(seen) > 40 and big > 0


def test_model_enumeration_reads_the_models():
    u = {n: a for n, _, a, _, _ in P.unet_convs(512, 16)}
    assert u["inc.c2"] == (16, 512, 512, 64, 64, 3, 1, 1) and u["down4.c1"] == (16, 32, 32, 512, 1024, 3, 1, 1)
    assert u["up1.up"] == (16, 64, 64, 512, 1024, 2, 2, 0) and u["up4.c1"] == (16, 512, 512, 128, 64, 3, 1, 1)
    assert len(u) == 23 and {n: c for n, _, _, c, _ in P.unet_convs(512, 16)}["up4.c1"] == 64
    c = {n: a for n, _, a, _, _ in P.cswin_convs(512, 16)}
    assert c["embed"] == (16, 512, 512, 3, 64, 7, 4, 2) and c["merge1"] == (16, 128, 128, 64, 128, 3, 2, 1)
    assert c["upsample4.encoder"] == (16, 16, 16, 128, 36, 3, 1, 1) and c["upsample1.encoder"] == (16, 128, 128, 16, 144, 3, 1, 1)
    assert len(c) == 8


def test_heuristic_thresholds_are_pinned():
    """id_pick's `>= id_cus()` thresholds, the `single` rule of configuration 11, wd_pick's order."""
    cus = P.plan(0, P.geom(1, 8, 8, 64, 64, 1), BF16).cus
    assert cus == 256

    def fwd_cfg(rows, n, **kw):      # 1x1 conv over `rows` pixels (one image row)
        p = P.plan(0, P.geom(1, 1, rows, 64, n, 1), BF16, ws_bytes=0, **kw)
        return p.phase_cfg[0]
    # configuration 7: ceil(M / 256) * (N / 256) >= CUs
    assert fwd_cfg(63 * 256 + 1, 1024) == 8 and fwd_cfg(63 * 256, 1024) != 8
    # configuration 2: ceil(M / 256) * (N / 128) >= CUs, N % 256 != 0 or too few 256-wide tiles
    assert fwd_cfg(51 * 256 + 1, 640) == 3 and fwd_cfg(51 * 256, 640) == 12
    assert fwd_cfg(63 * 256 + 1, 512) == 3 and fwd_cfg(63 * 256, 512) == 12
    # configuration 11: one problem only, ceil(M / 64) * (N / 128) >= CUs
    assert fwd_cfg(51 * 64 + 1, 640) == 12 and fwd_cfg(51 * 64, 640) == 0
    g2 = P.geom(1, 2 * 58, 2 * 58, 640, 64, 2, 2, 0)        # four phases of 58 x 58 rows each: never 11
    p = P.plan(1, g2, BF16)
    assert p.n_problems == 4 and [p.phase_cfg[i] for i in range(4)] == [0] * 4
    assert P.plan(0, P.geom(1, 58, 58, 64, 640, 1), BF16).phase_cfg[0] == 12
    # N = 64 and gathered channels % 64 != 0 stay on v2
    assert fwd_cfg(1 << 16, 64) == 0
    assert P.plan(0, P.geom(1, 1, 1 << 16, 32, 256, 1), BF16, ws_bytes=0).phase_cfg[0] == 0
    # wd_pick: halo 128, halo 64, 256 x 128 tile, 128 x 128 2-stage tile, v2 -- in this order
    def pick(*a, **kw):
        return P.plan(2, P.geom(*a, **kw), BF16).wgrad_pick
    assert pick(1, 8, 64, 64, 256, 3) == 6 and pick(1, 8, 64, 64, 192, 3) == 5 and pick(1, 8, 64, 64, 64, 3) == 5
    assert pick(1, 8, 32, 64, 256, 3) == 3 and pick(1, 8, 64, 64, 384, 1) == 3
    assert pick(1, 8, 32, 64, 128, 3) == 2 and pick(1, 8, 32, 128, 128, 3) == -1
    assert pick(1, 8, 32, 16, 144, 3) == 2 and pick(1, 8, 32, 8, 64, 3) == -1 and pick(1, 8, 32, 8, 64, 7, 4, 2) == 2
    assert pick(1, 8, 32, 64, 320, 3) == -1 and pick(1, 8, 32, 64, 64, 3) == -1
    assert P.plan(2, P.geom(1, 8, 64, 64, 256, 3), F32).wgrad_pick == -1


def _rc(op, g, dt=BF16, cfg=-1, wgs=0, cs=0, ws=0):
    from csu import _lib, ops
    L = _lib.lib()
    p = _lib.ConvPlan()
    rc = L.csu_conv2d_plan(op, ctypes.byref(g), ops.dtype_code_of(dt), cfg, wgs, cs, ws, ctypes.byref(p))
    return rc, L.csu_last_error_string()


def test_refusals():
    from csu import _lib, ops
    L = _lib.lib()
    g = P.steady_geom("k3", 0, 1)
    # wgs: a positive multiple of 8 or 0; the launch refuses it the same way, before any device work
    for wgs, ok in ((0, True), (8, True), (16, True), (512, True), (65536, True), (4, False), (12, False), (-8, False),
                    (65544, False), (1 << 20, False)):
        for op in (0, 1, 2):
            rc, msg = _rc(op, g, wgs=wgs)
            assert (rc == 0) == ok, (op, wgs, rc)
            if not ok:
                assert rc == -1 and b"wgs" in msg
        if not ok:
            for op in (0, 1):
                assert L.csu_conv2d_ex2(op, ctypes.byref(g), _lib.CSU_BF16, None, None, None, None, None, 0, 1, wgs, None, 0,
                                        None) == -1
                assert b"wgs" in L.csu_last_error_string() or b"null" in L.csu_last_error_string()
    # ineligible forced configurations
    assert _rc(0, g, cfg=13)[0] == -1 and _rc(0, g, cfg=20)[0] == -1 and _rc(0, g, cfg=21)[0] == -1
    assert _rc(0, P.geom(1, 8, 8, 64, 64, 3), cfg=1)[0] == -1             # 64 columns, BN 128
    assert _rc(0, P.geom(1, 8, 8, 32, 128, 3), cfg=1)[0] == -1            # 32 gathered channels
    assert _rc(0, P.geom(1, 8, 8, 64, 2048, 1), cfg=8)[0] == -1           # more columns than the LDS bias copy
    assert _rc(0, P.geom(1, 7, 64, 64, 64, 3), cfg=20)[0] == -1           # halo64 needs H even
    assert _rc(0, P.geom(1, 8, 32, 16, 144, 3), cfg=21)[0] == -1          # c16 needs W % 64 == 0
    assert _rc(0, g, dt=F32, cfg=1)[0] == -1 and _rc(1, g, dt=F32, cfg=1)[0] == -1
    assert _rc(2, g, cfg=8)[0] == -1 and _rc(2, P.geom(1, 8, 32, 64, 64, 3), cfg=6)[0] == -1
    assert _rc(3, g)[0] == -1
    # two sources: only where csu_conv2d_split_ok
    sg = P.split_geom()
    assert _rc(0, sg, cs=64)[0] == 0 and _rc(0, sg, cs=32)[0] == -2 and _rc(0, sg, dt=F32, cs=64)[0] == -2
    assert _rc(1, g, cs=64)[0] == -2 and _rc(2, g, cs=64)[0] == -2
    # the 2 GiB limits (32-bit buffer offsets): input, output, weight
    big = P.geom(64, 1024, 1024, 64, 64, 3)
    for op in (0, 1):
        rc, msg = _rc(op, big)
        assert rc == -2 and b"2 GiB" in msg
    assert _rc(0, P.geom(16, 512, 512, 64, 64, 3))[0] == 0                # 512 MiB: the flagship's largest
    assert _rc(0, P.geom(32, 512, 512, 64, 64, 3))[0] == 0 and _rc(0, P.geom(64, 512, 512, 64, 64, 3))[0] == -2
    assert _rc(0, P.geom(1, 64, 64, 64, 1024, 1), cfg=8)[0] == 0
    pb = P.plan(2, big, BF16)                                             # the weight gradient falls back to 64-bit offsets
    assert _rc(2, big)[0] == 0 and (pb.wgrad_pick, pb.wgrad_v2) == (-1, 3)
    assert P.plan(2, P.geom(1, 8, 32, 64, 64, 3), BF16).wgrad_v2 == 1 and P.plan(2, P.geom(1, 8, 32, 64, 36, 3), BF16).wgrad_v2 == 2
    assert P.plan(2, P.geom(1, 8, 32, 64, 1, 1), BF16).wgrad_v2 == 3 and P.plan(2, P.geom(1, 8, 32, 4, 64, 3), BF16).wgrad_v2 == 4
    assert P.plan(2, P.geom(1, 8, 32, 64, 64, 3), F32).wgrad_v2 == 5 and P.plan(2, P.geom(1, 8, 32, 4, 64, 3), F32).wgrad_v2 == 6
    assert P.plan(2, P.geom(1, 8, 64, 64, 64, 3), BF16).wgrad_v2 == 0


def test_plan_reports_the_workspace_the_entries_report():
    from csu import _lib
    L = _lib.lib()
    for name in P.AUTO_CASES:
        dt, ls = P.auto_launches(name)
        for form, op, g, cs, ws in ls:
            if op == 2 and dt == BF16:
                assert P.plan(2, g, dt, -1, 0, cs).wgrad_ws_bytes <= L.csu_conv2d_wgrad_workspace(ctypes.byref(g))
            elif op != 2 and ws is None and dt == BF16:
                n = L.csu_conv2d_workspace(op, ctypes.byref(g), _lib.CSU_BF16)
                p = P.plan(op, g, dt, -1, 0, 0, n)
                assert (p.ksplit > 1) == (n > 0), (name, form)
                if n:
                    assert n == p.ksplit * p.phase_rows[0] * (g.N if op == 0 else g.C) * 4
                    assert P.plan(op, g, dt, -1, 0, 0, n - 1).ksplit == 1     # a smaller workspace runs unsplit


def test_inputs_leave_half_of_the_bound():
    """The reference path alone -- the fp64 result rounded to bf16, the best any kernel can return -- uses at most
    half of the per-block criterion on the forced cases' inputs (tests/test_numeric_stress_inputs.py's rule)."""
    refs = [(P.steady_reference(kind, op, h)["ref"], 64) for kind in P.STEADY_KINDS for op in (0, 1) for h in (37,)]
    refs += [(P.stride2_reference("thin")["ref"], 64), (P.item_reference(20, 0)["ref"], 64), (P.item_reference(21, 1)["ref"], 64)]
    for ref, bm in refs:
        u = P.block_usage(ref.bfloat16(), ref, bm)
        assert u <= 0.5, u
        assert P.block_usage(ref.bfloat16() * 1.01, ref, bm) > 1.0      # and the criterion is not slack: 1 % is caught
