"""CPU checks of the stripe-attention launch plans (attn_plan_cases.py, csu_stripe_attn_plan): every plan
that the models select at their production batch sizes is one that a GPU test compares with a reference
(tests/test_gpu_attn_plans.py), the heuristic is pinned where its comment names its values, out-of-range
splits are refused, and the inputs of the plan cases leave the kernels half of the bf16 bound per row block."""
import ctypes

import pytest
import torch

import attn_plan_cases as P
import stress_inputs as S

F32, BF16, F64 = P.F32, P.BF16, P.F64
HALF = 0.5     # test_numeric_stress_inputs.py's rule: the inputs themselves use at most half of the bound


def _show(title, keys):
    print(title)
    for k in sorted(keys, key=str):
        print("   ", k)


def test_plan_function_matches_the_documented_formula():
    """sp = min(ceil(1024 / window-heads), ceil(roundup32(N) / 128)); even sp -> 8 waves, split sp / 2; a
    workgroup owns roundup32(ceil(npad / split)) rows; passes of 32 * waves."""
    seen_empty = False
    for shape, forced in P.PLAN_CASES:
        reso, idx, sw, cb, heads, B = shape
        N = P.shape_tokens(shape)
        npad = -(-N // 32) * 32
        nwin = reso * reso // N
        for split in (0, forced):
            p = P.plan(P.geometry(shape, split), B, BF16)
            sp = split or min(-(-1024 // (B * nwin * heads)), P.max_split(N))
            waves = 8 if sp % 2 == 0 else 4
            launched = sp // 2 if waves == 8 else sp
            rows = -(-(-(-npad // launched)) // 32) * 32
            assert (p.fwd.kernel, p.fwd.wm, p.fwd.sp, p.fwd.split, p.fwd.waves, p.fwd.rows) == \
                (1, 256 if N <= 256 else 512 if N <= 512 else 1024, sp, launched, waves, rows), (shape, split)
            own = [min(rows, npad - i * rows) for i in range(launched)]
            assert p.fwd.passes == max(-(-o // (32 * waves)) for o in own)
            ragged = any(o > 32 * waves and o % (32 * waves) for o in own)
            assert p.fwd.flags == (1 if ragged else 0) | (2 if min(own) <= 0 else 0)
            seen_empty = seen_empty or min(own) <= 0
            if N <= 512:
                assert (p.bwd.kernel, p.bwd.wm, p.bwd.waves) == (2, 128 if N <= 128 else 256 if N <= 256 else 512,
                                                                 8 if N > 256 else 4)
                assert p.lepe_kernel == 0 and p.lepe_nblk == B * nwin
            else:
                assert p.bwd.kernel == 1 and p.bwd.wm == 1024
                assert [getattr(p.bwd, f) for f in ("sp", "split", "waves", "rows", "passes", "flags")] == \
                    [getattr(p.fwd, f) for f in ("sp", "split", "waves", "rows", "passes", "flags")]
                assert p.lepe_kernel == p.wgrad_kernel and p.lepe_nblk == p.wgrad_nblk
    assert seen_empty


def test_empty_partner_plans_enumerated():
    """Every (N <= 1024, split) whose plan leaves a workgroup without rows, from the formula alone: only odd
    splits (4-wave workgroups); the heuristic reaches them (147..170 window-heads select sp 7, e.g. a 30 x 30
    full window with 16 heads at batch 10), and PLAN_SHAPES holds one such window."""
    from csu import ops
    empty = set()
    for N in range(1, 1025):
        npad = -(-N // 32) * 32
        for sp in range(1, P.max_split(N) + 1):
            launched = sp // 2 if sp % 2 == 0 else sp
            rows = -(-(-(-npad // launched)) // 32) * 32
            if (launched - 1) * rows >= npad:
                empty.add((N, sp))
    assert empty and all(sp % 2 for _, sp in empty)
    assert (900, 7) in empty and (784, 6) not in empty
    for reso in (28, 30, 31, 32):
        for sp in range(1, P.max_split(reso * reso) + 1):
            p = P.plan(ops.StripeGeometry(reso, 32, 1, [(reso, reso, 0)], 1.0, split=sp), 1, BF16)
            assert bool(p.fwd.flags & 2) == ((reso * reso, sp) in empty) == bool(p.bwd.flags & 2), (reso, sp)
    p = P.plan(ops.StripeGeometry(30, 512, 16, [(30, 30, 0)], 1.0), 10, BF16)
    assert p.fwd.sp == 7 and p.fwd.flags & 2 and p.bwd.flags & 2
    assert any(P.shape_tokens(s) == 900 and q == 7 for s, q in P.PLAN_CASES)


def test_tested_set_has_every_split():
    """T has every forward split 1 .. max at each LDS image size and every split of the split backward, and
    removing any one split from the case list loses a key."""
    T, _ = P.tested_keys()
    _show("tested plan keys", T)
    for wm, N in ((256, 256), (512, 512), (1024, 1024)):
        for sp in range(1, P.max_split(N) + 1):
            assert any(k[:4] == ("fwd", "window", wm, sp) for k in T), (wm, sp)
    for sp in range(1, 9):
        assert any(k[:4] == ("bwd", "window", 1024, sp) for k in T), sp
    # the multi-pass loops, a ragged trailing pass, both workgroup sizes
    for d in ("fwd", "bwd"):
        for waves in (4, 8):
            assert any(k[0] == d and k[1] == "window" and k[4] == waves and k[5] and k[6] & 1 for k in T), (d, waves)
            assert any(k[0] == d and k[1] == "window" and k[4] == waves and k[5] and not k[6] for k in T), (d, waves)
    # the kernels other files' cases reach: their keys are in T as well
    assert ("fwd", "streamed", 0, 0, 4, False, 0) in T and ("bwd", "streamed", 0, 0, 4, False, 0) in T
    for wm, waves in ((128, 4), (256, 4), (512, 8)):
        assert any(k[:3] == ("bwd", "fused-bwd", wm) and k[4] == waves for k in T), wm
    # an idle split partner (its first row at or past the padded window's end) runs in both directions
    for d in ("fwd", "bwd"):
        assert any(k[0] == d and k[1] == "window" and k[6] & 2 for k in T), d
    # PLAN_CASES alone supplies every split, and removing the forced cases of any one (WM, split) loses that
    # split's keys and no other
    wm_of = lambda shape: 256 if P.shape_tokens(shape) <= 256 else 512 if P.shape_tokens(shape) <= 512 else 1024
    K = P.forced_keys()
    pairs = sorted({(wm_of(s), q) for s, q in P.PLAN_CASES})
    assert pairs == [(wm, sp) for wm in (256, 512, 1024) for sp in range(1, P.max_split(wm) + 1)]
    for wm, sp in pairs:
        lost = K - P.forced_keys([(s, q) for s, q in P.PLAN_CASES if (wm_of(s), q) != (wm, sp)])
        assert any(k[:4] == ("fwd", "window", wm, sp) for k in lost), (wm, sp)
        assert all(k[2] == wm and k[3] == sp or k[1] == "fused-bwd" for k in lost), (wm, sp, lost)


def test_production_plans_are_tested():
    """Every plan a model stage selects at image 256 / 512 / 1024, split sizes (1, 2, 8, 8) and (1, 2, 7, 7)
    where the geometry allows them, per-GPU batch 1 .. 64, and the FULL_CONFIGS of test_gpu_train.py, is in T:
    a new heuristic or model size that selects an untested plan fails here."""
    T, TL = P.tested_keys()
    prod = P.production_launches()
    assert len(prod) >= 3 * 7 * 4 * 2
    missing, PK, PL = {}, set(), set()
    for name, geom, B, dt in prod:
        k, l = P.plan_keys(geom, B, dt)
        PK |= k
        PL |= l
        for key in (k - T) | (l - TL):
            missing.setdefault(key, name)
    _show("production plan keys", PK)
    _show("production LePE weight-gradient keys", PL)
    _show("tested LePE weight-gradient keys", TL)
    assert not missing, missing
    # the production set really holds the plans the small cases never select
    assert any(k[1] == "window" and k[5] for k in PK) and any(l[1] for l in PL)


def test_heuristic_is_pinned():
    """wsplit()'s comment: 512x512 gives 2 at stages 3 and 4 (the headline batch 16); 1024x1024 batch 4 gives 4
    at stage 3 and 8 at stage 4."""
    got = {}
    for img, B in ((512, 16), (1024, 4)):
        geoms = P.model_geometries(img, (1, 2, 8, 8))
        for stage, g in ((3, geoms[2]), (4, geoms[3])):
            p = P.plan(g, B, BF16)
            got[img, stage] = p.fwd.sp
            assert p.fwd.passes == 1 and p.fwd.kernel == 1
    assert got == {(512, 3): 2, (512, 4): 2, (1024, 3): 4, (1024, 4): 8}, got
    # the launches the issue of batch-dependent plans named
    assert P.plan(P.model_geometries(512, (1, 2, 8, 8))[2], 32, BF16).fwd.passes == 2
    p = P.plan(P.model_geometries(1024, (1, 2, 8, 8))[2], 16, BF16)
    assert (p.fwd.wm, p.fwd.sp, p.fwd.passes) == (512, 1, 4)
    p = P.plan(P.model_geometries(1024, (1, 2, 8, 8))[3], 16, BF16)
    assert (p.fwd.wm, p.fwd.sp, p.bwd.kernel, p.bwd.sp) == (1024, 4, 1, 4)


def test_natural_cases_select_their_plans():
    """The NATURAL_CASES reach their plans through B and heads alone (split 0)."""
    want = {(16, 256, 8, 128, BF16): dict(fwd=(256, 1, 4, 2), bwd=(2, 256), lepe=0),
            (24, 256, 8, 64, BF16): dict(fwd=(1024, 2, 8, 3), bwd=(1, 1024), lepe=1, tiles=6, flags=0),
            (16, 128, 4, 64, F32): dict(lepe=1, tiles=2, flags=0),
            (16, 128, 4, 128, F32): dict(lepe=1, tiles=4, flags=0),
            (14, 128, 4, 128, F32): dict(lepe=1, tiles=4, flags=3)}
    assert set(want) == set(P.NATURAL_CASES)
    for case, w in want.items():
        geom = P.natural_geometry(case)
        assert geom.split == 0
        p = P.plan(geom, case[3], case[4])
        if "fwd" in w:
            assert (p.fwd.wm, p.fwd.sp, p.fwd.waves, p.fwd.passes) == w["fwd"], case
            assert (p.bwd.kernel, p.bwd.wm) == w["bwd"], case
            if p.bwd.kernel == 1:
                assert (p.bwd.sp, p.bwd.waves, p.bwd.passes) == w["fwd"][1:], case
        else:
            assert p.fwd.kernel == 0 and p.bwd.kernel == 0
        assert p.lepe_kernel == w["lepe"], case
        if w["lepe"] == 1:
            assert (p.tiles_blk, p.wgrad_flags) == (w["tiles"], w["flags"]), case
            assert p.tile_rows * p.tiles_blk == p.rows_blk and p.wgrad_nblk == case[3] * -(-case[0] // p.rows_blk)
    p = P.plan(P.geometry(P.UNTILED_LEPE_CASE), P.UNTILED_LEPE_CASE[5], F32)
    assert (p.lepe_kernel, p.wgrad_kernel, p.tile_rows, p.tiles_blk) == (2, 2, 0, 0) and p.lepe_nblk == p.wgrad_nblk > 0
    order = P.natural_order(128)
    assert set(order) == set(range(P.NATURAL_DISTINCT)) and set(P.natural_order(64)) == set(order)
    assert all(order[:k] * (128 // k) != order for k in (1, 2, 4, 8, 16, 32, 64))      # no period


def test_bad_split_values_are_refused():
    from csu import _lib, ops
    L = _lib.lib()
    z = torch.zeros(1)
    for shape in [s for wm in P.PLAN_SHAPES for s in P.PLAN_SHAPES[wm]] + [(42, -1, 42, 64, 2, 1)]:
        top = P.max_split(P.shape_tokens(shape))
        for dt in (F32, BF16):
            for split, ok in ((0, True), (1, True), (top, True), (top + 1, False), (-1, False), (1 << 20, False)):
                a = P.geometry(shape, split).args(shape[5], [z], [z])
                plan = _lib.StripePlan()
                rc = L.csu_stripe_attn_plan(ctypes.byref(a), ops.dtype_code_of(dt), ctypes.byref(plan))
                assert (rc == 0) == ok, (shape, dt, split, rc)
                if not ok:
                    assert rc == -1 and b"split" in L.csu_last_error_string()
                    # the launches refuse it the same way, before any device work (null buffers come later)
                    assert L.csu_stripe_attn_fwd(ctypes.byref(a), ops.dtype_code_of(dt), None, None, None, None) == -1
                    assert b"split" in L.csu_last_error_string()
                    assert L.csu_stripe_attn_bwd(ctypes.byref(a), ops.dtype_code_of(dt), None, None, None, None, None,
                                                 None, None, 0, None) == -1
                    assert b"split" in L.csu_last_error_string()
    # ignored where no split kernel runs: the fp32 plan is the same with and without it
    s = (24, -1, 24, 64, 2, 1)
    assert P.plan_keys(P.geometry(s, 3), 1, F32) == P.plan_keys(P.geometry(s), 1, F32)
    with pytest.raises(_lib.CsuError):
        P.plan(P.geometry(s, 6), 1, BF16)


def test_workspace_and_nblk_agree_with_the_plan():
    from csu import _lib, ops
    L = _lib.lib()
    z = torch.zeros(1)
    for name, geom, B, dt in P.tested_launches():
        nb = len(geom.branches)
        a = geom.args(B, [z] * nb, [z] * nb)
        p = P.plan(geom, B, dt)
        assert L.csu_stripe_lepe_nblk(ctypes.byref(a), ops.dtype_code_of(dt)) == p.lepe_nblk, name
        assert L.csu_stripe_attn_bwd_workspace(ctypes.byref(a)) == nb * p.ws_blocks * geom.heads * 32 * 10 * 4, name
        assert p.ws_blocks >= max(p.lepe_nblk, p.wgrad_nblk), name


def _shapes():
    return [s for wm in (256, 512, 1024) for s in P.PLAN_SHAPES[wm]] + [P.FOUR_WINDOWS[0]]


@pytest.mark.parametrize("shape", _shapes(), ids=str)
def test_inputs_leave_half_of_the_bound_per_block(shape):
    """Precondition of the per-block criterion: the bf16 emulation (stress_inputs.attn_eval, emulate_bf16)
    against fp64 uses at most half of the bf16 bound in every (image, window, head, 32-row block) group."""
    inp, ref = P.plan_reference(shape)
    emu = S.attn_eval(inp, shape, F32, emulate_bf16=True)
    figs = P.case_figs(emu, ref, shape)
    for k, v in figs.items():
        print(f"  {shape} {k}: {v:.3f} of the bound")
    assert all(v <= HALF for v in figs.values()), figs
    # the vectorised figures of the large batches are by_kind's
    fast = P.case_figs(emu, ref, shape, use_by_kind=False)
    for k in ("out", "dq", "dk", "dv"):
        assert abs(fast[k] - figs[k]) <= 1e-9 * max(1.0, figs[k]), (k, fast[k], figs[k])


@pytest.mark.parametrize("case", P.DROP_CASES, ids=str)
def test_dropout_inputs_leave_half_of_the_bound_per_block(case):
    """The same under attention dropout (a CPU mask of the same rate stands in for the device's)."""
    shape, _ = case
    inp, _ = P.plan_reference(shape)

    def mask(shp):
        return (torch.rand(shp, generator=torch.Generator().manual_seed(11)) >= P.DROP_P).double() / (1 - P.DROP_P)

    ref = P.oracle_eval(inp, shape, attn_mask=mask)
    emu = S.attn_eval(inp, shape, F32, emulate_bf16=True, attn_mask=mask)
    figs = P.case_figs(emu, ref, shape)
    for k, v in figs.items():
        print(f"  dropout {shape} {k}: {v:.3f} of the bound")
    assert all(v <= HALF for v in figs.values()), figs


@pytest.mark.parametrize("t", P.TWO_BRANCH_CASES, ids=lambda t: f"reso{t['reso']}")
def test_two_branch_inputs_leave_half_of_the_bound_per_block(t):
    inp = P.two_branch_inputs(t)
    figs = P.two_branch_figs(t, P.two_branch_eval(inp, F32, emulate_bf16=True), P.two_branch_eval(inp))
    for k, v in figs.items():
        print(f"  two-branch reso {t['reso']} {k}: {v:.3f} of the bound")
    assert all(v <= HALF for v in figs.values()), figs


@pytest.mark.parametrize("case", [c for c in P.NATURAL_CASES if c[4] == BF16], ids=str)
def test_natural_inputs_leave_half_of_the_bound_per_block(case):
    reso, cb, heads, B, dtype = case
    inp, ref, order = P.natural_reference(case)
    shape = (reso, -1, reso, cb, heads, P.NATURAL_DISTINCT)
    emu = S.attn_eval(inp, shape, F32, emulate_bf16=True)
    figs = P.block_figs(emu, ref, P.block_ids(P.NATURAL_DISTINCT, reso, reso, reso, heads), cb, heads, use_by_kind=False)
    count = torch.bincount(torch.tensor(order), minlength=P.NATURAL_DISTINCT).double()
    per = [S.attn_eval(dict(inp, qkv=inp["qkv"][i:i + 1], gout=inp["gout"][i:i + 1]), shape[:5] + (1,), F32, emulate_bf16=True)
           for i in range(P.NATURAL_DISTINCT)]
    figs["dW_lepe"] = S.usage(sum(c * e[2] for c, e in zip(count, per)), ref[2], BF16)
    figs["db_lepe"] = S.usage(sum(c * e[3] for c, e in zip(count, per)), ref[3], BF16)
    for k, v in figs.items():
        print(f"  natural {case[:4]} {k}: {v:.3f} of the bound")
    assert all(v <= HALF for v in figs.values()), figs


def test_one_wrong_row_block_is_not_averaged_away():
    """Why the criterion is applied per row block: ONE 32-row block of one head off by 2.5 % (a wrong softmax
    normaliser in one pass, say) passes assert_close over the whole tensor -- max-abs within 3 % of the largest
    value, the L2 error diluted by the other blocks -- and fails the per-block figure."""
    shape = (32, -1, 32, 64, 2, 2)
    inp, ref = P.plan_reference(shape)
    emu = S.attn_eval(inp, shape, F32, emulate_bf16=True)
    out, dq = emu[0].clone(), emu[1].clone()
    out[1, 128:160, 32:] *= 1.025          # full window: rows are window positions; head 1
    dq[1, 128:160, 32:64] *= 1.025
    bad = (out, dq, emu[2], emu[3])
    assert S.usage(out, ref[0], BF16) < 1 and S.usage(dq, ref[1], BF16) < 1
    figs = P.case_figs(bad, ref, shape)
    assert figs["out"] > 1 and figs["dq"] > 1 and figs["dk"] <= HALF and figs["dv"] <= HALF, figs


def test_existing_cases_plan_table():
    """The plans of the attention cases the suite had before (printed: the table of the pull request): in
    every whole-window launch among them a wave makes one pass."""
    rows = {}
    for name, geom, B, dt in P.existing_cases():
        if dt != BF16:
            continue
        p = P.plan(geom, B, dt)
        rows[name] = (P.describe(p.fwd), P.describe(p.bwd), P.LEPE_NAMES[p.lepe_kernel], p.tiles_blk)
        if p.fwd.kernel == 1:
            assert p.fwd.passes == 1 and p.fwd.sp == P.max_split(geom.branches[0][0] * geom.branches[0][1]), name
        if p.bwd.kernel == 1:
            assert p.bwd.passes == 1, name
        assert p.tiles_blk <= 1, name
    for name, r in rows.items():
        print(f"{name}: fwd {r[0]} | bwd {r[1]} | LePE {r[2]}, {r[3]} tiles per block")
