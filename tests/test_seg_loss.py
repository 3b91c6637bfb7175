"""csu.losses on the CPU: SegLoss (BCE + Tversky / Dice family) against an fp64 restatement of its
formula, its relation to the Dice metric and the per-step sums of csu.train, the constructor's
checks, and the three csu_seg_loss_* C-ABI entry points.

The fp64 restatement (``ref_loss_grad``) is shared with tests/test_gpu_seg_loss.py.  Tolerances:
loss rtol 1e-5 (the project's BCE tolerance, test_bce_loss_vs_torch); gradient rtol 2e-6 with atol
1e-7 * max|g_ref| -- torch's fp32 composition of the formula measured against fp64 at these shapes
is within 1.9e-7 (gradient) / 7.4e-8 (loss) relative, ten times that allows another summation order."""
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (bce, tversky, alpha, beta, pos_weight)
PARAM_SETS = [(1.0, 0.0, 0.5, 0.5, 1.0), (0.0, 1.0, 0.5, 0.5, 1.0), (0.5, 1.0, 0.3, 0.7, 3.5), (1.0, 1.0, 1.0, 0.0, 1.0)]
SMOOTH = 0.5
UPSTREAM = 0.37
LOSS_RTOL = 1e-5
GRAD_RTOL = 2e-6
GRAD_ATOL_REL = 1e-7


def make_criterion(ps, per_sample, smooth=SMOOTH):
    from csu.losses import SegLoss
    bce, tv, alpha, beta, pw = ps
    return SegLoss(bce=bce, tversky=tv, alpha=alpha, beta=beta, smooth=smooth, pos_weight=pw, per_sample=per_sample)


def ref_loss_grad(p32, t32, ps, per_sample, smooth=SMOOTH, upstream=UPSTREAM):
    """fp64 loss and d(upstream * loss)/dp of fp32 inputs (upcast here: an fp64 input rounded to fp32
    would move 1 - p by percents near p = 1).  The Tversky part is differentiated by autograd; the
    BCE part by ATen's closed form (p (1 - t) - pos_weight t (1 - p)) / max(p (1 - p), 1e-12) / n, which is what
    nn.BCELoss back-propagates where the forward log is clamped at -100 (autograd of a clamped
    log would give 0 there)."""
    bce, tv, alpha, beta, pw = ps
    p = p32.detach().double().requires_grad_(True)
    t = t32.detach().double()
    rows = p.shape[0] if per_sample else 1
    pr, tr = p.reshape(rows, -1), t.reshape(rows, -1)
    tp, sp, st = (pr * tr).sum(1), pr.sum(1), tr.sum(1)
    ti = (tp + smooth) / ((1.0 - alpha - beta) * tp + alpha * sp + beta * st + smooth)
    tversky = (1.0 - ti).mean()
    (g_tv,) = torch.autograd.grad(tversky, p)
    with torch.no_grad():
        pd = p.detach()
        lp, lq = torch.log(pd).clamp_min(-100.0), torch.log1p(-pd).clamp_min(-100.0)
        bce_mean = (-(pw * t * lp + (1.0 - t) * lq)).sum() / pd.numel()
        g_bce = (pd * (1.0 - t) - pw * t * (1.0 - pd)) / (pd * (1.0 - pd)).clamp_min(1e-12) / pd.numel()
        loss = bce * bce_mean + tv * tversky.detach()
        grad = upstream * (bce * g_bce + tv * g_tv)
    return loss, grad


def check_grad(g, g_ref, mask=None):
    """rtol 2e-6, atol 1e-7 * max|g_ref| (the maximum over `mask` when given)."""
    scale = float((g_ref[mask] if mask is not None else g_ref).abs().max())
    torch.testing.assert_close(g.double().cpu(), g_ref, rtol=GRAD_RTOL, atol=GRAD_ATOL_REL * scale)


def _inputs(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(shape, generator=g) * 0.998 + 0.001
    t = (torch.rand(shape, generator=g) > 0.6).float()
    return p, t


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("ps", PARAM_SETS)
@pytest.mark.parametrize("shape", [(3, 1, 37, 41), (1, 1, 5, 3)])
def test_cpu_path_vs_fp64(shape, ps, per_sample):
    p, t = _inputs(shape)
    crit = make_criterion(ps, per_sample)
    pa = p.clone().requires_grad_(True)
    loss = crit(pa, t)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (loss * UPSTREAM).backward()
    ref, gref = ref_loss_grad(p, t, ps, per_sample)
    torch.testing.assert_close(loss.detach().double(), ref, rtol=LOSS_RTOL, atol=0)
    check_grad(pa.grad, gref)


def test_reference_closed_form_bce_gradient_is_autograd_away_from_clamps():
    """The closed-form BCE gradient of ref_loss_grad equals fp64 autograd of the whole formula on
    probabilities away from 0 and 1 (where no clamp acts)."""
    ps, smooth = PARAM_SETS[2], SMOOTH
    bce, tv, alpha, beta, pw = ps
    p32, t32 = _inputs((3, 1, 37, 41), seed=1)
    _, gref = ref_loss_grad(p32, t32, ps, True)
    p = p32.double().requires_grad_(True)
    t = t32.double()
    pr, tr = p.reshape(3, -1), t.reshape(3, -1)
    tp, sp, st = (pr * tr).sum(1), pr.sum(1), tr.sum(1)
    ti = (tp + smooth) / ((1.0 - alpha - beta) * tp + alpha * sp + beta * st + smooth)
    loss = bce * (-(pw * t * torch.log(p) + (1 - t) * torch.log1p(-p))).mean() + tv * (1.0 - ti).mean()
    (loss * UPSTREAM).backward()
    torch.testing.assert_close(p.grad, gref, rtol=1e-12, atol=1e-18)


@pytest.mark.parametrize("s", [1e-6, 1.0])
def test_dice_loss_is_one_minus_dice_metric(s):
    from csu.losses import dice_loss
    from csu.train import _dice_t
    p, t = _inputs((3, 1, 37, 41), seed=2)
    p, t = p.double(), t.double()
    crit = dice_loss(smooth=s)
    assert (crit.bce, crit.tversky, crit.alpha, crit.beta, crit.smooth) == (0.0, 1.0, 0.5, 0.5, s / 2)
    loss, _ = ref_loss_grad(p, t, (0.0, 1.0, 0.5, 0.5, 1.0), False, smooth=crit.smooth)
    torch.testing.assert_close(1.0 - loss, _dice_t(p, t, s), rtol=1e-14, atol=1e-15)
    # and the fp32 CPU path itself, to fp32 rounding
    torch.testing.assert_close(1.0 - crit(p.float(), t.float()).double(), _dice_t(p, t, s), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("per_sample", [False, True])
def test_loss_stats_sums_equal_step_stats(per_sample):
    from csu.losses import bce_dice_loss
    from csu.train import _step_stats
    p, t = _inputs((3, 1, 37, 41), seed=3)
    crit = bce_dice_loss(per_sample=per_sample)
    loss, stats = crit.loss_stats(p, t)
    assert stats.shape == (3,) and not stats.requires_grad
    assert torch.equal(loss, crit(p, t))
    assert torch.equal(stats.double(), _step_stats(loss, p, t)[1:])


def test_runs_in_fp32_under_autocast():
    from csu.losses import bce_dice_loss
    p, t = _inputs((2, 1, 8, 8), seed=4)
    crit = bce_dice_loss()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        a = crit(p.bfloat16(), t.bfloat16())
    assert a.dtype == torch.float32
    assert torch.equal(a, crit(p.bfloat16().float(), t.bfloat16().float()))


@pytest.mark.parametrize("kw", [dict(bce=-1.0), dict(tversky=-0.5), dict(alpha=-0.1), dict(beta=-0.1), dict(pos_weight=-2.0),
                                dict(smooth=0.0), dict(smooth=-1.0), dict(bce=0.0, tversky=0.0), dict(bce=float("nan")),
                                dict(smooth=float("nan")), dict(alpha=float("inf"))])
def test_constructor_rejects(kw):
    from csu.losses import SegLoss
    with pytest.raises(ValueError):
        SegLoss(**kw)


def test_shape_mismatch_rejected():
    from csu.losses import SegLoss
    with pytest.raises(ValueError):
        SegLoss()(torch.rand(2, 1, 4, 4), torch.rand(2, 1, 4, 5))


def test_instances_are_dict_keys_and_exported():
    import csu
    from csu.losses import SegLoss, bce_dice_loss, dice_loss, tversky_loss
    a, b = SegLoss(), SegLoss()
    d = {a: 1, b: 2}
    assert d[a] == 1 and d[b] == 2 and a != b and hash(a) == hash(a)
    assert ("train", (1,), a) != ("train", (1,), b)
    for f in (bce_dice_loss, dice_loss, tversky_loss):
        assert isinstance(f(), SegLoss) and hasattr(f(), "loss_stats")
    tv = tversky_loss(0.2, 0.8)
    assert (tv.bce, tv.alpha, tv.beta) == (0.0, 0.2, 0.8)
    assert csu.SegLoss is SegLoss and csu.dice_loss is dice_loss and csu.bce_dice_loss is bce_dice_loss
    assert csu.tversky_loss is tversky_loss


def test_abi_declares_and_exports_seg_loss():
    from csu import _lib
    src = open(os.path.join(REPO, "include", "csu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for n in ("csu_seg_loss_workspace", "csu_seg_loss_fwd", "csu_seg_loss_bwd"):
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(L, n) and n in _lib._SIGS, n
    assert len(_lib._SIGS["csu_seg_loss_fwd"][1]) == 16 and len(_lib._SIGS["csu_seg_loss_bwd"][1]) == 11
    # 6 partial sums per (row, chunk) item; a bad (n, rows) needs no workspace
    assert L.csu_seg_loss_workspace(15, 1) == 24 and L.csu_seg_loss_workspace(64 * 33, 33) == 33 * 24
    assert L.csu_seg_loss_workspace(16 * 512 * 512, 1) == 1024 * 24
    assert L.csu_seg_loss_workspace(10, 3) == 0 and L.csu_seg_loss_workspace(0, 1) == 0


def test_abi_rejects_bad_arguments_on_the_host():
    """Every bad argument is refused with CSU_E_ARG and a message before any launch (no device
    memory is touched: the pointers here are dummies that a launch would fault on)."""
    import ctypes
    from csu import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(n=16, rows=2, w_bce=1.0, pw=1.0, w_tv=1.0, alpha=0.5, beta=0.5, smooth=0.5)
    bad = [dict(n=0), dict(rows=0), dict(n=15), dict(smooth=0.0), dict(smooth=-1.0), dict(w_bce=-1.0), dict(w_tv=-1.0),
           dict(alpha=-0.5), dict(beta=-0.5), dict(pw=-1.0), dict(w_bce=0.0, w_tv=0.0)]
    for b in bad:
        a = dict(ok, **b)
        rc = L.csu_seg_loss_fwd(a["n"], a["rows"], q, q, a["w_bce"], a["pw"], a["w_tv"], a["alpha"], a["beta"], a["smooth"],
                                q, q, q, q, 1 << 20, None)
        assert rc == -1, (b, rc)     # CSU_E_ARG
        assert b"seg_loss_fwd" in L.csu_last_error_string()
    for b in bad:
        if set(b) & {"smooth", "alpha", "beta"}:
            continue
        a = dict(ok, **b)
        rc = L.csu_seg_loss_bwd(a["n"], a["rows"], q, q, q, q, a["w_bce"], a["pw"], a["w_tv"], q, None)
        assert rc == -1, (b, rc)
        assert b"seg_loss_bwd" in L.csu_last_error_string()
