"""csu.losses.LovaszSegLoss on the CPU (the Lovasz-Softmax surrogate of the IoU on top of the fused multi-class loss):
``reference_lovasz_softmax`` against an independent restatement of Berman's cumsum form, the torch-op path against
the reference, the hard-prediction identity LS = mean_c (1 - IoU_c), the edge cases, the constructor's checks, the
schedule, and the C-ABI entry points csu_sort_pairs* and csu_seg_lovasz_*.

The fp64 reference of loss and gradient (``ref_lovasz_loss_grad``) is shared with tests/test_gpu_lovasz.py.

Tolerances, derived as in tests/test_seg_ce.py.  torch's own fp32 composition of the formula (``LovaszSegLoss`` on
fp32 CPU logits: the torch-op path) was measured on the CPU against ``ref_lovasz_loss_grad`` at every shape of
GPU_SHAPES, both logits dtypes (bf16 values upcast exactly), both ``per_image`` settings, the three ``classes`` modes
and both parameter sets of LV_PARAM_SETS (``measure_fp32_error`` below prints the table).  The largest relative loss
error was 1.47e-7 ((2,5,33,33)), so the loss keeps test_seg_ce's LOSS_RTOL = 1.5e-6.  The largest gradient error,
relative to max|g_ref|, per shape:

    (2,3,7,9) 1.41e-6   (3,5,37,41) 2.96e-4   (2,19,16,16) 9.88e-6   (2,32,8,8) 1.11e-6
    (1030,4,3,3) 2.24e-4   (2,5,33,33) 1.25e-4   (2,6,300,333) 3.65e-3
    (2,33,9,11) 1.60e-6 (the torch route for more than 32 classes, which the GPU file runs on the device)

Two effects stand behind the larger figures, and any fp32 evaluation has both, the kernels included.  Where a class
of C is absent (make_case's last class for K >= 5, counted under 'all' and a list) its segment has g_1 = 1 and no
other increment, so one pixel carries the whole gradient p (1 - p) of that segment, and there p is 0.9998: 1 - p
cancels in fp32 (one element, 2.4e-4 of max|g_ref| at (3,5,37,41); under 'present' the same shape gives 2.0e-6).  And
with 10^5 and more pixels per segment fp32 and fp64 order some near-equal errors differently; a foreground and a
background pixel that swap ranks swap their increments.  That is benign for the loss (it moves by the difference of
the two errors).  GRAD_ATOL_REL holds ten times the measured figure per shape, absolute against max|g_ref| with no
relative term; bf16 gradients get one bf16 rounding (rtol 2**-8) on top.  Nothing here was measured against the
kernels, whose ranks tests/test_gpu_lovasz.py pins separately and exactly."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_seg_ce import BF16_RTOL, IGNORE, LOSS_RTOL, SMOOTH, UPSTREAM, class_weights, make_case, ref_ce_loss_grad

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GPU_SHAPES = [(2, 3, 7, 9), (3, 5, 37, 41), (2, 19, 16, 16), (2, 32, 8, 8), (1030, 4, 3, 3), (2, 5, 33, 33), (2, 6, 300, 333)]
SHAPES = GPU_SHAPES[:2] + [(2, 5, 33, 33)]
# ten times torch's fp32 gradient error against fp64 relative to max|g_ref| (the module docstring)
GRAD_ATOL_REL = {(2, 3, 7, 9): 1.41e-5, (3, 5, 37, 41): 2.96e-3, (2, 19, 16, 16): 9.88e-5, (2, 32, 8, 8): 1.11e-5,
                 (1030, 4, 3, 3): 2.24e-3, (2, 5, 33, 33): 1.25e-3, (2, 6, 300, 333): 3.65e-2, (2, 33, 9, 11): 1.60e-5}
# (ce, tversky, alpha, beta, weighted, include_background, lovasz): the term alone; weighted CE + Tversky(0.3, 0.7) + 0.7 LS
LV_PARAM_SETS = [(0.0, 0.0, 0.5, 0.5, False, True, 1.0), (0.5, 1.0, 0.3, 0.7, True, False, 0.7)]
CLASS_MODES = ["present", "all", "list"]


def class_arg(mode, K):
    """The ``classes`` argument of a mode; the list holds the first and the last class (absent from make_case's labels
    when K >= 5)."""
    return [0, K - 1] if mode == "list" else mode


def make_lovasz_criterion(K, ps, per_sample, mode, per_image, ignore_index=IGNORE, smooth=SMOOTH, schedule=None):
    from csu.losses import LovaszSegLoss
    ce, tv, alpha, beta, weighted, bg, lv = ps
    return LovaszSegLoss(K, ce=ce, tversky=tv, alpha=alpha, beta=beta, smooth=smooth,
                         class_weight=class_weights(K) if weighted else None, ignore_index=ignore_index,
                         per_sample=per_sample, include_background=bg, lovasz=lv, classes=class_arg(mode, K),
                         per_image=per_image, schedule=schedule)


def ref_lovasz_loss_grad(z, t, ps, per_sample, mode, per_image, ignore_index=IGNORE, upstream=UPSTREAM):
    """fp64 (loss, d(upstream * loss)/dz, (3, K) hard sums, LS): test_seg_ce's reference of the first two terms plus
    lovasz * reference_lovasz_softmax, for logits z (fp32 or bf16, upcast exactly) and int64 labels t."""
    from csu.losses import reference_lovasz_softmax
    base, gbase, stats = ref_ce_loss_grad(z, t, ps[:6], per_sample, ignore_index=ignore_index, upstream=upstream)
    z64 = z.detach().double().requires_grad_(True)
    ls = reference_lovasz_softmax(z64, t, class_arg(mode, z.shape[1]), per_image, ignore_index)
    (g,) = torch.autograd.grad(ls * (upstream * ps[6]), z64)
    return base + ps[6] * ls.detach(), gbase + g, stats, ls.detach()


def check_loss(loss, ref):
    torch.testing.assert_close(loss.detach().double().cpu(), ref, rtol=LOSS_RTOL, atol=1e-12)


def check_grad(g, g_ref, shape, bf16=False):
    scale = float(g_ref.abs().max())
    torch.testing.assert_close(g.double().cpu(), g_ref, rtol=BF16_RTOL if bf16 else 0.0, atol=GRAD_ATOL_REL[tuple(shape)] * scale)


def berman_lovasz_softmax(z, t, classes, per_image, ignore_index=IGNORE):
    """Berman's lovasz_softmax_flat restated independently in fp64 numpy: per segment the errors |fg - p_c| sorted
    descending (stable), the Jaccard loss along the order by cumulative sums, its first differences, and the dot
    product.  classes: 'present', 'all' or a list."""
    B, K = z.shape[0], z.shape[1]
    z64 = z.double().reshape(B, K, -1)
    p = torch.softmax(z64, 1).numpy()
    lab = t.reshape(B, -1).numpy()

    def flat(pb, lb):            # pb (K, n), lb (n,)
        keep = lb != ignore_index
        pb, lb = pb[:, keep], lb[keep]
        cls = range(K) if isinstance(classes, str) else classes
        losses = []
        for c in cls:
            fg = (lb == c).astype(np.float64)
            if classes == "present" and fg.sum() == 0:
                continue
            err = np.abs(fg - pb[c])
            order = np.argsort(-err, kind="stable")
            es, fs = err[order], fg[order]
            inter = fs.sum() - np.cumsum(fs)
            union = fs.sum() + np.cumsum(1.0 - fs)
            jac = 1.0 - inter / union
            jac[1:] = jac[1:] - jac[:-1]
            losses.append(float(np.dot(es, jac)))
        return sum(losses) / max(1, len(losses))

    if per_image:
        return sum(flat(p[b], lab[b]) for b in range(B)) / B
    return flat(p.transpose(1, 0, 2).reshape(K, -1), lab.reshape(-1))


def hard_case(shape=(2, 3, 7, 9)):
    """make_case's labels with logits of +-100 on a random prediction: the softmax is exactly 0 or 1 in fp32."""
    _, t = make_case(shape)
    g = torch.Generator().manual_seed(77)
    pred = torch.randint(0, shape[1], (shape[0],) + shape[2:], generator=g)
    z = torch.nn.functional.one_hot(pred, shape[1]).permute(0, 3, 1, 2).float() * 200.0 - 100.0
    return z.contiguous(), t, pred


def mean_one_minus_iou(pred, t, K, ignore_index=IGNORE):
    live = t != ignore_index
    vals = []
    for c in range(K):
        a, b = (pred == c) & live, (t == c) & live
        if int(b.sum()) > 0:
            vals.append(1.0 - float((a & b).sum()) / float((a | b).sum()))
    return sum(vals) / max(1, len(vals))


def measure_fp32_error(shapes=GPU_SHAPES):
    """Print torch's fp32 loss and gradient error of the torch-op path against the fp64 reference per shape (the
    figures of the module docstring): ``python tests/test_lovasz.py``."""
    for shape in shapes:
        worst_l = worst_g = 0.0
        for dtype in (torch.float32, torch.bfloat16):
            z, t = make_case(shape, dtype=dtype)
            for ps in LV_PARAM_SETS:
                for mode in CLASS_MODES:
                    for per_image in (False, True):
                        lref, gref, _, _ = ref_lovasz_loss_grad(z, t, ps, per_image, mode, per_image)
                        za = z.detach().float().clone().requires_grad_(True)
                        loss = make_lovasz_criterion(shape[1], ps, per_image, mode, per_image)(za, t)
                        (loss * UPSTREAM).backward()
                        worst_l = max(worst_l, abs(float(loss.detach()) - float(lref)) / abs(float(lref)))
                        worst_g = max(worst_g, float((za.grad.double() - gref).abs().max() / gref.abs().max()))
        print(f"{shape}: loss rel {worst_l:.3g}  grad / max|g_ref| {worst_g:.3g}", flush=True)


# ---- the reference and the torch-op path ------------------------------------------------------------------

@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("mode", CLASS_MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_equals_bermans_cumsum_form(shape, mode, per_image):
    from csu.losses import reference_lovasz_softmax
    z, t = make_case(shape)
    cls = class_arg(mode, shape[1])
    got = float(reference_lovasz_softmax(z, t, cls, per_image, IGNORE))
    want = berman_lovasz_softmax(z, t, cls, per_image)
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("mode", CLASS_MODES)
@pytest.mark.parametrize("ps", LV_PARAM_SETS)
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_path_vs_fp64(shape, ps, mode, per_image):
    z, t = make_case(shape)
    lref, gref, sref, lsref = ref_lovasz_loss_grad(z, t, ps, per_image, mode, per_image)
    crit = make_lovasz_criterion(shape[1], ps, per_image, mode, per_image)
    za = z.clone().requires_grad_(True)
    loss, stats = crit.loss_stats(za, t)
    (loss * UPSTREAM).backward()
    check_loss(loss, lref)
    check_grad(za.grad, gref, shape)
    assert stats.dtype == torch.float64 and torch.equal(stats, sref)
    assert crit.last_terms.shape == (2,)
    torch.testing.assert_close(crit.last_terms[1].double(), lsref, rtol=LOSS_RTOL, atol=1e-12)
    zb = z.clone().requires_grad_(True)
    assert torch.equal(crit(zb, t.unsqueeze(1)), loss.detach())          # (B, 1, H, W) labels


@pytest.mark.parametrize("per_image", [False, True])
def test_hard_predictions_give_mean_one_minus_iou(per_image):
    """Every error is exactly 0 or 1, so the order is all ties and LS is the Jaccard loss itself: both sides give
    0.807534 over the batch and 0.803819 per image on hard_case()'s prediction."""
    from csu.losses import lovasz_softmax_loss, reference_lovasz_softmax
    z, t, pred = hard_case()
    p = torch.softmax(z, 1)
    assert bool(((p == 0) | (p == 1)).all())
    if per_image:
        want = sum(mean_one_minus_iou(pred[b:b + 1], t[b:b + 1], 3) for b in range(2)) / 2
    else:
        want = mean_one_minus_iou(pred, t, 3)
    ref = reference_lovasz_softmax(z, t, "present", per_image, IGNORE)
    assert abs(float(ref) - want) <= 1e-12
    loss = lovasz_softmax_loss(3, per_image=per_image, ignore_index=IGNORE)(z, t)
    torch.testing.assert_close(loss.double(), torch.tensor(want, dtype=torch.float64), rtol=LOSS_RTOL, atol=0.0)


@pytest.mark.parametrize("mode", CLASS_MODES)
def test_all_ignored_batch_is_zero_with_a_zero_gradient(mode):
    z, _ = make_case((2, 3, 7, 9))
    t = torch.full((2, 7, 9), IGNORE, dtype=torch.int64)
    for ps in LV_PARAM_SETS:
        for per_image in (False, True):
            za = z.clone().requires_grad_(True)
            loss = make_lovasz_criterion(3, ps, False, mode, per_image)(za, t)
            loss.backward()
            assert float(loss.detach()) == 0.0 and float(za.grad.abs().max()) == 0.0


def test_an_absent_class_counts_under_all_but_not_under_present():
    """(3,5,37,41): class 4 is absent.  Its segment is all background, LS_4 = the largest p_4, and 'all' divides by
    5 where 'present' divides by 4."""
    from csu.losses import reference_lovasz_softmax
    shape = (3, 5, 37, 41)
    z, t = make_case(shape)
    assert int((t == 4).sum()) == 0
    pres = float(reference_lovasz_softmax(z, t, "present", False, IGNORE))
    allc = float(reference_lovasz_softmax(z, t, "all", False, IGNORE))
    p4 = torch.softmax(z.double(), 1)[:, 4][t != IGNORE].max()
    assert abs(allc - (4 * pres + float(p4)) / 5) <= 1e-12
    lp = make_lovasz_criterion(5, LV_PARAM_SETS[0], False, "present", False)(z, t)
    la = make_lovasz_criterion(5, LV_PARAM_SETS[0], False, "all", False)(z, t)
    torch.testing.assert_close(lp.double(), torch.tensor(pres, dtype=torch.float64), rtol=LOSS_RTOL, atol=0.0)
    torch.testing.assert_close(la.double(), torch.tensor(allc, dtype=torch.float64), rtol=LOSS_RTOL, atol=0.0)


@pytest.mark.parametrize("per_sample", [False, True])
def test_zero_weight_is_multiclass_seg_loss(per_sample):
    from csu.losses import LovaszSegLoss, MultiClassSegLoss
    z, t = make_case((3, 5, 37, 41))
    kw = dict(ce=0.5, tversky=1.0, alpha=0.3, beta=0.7, class_weight=class_weights(5), ignore_index=IGNORE,
              per_sample=per_sample, include_background=False)
    za, zb = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    la, lb = LovaszSegLoss(5, lovasz=0.0, **kw)(za, t), MultiClassSegLoss(5, **kw)(zb, t)
    la.backward()
    lb.backward()
    assert torch.equal(la.detach(), lb.detach()) and torch.equal(za.grad, zb.grad)


@pytest.mark.parametrize("kw", [dict(lovasz=-1.0), dict(lovasz=float("inf")), dict(lovasz=float("nan")), dict(classes="some"),
                                dict(classes=[]), dict(classes=[0, 0]), dict(classes=[3]), dict(classes=[-1]),
                                dict(classes=[1.0]), dict(classes=5), dict(schedule=3), dict(smooth=0.0), dict(ce=-1.0)])
def test_constructor_rejects(kw):
    from csu.losses import LovaszSegLoss
    with pytest.raises(ValueError):
        LovaszSegLoss(3, **kw)


def test_weight_schedule_factories_and_exports():
    import csu
    from csu.losses import LovaszSegLoss, MultiClassSegLoss, ce_lovasz_loss, lovasz_softmax_loss, reference_lovasz_softmax
    c = ce_lovasz_loss(4, ce=0.5, lovasz=2.0, classes=[1, 2], per_image=True, ignore_index=IGNORE, schedule=lambda e: 0.25 * e)
    assert isinstance(c, LovaszSegLoss) and isinstance(c, MultiClassSegLoss) and hasattr(c, "loss_stats")
    assert (c.ce, c.tversky, c.lovasz_weight, c.classes, c.per_image) == (0.5, 0.0, 2.0, [1, 2], True)
    assert not hasattr(c, "boundary_weight") and getattr(c, "top_k", None) is None        # no history key in train_model
    z, t = make_case((2, 4, 5, 6))
    c(z, t)
    c.on_epoch(3)
    assert c.lovasz_weight == 0.75 and float(c._scalar(z.device)) == 0.75
    want = 0.5 * float(c.last_terms[0]) / 0.5 + 0.75 * float(c.last_terms[1])
    assert abs(float(c(z, t)) - want) <= 1e-6
    with pytest.raises(ValueError):
        c.set_lovasz_weight(-1.0)
    a = lovasz_softmax_loss(4)
    assert (a.ce, a.tversky, a.lovasz_weight, a.classes, a.per_image) == (0.0, 0.0, 1.0, "present", False)
    assert {a: 1}[a] == 1 and "lovasz=1.0" in repr(a) and "classes='present'" in repr(a)
    for n, obj in (("LovaszSegLoss", LovaszSegLoss), ("lovasz_softmax_loss", lovasz_softmax_loss),
                   ("ce_lovasz_loss", ce_lovasz_loss), ("reference_lovasz_softmax", reference_lovasz_softmax)):
        assert getattr(csu, n) is obj and n in csu.__all__


def test_runs_in_fp32_under_autocast_and_takes_33_classes():
    z, t = make_case((2, 33, 5, 6))
    lref, gref, _, _ = ref_lovasz_loss_grad(z, t, LV_PARAM_SETS[0], False, "present", False)
    za = z.clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        loss = make_lovasz_criterion(33, LV_PARAM_SETS[0], False, "present", False)(za, t)
    assert loss.dtype == torch.float32
    check_loss(loss, lref)


# ---- the C ABI ----------------------------------------------------------------------------------------

NEW_ABI = ("csu_sort_pairs_workspace", "csu_sort_pairs", "csu_sort_pairs_tile", "csu_seg_lovasz_workspace",
           "csu_seg_lovasz_fwd", "csu_seg_lovasz_bwd")


def test_abi_declares_and_exports_the_new_entry_points():
    from csu import _lib
    src = open(os.path.join(REPO, "include", "csu.h")).read()
    assert "csrc/sort_pairs.hip" in src[:src.index("csu_sort_pairs_workspace(")]
    assert "Berman" in src[src.index("csu_sort_pairs_tile(void)"):src.index("csu_seg_lovasz_workspace(")]
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for n in NEW_ABI:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(L, n) and n in _lib._SIGS, n
    assert len(_lib._SIGS["csu_sort_pairs"][1]) == 10
    assert len(_lib._SIGS["csu_seg_lovasz_fwd"][1]) == 34 and len(_lib._SIGS["csu_seg_lovasz_bwd"][1]) == 24
    T = L.csu_sort_pairs_tile()
    assert T >= 256 and T % 64 == 0
    ws = L.csu_sort_pairs_workspace
    # per segment 256 digit rows of one count per tile, and the 256 row totals
    assert ws(1, 1) == (256 + 256) * 4 and ws(3, T) == 3 * 512 * 4 and ws(2, 3 * T + 5) == 2 * (4 * 256 + 256) * 4
    assert ws(0, 5) == 0 and ws(1, 0) == 0 and ws(2, 1 << 30) == 0
    lw = L.csu_seg_lovasz_workspace
    assert lw(2, 3, 63, 0b111, 0) > 0 and lw(2, 3, 63, 0b111, 0) % 8 == 0 and lw(2, 3, 63, 0b101, 1) % 8 == 0
    assert lw(2, 3, 63, 0b111, 0) >= L.csu_seg_ce_workspace(2, 3, 63) + 2 * 4 * 3 * 2 * 63 + ws(3, 2 * 63)
    assert lw(2, 3, 63, 0, 0) == 0 and lw(2, 3, 63, 0b1000, 0) == 0 and lw(0, 3, 63, 1, 0) == 0 and lw(2, 33, 63, 1, 0) == 0
    assert lw(2, 32, 63, 0x80000000, 0) > 0 and lw(1 << 10, 3, 1 << 20, 0b111, 0) == 0       # |C| B HW >= 2^31


def test_abi_rejects_bad_arguments_on_the_host():
    """Every bad argument is refused before any launch (the pointers are dummies that a launch would fault on)."""
    from csu import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(q.value + 2)
    big = 1 << 24
    ok = dict(segments=2, len=5, bits=31, keys=q, vals=q, ka=q, va=q, ws=q, nws=big)
    bad = [dict(segments=0), dict(len=0), dict(segments=2, len=1 << 30), dict(bits=0), dict(bits=33), dict(keys=None),
           dict(vals=None), dict(ka=None), dict(va=None), dict(keys=odd), dict(va=odd)]
    for b in bad:
        a = dict(ok, **b)
        rc = L.csu_sort_pairs(a["segments"], a["len"], a["bits"], a["keys"], a["vals"], a["ka"], a["va"], a["ws"], a["nws"], None)
        assert rc == -1, (b, rc)     # CSU_E_ARG
        assert b"sort_pairs" in L.csu_last_error_string()
    for b in (dict(ws=None), dict(nws=4), dict(ws=odd)):
        a = dict(ok, **b)
        assert L.csu_sort_pairs(2, 5, 31, q, q, q, q, a["ws"], a["nws"], None) == -3, b     # CSU_E_WORKSPACE

    ok = dict(B=2, K=3, HW=8, rows=2, dtype=0, s_b=24, s_k=8, s_pix=1, lab=1, w_ce=1.0, w_tv=1.0, alpha=0.5, beta=0.5,
              smooth=0.5, mask=0b111, w_lv=q, sk=q, sv=q, psi=q, terms=q, nws=big, ws=q)
    bad = [dict(B=0), dict(HW=0), dict(K=1), dict(K=33), dict(rows=3), dict(dtype=2), dict(lab=2), dict(s_k=0), dict(s_pix=0),
           dict(s_b=-1), dict(w_ce=-1.0), dict(w_tv=-1.0), dict(smooth=0.0), dict(alpha=-0.5), dict(beta=-0.5), dict(mask=0),
           dict(mask=0b1000), dict(w_lv=None), dict(sk=None), dict(sv=None), dict(psi=None), dict(terms=None), dict(sk=odd)]

    def fwd(a):
        return L.csu_seg_lovasz_fwd(a["B"], a["K"], a["HW"], a["rows"], a["dtype"], q, a["s_b"], a["s_k"], a["s_pix"], 0,
                                    a["lab"], q, -100, None, a["w_ce"], a["w_tv"], a["alpha"], a["beta"], a["smooth"], 1,
                                    a["mask"], 1, 0, a["w_lv"], a["sk"], a["sv"], a["psi"], q, a["terms"], q, q, a["ws"],
                                    a["nws"], None)

    for b in bad:
        rc = fwd(dict(ok, **b))
        assert rc == -1, (b, rc)
        assert b"seg_lovasz_fwd" in L.csu_last_error_string()
    assert fwd(dict(ok, nws=8)) == -3 and fwd(dict(ok, ws=None)) == -3
    assert fwd(dict(ok, w_ce=0.0, w_tv=0.0, nws=8)) == -3        # both weights zero is legal: it gets as far as the workspace
    for b in bad:
        if set(b) & {"smooth", "alpha", "beta", "sk", "sv", "terms"}:
            continue
        a = dict(ok, **b)
        rc = L.csu_seg_lovasz_bwd(a["B"], a["K"], a["HW"], a["rows"], a["dtype"], q, a["s_b"], a["s_k"], a["s_pix"], 0,
                                  a["lab"], q, -100, None, q, q, a["w_ce"], a["w_tv"], 1, a["mask"], a["psi"], a["w_lv"], q,
                                  None)
        assert rc == -1, (b, rc)
        assert b"seg_lovasz_bwd" in L.csu_last_error_string()


if __name__ == "__main__":
    import sys
    sys.path[:0] = [REPO, os.path.join(REPO, "cswin-simam-unet_amd")]
    measure_fp32_error()
