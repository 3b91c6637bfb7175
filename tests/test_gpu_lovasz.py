"""csu_seg_lovasz_* on the MI355X: the fused Lovasz-Softmax loss in every layout, logits dtype and label dtype the
kernels read, both ``per_image`` settings and the three ``classes`` modes, checked at three levels:

(a) every pixel's error e is decoded from the sorted keys and values and compared with the fp64 e at ten times
    torch's own fp32 error of e for the case; per segment the values are a permutation of the segment's pixels,
    the fg bits equal the labels, the keys ascend (ties in ascending index: the stable order) and the dead pixels
    come last;
(b) psi is recomputed in numpy fp64 from the kernel's own order by the closed forms and must equal the kernel's
    bit for bit: both sides form g from the same integers with the same IEEE operations (1 / U, I / (U (U + 1)),
    times 1 / (counted x B)) and round once to fp32, and the ranks are the kernel's own, so near-ties cannot matter;
(c) the loss and dz against the fp64 reference of tests/test_lovasz.py with that file's tolerances (LOSS_RTOL; ten
    times torch's fp32 gradient error per shape, measured there on the CPU; bf16 gradients one bf16 rounding on
    top).

Then the all-ties hard-prediction case, ignored batches and images, w_lv = 0 against csu_seg_ce_* bit for bit, the
weight changed between replays of a captured graph, repeatability and a captured train_model epoch."""
import copy

import numpy as np
import pytest
import torch

from test_gpu_seg_ce import LAYOUTS, dev, place
from test_lovasz import (CLASS_MODES, GPU_SHAPES, LV_PARAM_SETS, check_grad, check_loss, class_arg, hard_case,
                         make_lovasz_criterion, mean_one_minus_iou, ref_lovasz_loss_grad)
from test_seg_ce import IGNORE, LOSS_RTOL, PARAM_SETS, SMOOTH, UPSTREAM, class_weights, make_case, make_criterion

pytestmark = pytest.mark.gpu

LARGE = (2, 6, 300, 333)
SHAPES = GPU_SHAPES
_REFS = {}


def class_list(mode, K):
    return list(range(K)) if mode != "list" else class_arg(mode, K)


def pixel_errors(z, t, cls):
    """e (|C|, B, HW) in z's floating dtype by the definition: sum_{k != c} p_k on the foreground, p_c elsewhere, at most 1."""
    B, K = z.shape[0], z.shape[1]
    p = torch.softmax(z.reshape(B, K, -1), 1)
    t2 = t.reshape(B, -1)
    out = []
    for c in cls:
        others = sum(p[:, k] for k in range(K) if k != c)
        out.append(torch.where(t2 == c, others, p[:, c]).clamp(max=1.0))
    return torch.stack(out)


def ref(shape, dtype, ps, mode, per_image):
    """(z, t, loss, grad, stats, fp64 e, tolerance of e) on the CPU, made once per case and left unchanged."""
    key = (shape, dtype, LV_PARAM_SETS.index(ps), mode, per_image)
    if key not in _REFS:
        z, t = make_case(shape, dtype=dtype)
        cls = class_list(mode, shape[1])
        ekey = (shape, dtype, mode == "list")
        if ekey not in _REFS:
            e64, e32 = pixel_errors(z.double(), t, cls), pixel_errors(z.float(), t, cls)
            live = (t != IGNORE).reshape(1, shape[0], -1).expand_as(e64)
            _REFS[ekey] = (e64.numpy(), 10.0 * float((e32.double() - e64)[live].abs().max()))
        _REFS[key] = (z, t) + ref_lovasz_loss_grad(z, t, ps, per_image, mode, per_image)[:3] + _REFS[ekey]
    return _REFS[key]


def check_order_and_psi(skeys, svals, psi, t, cls, mode, per_image, e64, e_tol):
    """Levels (a) and (b) of the module docstring."""
    B, n = t.shape[0], t[0].numel()
    nc = len(cls)
    segs, length = (nc * B, n) if per_image else (nc, B * n)
    k = skeys.cpu().numpy().view(np.uint32).reshape(segs, length)
    v = svals.cpu().numpy().view(np.uint32).reshape(segs, length)
    idx, fg = (v & np.uint32(0x7FFFFFFF)).astype(np.int64), (v >> np.uint32(31)).astype(np.int64)
    dead = ((k >> np.uint32(30)) & 1).astype(bool)
    lab = t.reshape(B, n).numpy()
    lab_seg = np.stack([lab.reshape(segs // nc, length)] * nc).reshape(segs, length)        # the labels of a segment's pixels
    cls_seg = np.repeat(np.asarray(cls), segs // nc).reshape(segs, 1)
    lab_sorted = np.take_along_axis(lab_seg, idx.clip(0, length - 1), 1)
    # (a)
    assert np.array_equal(np.sort(idx, axis=1), np.broadcast_to(np.arange(length), (segs, length))), "not a permutation"
    assert np.array_equal(fg == 1, lab_sorted == cls_seg), "fg bits"
    assert np.array_equal(dead, lab_sorted == IGNORE), "dead flags"
    assert (k < (1 << 31)).all() and (np.diff(k.astype(np.int64), axis=1) >= 0).all(), "keys ascend, dead pixels last"
    ties = np.diff(k.astype(np.int64), axis=1) == 0
    assert (np.diff(idx, axis=1)[ties] > 0).all(), "ties in ascending index"
    e_sorted = (np.uint32(0x3F800000) - (k & np.uint32(0x3FFFFFFF))).view(np.float32).astype(np.float64)
    e_pix = np.empty((segs, length))
    np.put_along_axis(e_pix, idx, e_sorted, 1)
    live_pix = lab_seg != IGNORE
    err = np.abs(e_pix - e64.reshape(segs, length))[live_pix]
    print(f"    e: max |kernel - fp64| {err.max() if err.size else 0.0:.3g} (allowed {e_tol:.3g})")
    assert err.size == 0 or err.max() <= e_tol
    # (b)
    G = fg.sum(1, keepdims=True)
    I = G - (np.cumsum(fg, 1) - fg)
    U = I + np.arange(length)[None, :]
    safe = np.where(U > 0, U, 1).astype(np.float64)
    g = np.where(fg == 1, 1.0 / safe, np.where(U > 0, I.astype(np.float64) / (safe * (safe + 1.0)), 1.0))
    present = (G.reshape(nc, -1) > 0)
    counted = present if mode == "present" else np.ones_like(present)
    number = np.maximum(counted.sum(0, keepdims=True), 1).astype(np.float64) * float(B if per_image else 1)
    scale = np.where(counted, 1.0 / number, 0.0).reshape(segs, 1)
    want_sorted = np.where(dead, 0.0, np.where(fg == 1, -g, g) * scale).astype(np.float32)
    want = np.empty((segs, length), np.float32)
    np.put_along_axis(want, idx, want_sorted, 1)
    got = psi.cpu().numpy().reshape(segs, length)
    assert np.array_equal(got, want), \
        f"psi differs at {int((got != want).sum())} places, max |diff| {np.abs(got.astype(np.float64) - want).max():.3g}"


def run_debug(za, td, ps, mode, per_image, K, d):
    """ops.seg_lovasz with debug=True on the arguments LovaszSegLoss passes."""
    from csu import ops
    ce, tv, alpha, beta, weighted, bg, lv = ps
    cw = torch.tensor(class_weights(K), device=d) if weighted else None
    w = torch.full((1,), lv, device=d)
    return ops.seg_lovasz(za, td, w, (ce, tv, alpha, beta, SMOOTH), class_list(mode, K), mode == "present", per_image, cw,
                          IGNORE, za.shape[0] if per_image else 1, bg, with_stats=True, debug=True)


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("mode", CLASS_MODES)
@pytest.mark.parametrize("ps", LV_PARAM_SETS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_vs_fp64(shape, dtype, ps, mode, per_image):
    """per_sample follows per_image, so the Tversky rows are covered in both settings too."""
    d = dev()
    z, t, lref, gref, sref, e64, e_tol = ref(shape, dtype, ps, mode, per_image)
    K = shape[1]
    for li, layout in enumerate(LAYOUTS):
        for bi, lab in enumerate((torch.int64, torch.uint8)):
            za = place(z, layout, d)
            loss, terms, stats, skeys, svals, psi = run_debug(za, t.to(d).to(lab), ps, mode, per_image, K, d)
            (loss * UPSTREAM).backward()
            g = za.grad.double().cpu()
            lv = float(loss.detach())
            print(f"{layout} {lab}: loss {lv:.9g} ref {float(lref):.9g} rel {abs(lv - float(lref)) / abs(float(lref)):.2e}"
                  f"  grad err / max|g_ref| {float((g - gref).abs().max() / gref.abs().max()):.2e}")
            assert za.grad.dtype == dtype and terms.shape == (2,) and not bool(torch.isnan(psi).any())
            if shape != LARGE or (li + bi) % 2 == 0:      # the large shape: the numpy side of (a), (b) in half of the runs
                check_order_and_psi(skeys, svals, psi, t, class_list(mode, K), mode, per_image, e64, e_tol)
            check_loss(loss, lref)
            check_grad(za.grad, gref, shape, bf16=dtype == torch.bfloat16)
            assert stats.dtype == torch.float64 and torch.equal(stats.cpu(), sref)
            torch.testing.assert_close(terms[0].double().cpu() + ps[6] * terms[1].double().cpu(), lref, rtol=LOSS_RTOL, atol=1e-12)


# ---- exact and edge cases -------------------------------------------------------------------------------

@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_hard_predictions_all_ties(layout, per_image):
    """Logits of +-100: every error is exactly 0 or 1, the order is all ties, and LS = mean_c (1 - IoU_c)."""
    from csu.losses import lovasz_softmax_loss
    d = dev()
    z, t, pred = hard_case()
    if per_image:
        want = sum(mean_one_minus_iou(pred[b:b + 1], t[b:b + 1], 3) for b in range(2)) / 2
    else:
        want = mean_one_minus_iou(pred, t, 3)
    crit = lovasz_softmax_loss(3, per_image=per_image, ignore_index=IGNORE)
    za = place(z, layout, d)
    loss = crit(za, t.to(d))
    loss.backward()
    torch.testing.assert_close(loss.detach().double().cpu(), torch.tensor(want, dtype=torch.float64), rtol=LOSS_RTOL, atol=0.0)
    assert float(za.grad.abs().max()) == 0.0          # a saturated softmax
    ps = LV_PARAM_SETS[0]
    _, _, _, skeys, svals, psi = run_debug(za.detach(), t.to(d), ps, "present", per_image, 3, d)
    e = pixel_errors(z, t, [0, 1, 2])          # exactly 0 or 1 in fp32 (in fp64 the saturated softmax leaves 1e-87)
    assert bool(((e == 0) | (e == 1)).all())
    check_order_and_psi(skeys, svals, psi, t, [0, 1, 2], "present", per_image, e.double().numpy(), 0.0)


@pytest.mark.parametrize("mode", CLASS_MODES)
@pytest.mark.parametrize("per_image", [False, True])
def test_all_ignored_batch_is_zero_not_nan(per_image, mode):
    d = dev()
    z, _ = make_case((2, 3, 7, 9))
    t = torch.full((2, 7, 9), IGNORE, dtype=torch.int64)
    for ps in LV_PARAM_SETS:
        crit = make_lovasz_criterion(3, ps, per_image, mode, per_image)
        za = place(z, "nchw", d)
        loss, stats = crit.loss_stats(za, t.to(d))
        loss.backward()
        assert float(loss.detach()) == 0.0 and float(za.grad.abs().max()) == 0.0 and float(stats.abs().max()) == 0.0
        assert float(crit.last_terms.abs().max()) == 0.0


@pytest.mark.parametrize("mode", CLASS_MODES)
def test_an_ignored_image_counts_in_b_under_per_image(mode):
    """(3,5,37,41): image 1 is ignored entirely; under per_image it adds 0 and the mean is still over 3 images."""
    d = dev()
    shape, ps = (3, 5, 37, 41), LV_PARAM_SETS[0]
    z, t, lref, gref, _, _, _ = ref(shape, torch.float32, ps, mode, True)
    assert bool((t[1] == IGNORE).all())
    crit = make_lovasz_criterion(5, ps, True, mode, True)
    za = place(z, "nchw", d)
    loss = crit(za, t.to(d))
    (loss * UPSTREAM).backward()
    check_loss(loss, lref)
    check_grad(za.grad, gref, shape)
    assert float(za.grad[1].abs().max()) == 0.0
    keep = torch.tensor([0, 2])
    zb = place(z[keep], "nchw", d)
    two = make_lovasz_criterion(5, ps, True, mode, True)(zb, t[keep].to(d))
    torch.testing.assert_close(loss.detach() * 3.0, two.detach() * 2.0, rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (3, 5, 37, 41), (2, 5, 33, 33)])
def test_zero_weight_is_seg_ce_bit_for_bit(shape, layout, per_sample):
    d = dev()
    z, t = make_case(shape)
    ps = PARAM_SETS[2]
    lv = make_lovasz_criterion(shape[1], ps + (0.0,), per_sample, "present", per_sample)
    ce = make_criterion(shape[1], ps, per_sample)
    for dtype in (torch.float32, torch.bfloat16):
        za, zb = place(z.to(dtype), layout, d), place(z.to(dtype), layout, d)
        la, sa = lv.loss_stats(za, t.to(d))
        lb, sb = ce.loss_stats(zb, t.to(d))
        (la * UPSTREAM).backward()
        (lb * UPSTREAM).backward()
        assert torch.equal(la.detach(), lb.detach()) and torch.equal(za.grad, zb.grad) and torch.equal(sa, sb)
        assert float(lv.last_terms[1]) > 0.0 and torch.equal(lv.last_terms[0], lb.detach())


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_bitwise_repeatable(layout, per_image):
    d = dev()
    z, t = make_case(LARGE)
    crit = make_lovasz_criterion(6, LV_PARAM_SETS[1], True, "present", per_image)
    td = t.to(d)
    res = []
    for _ in range(2):
        za = place(z, layout, d)
        loss, stats = crit.loss_stats(za, td)
        (loss * UPSTREAM).backward()
        res.append((loss.detach(), stats, za.grad, crit.last_terms))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_33_classes_take_the_torch_route_on_the_device():
    d = dev()
    z, t = make_case((2, 33, 9, 11))
    ps = LV_PARAM_SETS[1]
    lref, gref, sref, _ = ref_lovasz_loss_grad(z, t, ps, False, "present", False)
    crit = make_lovasz_criterion(33, ps, False, "present", False)
    za = z.to(d).requires_grad_(True)
    loss, stats = crit.loss_stats(za, t.to(d))
    (loss * UPSTREAM).backward()
    assert loss.is_cuda and stats.is_cuda and crit.last_terms.is_cuda
    check_loss(loss, lref)
    check_grad(za.grad, gref, (2, 33, 9, 11))
    assert torch.equal(stats.cpu(), sref)


def test_ops_argument_checks():
    from csu import ops
    from csu._lib import CsuError
    d = dev()
    z = torch.randn(2, 3, 4, 4, device=d)
    t = torch.zeros(2, 4, 4, dtype=torch.int64, device=d)
    prm, w = (1.0, 1.0, 0.5, 0.5, 0.5), torch.full((1,), 0.5, device=d)
    with pytest.raises(CsuError):
        ops.seg_lovasz(z.cpu(), t.cpu(), w.cpu(), prm)
    with pytest.raises(CsuError):
        ops.seg_lovasz(z, t, w.cpu(), prm)
    for a, b, ww, p, kw in ((z.double(), t, w, prm, {}), (z, t.float(), w, prm, {}), (z, t[:1], w, prm, {}),
                            (z, t, w, prm, dict(rows=3)), (z, t, w, prm[:4], {}), (z[:, :1], t, w, prm, {}),
                            (z, t, w, prm, dict(class_weight=torch.ones(2, device=d))), (z, t, w.double(), prm, {}),
                            (z, t, torch.ones(2, device=d), prm, {}), (z, t, w, prm, dict(classes=[])),
                            (z, t, w, prm, dict(classes=[3])), (z, t, w, prm, dict(classes=[-1]))):
        with pytest.raises(ValueError):
            ops.seg_lovasz(a, b, ww, p, **kw)
    with pytest.raises(CsuError, match="smooth"):
        ops.seg_lovasz(z, t, w, (1.0, 1.0, 0.5, 0.5, 0.0))


# ---- graphs and the train loop --------------------------------------------------------------------------

def test_set_lovasz_weight_between_replays_of_a_captured_graph():
    d = dev()
    shape, ps = (2, 5, 33, 33), LV_PARAM_SETS[1]
    z, t = make_case(shape)
    td = t.to(d)
    eager = []
    for w in (0.7, 0.2, 0.0):
        za = place(z, "nchw", d)
        c = make_lovasz_criterion(5, ps[:6] + (w,), True, "present", True)
        loss = c(za, td)
        loss.backward()
        eager.append((loss.detach().clone(), za.grad.clone(), c.last_terms.clone()))
    crit = make_lovasz_criterion(5, ps, True, "present", True)
    zs = z.to(d).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        crit(zs, td).backward()           # warm-up: makes the device scalar
    torch.cuda.current_stream().wait_stream(side)
    zs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = crit(zs, td)
        loss.backward()
    for w, want in zip((0.7, 0.2, 0.0), eager):
        crit.set_lovasz_weight(w)
        graph.replay()
        assert torch.equal(loss.detach(), want[0]) and torch.equal(zs.grad, want[1])
        assert torch.equal(crit.last_terms, want[2])


def test_train_model_graphed_equals_eager_ce_lovasz():
    """train_model on the 3-class logits-head model of test_gpu_seg_ce under bf16 autocast with ce_lovasz_loss and a
    schedule: the captured run follows the schedule, adds no history key, and Dice / IoU equal the eager run's."""
    from csu.losses import ce_lovasz_loss
    from csu.train import make_optimizer, train_model
    from test_gpu_seg_ce import _multiclass_setup
    d, m0, train, test = _multiclass_setup()
    hs, crits = [], []
    for graph in (True, False):
        m = copy.deepcopy(m0).to(d)
        opt = make_optimizer(m)
        crit = ce_lovasz_loss(3, lovasz=1.0, schedule=lambda e: 0.5)
        hs.append(train_model(m, train, test, crit, opt, None, d, num_epochs=1, verbose=False, amp_dtype=torch.bfloat16,
                              graph=graph))
        crits.append(crit)
    assert crits[0].lovasz_weight == 0.5 and crits[1].lovasz_weight == 0.5
    assert set(hs[0]) == set(hs[1]) and "train_class_dice" in hs[0]
    assert "boundary_weight" not in hs[0] and "top_k" not in hs[0] and "lovasz_weight" not in hs[0]
    for k in hs[0]:
        np.testing.assert_allclose(hs[0][k], hs[1][k], rtol=1e-5, atol=1e-6, err_msg=k)
    assert 0.0 < hs[0]["test_dice"][0] <= 1.0 and np.isfinite(hs[0]["train_loss"][0])
    assert float(crits[0].last_terms[1]) > 0.0
