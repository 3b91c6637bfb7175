"""csu_seg_ce_* on the MI355X: the fused softmax-CE + per-class Tversky kernels against the fp64
restatement of tests/test_seg_ce.py (loss, gradient under a non-unit upstream factor, exact (3, K)
hard sums) in every layout, logits dtype and label dtype they read, and the graph-captured train /
eval routes of a multi-class criterion.

Tolerances are those of tests/test_seg_ce.py (ten times torch's own fp32 error against fp64,
measured at these shapes; bf16 gradients get one bf16 rounding, rtol 2**-8, on top)."""
import copy

import numpy as np
import pytest
import torch

from test_seg_ce import (IGNORE, PARAM_SETS, UPSTREAM, check_grad, check_loss, make_case, make_criterion, ref_ce_loss_grad,
                         ref_hard_stats)

pytestmark = pytest.mark.gpu

# (1,2,3,5): under one vector and one workgroup, minimum K; (2,3,7,9): odd K, dense class-last pixels
# start off 16-B boundaries; (3,5,37,41): ragged rows, class 4 absent, image 1 ignored; (2,19,16,16) and
# (2,32,8,8): the top bucket and its edge; (1030,4,3,3): more images than workgroups; (2,6,300,333): 98
# chunks of 1020 pixels per image, the last one 960, several rounds per thread, 1.2M logits
SHAPES = [(1, 2, 3, 5), (2, 3, 7, 9), (3, 5, 37, 41), (2, 19, 16, 16), (2, 32, 8, 8), (1030, 4, 3, 3), (2, 6, 300, 333)]
LAYOUTS = ["nchw", "class_last_padded", "class_last_dense"]

_REFS = {}


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def ref(shape, dtype, ps, per_sample):
    """(z, t, loss, grad, stats) on the CPU, made once per case and left unchanged."""
    key = (shape, dtype, PARAM_SETS.index(ps), per_sample)
    if key not in _REFS:
        z, t = make_case(shape, dtype=dtype)
        _REFS[key] = (z, t) + ref_ce_loss_grad(z, t, ps, per_sample)
    return _REFS[key]


def place(z, layout, d):
    """The logits (B, K, H, W) on the device in a memory layout, as a leaf that requires grad."""
    B, K, H, W = z.shape
    if layout == "nchw":
        v = z.to(d)
    else:
        pitch = (K + 7) // 8 * 8 if layout == "class_last_padded" else K
        buf = torch.full((B, H * W, pitch), float("nan"), dtype=z.dtype, device=d)     # the padding is never used
        buf[..., :K] = z.to(d).reshape(B, K, H * W).transpose(1, 2)
        v = buf[..., :K].transpose(1, 2).reshape(B, K, H, W)
        assert v.data_ptr() == buf.data_ptr() and v.stride()[1:] == (1, W * pitch, pitch)
    return v.detach().requires_grad_(True)


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("ps", PARAM_SETS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_vs_fp64(shape, layout, dtype, ps, per_sample):
    d = dev()
    z, t, lref, gref, sref = ref(shape, dtype, ps, per_sample)
    crit = make_criterion(shape[1], ps, per_sample)
    for lab in (torch.int64, torch.uint8):
        za = place(z, layout, d)
        loss, stats = crit.loss_stats(za, t.to(d).to(lab))
        (loss * UPSTREAM).backward()
        g = za.grad.double().cpu()
        lv = float(loss.detach())
        print(f"{lab}: loss {lv:.9g} ref {float(lref):.9g} rel {abs(lv - float(lref)) / abs(float(lref)):.2e}"
              f"  grad err / max|g_ref| {float((g - gref).abs().max() / gref.abs().max()):.2e}")
        assert za.grad.dtype == dtype
        check_loss(loss, lref)
        check_grad(za.grad, gref, bf16=dtype == torch.bfloat16)
        assert stats.dtype == torch.float64 and torch.equal(stats.cpu(), sref)


def test_argmax_tie_lowest_index_wins():
    """bf16 logits with many exact ties (values on a grid of 4 levels): the hard sums follow the
    first-maximum rule, in both layouts."""
    d = dev()
    g = torch.Generator().manual_seed(11)
    z = torch.randint(0, 4, (2, 5, 16, 24), generator=g).to(torch.bfloat16)
    t = torch.randint(0, 5, (2, 16, 24), generator=g)
    sref = ref_hard_stats(z, t)
    assert int((z.float().max(1, keepdim=True).values == z.float()).sum(1).max()) > 1     # ties exist
    crit = make_criterion(5, PARAM_SETS[0], False)
    for layout in LAYOUTS:
        _, stats = crit.loss_stats(place(z, layout, d), t.to(d))
        assert torch.equal(stats.cpu(), sref), layout


@pytest.mark.parametrize("layout", LAYOUTS)
def test_saturated_logits_stay_finite(layout):
    """Logits of +-80 and a spread of 1e4: no overflow, a saturated softmax gives finite gradients."""
    d = dev()
    z, t = make_case((2, 6, 16, 24), seed=12)
    z = torch.where(z > 0, torch.full_like(z, 80.0), torch.full_like(z, -80.0))
    z[0, :, :4] *= 125.0                       # +-1e4
    ps = PARAM_SETS[2]
    lref, gref, sref = ref_ce_loss_grad(z, t, ps, True)
    za = place(z, layout, d)
    loss, stats = make_criterion(6, ps, True).loss_stats(za, t.to(d))
    (loss * UPSTREAM).backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(za.grad).all())
    check_loss(loss, lref)
    check_grad(za.grad, gref)
    assert torch.equal(stats.cpu(), sref)


def test_all_ignored_batch_is_zero_not_nan():
    d = dev()
    z, _ = make_case((2, 3, 7, 9))
    t = torch.full((2, 7, 9), IGNORE, dtype=torch.int64)
    for ps in PARAM_SETS:
        za = place(z, "nchw", d)
        loss, stats = make_criterion(3, ps, False).loss_stats(za, t.to(d))
        loss.backward()
        assert float(loss.detach()) == 0.0 and float(za.grad.abs().max()) == 0.0 and float(stats.abs().max()) == 0.0


@pytest.mark.parametrize("per_sample", [False, True])
def test_33_classes_take_the_torch_route_on_the_device(per_sample):
    d = dev()
    z, t = make_case((2, 33, 9, 11))
    ps = PARAM_SETS[2]
    lref, gref, sref = ref_ce_loss_grad(z, t, ps, per_sample)
    za = z.to(d).requires_grad_(True)
    loss, stats = make_criterion(33, ps, per_sample).loss_stats(za, t.to(d))
    (loss * UPSTREAM).backward()
    assert loss.is_cuda and stats.is_cuda
    check_loss(loss, lref)
    check_grad(za.grad, gref)
    assert torch.equal(stats.cpu(), sref)
    from csu import ops
    with pytest.raises(ValueError):
        ops.seg_ce(za, t.to(d), (1.0, 1.0, 0.5, 0.5, 0.5))


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_bitwise_repeatable(layout, per_sample):
    d = dev()
    z, t = make_case((2, 6, 300, 333))
    crit = make_criterion(6, PARAM_SETS[2], per_sample)
    td = t.to(d)
    res = []
    for _ in range(2):
        za = place(z, layout, d)
        loss, stats = crit.loss_stats(za, td)
        (loss * UPSTREAM).backward()
        res.append((loss.detach(), stats, za.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_nchw_views_off_a_16_byte_boundary():
    """Dense NCHW logits (class planes a multiple of 4 long) that start 1, 2, 3 elements off a 16-B
    boundary: the first and last unit of every chunk are read per element, the rest as vectors."""
    d = dev()
    shape, ps = (2, 5, 36, 52), PARAM_SETS[2]
    z, t, lref, gref, sref = ref(shape, torch.float32, ps, True)
    for off in (1, 2, 3):
        buf = torch.zeros(z.numel() + 8, device=d)
        za = buf[off:off + z.numel()].view(shape).copy_(z).detach().requires_grad_(True)
        assert za.data_ptr() % 16 == 4 * off
        loss, stats = make_criterion(5, ps, True).loss_stats(za, t.to(d))
        (loss * UPSTREAM).backward()
        check_loss(loss, lref)
        check_grad(za.grad, gref)
        assert torch.equal(stats.cpu(), sref)


def test_ops_seg_ce_argument_checks():
    from csu import ops
    from csu._lib import CsuError
    d = dev()
    z = torch.randn(2, 3, 4, 4, device=d)
    t = torch.zeros(2, 4, 4, dtype=torch.int64, device=d)
    prm = (1.0, 1.0, 0.5, 0.5, 0.5)
    with pytest.raises(CsuError):
        ops.seg_ce(z.cpu(), t.cpu(), prm)
    for a, b, p, kw in ((z.double(), t, prm, {}), (z, t.float(), prm, {}), (z, t[:1], prm, {}), (z, t, prm, dict(rows=3)),
                        (z, t, prm[:4], {}), (z[:, :1], t, prm, {}), (z, t, prm, dict(class_weight=torch.ones(2, device=d)))):
        with pytest.raises(ValueError):
            ops.seg_ce(a, b, p, **kw)
    with pytest.raises(CsuError, match="smooth"):      # refused by the C entry point before any launch
        ops.seg_ce(z, t, (1.0, 1.0, 0.5, 0.5, 0.0))


# ---- the train loop ----------------------------------------------------------------------------

def _multiclass_setup():
    from csu.data import SyntheticSegmentation
    from csu.model import CSWinTransformer
    d = dev()
    torch.manual_seed(0)
    m0 = CSWinTransformer(img_size=64, split_size=[1, 2, 2, 2], num_classes=3).set_head("logits")
    ds = SyntheticSegmentation(28, 64, seed=5, num_classes=3)
    batches = [tuple(torch.stack(v) for v in zip(*[ds[4 * b + i] for i in range(4)])) for b in range(7)]
    return d, m0, batches[:5], batches[5:]


def test_train_model_graphed_equals_eager_multiclass():
    """train_model on a 3-class logits-head model under bf16 autocast with ce_dice_loss: graph=True
    (two eager steps, then the captured step with the per-class sums inside the graph; captured eval)
    == graph=False, per-class history keys included (tolerances of test_train_model_graphed_equals_eager)."""
    from csu.losses import ce_dice_loss
    from csu.train import make_optimizer, train_model
    d, m0, train, test = _multiclass_setup()
    assert train[0][1].dtype == torch.int64 and train[0][1].shape == (4, 64, 64)
    hs, ps = [], []
    for graph in (True, False):
        m = copy.deepcopy(m0).to(d)
        assert m._head == "logits"
        opt = make_optimizer(m)
        hs.append(train_model(m, train, test, ce_dice_loss(3), opt, None, d, num_epochs=1, verbose=False,
                              amp_dtype=torch.bfloat16, graph=graph))
        ps.append([p.detach().clone() for p in m.parameters()])
    for k in ("train_class_dice", "train_class_iou", "test_class_dice", "test_class_iou"):
        assert k in hs[0] and len(hs[0][k]) == 1 and len(hs[0][k][0]) == 3, k
    assert set(hs[0]) == set(hs[1])
    for k in hs[0]:
        np.testing.assert_allclose(hs[0][k], hs[1][k], rtol=1e-5, atol=1e-6, err_msg=k)
    assert 0.0 < hs[0]["test_dice"][0] <= 1.0 and np.isfinite(hs[0]["train_loss"][0])
    for a, b in zip(*ps):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)


def test_evaluate_model_per_class_vs_torch_sums():
    """evaluate_model(per_class=True): the eager route's per-class Dice / IoU equal those formed from
    torch sums (first-maximum rule) of the same forward's logits; the captured route agrees with it."""
    from csu.losses import ce_dice_loss
    from csu.train import evaluate_model
    d, m0, _, test = _multiclass_setup()
    m = m0.to(d)
    crit = ce_dice_loss(3)
    loss, dice, iou, cd, ci = evaluate_model(m, test, crit, d, amp_dtype=torch.bfloat16, graph=False, per_class=True)
    tot = torch.zeros(3, 3, dtype=torch.float64)
    losses = []
    with torch.no_grad():
        for x, t in test:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                z = m(x.to(d))
            assert z.dtype == torch.bfloat16
            tot += ref_hard_stats(z.float().cpu(), t, ignore_index=-100)
            losses.append(float(crit(z, t.to(d))))
    I, Pr, T = tot
    s = 1e-6
    np.testing.assert_allclose(cd, ((2 * I + s) / (Pr + T + s)).numpy(), rtol=1e-12)
    np.testing.assert_allclose(ci, ((I + s) / (Pr + T - I + s)).numpy(), rtol=1e-12)
    seen = (Pr + T > 0).numpy()
    np.testing.assert_allclose([dice, iou], [np.mean(np.asarray(cd)[seen]), np.mean(np.asarray(ci)[seen])], rtol=1e-12)
    np.testing.assert_allclose(loss, np.mean(losses), rtol=1e-6)
    assert evaluate_model(m, test, crit, d, amp_dtype=torch.bfloat16, graph=False) == (loss, dice, iou)
    g = evaluate_model(m, test, crit, d, amp_dtype=torch.bfloat16, graph=None, per_class=True)
    np.testing.assert_allclose(g[:3], [loss, dice, iou], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(g[3], cd, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(g[4], ci, rtol=1e-5, atol=1e-6)
