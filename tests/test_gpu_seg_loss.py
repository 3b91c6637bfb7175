"""csu_seg_loss_* on the MI355X: the fused BCE + Tversky kernels against the fp64 restatement of
tests/test_seg_loss.py, their agreement with the BCE kernels, bitwise repeatability, and the
graph-captured train / eval routes a criterion with ``loss_stats`` takes.

Inputs are drawn in fp32 and upcast for the reference.  Row 0 carries test_bce_loss_vs_torch's edge
probabilities (0, 1, 1e-30, 1 - 1e-7, 0.5: the -100 log clamp and the 1e-12 gradient clamp); with
three rows or more, row 1 has an all-zero target and the last row an all-ones target (with two
rows the second is all ones).
Tolerances (tests/test_seg_loss.py): loss rtol 1e-5; gradient rtol 2e-6, atol 1e-7 * max|g_ref|
with the maximum taken over the unclamped elements only (the clamped ones reach 1e12 / n, which
would make the absolute term meaningless for every other element)."""
import copy

import numpy as np
import pytest
import torch

from test_seg_loss import LOSS_RTOL, PARAM_SETS, UPSTREAM, check_grad, make_criterion, ref_loss_grad

pytestmark = pytest.mark.gpu

# (1,1,5,3): under one vector and one workgroup; (3,1,37,41): row length 1517, rows 1 and 2 start off a
# 16-B boundary; (2,1,36,52): aligned rows, ragged last vector round; (33,1,8,8): more rows than the
# finish kernel has waves; (1030,1,3,3): more rows than the grid has workgroups, odd row length;
# (5,1,512,512): several chunks per row, a ragged last chunk, more than one round per thread
SHAPES = [(1, 1, 5, 3), (3, 1, 37, 41), (2, 1, 36, 52), (33, 1, 8, 8), (1030, 1, 3, 3), (5, 1, 512, 512)]

_CASES = {}


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def case(shape):
    """(p, t) fp32 on the CPU for a shape, made once."""
    if shape not in _CASES:
        g = torch.Generator().manual_seed(shape[0] * 1000 + shape[2])
        p = torch.rand(shape, generator=g)
        t = (torch.rand(shape, generator=g) > 0.6).float()
        B = shape[0]
        if B >= 3:
            t[1] = 0.0
        if B >= 2:
            t[-1] = 1.0
        pf, tf = p.view(-1), t.view(-1)
        pf[:7] = torch.tensor([0.0, 1.0, 1e-30, 1 - 1e-7, 0.5, 1.0, 0.0])
        tf[:7] = torch.tensor([1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0])
        _CASES[shape] = (p, t)
    return _CASES[shape]


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("ps", PARAM_SETS)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_vs_fp64(shape, ps, per_sample):
    d = dev()
    p, t = case(shape)
    crit = make_criterion(ps, per_sample)
    pa = p.to(d).requires_grad_(True)
    loss, stats = crit.loss_stats(pa, t.to(d))
    (loss * UPSTREAM).backward()
    ref, gref = ref_loss_grad(p, t, ps, per_sample)
    print(f"loss {float(loss):.9g} ref {float(ref):.9g} rel {abs(float(loss) - float(ref)) / abs(float(ref)):.2e}")
    torch.testing.assert_close(loss.detach().double().cpu(), ref, rtol=LOSS_RTOL, atol=0)
    pd = p.double()
    unclamped = pd * (1 - pd) >= 1e-12
    g = pa.grad.double().cpu()
    err = ((g - gref).abs() / gref.abs().clamp_min(1e-300))[unclamped]
    print(f"grad max rel err (unclamped) {float(err.max()):.2e}, max|g_ref| there {float(gref[unclamped].abs().max()):.3e}")
    check_grad(pa.grad, gref, unclamped)
    pred = (p > 0.5).double()
    assert torch.equal(stats.double().cpu(), torch.stack([(pred * t).sum(), pred.sum(), t.double().sum()]))


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_views_off_a_16_byte_boundary(offset):
    """p, t sharing an offset within 16 B (head peel), and p off by `offset` floats against t (scalar path)."""
    d = dev()
    p, t = case((2, 1, 36, 52))
    ps = PARAM_SETS[2]
    ref, gref = ref_loss_grad(p, t, ps, True)
    n = p.numel()
    for shift_t in (offset, 0):
        bp, bt = torch.zeros(n + 8, device=d), torch.zeros(n + 8, device=d)
        pv = bp[offset:offset + n].view(p.shape).copy_(p).requires_grad_(True)
        tv = bt[shift_t:shift_t + n].view(t.shape).copy_(t)
        assert pv.data_ptr() % 16 == 4 * offset and pv.is_contiguous()
        loss = make_criterion(ps, True)(pv, tv)
        (loss * UPSTREAM).backward()
        torch.testing.assert_close(loss.detach().double().cpu(), ref, rtol=LOSS_RTOL, atol=0)
        pd = p.double()
        check_grad(pv.grad, gref, pd * (1 - pd) >= 1e-12)


@pytest.mark.parametrize("shape", [(3, 1, 37, 41), (5, 1, 512, 512)])
def test_matches_bce_kernels(shape):
    """(bce=1, tversky=0, pos_weight=1) is ops.bce_loss: loss and gradient to rtol 1e-6, the
    thresholded sums equal to ops.bce_loss_stats' (0/1 sums, exact in fp32 at these sizes)."""
    from csu import ops
    d = dev()
    p, t = (v.to(d) for v in case(shape))
    crit = make_criterion(PARAM_SETS[0], False)
    pa, pb = p.clone().requires_grad_(True), p.clone().requires_grad_(True)
    la, sa = crit.loss_stats(pa, t)
    lb, sb = ops.bce_loss_stats(pb, t)
    torch.testing.assert_close(la, lb, rtol=1e-6, atol=0)
    assert torch.equal(sa, sb)
    la.backward()
    lb.backward()
    torch.testing.assert_close(pa.grad, pb.grad, rtol=1e-6, atol=0)


@pytest.mark.parametrize("per_sample", [False, True])
def test_bitwise_repeatable(per_sample):
    d = dev()
    p, t = (v.to(d) for v in case((5, 1, 512, 512)))
    crit = make_criterion(PARAM_SETS[2], per_sample)
    res = []
    for _ in range(2):
        pa = p.clone().requires_grad_(True)
        loss, stats = crit.loss_stats(pa, t)
        (loss * UPSTREAM).backward()
        res.append((loss.detach(), stats, pa.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_ops_seg_loss_argument_checks():
    from csu import ops
    from csu._lib import CsuError
    d = dev()
    p = torch.rand(2, 1, 4, 4, device=d)
    prm = (1.0, 1.0, 1.0, 0.5, 0.5, 0.5)
    with pytest.raises(CsuError):
        ops.seg_loss(p.cpu(), p.cpu(), prm, 1)
    with pytest.raises(ValueError):
        ops.seg_loss(p.double(), p.double(), prm, 1)
    with pytest.raises(ValueError):
        ops.seg_loss(p, p[:1], prm, 1)
    with pytest.raises(ValueError):
        ops.seg_loss(p, p, prm, 3)
    with pytest.raises(ValueError):
        ops.seg_loss(p, p, prm[:5], 1)
    with pytest.raises(CsuError, match="smooth"):      # refused by the C entry point before any launch
        ops.seg_loss(p, p, (1.0, 1.0, 1.0, 0.5, 0.5, 0.0), 1)


def _model_and_batches(nbatch, seed):
    from csu.data import ellipse_batch
    from csu.model import CSWinTransformer
    d = dev()
    torch.manual_seed(0)
    m0 = CSWinTransformer(img_size=128, split_size=[1, 2, 4, 4])
    rng = np.random.default_rng(seed)
    return d, m0, [tuple(v.to(d) for v in ellipse_batch(rng, 4, 128)) for _ in range(nbatch)]


def test_graphed_step_metrics_in_graph_seg_loss():
    """GraphedTrainStep(metrics=True) with bce_dice_loss(): the sums of the fused loss kernel inside
    the graph equal torch's on the step's output, the loss equals the criterion re-evaluated eagerly
    (tolerances of test_graphed_step_metrics_in_graph); a criterion without loss_stats still raises."""
    from csu.losses import bce_dice_loss
    from csu.train import GraphedTrainStep, make_optimizer
    d, m0, ((x, t),) = _model_and_batches(1, 2)
    m = m0.to(d)
    crit = bce_dice_loss()
    gs = GraphedTrainStep(m, make_optimizer(m, capturable=True), crit, x, t, torch.bfloat16, warmup=2, metrics=True)
    loss, out = gs(x, t)
    torch.cuda.synchronize()
    pred = (out > 0.5).double()
    ref = torch.stack([(pred * t).sum(), pred.sum(), t.double().sum()])
    torch.testing.assert_close(gs.stats.double(), ref, rtol=1e-6, atol=1e-3)
    torch.testing.assert_close(loss, crit(out, t).detach(), rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError, match="loss_stats"):
        GraphedTrainStep(m, make_optimizer(m, capturable=True), torch.nn.BCELoss(), x, t, torch.bfloat16, warmup=1,
                         metrics=True)


def test_graph_replays_bitwise_reproducible_seg_loss():
    """Two independent captures of the bf16 train step with bce_dice_loss() replayed on the same two
    batches for 5 steps: bitwise-equal losses and parameters."""
    from csu.losses import bce_dice_loss
    from csu.train import GraphedTrainStep, make_optimizer
    d, m0, batches = _model_and_batches(2, 1)
    res = []
    for _ in range(2):
        m = copy.deepcopy(m0).to(d)
        opt = make_optimizer(m, capturable=True)
        gs = GraphedTrainStep(m, opt, bce_dice_loss(), batches[0][0], batches[0][1], torch.bfloat16, warmup=2)
        losses = [float(gs(*batches[i % 2])[0].item()) for i in range(5)]
        torch.cuda.synchronize()
        res.append((losses, [p.detach().clone() for p in m.parameters()]))
        del gs, opt
    assert res[0][0] == res[1][0]
    names = [n for n, _ in m0.named_parameters()]
    diff = [(n, float((a - b).abs().max())) for n, a, b in zip(names, res[0][1], res[1][1]) if not torch.equal(a, b)]
    assert not diff, diff


def test_train_model_graphed_equals_eager_seg_loss():
    """train_model with SegLoss(per_sample=True): graph=None (captured train and eval steps through
    loss_stats, a ragged last batch eager) == graph=False over 2 epochs (tolerances of
    test_train_model_graphed_equals_eager)."""
    from csu.data import ellipse_batch
    from csu.losses import SegLoss
    from csu.model import CSWinTransformer
    from csu.train import make_optimizer, train_model
    d = dev()
    torch.manual_seed(0)
    m0 = CSWinTransformer(img_size=128, split_size=[1, 2, 4, 4])
    rng = np.random.default_rng(8)
    train = [ellipse_batch(rng, 4, 128) for _ in range(5)] + [ellipse_batch(rng, 2, 128)]
    test = [ellipse_batch(rng, 4, 128), ellipse_batch(rng, 3, 128)]
    hs, ps = [], []
    for graph in (None, False):
        m = copy.deepcopy(m0).to(d)
        opt = make_optimizer(m)
        hs.append(train_model(m, train, test, SegLoss(per_sample=True), opt, None, d, num_epochs=2, verbose=False,
                              graph=graph))
        ps.append([p.detach().clone() for p in m.parameters()])
    for k in hs[0]:
        np.testing.assert_allclose(hs[0][k], hs[1][k], rtol=1e-5, atol=1e-6, err_msg=k)
    for a, b in zip(*ps):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
