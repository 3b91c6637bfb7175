"""csu_seg_hard_* and csu_kth_largest on the MI355X: the fused hard-example loss (focal and top-k cross-entropy)
against the fp64 restatement of tests/test_seg_hard.py in every layout, logits dtype and label dtype the kernels
read; exact tie cases; the selection kernel against torch.sort on adversarial keys, bit for bit; the fraction
changed between replays of a captured graph; a captured train_model epoch.

Tolerances are those of tests/test_seg_hard.py (ten times torch's own fp32 error against fp64, measured at these
shapes; bf16 gradients get one bf16 rounding, rtol 2**-8, on top).  Every gradient case with a selection first
asserts the selection precondition of that file (margin >= 32).  The large shape (2,6,300,333) does not meet it
with the default seed, so with a selection it is checked for the loss value, k and repeatability; its gradients are
checked without a selection and at top_k = 1.0 (where every pixel is selected).

last_terms: k equals the reference's exactly everywhere.  tau is the kernel's own fp32 value of l at rank k and the
reference's is an fp64 value, so the two cannot agree to the bit; where the precondition holds they are compared
to ten times torch's fp32 error of l for the case (``check_tau``).  Exactness of tau itself is what
test_kth_largest_vs_sort checks, bit for bit, and the tie cases check k and f exactly."""
import copy

import numpy as np
import pytest
import torch

from test_gpu_seg_ce import LAYOUTS, SHAPES as CE_SHAPES, dev, place
from test_seg_ce import IGNORE, PARAM_SETS, UPSTREAM, make_case, make_criterion
from test_seg_hard import (GAMMAS, HARD_PARAM_SETS, MARGIN, TOP_KS, check_grad, check_loss, check_tau, make_hard_criterion,
                           rank_k, ref_hard_loss_grad, selection_margin, two_level_case, uniform_case)

pytestmark = pytest.mark.gpu

# test_gpu_seg_ce's shapes, and (2,5,33,33): HW = 1089 > 1024 gives two chunks per image, the second one ragged
LARGE = (2, 6, 300, 333)
SHAPES = CE_SHAPES[:-1] + [(2, 5, 33, 33), LARGE]

_REFS = {}


def ref(shape, dtype, gamma, top_k, ps, per_sample):
    """(z, t, loss, grad, stats, info, margin) on the CPU, made once per case and left unchanged."""
    key = (shape, dtype, gamma, top_k, HARD_PARAM_SETS.index(ps), per_sample)
    if key not in _REFS:
        z, t = make_case(shape, dtype=dtype)
        margin = float("inf") if top_k is None else selection_margin(z, t, ps[4], gamma, top_k)
        _REFS[key] = (z, t) + ref_hard_loss_grad(z, t, ps, per_sample, gamma, top_k) + (margin,)
    return _REFS[key]


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("ps", HARD_PARAM_SETS)
@pytest.mark.parametrize("top_k", TOP_KS)
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_vs_fp64(shape, dtype, gamma, top_k, ps, per_sample):
    d = dev()
    z, t, lref, gref, sref, info, margin = ref(shape, dtype, gamma, top_k, ps, per_sample)
    grads = shape != LARGE or top_k in (None, 1.0)
    if grads:
        assert margin >= MARGIN, margin
    crit = make_hard_criterion(shape[1], ps, per_sample, gamma, top_k)
    for layout in LAYOUTS:
        for lab in (torch.int64, torch.uint8):
            za = place(z, layout, d)
            loss, stats = crit.loss_stats(za, t.to(d).to(lab))
            (loss * UPSTREAM).backward()
            g = za.grad.double().cpu()
            lv, lt = float(loss.detach()), crit.last_terms.cpu()
            print(f"{layout} {lab}: loss {lv:.9g} ref {float(lref):.9g} rel {abs(lv - float(lref)) / abs(float(lref)):.2e}"
                  f"  grad err / max|g_ref| {float((g - gref).abs().max() / gref.abs().max()):.2e}"
                  f"  tau {float(lt[2]):.9g} ref {info['tau']:.9g}  k {int(lt[3])} margin {margin:.3g}")
            assert za.grad.dtype == dtype and lt.dtype == torch.float64 and lt.shape == (4,)
            check_loss(loss, lref)
            assert stats.dtype == torch.float64 and torch.equal(stats.cpu(), sref)
            assert float(lt[3]) == info["k"]
            if margin >= MARGIN:
                check_tau(lt[2], info)
            if grads:
                check_grad(za.grad, gref, bf16=dtype == torch.bfloat16)


# ---- ties ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("rho", [0.1, 0.37, 1.0])
def test_all_pixels_tied(rho, gamma, layout):
    """Every pixel has the same logits and label, whether a thread read it in a vector or alone, first or last in
    its chunk: one key value, k of n places shared equally, the loss of no selection and a uniform gradient."""
    d = dev()
    z, t = uniform_case((2, 3, 33, 35))        # HW = 1155: two chunks per image, rows off vector boundaries
    ps = HARD_PARAM_SETS[0]
    crit = make_hard_criterion(3, ps, False, gamma, rho)
    za, zb = place(z, layout, d), place(z, layout, d)
    la, lb = crit(za, t.to(d)), make_hard_criterion(3, ps, False, gamma, None)(zb, t.to(d))
    la.backward()
    lb.backward()
    lref, gref, _, info = ref_hard_loss_grad(z, t, ps, False, gamma, rho, upstream=1.0)
    n = t.numel()
    assert (info["k"], info["n_gt"], info["n_eq"]) == (rank_k(rho, n), 0, n)
    assert float(crit.last_terms[3]) == info["k"]
    check_loss(la, lref)
    check_loss(lb, lref)
    check_grad(za.grad, gref)
    assert torch.equal(za.grad, za.grad[:1, :, :1, :1].expand_as(za.grad))      # f is one number


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_two_level_map(gamma, layout):
    """k = 120 of 160 pixels: the 80 hard ones in full and the 80 tied easy ones with f = 0.5, exactly."""
    d = dev()
    z, t = two_level_case()
    ps = HARD_PARAM_SETS[0]
    crit = make_hard_criterion(3, ps, False, gamma, 0.75)
    za = place(z, layout, d)
    loss = crit(za, t.to(d))
    loss.backward()
    lref, gref, _, info = ref_hard_loss_grad(z, t, ps, False, gamma, 0.75, upstream=1.0)
    assert (info["k"], info["n_gt"], info["n_eq"], info["f"]) == (120, 80, 80, 0.5)
    assert float(crit.last_terms[3]) == 120
    check_tau(crit.last_terms[2], info)
    check_loss(loss, lref)
    check_grad(za.grad, gref)
    for b in (0, 1):
        assert torch.equal(za.grad[b], za.grad[b, :, :1, :1].expand_as(za.grad[b]))
    # f exactly 0.5: the easy level's gradient is half of that under k = n (f = 1) times the ratio of the denominators
    zc = place(z, layout, d)
    make_hard_criterion(3, ps, False, gamma, 1.0)(zc, t.to(d)).backward()
    torch.testing.assert_close(za.grad[1].double(), zc.grad[1].double() * (160 / 120) * 0.5, rtol=1e-6, atol=0.0)


# ---- edge cases ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("top_k", [None, 0.3])
@pytest.mark.parametrize("gamma", [0.5, 2.0])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_saturated_logits_stay_finite(layout, gamma, top_k):
    """Logits of +-80 and a spread of 1e4: u = 0 and l = 0 occur (many keys tie at +0), nothing overflows."""
    d = dev()
    z, t = make_case((2, 6, 16, 24), seed=12)
    z = torch.where(z > 0, torch.full_like(z, 80.0), torch.full_like(z, -80.0))
    z[0, :, :4] *= 125.0                       # +-1e4
    ps = HARD_PARAM_SETS[1]
    lref, gref, sref, info = ref_hard_loss_grad(z, t, ps, True, gamma, top_k)
    crit = make_hard_criterion(6, ps, True, gamma, top_k)
    za = place(z, layout, d)
    loss, stats = crit.loss_stats(za, t.to(d))
    (loss * UPSTREAM).backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(za.grad).all()) and bool(torch.isfinite(crit.last_terms).all())
    assert float(crit.last_terms[3]) == info["k"]
    check_loss(loss, lref)
    check_grad(za.grad, gref)
    assert torch.equal(stats.cpu(), sref)


@pytest.mark.parametrize("top_k", [None, 0.3])
def test_all_ignored_batch_is_zero_not_nan(top_k):
    d = dev()
    z, _ = make_case((2, 3, 7, 9))
    t = torch.full((2, 7, 9), IGNORE, dtype=torch.int64)
    for ps in HARD_PARAM_SETS:
        crit = make_hard_criterion(3, ps, False, 2.0, top_k)
        za = place(z, "nchw", d)
        loss, stats = crit.loss_stats(za, t.to(d))
        loss.backward()
        assert float(loss.detach()) == 0.0 and float(za.grad.abs().max()) == 0.0 and float(stats.abs().max()) == 0.0
        assert float(crit.last_terms.abs().max()) == 0.0


def test_nchw_views_off_a_16_byte_boundary():
    d = dev()
    shape, ps, gamma, rho = (2, 5, 36, 52), HARD_PARAM_SETS[1], 2.0, 0.3
    z, t = make_case(shape)
    assert selection_margin(z, t, ps[4], gamma, rho) >= MARGIN
    lref, gref, sref, info = ref_hard_loss_grad(z, t, ps, True, gamma, rho)
    for off in (1, 2, 3):
        buf = torch.zeros(z.numel() + 8, device=d)
        za = buf[off:off + z.numel()].view(shape).copy_(z).detach().requires_grad_(True)
        assert za.data_ptr() % 16 == 4 * off
        crit = make_hard_criterion(5, ps, True, gamma, rho)
        loss, stats = crit.loss_stats(za, t.to(d))
        (loss * UPSTREAM).backward()
        check_loss(loss, lref)
        check_grad(za.grad, gref)
        check_tau(crit.last_terms[2], info)
        assert float(crit.last_terms[3]) == info["k"] and torch.equal(stats.cpu(), sref)


@pytest.mark.parametrize("top_k", [None, 0.1])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_bitwise_repeatable(layout, top_k):
    d = dev()
    z, t = make_case(LARGE)
    crit = make_hard_criterion(6, HARD_PARAM_SETS[1], True, 2.0, top_k)
    td = t.to(d)
    res = []
    for _ in range(2):
        za = place(z, layout, d)
        loss, stats = crit.loss_stats(za, td)
        (loss * UPSTREAM).backward()
        res.append((loss.detach(), stats, za.grad, crit.last_terms))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (3, 5, 37, 41), LARGE])
def test_gamma_zero_without_selection_is_multiclass_seg_loss(shape, per_sample):
    d = dev()
    z, t = make_case(shape)
    ps = PARAM_SETS[2]
    za, zb = place(z, "nchw", d), place(z, "nchw", d)
    la = make_hard_criterion(shape[1], ps, per_sample, 0.0, None)(za, t.to(d))
    lb = make_criterion(shape[1], ps, per_sample)(zb, t.to(d))
    la.backward()
    lb.backward()
    check_loss(la, lb.detach().double().cpu())
    check_grad(za.grad, zb.grad.double().cpu())


def test_33_classes_take_the_torch_route_on_the_device():
    d = dev()
    z, t = make_case((2, 33, 9, 11))
    ps, gamma, rho = HARD_PARAM_SETS[1], 2.0, 0.3
    assert selection_margin(z, t, ps[4], gamma, rho) >= MARGIN
    lref, gref, sref, info = ref_hard_loss_grad(z, t, ps, False, gamma, rho)
    crit = make_hard_criterion(33, ps, False, gamma, rho)
    za = z.to(d).requires_grad_(True)
    loss, stats = crit.loss_stats(za, t.to(d))
    (loss * UPSTREAM).backward()
    assert loss.is_cuda and stats.is_cuda and crit.last_terms.is_cuda
    check_loss(loss, lref)
    check_grad(za.grad, gref)
    assert torch.equal(stats.cpu(), sref) and float(crit.last_terms[3]) == info["k"]


def test_ops_argument_checks():
    from csu import ops
    from csu._lib import CsuError
    d = dev()
    z = torch.randn(2, 3, 4, 4, device=d)
    t = torch.zeros(2, 4, 4, dtype=torch.int64, device=d)
    prm, rho = (1.0, 1.0, 0.5, 0.5, 0.5), torch.full((1,), 0.5, device=d)
    with pytest.raises(CsuError):
        ops.seg_hard(z.cpu(), t.cpu(), prm)
    with pytest.raises(CsuError):
        ops.seg_hard(z, t, prm, rho=rho.cpu())
    for a, b, p, kw in ((z.double(), t, prm, {}), (z, t.float(), prm, {}), (z, t[:1], prm, {}), (z, t, prm, dict(rows=3)),
                        (z, t, prm[:4], {}), (z[:, :1], t, prm, {}), (z, t, prm, dict(class_weight=torch.ones(2, device=d))),
                        (z, t, prm, dict(gamma=-1.0)), (z, t, prm, dict(gamma=float("nan"))), (z, t, prm, dict(rho=rho.double())),
                        (z, t, prm, dict(rho=torch.ones(2, device=d)))):
        with pytest.raises(ValueError):
            ops.seg_hard(a, b, p, **kw)
    with pytest.raises(CsuError, match="smooth"):
        ops.seg_hard(z, t, (1.0, 1.0, 0.5, 0.5, 0.0))
    with pytest.raises(CsuError):
        ops.kth_largest(z.cpu(), rho.cpu())
    for a, b in ((z.double(), rho), (z[:0], rho), (z, rho.double()), (z, torch.ones(2, device=d))):
        with pytest.raises(ValueError):
            ops.kth_largest(a, b)


# ---- the selection kernel -------------------------------------------------------------------------------

def _key_sets(n, g):
    """name -> n non-negative fp32 keys (as int32 bit patterns where that is what matters)."""
    bits = lambda v: v.to(torch.int32).view(torch.float32)
    ramp = torch.arange(n, 0, -1, dtype=torch.float32) * 0.37
    low = bits(0x3F800000 + torch.randint(0, 256, (n,), generator=g))
    top = bits(torch.randint(0, 0x7F, (n,), generator=g) << 24)
    zeros = torch.where(torch.rand(n, generator=g) < 0.6, torch.zeros(n), torch.rand(n, generator=g))
    den = bits(torch.randint(0, 1 << 23, (n,), generator=g))                          # denormals and +0
    den = torch.where(torch.rand(n, generator=g) < 0.3, torch.rand(n, generator=g), den)
    inf = torch.where(torch.rand(n, generator=g) < 0.2, torch.full((n,), float("inf")), torch.rand(n, generator=g) * 9.0)
    mixed = torch.rand(n, generator=g) * 5.0
    mixed = torch.where(torch.rand(n, generator=g) < 0.4, -1.0 - mixed, mixed)        # skipped entries
    return {"equal": torch.full((n,), 0.7310586), "low_byte": low, "top_byte": top, "ramp": ramp, "zeros": zeros,
            "denormals": den, "inf": inf, "skipped": mixed}


def _kth_ref(keys, rho):
    """(tau bits, n_gt, n_eq, k, n) by torch.sort on the CPU."""
    live = keys.view(torch.int32) >= 0
    lv = keys[live].view(torch.int32)
    n = int(lv.numel())
    k = rank_k(rho, n)
    if n == 0:
        return 0, 0, 0, 0, 0
    tau = int(torch.sort(lv, descending=True).values[k - 1])
    return tau, int((lv > tau).sum()), int((lv == tau).sum()), k, n


@pytest.mark.parametrize("n", [1, 2, 255, 257, 70001])
def test_kth_largest_vs_sort(n):
    """Exact: the bits of tau, n_gt, n_eq, k and n, for k = 1, k = n and k near n / 2, on keys that are all equal,
    differ in one byte only, descend, hold zeros, denormals, +inf, and skipped (negative) entries; from a buffer on
    a 16-B boundary and from one 4 B off it."""
    from csu import ops
    d = dev()
    g = torch.Generator().manual_seed(n)
    for name, keys in _key_sets(n, g).items():
        buf = torch.empty(n + 1, device=d)
        for off in (0, 1):
            kd = buf[off:off + n].copy_(keys)
            for rho in (1e-9, 0.5, 1.0):
                out = ops.kth_largest(kd, torch.full((1,), rho, device=d)).cpu()
                want = _kth_ref(keys, rho)
                got = (int(out[0].float().view(torch.int32)),) + tuple(int(v) for v in out[1:])
                assert got == want, (name, off, rho, got, want)


def test_kth_largest_nothing_live_and_nan_keys():
    from csu import ops
    d = dev()
    out = ops.kth_largest(torch.full((300,), -2.0, device=d), torch.full((1,), 0.5, device=d))
    assert float(out.abs().max()) == 0.0
    keys = torch.rand(300)
    keys[::7] = float("nan")           # a caller error; sorts by its bits (above +inf) and must not fault
    out = ops.kth_largest(keys.to(d), torch.full((1,), 0.5, device=d)).cpu()
    want = _kth_ref(keys, 0.5)
    assert (int(out[0].float().view(torch.int32)),) + tuple(int(v) for v in out[1:]) == want


# ---- graphs and the train loop --------------------------------------------------------------------------

def test_set_top_k_between_replays_of_a_captured_graph():
    d = dev()
    shape, ps = (2, 5, 33, 33), HARD_PARAM_SETS[1]
    z, t = make_case(shape)
    td = t.to(d)
    eager = []
    for rho in (0.3, 0.1):
        za = place(z, "nchw", d)
        c = make_hard_criterion(5, ps, True, 2.0, rho)
        loss = c(za, td)
        loss.backward()
        eager.append((loss.detach().clone(), za.grad.clone(), c.last_terms.clone()))
    crit = make_hard_criterion(5, ps, True, 2.0, 0.3)
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
    for rho, want in zip((0.3, 0.1), eager):
        crit.set_top_k(rho)
        graph.replay()
        assert torch.equal(loss.detach(), want[0]) and torch.equal(zs.grad, want[1])
        assert torch.equal(crit.last_terms, want[2])


def test_train_model_graphed_equals_eager_dice_topk():
    """train_model on the 3-class logits-head model of test_gpu_seg_ce under bf16 autocast with dice_topk_loss and a
    schedule: the captured run's history has top_k, and Dice / IoU equal the eager run's."""
    from csu.losses import dice_topk_loss
    from csu.train import make_optimizer, train_model
    from test_gpu_seg_ce import _multiclass_setup
    d, m0, train, test = _multiclass_setup()
    hs = []
    for graph in (True, False):
        m = copy.deepcopy(m0).to(d)
        opt = make_optimizer(m)
        crit = dice_topk_loss(3, top_k=0.5, schedule=lambda e: 0.25)
        hs.append(train_model(m, train, test, crit, opt, None, d, num_epochs=1, verbose=False, amp_dtype=torch.bfloat16,
                              graph=graph))
    assert hs[0]["top_k"] == [0.25] and hs[1]["top_k"] == [0.25]
    assert set(hs[0]) == set(hs[1]) and "train_class_dice" in hs[0]
    for k in hs[0]:
        np.testing.assert_allclose(hs[0][k], hs[1][k], rtol=1e-5, atol=1e-6, err_msg=k)
    assert 0.0 < hs[0]["test_dice"][0] <= 1.0 and np.isfinite(hs[0]["train_loss"][0])
