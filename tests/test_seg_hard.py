"""csu.losses.HardExampleSegLoss on the CPU (focal and top-k cross-entropy in the fused multi-class loss) against an
fp64 restatement of its formula with a sort-based selection and the tie rule, its three limit identities, the
textbook focal loss, exact tie cases, the constructor's checks, the schedule, and the new C-ABI entry points.

The fp64 restatement (``ref_hard_loss_grad``) and the selection precondition (``selection_margin``) are shared with
tests/test_gpu_seg_hard.py.

Tolerances, derived as in tests/test_seg_ce.py.  torch's own fp32 composition of the formula
(``HardExampleSegLoss._torch`` on fp32 logits) was measured on the CPU against the fp64 restatement at every shape
of SHAPES here and of the GPU file, both logits dtypes, and every (gamma, top_k, parameter set, per_sample) of the
grid below, and at the other shapes that file uses ((2,33,9,11), (2,5,36,52)) (gradients: where the GPU file checks
them).  The largest relative loss error was 1.76e-7 ((2,33,9,11) fp32, gamma 2, top_k 0.3, weighted CE + Tversky, per
sample) and the largest gradient error 9.28e-6 of max|g_ref| ((2,33,9,11) bf16 values, gamma 2, top_k 0.1, CE only:
torch's pow backward in fp32).  Ten times that: LOSS_RTOL 1.8e-6 and an absolute gradient tolerance of GRAD_ATOL_REL =
9.3e-5 times max|g_ref| with no relative term; bf16 gradients get one bf16 rounding (rtol 2**-8) on top.

Selection precondition.  A hard selection is discontinuous, so a gradient comparison with ``top_k`` is only
meaningful when fp32 rounding cannot move a pixel across the threshold: ``selection_margin`` gives the gap between
the k-th and (k+1)-th largest l in fp64 over the largest |l_fp32 - l_fp64| of the case, and every gradient case with
a selection asserts that it is at least 32.  With ``make_case``'s default seeds this holds at every shape but the
large one for rho in {0.1, 0.3} and both logits dtypes (the smallest ratio measured is 67.8, at (1030,4,3,3) fp32,
gamma 0.5, rho 0.3, weighted); the large shape (2,6,300,333) is used for the
loss value, repeatability and gradients without a selection only."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from test_seg_ce import IGNORE, SMOOTH, UPSTREAM, class_weights, make_case, ref_hard_stats

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOSS_RTOL = 1.8e-6
GRAD_ATOL_REL = 9.3e-5
BF16_RTOL = 2.0 ** -8
MARGIN = 32.0
GAMMAS = [0.0, 0.5, 2.0]
TOP_KS = [None, 0.1, 0.3, 1.0]
# (ce, tversky, alpha, beta, weighted, include_background): CE term only; weighted CE term + Tversky(0.3, 0.7)
HARD_PARAM_SETS = [(1.0, 0.0, 0.5, 0.5, False, True), (0.5, 1.0, 0.3, 0.7, True, False)]
SHAPES = [(1, 2, 3, 5), (2, 3, 7, 9), (3, 5, 37, 41)]


def make_hard_criterion(K, ps, per_sample, gamma, top_k, ignore_index=IGNORE, smooth=SMOOTH):
    from csu.losses import HardExampleSegLoss
    ce, tv, alpha, beta, weighted, bg = ps
    return HardExampleSegLoss(K, ce=ce, tversky=tv, alpha=alpha, beta=beta, smooth=smooth,
                              class_weight=class_weights(K) if weighted else None, ignore_index=ignore_index,
                              per_sample=per_sample, include_background=bg, gamma=gamma, top_k=top_k)


def pixel_terms(z, t, weighted, gamma, ignore_index=IGNORE):
    """(l, w[t], live) per pixel, flattened, in z's floating dtype: l = w[t] u^gamma L of the live pixels, 0 elsewhere."""
    K = z.shape[1]
    w = torch.tensor(class_weights(K), dtype=z.dtype) if weighted else torch.ones(K, dtype=z.dtype)
    live = t != ignore_index
    tc = torch.where(live, t, torch.zeros_like(t))
    lsm = torch.log_softmax(z, 1)
    L = -lsm.gather(1, tc.unsqueeze(1)).squeeze(1)
    oh = F.one_hot(tc, K).movedim(-1, 1).to(z.dtype)
    u = (lsm.exp() * (1.0 - oh)).sum(1)
    if gamma == 0.0:
        ug = torch.ones_like(u)
    else:
        safe = torch.where(u > 0, u, torch.ones_like(u))
        ug = torch.where(u > 0, safe.pow(gamma), torch.zeros_like(u))
    wt = w[tc] * live.to(z.dtype)
    return (wt * ug * L).reshape(-1), wt.reshape(-1), live.reshape(-1)


def rank_k(rho, n):
    """k = max(1, floor(double(float32(rho)) n)), at most n; 0 when n = 0."""
    if n == 0:
        return 0
    r32 = float(torch.tensor(rho, dtype=torch.float32))
    return min(n, max(1, int(r32 * n // 1)))


def select(l, live, rho):
    """(m, tau, k, n_gt, n_eq, f) of the tie rule on the values l (a 1-D tensor) of the live pixels."""
    n = int(live.sum())
    k = rank_k(rho, n)
    m = torch.zeros_like(l)
    if k == 0:
        return m, 0.0, 0, 0, 0, 0.0
    lv = l.detach()[live]
    tau = torch.sort(lv, descending=True).values[k - 1]
    n_gt, n_eq = int((lv > tau).sum()), int((lv == tau).sum())
    f = (k - n_gt) / n_eq
    m = torch.where(live & (l.detach() > tau), torch.ones_like(l), m)
    m = torch.where(live & (l.detach() == tau), torch.full_like(l, f), m)
    return m, float(tau), k, n_gt, n_eq, f


def ref_hard_loss_grad(z, t, ps, per_sample, gamma, top_k, ignore_index=IGNORE, smooth=SMOOTH, upstream=UPSTREAM):
    """fp64 (loss, d(upstream * loss)/dz, (3, K) hard sums, info) for logits z (fp32 or bf16, upcast exactly) and
    int64 labels t; info = dict(hce, tau, k, n_gt, n_eq, f, l_err), l_err = the largest |l_fp32 - l_fp64| of torch's
    fp32 composition of l.  Selection by a sort, ties by the rule, gradient by autograd with the selection weights
    held constant."""
    ce, tv, alpha, beta, weighted, bg = ps
    B, K = z.shape[0], z.shape[1]
    z64 = z.detach().double().requires_grad_(True)
    l, wt, live = pixel_terms(z64, t, weighted, gamma, ignore_index)
    if top_k is None:
        m, tau, k, n_gt, n_eq, f = live.double(), 0.0, int(live.sum()), 0, 0, 1.0
    else:
        m, tau, k, n_gt, n_eq, f = select(l, live, top_k)
    num, W = (m * l).sum(), (m * wt).sum()
    hce = num / W if float(W) > 0 else num * 0.0
    rows = B if per_sample else 1
    lv = (t != ignore_index).unsqueeze(1).double()
    p = torch.softmax(z64, 1) * lv
    oh = F.one_hot(torch.where(t != ignore_index, t, torch.zeros_like(t)), K).movedim(-1, 1).double() * lv
    if rows == B:
        pr, tr = p.reshape(B, K, -1), oh.reshape(B, K, -1)
    else:
        pr, tr = p.transpose(0, 1).reshape(1, K, -1), oh.transpose(0, 1).reshape(1, K, -1)
    tp, sp, st = (pr * tr).sum(-1), pr.sum(-1), tr.sum(-1)
    ti = (tp + smooth) / ((1.0 - alpha - beta) * tp + alpha * sp + beta * st + smooth)
    classes = slice(None) if bg else slice(1, None)
    loss = ce * hce + tv * (1.0 - ti)[:, classes].mean()
    (grad,) = torch.autograd.grad(loss * upstream, z64)
    l32, _, _ = pixel_terms(z.detach().float(), t, weighted, gamma, ignore_index)
    l_err = float((l32.double() - l.detach())[live].abs().max()) if bool(live.any()) else 0.0
    info = dict(hce=float(hce.detach()), tau=tau, k=k, n_gt=n_gt, n_eq=n_eq, f=f, l_err=l_err)
    return loss.detach(), grad, ref_hard_stats(z, t, ignore_index), info


def selection_margin(z, t, weighted, gamma, rho, ignore_index=IGNORE):
    """(gap between the k-th and (k+1)-th largest l in fp64) / (largest |l_fp32 - l_fp64|); inf when k = n."""
    l64, _, live = pixel_terms(z.detach().double(), t, weighted, gamma, ignore_index)
    l32, _, _ = pixel_terms(z.detach().float(), t, weighted, gamma, ignore_index)
    n = int(live.sum())
    k = rank_k(rho, n)
    if k == 0 or k == n:
        return float("inf")
    s = torch.sort(l64[live], descending=True).values
    err = float((l32.double() - l64)[live].abs().max())
    return float(s[k - 1] - s[k]) / err if err > 0 else float("inf")


def check_tau(tau, info):
    """tau is an fp32 value of l formed by the code under test, the reference's an fp64 one: they agree to the fp32
    error of l (ten times torch's own, as the other tolerances), not to the bit."""
    assert abs(float(tau) - info["tau"]) <= 10.0 * info["l_err"], (float(tau), info)


def check_loss(loss, ref):
    torch.testing.assert_close(loss.detach().double().cpu(), ref, rtol=LOSS_RTOL, atol=1e-12)


def check_grad(g, g_ref, bf16=False):
    scale = float(g_ref.abs().max())
    torch.testing.assert_close(g.double().cpu(), g_ref, rtol=BF16_RTOL if bf16 else 0.0, atol=GRAD_ATOL_REL * scale)


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("ps", HARD_PARAM_SETS)
@pytest.mark.parametrize("top_k", TOP_KS)
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_path_vs_fp64(shape, gamma, top_k, ps, per_sample):
    z, t = make_case(shape)
    if top_k is not None:
        assert selection_margin(z, t, ps[4], gamma, top_k) >= MARGIN
    crit = make_hard_criterion(shape[1], ps, per_sample, gamma, top_k)
    za = z.clone().requires_grad_(True)
    loss, stats = crit.loss_stats(za, t)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (loss * UPSTREAM).backward()
    ref, gref, sref, info = ref_hard_loss_grad(z, t, ps, per_sample, gamma, top_k)
    check_loss(loss, ref)
    check_grad(za.grad, gref)
    assert torch.equal(stats, sref)
    lt = crit.last_terms
    assert lt.dtype == torch.float64 and lt.shape == (4,) and not lt.requires_grad
    assert float(lt[3]) == info["k"]
    check_tau(lt[2], info)
    torch.testing.assert_close(float(lt[0]), info["hce"], rtol=LOSS_RTOL, atol=1e-12)
    assert torch.equal(crit(z, t.unsqueeze(1).to(torch.uint8)), loss.detach())
    assert float(za.grad[t.unsqueeze(1).expand_as(z) == IGNORE].abs().max()) == 0.0


# ---- the three limit identities --------------------------------------------------------------------

@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_top_k_one_is_no_selection(shape, gamma):
    z, t = make_case(shape)
    ps = HARD_PARAM_SETS[1]
    res = []
    for top_k in (1.0, None):
        za = z.clone().requires_grad_(True)
        loss = make_hard_criterion(shape[1], ps, False, gamma, top_k)(za, t)
        loss.backward()
        res.append((loss.detach(), za.grad))
    torch.testing.assert_close(res[0][0], res[1][0], rtol=LOSS_RTOL, atol=0.0)
    check_grad(res[0][1], res[1][1].double())


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_gamma_zero_without_selection_is_multiclass_seg_loss(shape, per_sample):
    from test_seg_ce import PARAM_SETS, make_criterion
    z, t = make_case(shape)
    ps = PARAM_SETS[2]
    za, zb = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    la = make_hard_criterion(shape[1], ps, per_sample, 0.0, None)(za, t)
    lb = make_criterion(shape[1], ps, per_sample)(zb, t)
    la.backward()
    lb.backward()
    torch.testing.assert_close(la.detach(), lb.detach(), rtol=LOSS_RTOL, atol=0.0)
    check_grad(za.grad, zb.grad.double())


@pytest.mark.parametrize("shape,rho", [((2, 3, 8, 10), 0.25), ((1, 4, 10, 10), 0.1), ((3, 5, 20, 20), 0.5)])
def test_topk_ce_is_torch_topk_mean(shape, rho):
    """Unit weights, nothing ignored, rho n an integer: exactly nnU-Net's TopKLoss."""
    from csu.losses import topk_ce_loss
    B, K, H, W = shape
    g = torch.Generator().manual_seed(3)
    z = torch.randn(shape, generator=g) * 3.0
    t = torch.randint(0, K, (B, H, W), generator=g)
    k = int(rho * B * H * W)
    assert k == rho * B * H * W
    crit = topk_ce_loss(K, top_k=rho)
    loss = crit(z, t)
    want = torch.topk(F.cross_entropy(z.double(), t, reduction="none").view(-1), k).values.mean()
    torch.testing.assert_close(loss.double(), want, rtol=LOSS_RTOL, atol=0.0)
    assert float(crit.last_terms[3]) == k


@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0, 3.0])
def test_focal_loss_is_the_textbook_formula(gamma):
    from csu.losses import focal_loss
    z, t = make_case((2, 4, 9, 11), seed=8)
    live = t != IGNORE
    pt = torch.softmax(z.double(), 1).gather(1, torch.where(live, t, torch.zeros_like(t)).unsqueeze(1)).squeeze(1)
    want = (-(1.0 - pt) ** gamma * pt.log())[live].mean()
    loss = focal_loss(4, gamma=gamma, ignore_index=IGNORE)(z, t)
    torch.testing.assert_close(loss.double(), want, rtol=LOSS_RTOL, atol=0.0)


# ---- ties ----------------------------------------------------------------------------------------------

def uniform_case(shape=(2, 3, 6, 7)):
    B, K, H, W = shape
    z = torch.tensor([0.5, -1.25, 2.0])[:K].view(1, K, 1, 1).expand(shape).contiguous()
    t = torch.ones(B, H, W, dtype=torch.int64)
    return z, t


def two_level_case(shape=(2, 3, 8, 10)):
    """Half the pixels (image 0) hard, half (image 1) easy, every pixel of a level identical."""
    B, K, H, W = shape
    z = torch.empty(shape)
    z[0] = torch.tensor([2.0, -1.0, 0.5]).view(K, 1, 1)      # label 1: the hard half
    z[1] = torch.tensor([-1.0, 3.0, 0.25]).view(K, 1, 1)     # label 1: the easy half
    t = torch.ones(B, H, W, dtype=torch.int64)
    return z, t


@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("rho", [0.1, 0.37, 1.0])
def test_all_pixels_tied(rho, gamma):
    """Every pixel has the same logits and label: the loss is that of no selection and the gradient is uniform."""
    z, t = uniform_case()
    ps = HARD_PARAM_SETS[0]
    za, zb = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    crit = make_hard_criterion(3, ps, False, gamma, rho)
    la, lb = crit(za, t), make_hard_criterion(3, ps, False, gamma, None)(zb, t)
    la.backward()
    lb.backward()
    n = t.numel()
    assert float(crit.last_terms[3]) == rank_k(rho, n)
    torch.testing.assert_close(la.detach(), lb.detach(), rtol=LOSS_RTOL, atol=0.0)
    check_grad(za.grad, zb.grad.double())
    assert torch.equal(za.grad, za.grad[:1, :, :1, :1].expand_as(za.grad))


@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_two_level_map(gamma):
    """rho = 0.75 of 160 pixels: k = 120 takes the 80 hard pixels and 40 of the 80 tied easy ones, f = 0.5; the
    gradient of an easy pixel is half of what it would be if the pixel counted in full."""
    z, t = two_level_case()
    ps = HARD_PARAM_SETS[0]
    crit = make_hard_criterion(3, ps, False, gamma, 0.75)
    za = z.clone().requires_grad_(True)
    loss = crit(za, t)
    loss.backward()
    ref, gref, _, info = ref_hard_loss_grad(z, t, ps, False, gamma, 0.75, upstream=1.0)
    assert (info["k"], info["n_gt"], info["n_eq"], info["f"]) == (120, 80, 80, 0.5)
    assert float(crit.last_terms[3]) == 120
    check_loss(loss, ref)
    check_grad(za.grad, gref)
    for b in (0, 1):      # uniform per level
        assert torch.equal(za.grad[b], za.grad[b, :, :1, :1].expand_as(za.grad[b]))
    # the easy level against the same pixels counted in full: W = 80 + 0.5 * 80 = 120 either way
    l, _, _ = pixel_terms(z.double(), t, False, gamma)
    want = (80 * float(l[0]) + 40 * float(l[-1])) / 120
    torch.testing.assert_close(float(loss), want, rtol=LOSS_RTOL, atol=0.0)
    zc = z.clone().requires_grad_(True)
    full = make_hard_criterion(3, ps, False, gamma, None)(zc, t)
    full.backward()
    torch.testing.assert_close(za.grad[1].double(), zc.grad[1].double() * (160 / 120) * 0.5, rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(za.grad[0].double(), zc.grad[0].double() * (160 / 120), rtol=1e-5, atol=1e-9)


# ---- edge cases and the interface ----------------------------------------------------------------------

@pytest.mark.parametrize("top_k", [None, 0.3])
@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_all_ignored_batch_is_zero_not_nan(gamma, top_k):
    z, _ = make_case((2, 3, 7, 9))
    t = torch.full((2, 7, 9), IGNORE, dtype=torch.int64)
    for ps in HARD_PARAM_SETS:
        crit = make_hard_criterion(3, ps, False, gamma, top_k)
        za = z.clone().requires_grad_(True)
        loss, stats = crit.loss_stats(za, t)
        loss.backward()
        assert float(loss.detach()) == 0.0 and float(za.grad.abs().max()) == 0.0 and float(stats.abs().max()) == 0.0
        assert float(crit.last_terms[3]) == 0.0


@pytest.mark.parametrize("kw", [dict(gamma=-0.5), dict(gamma=float("inf")), dict(gamma=float("nan")), dict(top_k=0.0),
                                dict(top_k=1.5), dict(top_k=-0.1), dict(top_k=float("nan")), dict(top_k=True),
                                dict(schedule=3), dict(schedule=lambda e: 0.1), dict(ce=-1.0), dict(ce=0.0, tversky=0.0),
                                dict(smooth=0.0)])
def test_constructor_rejects(kw):
    from csu.losses import HardExampleSegLoss
    with pytest.raises(ValueError):
        HardExampleSegLoss(3, **kw)


def test_set_top_k_schedule_and_on_epoch():
    from csu.losses import HardExampleSegLoss, dice_topk_loss
    z, t = make_case((2, 3, 7, 9))
    crit = dice_topk_loss(3, top_k=0.5, ignore_index=IGNORE, schedule=lambda e: max(0.1, 0.5 - 0.2 * e))
    assert crit.top_k == 0.5
    a = crit(z, t)
    crit.on_epoch(1)
    assert crit.top_k == pytest.approx(0.3)
    b = crit(z, t)
    want = dice_topk_loss(3, top_k=0.3, ignore_index=IGNORE)(z, t)
    assert torch.equal(b, want) and not torch.equal(a, b)
    crit.on_epoch(5)
    assert crit.top_k == 0.1
    crit.set_top_k(1.0)
    assert crit.top_k == 1.0
    for bad in (0.0, 1.01, float("nan")):
        with pytest.raises(ValueError):
            crit.set_top_k(bad)
    plain = HardExampleSegLoss(3, gamma=2.0)
    assert plain.top_k is None
    plain.on_epoch(0)
    with pytest.raises(ValueError):
        plain.set_top_k(0.5)
    assert "gamma=2.0" in repr(plain) and "top_k=None" in repr(plain)


def test_helpers_are_exported_and_hashable():
    import csu
    for name in ("HardExampleSegLoss", "focal_loss", "dice_focal_loss", "topk_ce_loss", "dice_topk_loss"):
        assert name in csu.__all__ and hasattr(csu, name)
    c = csu.dice_focal_loss(4)
    assert isinstance(c, csu.HardExampleSegLoss) and isinstance(c, csu.MultiClassSegLoss)
    assert (c.gamma, c.top_k, c.ce, c.tversky, c.smooth) == (2.0, None, 1.0, 1.0, 0.5)
    assert csu.focal_loss(4).tversky == 0.0 and csu.topk_ce_loss(4).top_k == 0.1 and csu.dice_topk_loss(4).top_k == 0.1
    assert {c: 1}[c] == 1


def test_abi_declares_and_exports_seg_hard_and_kth_largest():
    from csu import _lib
    names = ["csu_kth_largest_workspace", "csu_kth_largest", "csu_seg_hard_workspace", "csu_seg_hard_fwd", "csu_seg_hard_bwd"]
    with open(os.path.join(REPO, "include", "csu.h")) as f:
        header = f.read()
    for n in names:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib._SIGS, n
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n), n
    assert len(_lib._SIGS["csu_seg_hard_fwd"][1]) == 30 and len(_lib._SIGS["csu_seg_hard_bwd"][1]) == 23
    assert len(_lib._SIGS["csu_kth_largest"][1]) == 7
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    # refused on the host before any launch: gamma < 0, rho without keys, a null terms, a short workspace
    def fwd(gamma=2.0, rho=q, keys=q, terms=q, nws=1 << 20):
        return lib.csu_seg_hard_fwd(2, 3, 8, 2, 0, q, 24, 8, 1, 0, 1, q, -100, None, 1.0, 1.0, 0.5, 0.5, 0.5, 1, gamma, rho, keys,
                                    q, terms, q, q, q, nws, None)
    assert fwd(gamma=-1.0) == -1 and fwd(gamma=float("inf")) == -1 and fwd(keys=None) == -1 and fwd(rho=None) == -1
    assert fwd(terms=None) == -1 and fwd(nws=64) == -3
    assert lib.csu_seg_hard_bwd(2, 3, 8, 2, 0, q, 24, 8, 1, 0, 1, q, -100, None, q, q, 1.0, 1.0, 1, -1.0, q, q, None) == -1
    assert lib.csu_kth_largest(0, q, q, q, q, 1 << 20, None) == -1 and lib.csu_kth_largest(8, q, None, q, q, 1 << 20, None) == -1
    assert lib.csu_kth_largest(8, q, q, q, q, 8, None) == -3
    assert lib.csu_kth_largest_workspace(0) == 0 and lib.csu_kth_largest_workspace(1000) % 8 == 0
    assert lib.csu_seg_hard_workspace(2, 33, 100) == 0 and lib.csu_seg_hard_workspace(0, 3, 100) == 0
    # the kth-largest workspace, 6 doubles, and (2 + 5 K) + 3 floats per item (2 images of one chunk each)
    # (rounded up to 8 bytes)
    assert lib.csu_seg_hard_workspace(2, 3, 100) == lib.csu_kth_largest_workspace(200) + 48 + 2 * (17 + 3) * 4
    assert lib.csu_seg_hard_workspace(1, 2, 15) == lib.csu_kth_largest_workspace(15) + 48 + (12 + 3) * 4 + 4
