"""csu.losses.MultiClassSegLoss on the CPU (softmax CE + per-class Tversky / Dice on integer label
maps) against an fp64 restatement of its formula, its relation to F.cross_entropy and to the binary
dice_loss, the constructor's checks, the three csu_seg_ce_* C-ABI entry points, and the multi-class
pieces of csu.train and csu.data.

The fp64 restatement (``ref_ce_loss_grad``) is shared with tests/test_gpu_seg_ce.py.

Tolerances.  torch's own fp32 composition of the formula (``MultiClassSegLoss._torch`` on fp32
logits) was measured on the CPU against the fp64 restatement at every shape of SHAPES here and of the
GPU file (and the 33-class one), every parameter set and both ``per_sample`` settings: the largest
relative loss error was 1.46e-7 ((2,6,300,333), CE only) and the largest gradient error 1.10e-6 of
max|g_ref| ((2,6,300,333), Dice only).  Ten times that (the precedent of tests/test_seg_loss.py)
allows another summation order: LOSS_RTOL 1.5e-6, and an absolute gradient tolerance of
GRAD_ATOL_REL = 1.1e-5 times max|g_ref| with no relative term (a relative one would say nothing
about the many softmax-suppressed elements).  For bf16 logits the reference takes the bf16 values
upcast exactly and the gradient, which the kernel writes in bf16, gets one bf16 rounding on top: rtol 2**-8."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IGNORE = 255            # representable in uint8 labels too
UPSTREAM = 0.37
LOSS_RTOL = 1.5e-6
GRAD_ATOL_REL = 1.1e-5
BF16_RTOL = 2.0 ** -8
SMOOTH = 0.5
# (ce, tversky, alpha, beta, weighted, include_background): CE only, Dice only, weighted CE + Tversky(0.3, 0.7)
PARAM_SETS = [(1.0, 0.0, 0.5, 0.5, False, True), (0.0, 1.0, 0.5, 0.5, False, True), (0.5, 1.0, 0.3, 0.7, True, False)]
SHAPES = [(1, 2, 3, 5), (2, 3, 7, 9), (3, 5, 37, 41)]


def class_weights(K):
    return [0.5 + 0.75 * (c % 3) for c in range(K)]


def make_criterion(K, ps, per_sample, ignore_index=IGNORE, smooth=SMOOTH):
    from csu.losses import MultiClassSegLoss
    ce, tv, alpha, beta, weighted, bg = ps
    return MultiClassSegLoss(K, ce=ce, tversky=tv, alpha=alpha, beta=beta, smooth=smooth,
                             class_weight=class_weights(K) if weighted else None, ignore_index=ignore_index,
                             per_sample=per_sample, include_background=bg)


def make_case(shape, seed=None, dtype=torch.float32):
    """(logits (B, K, H, W) in dtype, labels (B, H, W) int64): logits N(0, 3^2); about 10 % of the
    pixels ignored; with K >= 5 the last class is absent from the labels; with B >= 3 image 1 is
    ignored entirely."""
    B, K, H, W = shape
    g = torch.Generator().manual_seed(B * 1000 + K * 37 + H if seed is None else seed)
    z = (torch.randn(shape, generator=g) * 3.0).to(dtype)
    t = torch.randint(0, K - 1 if K >= 5 else K, (B, H, W), generator=g)
    t[torch.rand(B, H, W, generator=g) < 0.1] = IGNORE
    if B >= 3:
        t[1] = IGNORE
    return z, t


def first_max(z):
    """argmax over dim 1 by the explicit rule: ascending classes, a strictly larger value wins."""
    best = z[:, 0].clone()
    arg = torch.zeros_like(best, dtype=torch.int64)
    for k in range(1, z.shape[1]):
        up = z[:, k] > best
        best = torch.where(up, z[:, k], best)
        arg = torch.where(up, torch.full_like(arg, k), arg)
    return arg


def ref_hard_stats(z, t, ignore_index=IGNORE):
    K = z.shape[1]
    pred, live = first_max(z.double()), t != ignore_index
    rows = [[((pred == c) & (t == c) & live).sum() for c in range(K)], [((pred == c) & live).sum() for c in range(K)],
            [((t == c) & live).sum() for c in range(K)]]
    return torch.tensor([[int(v) for v in r] for r in rows], dtype=torch.float64)


def ref_ce_loss_grad(z, t, ps, per_sample, ignore_index=IGNORE, smooth=SMOOTH, upstream=UPSTREAM):
    """fp64 loss, d(upstream * loss)/dz and the (3, K) hard sums for logits z (fp32 or bf16, upcast
    exactly) and int64 labels t.  CE = F.cross_entropy(sum) / sum w (0 when sum w = 0); the Tversky
    part is differentiated by autograd."""
    ce, tv, alpha, beta, weighted, bg = ps
    B, K = z.shape[0], z.shape[1]
    z64 = z.detach().double().requires_grad_(True)
    w = torch.tensor(class_weights(K), dtype=torch.float64) if weighted else torch.ones(K, dtype=torch.float64)
    live = t != ignore_index
    sw = w[t[live]].sum()
    ce_sum = F.cross_entropy(z64, t, weight=w, ignore_index=ignore_index, reduction="sum")
    ce_term = ce_sum / sw if float(sw) > 0 else ce_sum * 0.0
    rows = B if per_sample else 1
    lv = live.unsqueeze(1).double()
    p = torch.softmax(z64, 1) * lv
    oh = F.one_hot(torch.where(live, t, torch.zeros_like(t)), K).permute(0, 3, 1, 2).double() * lv
    if rows == B:
        pr, tr = p.reshape(B, K, -1), oh.reshape(B, K, -1)
    else:
        pr, tr = p.transpose(0, 1).reshape(1, K, -1), oh.transpose(0, 1).reshape(1, K, -1)
    tp, sp, st = (pr * tr).sum(-1), pr.sum(-1), tr.sum(-1)
    ti = (tp + smooth) / ((1.0 - alpha - beta) * tp + alpha * sp + beta * st + smooth)
    classes = slice(None) if bg else slice(1, None)
    loss = ce * ce_term + tv * (1.0 - ti)[:, classes].mean()
    (grad,) = torch.autograd.grad(loss * upstream, z64)
    return loss.detach(), grad, ref_hard_stats(z, t, ignore_index)


def check_loss(loss, ref):
    torch.testing.assert_close(loss.detach().double().cpu(), ref, rtol=LOSS_RTOL, atol=1e-12)


def check_grad(g, g_ref, bf16=False):
    scale = float(g_ref.abs().max())
    torch.testing.assert_close(g.double().cpu(), g_ref, rtol=BF16_RTOL if bf16 else 0.0, atol=GRAD_ATOL_REL * scale)


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("ps", PARAM_SETS)
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_path_vs_fp64(shape, ps, per_sample):
    z, t = make_case(shape)
    crit = make_criterion(shape[1], ps, per_sample)
    za = z.clone().requires_grad_(True)
    loss, stats = crit.loss_stats(za, t)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert stats.shape == (3, shape[1]) and stats.dtype == torch.float64 and not stats.requires_grad
    (loss * UPSTREAM).backward()
    ref, gref, sref = ref_ce_loss_grad(z, t, ps, per_sample)
    check_loss(loss, ref)
    check_grad(za.grad, gref)
    assert torch.equal(stats, sref)
    assert torch.equal(crit(z, t), loss.detach())
    # (B, 1, H, W) and uint8 labels are the same labels
    assert torch.equal(crit(z, t.unsqueeze(1).to(torch.uint8)), loss.detach())
    assert float(za.grad[t.unsqueeze(1).expand_as(z) == IGNORE].abs().max()) == 0.0


def test_ce_loss_is_cross_entropy():
    from csu.losses import ce_loss
    g = torch.Generator().manual_seed(5)
    z = torch.randn(3, 5, 17, 13, generator=g) * 3
    t = torch.randint(0, 5, (3, 17, 13), generator=g)
    for w in (None, class_weights(5)):
        crit = ce_loss(5, class_weight=w)
        assert crit.tversky == 0.0 and crit.ignore_index == -100
        ref = F.cross_entropy(z.double(), t, weight=None if w is None else torch.tensor(w, dtype=torch.float64))
        torch.testing.assert_close(crit(z, t).double(), ref, rtol=LOSS_RTOL, atol=0)


@pytest.mark.parametrize("s", [1e-6, 1.0])
def test_two_class_dice_without_background_is_binary_dice(s):
    from csu.losses import dice_loss, multiclass_dice_loss
    g = torch.Generator().manual_seed(6)
    z = torch.randn(3, 2, 17, 13, generator=g) * 2
    t = torch.randint(0, 2, (3, 17, 13), generator=g)
    mc = multiclass_dice_loss(2, smooth=s, include_background=False)
    assert (mc.ce, mc.tversky, mc.smooth) == (0.0, 1.0, s / 2)
    p1 = torch.softmax(z.double(), 1)[:, 1:2]
    ref = dice_loss(smooth=s)._torch(p1, t.unsqueeze(1).double())
    torch.testing.assert_close(mc(z, t).double(), ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("kw", [dict(num_classes=1), dict(num_classes=0), dict(num_classes=2.0), dict(ce=-1.0),
                                dict(tversky=-0.5), dict(alpha=-0.1), dict(beta=-0.1), dict(smooth=0.0), dict(smooth=-1.0),
                                dict(ce=0.0, tversky=0.0), dict(ce=float("nan")), dict(smooth=float("nan")),
                                dict(alpha=float("inf")), dict(class_weight=[1.0, 2.0]), dict(class_weight=[1.0, -1.0, 1.0]),
                                dict(class_weight=[1.0, float("nan"), 1.0]), dict(ignore_index=1.5)])
def test_constructor_rejects(kw):
    from csu.losses import MultiClassSegLoss
    with pytest.raises(ValueError):
        MultiClassSegLoss(**dict(dict(num_classes=3), **kw))


def test_call_rejects_bad_shapes_and_dtypes():
    from csu.losses import MultiClassSegLoss
    crit = MultiClassSegLoss(3)
    z, t = torch.randn(2, 3, 4, 4), torch.zeros(2, 4, 4, dtype=torch.int64)
    for a, b in ((z[:, :2], t), (z, t[:, :3]), (z, t.float()), (z, t.int()), (z, torch.zeros(2, 2, 4, 4, dtype=torch.int64))):
        with pytest.raises(ValueError):
            crit(a, b)


@pytest.mark.parametrize("ps", PARAM_SETS)
def test_all_ignored_batch_is_zero_not_nan(ps):
    z, _ = make_case((2, 3, 7, 9))
    t = torch.full((2, 7, 9), -100, dtype=torch.int64)
    crit = make_criterion(3, ps, False, ignore_index=-100)
    za = z.clone().requires_grad_(True)
    loss, stats = crit.loss_stats(za, t)
    loss.backward()
    assert float(loss.detach()) == 0.0 and float(za.grad.abs().max()) == 0.0 and not bool(torch.isnan(za.grad).any())
    assert float(stats.abs().max()) == 0.0


def test_runs_in_fp32_under_autocast():
    z, t = make_case((2, 3, 7, 9))
    crit = make_criterion(3, PARAM_SETS[2], False)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        a = crit(z.bfloat16(), t)
    assert a.dtype == torch.float32
    assert torch.equal(a, crit(z.bfloat16().float(), t))


def test_instances_are_dict_keys_and_exported():
    import csu
    from csu.losses import MultiClassSegLoss, ce_dice_loss, ce_loss, multiclass_dice_loss
    a, b = MultiClassSegLoss(3), MultiClassSegLoss(3)
    d = {a: 1, b: 2}
    assert d[a] == 1 and d[b] == 2 and a != b and hash(a) == hash(a)
    for f in (ce_loss, ce_dice_loss, multiclass_dice_loss):
        assert isinstance(f(4), MultiClassSegLoss) and hasattr(f(4), "loss_stats") and f(4).num_classes == 4
    cd = ce_dice_loss(4, ce=0.5, dice=2.0, smooth=1.0)
    assert (cd.ce, cd.tversky, cd.alpha, cd.beta, cd.smooth) == (0.5, 2.0, 0.5, 0.5, 0.5)
    assert csu.MultiClassSegLoss is MultiClassSegLoss and csu.ce_loss is ce_loss
    assert csu.ce_dice_loss is ce_dice_loss and csu.multiclass_dice_loss is multiclass_dice_loss
    assert "ignore_index=-100" in repr(a)


def test_abi_declares_and_exports_seg_ce():
    from csu import _lib
    src = open(os.path.join(REPO, "include", "csu.h")).read()
    assert "cswin:924" in src[src.index("csrc/seg_ce.hip"):src.index("csu_seg_ce_workspace(")]
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for n in ("csu_seg_ce_workspace", "csu_seg_ce_fwd", "csu_seg_ce_bwd"):
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(L, n) and n in _lib._SIGS, n
    assert len(_lib._SIGS["csu_seg_ce_fwd"][1]) == 26 and len(_lib._SIGS["csu_seg_ce_bwd"][1]) == 21
    # 2 + 5 K partial sums per (image, chunk) item; a bad (B, K, HW) needs no workspace
    ws = L.csu_seg_ce_workspace
    assert ws(1, 2, 15) == 12 * 4 and ws(33, 3, 64) == 33 * 17 * 4
    assert ws(16, 8, 512 * 512) == 1024 * 42 * 4            # 64 chunks per image
    assert ws(2, 6, 300 * 333) == 2 * 98 * 32 * 4           # 98 chunks of 1020 pixels, the last one ragged
    assert ws(1030, 4, 9) == 1030 * 22 * 4
    assert ws(0, 3, 9) == 0 and ws(1, 1, 9) == 0 and ws(1, 33, 9) == 0 and ws(1, 3, 0) == 0


def test_abi_rejects_bad_arguments_on_the_host():
    """Every bad argument is refused with CSU_E_ARG and a message before any launch (no device
    memory is touched: the pointers here are dummies that a launch would fault on)."""
    import ctypes
    from csu import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(B=2, K=3, HW=8, rows=2, dtype=0, s_b=24, s_k=8, s_pix=1, lab=1, w_ce=1.0, w_tv=1.0, alpha=0.5, beta=0.5,
              smooth=0.5)
    bad = [dict(B=0), dict(HW=0), dict(K=1), dict(K=33), dict(rows=3), dict(rows=0), dict(dtype=2), dict(lab=2),
           dict(s_k=0), dict(s_pix=0), dict(s_b=-1), dict(w_ce=-1.0), dict(w_tv=-1.0), dict(w_ce=0.0, w_tv=0.0),
           dict(smooth=0.0), dict(smooth=-1.0), dict(alpha=-0.5), dict(beta=-0.5)]
    for b in bad:
        a = dict(ok, **b)
        rc = L.csu_seg_ce_fwd(a["B"], a["K"], a["HW"], a["rows"], a["dtype"], q, a["s_b"], a["s_k"], a["s_pix"], 0, a["lab"],
                              q, -100, None, a["w_ce"], a["w_tv"], a["alpha"], a["beta"], a["smooth"], 1, q, q, q, q, 1 << 20,
                              None)
        assert rc == -1, (b, rc)     # CSU_E_ARG
        assert b"seg_ce_fwd" in L.csu_last_error_string()
    for b in bad:
        if set(b) & {"smooth", "alpha", "beta"}:
            continue
        a = dict(ok, **b)
        rc = L.csu_seg_ce_bwd(a["B"], a["K"], a["HW"], a["rows"], a["dtype"], q, a["s_b"], a["s_k"], a["s_pix"], 0, a["lab"],
                              q, -100, None, q, q, a["w_ce"], a["w_tv"], 1, q, None)
        assert rc == -1, (b, rc)
        assert b"seg_ce_bwd" in L.csu_last_error_string()
    assert L.csu_seg_ce_fwd(2, 3, 8, 2, 0, None, 24, 8, 1, 0, 1, q, -100, None, 1.0, 1.0, 0.5, 0.5, 0.5, 1, q, q, q, q, 1 << 20,
                            None) == -1
    assert L.csu_seg_ce_fwd(2, 3, 8, 2, 0, q, 24, 8, 1, 0, 1, q, -100, None, 1.0, 1.0, 0.5, 0.5, 0.5, 1, q, q, q, q, 4,
                            None) == -3    # CSU_E_WORKSPACE


# ---- csu.train ---------------------------------------------------------------------------------

def test_epoch_means_multiclass_rows():
    """Rows of 1 + 3 K columns: I, Pr, T summed over the steps, per-class Dice / IoU of the totals,
    macro mean over the classes that occur (class 2 here never does); 4-column rows as before."""
    from csu.train import _epoch_means
    K, s = 3, 1e-6
    r0 = torch.tensor([0.5, 4, 1, 0, 6, 2, 0, 5, 3, 0], dtype=torch.float64)
    r1 = torch.tensor([1.5, 2, 3, 0, 2, 5, 0, 3, 4, 0], dtype=torch.float64)
    loss, dice, iou, cd, ci = _epoch_means([r0, r1], per_class=True)
    I, Pr, T = np.array([6.0, 4.0, 0.0]), np.array([8.0, 7.0, 0.0]), np.array([8.0, 7.0, 0.0])
    d, j = (2 * I + s) / (Pr + T + s), (I + s) / (Pr + T - I + s)
    assert loss == 1.0
    np.testing.assert_allclose(cd, d, rtol=1e-12)
    np.testing.assert_allclose(ci, j, rtol=1e-12)
    np.testing.assert_allclose([dice, iou], [d[:2].mean(), j[:2].mean()], rtol=1e-12)
    assert _epoch_means([r0, r1]) == (loss, dice, iou)
    # binary rows: today's arithmetic (mean over steps of the per-step Dice / IoU)
    b0, b1 = torch.tensor([0.5, 4, 6, 5], dtype=torch.float64), torch.tensor([1.5, 2, 2, 3], dtype=torch.float64)
    bl, bd, bi = _epoch_means([b0, b1])
    np.testing.assert_allclose([bl, bd, bi], [1.0, ((8 + s) / (11 + s) + (4 + s) / (5 + s)) / 2,
                                              ((4 + s) / (7 + s) + (2 + s) / (3 + s)) / 2], rtol=1e-12)
    assert _epoch_means([b0, b1], per_class=True)[3:] == (None, None)
    assert _epoch_means([], per_class=True) == (0.0, 0.0, 0.0, None, None)


def test_step_stats_multiclass_branch():
    from csu.train import _step_stats
    z, t = make_case((3, 5, 37, 41))
    t = torch.where(t == IGNORE, torch.zeros_like(t), t)      # the eager route knows no ignore_index
    z[0, 1, 0, 0] = z[0, 3, 0, 0] = 50.0                      # a tie: class 1 is the prediction
    loss = torch.tensor(0.25)
    ref = ref_hard_stats(z, t, ignore_index=-1)
    for tt in (t, t.unsqueeze(1), t.to(torch.uint8)):
        st = _step_stats(loss, z, tt)
        assert st.shape == (16,) and st.dtype == torch.float64
        assert float(st[0]) == 0.25 and torch.equal(st[1:].view(3, 5), ref)
    # the binary branch is untouched: float masks of the output's shape
    p, m = torch.rand(2, 1, 4, 4), (torch.rand(2, 1, 4, 4) > 0.5).float()
    pred = (p > 0.5).double()
    assert torch.equal(_step_stats(loss, p, m)[1:], torch.stack([(pred * m).sum(), pred.sum(), m.double().sum()]))


# ---- csu.data ----------------------------------------------------------------------------------

def test_synthetic_binary_samples_unchanged(golden_dir):
    """SyntheticSegmentation(num_classes=1): the samples the code drew before num_classes existed
    (recorded from that code path as tests/golden/synthetic_seg_binary.npz)."""
    from csu.data import SyntheticSegmentation
    gold = np.load(os.path.join(golden_dir, "synthetic_seg_binary.npz"))
    ds = SyntheticSegmentation(3, 32, seed=7)
    for i in range(3):
        img, mask = ds[i]
        assert np.array_equal(np.asarray(img), gold[f"img{i}"]) and np.array_equal(np.asarray(mask), gold[f"mask{i}"])
        assert str(np.asarray(img).dtype) == str(gold[f"img{i}"].dtype)
        assert str(np.asarray(mask).dtype) == str(gold[f"mask{i}"].dtype)


def test_synthetic_multiclass_label_maps():
    from csu.data import SyntheticSegmentation
    ds = SyntheticSegmentation(4, 32, seed=3, num_classes=4)
    seen = set()
    for i in range(4):
        img, mask = ds[i]
        assert mask.dtype == torch.int64 and tuple(mask.shape) == (32, 32) and tuple(img.shape) == (3, 32, 32)
        assert int(mask.min()) >= 0 and int(mask.max()) <= 3
        seen |= set(mask.unique().tolist())
        img2, mask2 = ds[i]
        assert torch.equal(mask, mask2) and torch.equal(img, img2)
    assert 0 in seen and len(seen) > 2
    with pytest.raises(ValueError):
        SyntheticSegmentation(4, 32, num_classes=0)


def test_label_mode_resizes_nearest(tmp_path):
    """label_mode reads raw class indices and resizes them nearest-neighbour: every value of the
    (H, W) int64 result is one of the file's indices (bilinear would blend 1 and 7 into 2 .. 6)."""
    Image = pytest.importorskip("PIL.Image")
    from csu.data import SegmentationDataset
    (tmp_path / "img").mkdir()
    (tmp_path / "mask").mkdir()
    rng = np.random.default_rng(0)
    lab = np.zeros((40, 40), np.uint8)
    lab[:, 13:] = 1
    lab[17:, :] = 7
    Image.fromarray(rng.integers(0, 255, (40, 40, 3), dtype=np.uint8)).save(tmp_path / "img" / "a.png")
    Image.fromarray(lab).save(tmp_path / "mask" / "a.png")
    ds = SegmentationDataset(str(tmp_path / "img"), str(tmp_path / "mask"), image_size=(32, 32), label_mode=True)
    img, mask = ds[0]
    assert mask.dtype == torch.int64 and tuple(mask.shape) == (32, 32) and tuple(img.shape) == (3, 32, 32)
    assert set(mask.unique().tolist()) == {0, 1, 7}
    ref = torch.from_numpy(np.asarray(Image.fromarray(lab).resize((32, 32), Image.NEAREST)).astype(np.int64))
    assert torch.equal(mask, ref)
    with pytest.raises(ValueError):
        SegmentationDataset(str(tmp_path / "img"), str(tmp_path / "mask"), image_size=(32, 32), label_mode=True,
                            device_augment=True)
