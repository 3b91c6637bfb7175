"""The boundary loss on the CPU: csu.boundary's reference signed distance maps against a literal scipy
restatement of Kervadec's one_hot2dist and hand cases; csu.losses.BoundarySegLoss' torch path against an fp64
restatement of its formula (own autograd, non-unit upstream factor); the constructor's and the call's checks;
the csu_signed_distance / csu_seg_bd_* C-ABI entry points; and train_model's schedule hook.

The fp64 restatement (``ref_bd_loss_grad``) and the inputs are shared with tests/test_gpu_boundary.py.

Tolerances, derived as tests/test_seg_ce.py documents.  torch's own fp32 composition of the formula
(``BoundarySegLoss`` on fp32 CPU logits, with the random N(0, 20^2) maps of ``make_phi``) was measured against the
fp64 restatement at every shape of SHAPES (the GPU file uses the same list) and of OTHER_GPU_SHAPES, every weight combination of
COMBOS, both ``bd_background`` settings and both ``per_sample`` settings (``measure_fp32_composition`` below
prints the table).  phi has both signs, so BD is a sum with cancellation and an error relative to |BD| would
say nothing; the errors are taken relative to the size of what is summed:
    loss      |loss - ref| / (|base| + w_bd A),   A = sum |p_c phi_c| / (n |Cb|)     largest 1.55e-7 ((2,6,300,333), w_bd = 0, per image)
    terms[1]  |BD - ref| / A                                                         largest 1.40e-8 ((2,3,7,9), foreground classes)
    gradient  max |g - g_ref| / max |g_ref|                                          largest 7.64e-7 ((2,6,300,333), w_bd = 0)
Ten times the largest: one loss tolerance BD_LOSS_TOL = 1.6e-6 (of |base| + w_bd A for the loss, of A for terms[1])
and BD_GRAD_ATOL_REL = 7.7e-6 of max|g_ref| with no relative term (a relative one would say nothing about the
softmax-suppressed elements).  terms[0], the loss without the boundary term, keeps test_seg_ce.py's LOSS_RTOL.
bf16 logits: the reference takes the bf16 values upcast exactly and the gradient,
written in bf16, gets one bf16 rounding (rtol 2**-8) on top."""
import os
import re

import numpy as np
import pytest
import torch

from test_seg_ce import BF16_RTOL, IGNORE, LOSS_RTOL, UPSTREAM, make_case, ref_ce_loss_grad

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BD_LOSS_TOL = 1.6e-6
BD_GRAD_ATOL_REL = 7.7e-6
SMOOTH = 0.5
# (1,2,3,5): minimum K, under one vector; (2,3,7,9): odd K, ragged; (3,5,37,41): class 4 absent, image 1 ignored;
# (2,32,8,8): the top bucket; (2,6,300,333): 98 chunks per image, several rounds per thread
SHAPES = [(1, 2, 3, 5), (2, 3, 7, 9), (3, 5, 37, 41), (2, 32, 8, 8), (2, 6, 300, 333)]
# (ce, dice, w_bd): CE + Dice + BD, BD alone, the boundary term switched off
COMBOS = [(1.0, 1.0, 0.5), (0.0, 0.0, 1.0), (0.5, 1.0, 0.0)]
OTHER_GPU_SHAPES = [(2, 33, 9, 11), (2, 5, 37, 53)]      # the GPU files' torch-route and guard-band cases


def make_phi(shape, seed=None):
    """fp32 (B, K, H, W) N(0, 20^2): the loss takes phi as data; one class's plane is all zeros (class 1; class 0
    of two, so that the foreground term does not vanish)."""
    B, K, H, W = shape
    g = torch.Generator().manual_seed(7 + B * 1000 + K * 37 + H if seed is None else seed)
    phi = torch.randn(shape, generator=g) * 20.0
    phi[:, 1 if K > 2 else 0] = 0.0
    return phi


def make_criterion(K, combo, bd_background, per_sample, ignore_index=IGNORE, **kw):
    from csu.losses import BoundarySegLoss
    ce, dice, w_bd = combo
    return BoundarySegLoss(K, ce=ce, tversky=dice, smooth=SMOOTH, ignore_index=ignore_index, per_sample=per_sample,
                           boundary=w_bd, boundary_background=bd_background, **kw)


def ref_bd_loss_grad(z, t, phi, combo, bd_background, per_sample, ignore_index=IGNORE, upstream=UPSTREAM):
    """fp64 (loss, d(upstream * loss)/dz, terms (2,), A, (3, K) hard sums) for logits z (fp32 or bf16, upcast
    exactly), int64 labels t and fp32 maps phi.  n = sum_c T_c, BD = sum over live pixels and c in Cb of
    p_c phi_c / (n |Cb|) (0 when n = 0), loss = [ce CE + dice mean(1 - Dice)] + w_bd BD; the region terms come
    from test_seg_ce.ref_ce_loss_grad, BD is differentiated here.  A = sum |p_c phi_c| / (n |Cb|)."""
    ce, dice, w_bd = combo
    K = z.shape[1]
    base, gbase, stats = ref_ce_loss_grad(z, t, (ce, dice, 0.5, 0.5, False, True), per_sample, ignore_index, SMOOTH, upstream)
    z64 = z.detach().double().requires_grad_(True)
    live = t != ignore_index
    n = sum(int(((t == c) & live).sum()) for c in range(K))
    first = 0 if bd_background else 1
    p = torch.softmax(z64, 1)
    terms = (p * phi.double())[:, first:] * live.unsqueeze(1).double()
    if n > 0:
        bd = terms.sum() / (n * (K - first))
        scale = float(terms.detach().abs().sum() / (n * (K - first)))
    else:
        bd, scale = terms.sum() * 0.0, 0.0
    (gbd,) = torch.autograd.grad(bd * (w_bd * upstream), z64)
    loss = base + w_bd * bd.detach()
    return loss, gbase + gbd, torch.stack([base, bd.detach()]), scale, stats


def check_bd_loss(loss, terms, lref, tref, scale, w_bd):
    l, tm = loss.detach().double().cpu(), terms.detach().double().cpu()
    torch.testing.assert_close(tm[0], tref[0], rtol=LOSS_RTOL, atol=1e-12)
    torch.testing.assert_close(tm[1], tref[1], rtol=0.0, atol=BD_LOSS_TOL * scale + 1e-30)
    torch.testing.assert_close(l, lref, rtol=0.0, atol=BD_LOSS_TOL * (abs(float(tref[0])) + w_bd * scale) + 1e-30)


def check_bd_grad(g, g_ref, bf16=False):
    scale = float(g_ref.abs().max())
    torch.testing.assert_close(g.double().cpu(), g_ref, rtol=BF16_RTOL if bf16 else 0.0, atol=BD_GRAD_ATOL_REL * scale)


def measure_fp32_composition():
    """The table behind BD_LOSS_TOL and BD_GRAD_ATOL_REL: python -c "import test_boundary as t; t.measure_fp32_composition()"."""
    worst = [0.0, 0.0, 0.0]
    for shape in SHAPES + OTHER_GPU_SHAPES:
        z, t = make_case(shape)
        phi = make_phi(shape)
        for combo in COMBOS:
            for bg in (False, True):
                for per_sample in (False, True):
                    lref, gref, tref, scale, _ = ref_bd_loss_grad(z, t, phi, combo, bg, per_sample)
                    crit = make_criterion(shape[1], combo, bg, per_sample)
                    za = z.clone().requires_grad_(True)
                    loss = crit(za, t, dist=phi)
                    (loss * UPSTREAM).backward()
                    el = abs(float(loss.detach().double() - lref)) / (abs(float(tref[0])) + combo[2] * scale)
                    et = abs(float(crit.last_terms[1].double() - tref[1])) / scale
                    eg = float((za.grad.double() - gref).abs().max() / gref.abs().max())
                    print(f"{shape} {combo} bg={int(bg)} per_sample={int(per_sample)}: loss {el:.2e} BD {et:.2e} grad {eg:.2e}")
                    worst = [max(a, b) for a, b in zip(worst, (el, et, eg))]
    print("largest: loss %.3g  BD %.3g  grad %.3g" % tuple(worst))


# ---- the reference maps ------------------------------------------------------------------------

def label_maps(seed, shape, K, ignore=0.1):
    """int64 (B, H, W): K values over blobs, class K - 1 absent, 10 % ignored, image 0 of a batch a single class."""
    rng = np.random.default_rng(seed)
    B, H, W = shape
    coarse = rng.integers(0, K - 1, (B, (H + 3) // 4, (W + 3) // 4))
    m = np.repeat(np.repeat(coarse, 4, 1), 4, 2)[:, :H, :W].copy()
    m[rng.random(shape) < 0.05] = 0
    if ignore:
        m[rng.random(shape) < ignore] = IGNORE
    if B > 1:
        m[0] = 2 % (K - 1)      # with no pixel ignored: the class fills the image
    return torch.from_numpy(m)


def one_hot2dist(seg, K, spacing):
    """Kervadec's one_hot2dist (utils.py of the boundary-loss repository) restated with scipy, per image and
    class; with a spacing, `sampling=` and min(spacing) in place of the 1."""
    edt = pytest.importorskip("scipy.ndimage").distance_transform_edt
    seg = seg.numpy()
    res = np.zeros((seg.shape[0], K) + seg.shape[1:], np.float64)
    for b in range(seg.shape[0]):
        for k in range(K):
            posmask = seg[b] == k
            if posmask.any() and not posmask.all():
                negmask = ~posmask
                res[b, k] = edt(negmask, sampling=spacing) * negmask - (edt(posmask, sampling=spacing) - min(spacing)) * posmask
    return torch.from_numpy(res)


@pytest.mark.parametrize("spacing", [(1.0, 1.0), (0.7, 1.3)])
def test_reference_maps_vs_scipy_one_hot2dist(spacing):
    from csu.boundary import reference_signed_distance_map, signed_distance_map
    t = label_maps(3, (2, 19, 23), 5)
    want = one_hot2dist(t, 5, spacing)
    got = reference_signed_distance_map(t, 5, spacing)
    assert got.dtype == torch.float64 and got.shape == (2, 5, 19, 23)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    assert float(got[0].abs().max()) == 0.0 and float(got[:, 4].abs().max()) == 0.0      # one class; an absent class
    assert float(got[1, :4].min()) < 0.0 < float(got[1, :4].max())
    # the public function on CPU tensors is the reference rounded to fp32; uint8 labels and an (H, W) map alike
    pub = signed_distance_map(t, 5, spacing)
    assert pub.dtype == torch.float32 and torch.equal(pub, got.float())
    assert torch.equal(signed_distance_map(t.to(torch.uint8), 5, spacing), pub)
    assert torch.equal(signed_distance_map(t[1], 5, spacing), pub[1])
    assert torch.equal(signed_distance_map(t.numpy(), 5, spacing, classes=(1, 3)), pub[:, 1:3])


def test_reference_maps_hand_cases():
    from csu.boundary import reference_signed_distance_map as ref
    t = torch.zeros(5, 7, dtype=torch.int64)
    t[2, 3] = 1
    phi = ref(t, 3)
    yy, xx = torch.meshgrid(torch.arange(5.0, dtype=torch.float64), torch.arange(7.0, dtype=torch.float64), indexing="ij")
    d = ((yy - 2) ** 2 + (xx - 3) ** 2).sqrt()
    assert phi.shape == (3, 5, 7)
    assert torch.equal(phi[1], d)                               # a single pixel: the distance to it, 0 on it
    # class 0 is everything else: 1 on the hole, 0 on the ring around it, negative further in; the image edge is no border
    assert float(phi[0][2, 3]) == 1.0 and float(phi[0][2, 2]) == 0.0 and float(phi[0][4, 3]) == -1.0
    assert torch.equal(phi[0], 1 - d) and abs(float(phi[0][0, 0]) + 13 ** 0.5 - 1) < 1e-15
    assert float(phi[2].abs().max()) == 0.0                     # an absent class
    assert float(ref(torch.full((4, 4), 2), 3).abs().max()) == 0.0              # a class that fills the image
    assert float(ref(torch.full((2, 4, 4), IGNORE), 3).abs().max()) == 0.0     # all ignore_index: no class anywhere
    # an ignored pixel is outside every class
    t2 = torch.ones(1, 5, dtype=torch.int64)
    t2[0, 2] = IGNORE
    assert ref(t2, 2)[1].tolist() == [[-1.0, 0.0, 1.0, 0.0, -1.0]] and float(ref(t2, 2)[0].abs().max()) == 0.0
    # spacing: the finer axis is the unit of the inner border; clip clamps both signs
    t3 = torch.zeros(9, 9, dtype=torch.int64)
    t3[2:7, 2:7] = 1
    p3 = ref(t3, 2, (0.5, 2.0))[1]
    assert float(p3[2, 4]) == 0.0 and float(p3[4, 4]) == -1.0 and float(p3[4, 2]) == -1.0 and float(p3[4, 0]) == 4.0
    c3 = ref(t3, 2, (0.5, 2.0), clip=0.75)[1]
    assert torch.equal(c3, p3.clamp(-0.75, 0.75)) and float(c3.min()) == -0.75 and float(c3.max()) == 0.75
    for bad in (dict(clip=0.0), dict(clip=-1.0), dict(clip=float("inf")), dict(spacing=(0.0, 1.0)), dict(classes=(2, 1)),
                dict(classes=(0, 3))):
        with pytest.raises(ValueError):
            ref(t3, 2, **bad)
    with pytest.raises(ValueError):
        ref(t3.float(), 2)


# ---- the criterion -----------------------------------------------------------------------------

@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("bd_background", [False, True])
@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("shape", SHAPES[:3])
def test_cpu_path_vs_fp64(shape, combo, bd_background, per_sample):
    z, t = make_case(shape)
    phi = make_phi(shape)
    crit = make_criterion(shape[1], combo, bd_background, per_sample)
    za = z.clone().requires_grad_(True)
    loss, stats = crit.loss_stats(za, t, dist=phi)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and crit.last_terms.shape == (2,)
    assert not crit.last_terms.requires_grad
    (loss * UPSTREAM).backward()
    lref, gref, tref, scale, sref = ref_bd_loss_grad(z, t, phi, combo, bd_background, per_sample)
    check_bd_loss(loss, crit.last_terms, lref, tref, scale, combo[2])
    check_bd_grad(za.grad, gref)
    assert torch.equal(stats, sref)
    assert torch.equal(crit(z, t, dist=phi), loss.detach())
    assert torch.equal(crit(z, t.unsqueeze(1).to(torch.uint8), dist=phi), loss.detach())
    assert float(za.grad[t.unsqueeze(1).expand_as(z) == IGNORE].abs().max()) == 0.0


def test_maps_are_made_from_the_target_and_the_weight_is_live():
    """Without dist= the maps come from signed_distance_map(target) with the criterion's spacing and clip; the
    weight can be changed in place; w_bd = 0 is the parent criterion."""
    from csu.boundary import signed_distance_map
    from csu.losses import MultiClassSegLoss
    z, _ = make_case((2, 3, 7, 9))
    t = label_maps(5, (2, 7, 9), 3)
    crit = make_criterion(3, COMBOS[0], False, False, spacing=(0.7, 1.3), clip=2.0)
    phi = signed_distance_map(t, 3, (0.7, 1.3), 2.0)
    assert float(phi.abs().max()) == 2.0
    a = crit(z, t)
    base, bd = crit.last_terms.tolist()
    assert torch.equal(a, crit(z, t, dist=phi)) and not torch.equal(a, crit(z, t, dist=phi * 2))
    assert crit.boundary_weight == 0.5
    crit.set_boundary_weight(0.25)
    assert crit.boundary_weight == 0.25
    torch.testing.assert_close(crit(z, t), torch.tensor(base + 0.25 * bd), rtol=1e-6, atol=0)
    crit.set_boundary_weight(0.0)
    parent = MultiClassSegLoss(3, ce=1.0, tversky=1.0, smooth=SMOOTH, ignore_index=IGNORE)
    assert torch.equal(crit(z, t), parent(z, t))


def test_all_ignored_batch_is_zero_not_nan():
    z, _ = make_case((2, 3, 7, 9))
    t = torch.full((2, 7, 9), -100, dtype=torch.int64)
    for combo in COMBOS:
        crit = make_criterion(3, combo, False, False, ignore_index=-100)
        za = z.clone().requires_grad_(True)
        loss, stats = crit.loss_stats(za, t)
        loss.backward()
        assert float(loss.detach()) == 0.0 and float(za.grad.abs().max()) == 0.0 and not bool(torch.isnan(za.grad).any())
        assert float(crit.last_terms.abs().max()) == 0.0 and float(stats.abs().max()) == 0.0


@pytest.mark.parametrize("kw", [dict(boundary=-1.0), dict(boundary=float("nan")), dict(boundary=float("inf")),
                                dict(spacing=(1.0,)), dict(spacing=(0.0, 1.0)), dict(spacing=(1.0, float("inf"))),
                                dict(spacing=1.0), dict(clip=0.0), dict(clip=-2.0), dict(clip=float("nan")),
                                dict(schedule=0.5), dict(num_classes=1), dict(ce=-1.0), dict(smooth=0.0)])
def test_constructor_rejects(kw):
    from csu.losses import BoundarySegLoss
    with pytest.raises(ValueError):
        BoundarySegLoss(**dict(dict(num_classes=3), **kw))


def test_call_and_weight_rejections():
    from csu.losses import BoundarySegLoss, MultiClassSegLoss, linear_ramp
    crit = BoundarySegLoss(3)
    z, t = torch.randn(2, 3, 4, 4), torch.zeros(2, 4, 4, dtype=torch.int64)
    phi = torch.zeros(2, 3, 4, 4)
    for a, b, d in ((z[:, :2], t, None), (z, t[:, :3], None), (z, t.float(), None), (z, t, phi[:, :2]), (z, t, phi.long()),
                    (z, t, phi.numpy())):
        with pytest.raises(ValueError):
            crit(a, b, dist=d)
    for w in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            crit.set_boundary_weight(w)
    for kw in (dict(start=-0.1), dict(start=2.0), dict(step=-0.01), dict(stop=float("inf"))):
        with pytest.raises(ValueError):
            linear_ramp(**kw)
    BoundarySegLoss(3, ce=0.0, tversky=0.0)                     # legal here ...
    with pytest.raises(ValueError):
        MultiClassSegLoss(3, ce=0.0, tversky=0.0)               # ... and still refused there


def test_schedule_helpers_and_exports():
    import csu
    from csu.losses import BoundarySegLoss, MultiClassSegLoss, boundary_loss, ce_dice_boundary_loss, linear_ramp
    ramp = linear_ramp()
    assert [ramp(e) for e in (0, 1, 2)] == [0.01, 0.02, 0.03] and ramp(99) == 1.0 and ramp(5000) == 1.0
    assert linear_ramp(0.5, 0.25, 0.9)(1) == 0.75 and linear_ramp(0.5, 0.25, 0.9)(2) == 0.9
    c = ce_dice_boundary_loss(4, ce=0.5, dice=2.0, boundary=0.3, smooth=1.0, schedule=ramp, clip=8.0, spacing=(2, 1))
    assert isinstance(c, BoundarySegLoss) and isinstance(c, MultiClassSegLoss) and hasattr(c, "loss_stats")
    assert (c.ce, c.tversky, c.alpha, c.beta, c.smooth, c.boundary_weight) == (0.5, 2.0, 0.5, 0.5, 0.5, 0.3)
    assert (c.clip, c.spacing, c.boundary_background) == (8.0, (2.0, 1.0), False)
    c.on_epoch(4)
    assert c.boundary_weight == ramp(4)
    b = boundary_loss(4, boundary_background=True)
    assert (b.ce, b.tversky, b.boundary_weight, b.boundary_background, b.schedule) == (0.0, 0.0, 1.0, True, None)
    b.on_epoch(3)
    assert b.boundary_weight == 1.0                             # no schedule: on_epoch leaves the weight
    d = {c: 1, b: 2}
    assert d[c] == 1 and d[b] == 2
    assert "boundary=1.0" in repr(b) and "num_classes=4" in repr(b)
    for n in ("BoundarySegLoss", "boundary_loss", "ce_dice_boundary_loss", "linear_ramp", "signed_distance_map",
              "reference_signed_distance_map"):
        assert n in csu.__all__ and hasattr(csu, n), n


# ---- the C ABI ---------------------------------------------------------------------------------

NEW_ENTRY_POINTS = ("csu_signed_distance_workspace", "csu_signed_distance", "csu_seg_bd_workspace", "csu_seg_bd_fwd",
                    "csu_seg_bd_bwd")


def test_abi_declares_and_exports_the_entry_points():
    from csu import _lib
    src = open(os.path.join(REPO, "include", "csu.h")).read()
    assert "n |Cb|" in src[src.index("Kervadec"):src.index("csu_seg_bd_workspace(")]
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for n in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(L, n) and n in _lib._SIGS, n
    assert len(_lib._SIGS["csu_seg_bd_fwd"][1]) == 30 and len(_lib._SIGS["csu_seg_bd_bwd"][1]) == 24
    assert len(_lib._SIGS["csu_signed_distance"][1]) == 16
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for n in NEW_ENTRY_POINTS:
        assert n in doc, n
    # one more partial sum per (image, chunk) item than csu_seg_ce_workspace
    ws, ce = L.csu_seg_bd_workspace, L.csu_seg_ce_workspace
    assert ws(1, 2, 15) == 13 * 4 and ws(33, 3, 64) == 33 * 18 * 4 and ws(16, 8, 512 * 512) == 1024 * 43 * 4
    assert ws(2, 6, 300 * 333) == 2 * 98 * 33 * 4 and ws(2, 6, 300 * 333) - ce(2, 6, 300 * 333) == 2 * 98 * 4
    assert ws(0, 3, 9) == 0 and ws(1, 1, 9) == 0 and ws(1, 33, 9) == 0 and ws(1, 3, 0) == 0
    # two uint16 fields per (image, class), rounded up to 256
    sd = L.csu_signed_distance_workspace
    assert sd(2, 5, 37, 53) == (4 * 2 * 5 * 37 * 53 + 255) // 256 * 256 and sd(1, 1, 1, 1) == 256
    assert sd(16, 5, 512, 512) == 4 * 16 * 5 * 512 * 512 and sd(1, 1, 16383, 16383) == (4 * 16383 * 16383 + 255) // 256 * 256
    assert sd(0, 1, 4, 4) == 0 and sd(1, 0, 4, 4) == 0 and sd(1, 33, 4, 4) == 0 and sd(1, 1, 0, 4) == 0
    assert sd(1, 1, 16384, 4) == 0 and sd(1, 1, 4, 16384) == 0 and sd(1024, 32, 4, 4) == 0


def test_abi_rejects_bad_arguments_on_the_host():
    """Every bad argument is refused with CSU_E_ARG and a message before any launch (the pointers are dummies that
    a launch would fault on)."""
    import ctypes
    from csu import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(B=2, K=3, HW=8, rows=2, dtype=0, s_b=24, s_k=8, s_pix=1, lab=1, w_ce=1.0, w_tv=1.0, alpha=0.5, beta=0.5,
              smooth=0.5, z=q, t=q, phi=q, w_bd=q, loss=q, terms=q, coef=q, dz=q, dloss=q)
    bad = [dict(B=0), dict(HW=0), dict(K=1), dict(K=33), dict(rows=3), dict(rows=0), dict(dtype=2), dict(lab=2),
           dict(s_k=0), dict(s_pix=0), dict(s_b=-1), dict(w_ce=-1.0), dict(w_tv=-1.0), dict(smooth=0.0), dict(smooth=-1.0),
           dict(alpha=-0.5), dict(beta=-0.5), dict(z=None), dict(t=None), dict(phi=None), dict(w_bd=None), dict(loss=None),
           dict(terms=None), dict(coef=None), dict(dz=None), dict(dloss=None)]

    def fwd(a):
        return L.csu_seg_bd_fwd(a["B"], a["K"], a["HW"], a["rows"], a["dtype"], a["z"], a["s_b"], a["s_k"], a["s_pix"], 0,
                                a["lab"], a["t"], -100, None, a["w_ce"], a["w_tv"], a["alpha"], a["beta"], a["smooth"], 1,
                                a["phi"], a["w_bd"], 0, a["loss"], a["terms"], None, a["coef"], q, 1 << 20, None)

    def bwd(a):
        return L.csu_seg_bd_bwd(a["B"], a["K"], a["HW"], a["rows"], a["dtype"], a["z"], a["s_b"], a["s_k"], a["s_pix"], 0,
                                a["lab"], a["t"], -100, None, a["dloss"], a["coef"], a["w_ce"], a["w_tv"], 1, a["phi"],
                                a["w_bd"], 0, a["dz"], None)

    for b in bad:
        a = dict(ok, **b)
        if not set(b) & {"dz", "dloss"}:
            assert fwd(a) == -1, b      # CSU_E_ARG
            assert b"seg_bd_fwd" in L.csu_last_error_string()
        if not set(b) & {"smooth", "alpha", "beta", "loss", "terms"}:
            assert bwd(a) == -1, b
            assert b"seg_bd_bwd" in L.csu_last_error_string()
    assert L.csu_seg_bd_fwd(2, 3, 8, 2, 0, q, 24, 8, 1, 0, 1, q, -100, None, 0.0, 0.0, 0.5, 0.5, 0.5, 1, q, q, 0, q, q, None, q,
                            q, 4, None) == -3      # both weights zero pass the argument checks: CSU_E_WORKSPACE
    assert L.csu_seg_bd_fwd(2, 3, 8, 2, 0, q, 24, 8, 1, 0, 1, q, -100, None, 1.0, 1.0, 0.5, 0.5, 0.5, 1, q, q, 0, q, q, None, q,
                            None, 1 << 20, None) == -3

    sok = dict(B=2, C=3, H=8, W=9, c0=0, dtype=0, lab=q, sy=1.0, sx=1.0, clip=-1.0, ws=q, nws=1 << 20, out=q, oc=3, o0=0)
    sbad = [dict(B=0), dict(C=0), dict(C=33), dict(H=0), dict(W=0), dict(H=16384), dict(W=16384), dict(B=4096, C=8),
            dict(dtype=2), dict(dtype=-1), dict(sy=0.0), dict(sx=-1.0), dict(sy=float("inf")), dict(sx=float("nan")),
            dict(clip=0.0), dict(clip=float("inf")), dict(clip=float("nan")), dict(oc=2), dict(o0=1), dict(o0=-1),
            dict(lab=None), dict(ws=None), dict(out=None)]
    for b in sbad:
        a = dict(sok, **b)
        rc = L.csu_signed_distance(a["B"], a["C"], a["H"], a["W"], a["c0"], a["dtype"], a["lab"], a["sy"], a["sx"], a["clip"],
                                   a["ws"], a["nws"], a["out"], a["oc"], a["o0"], None)
        assert rc == -1, (b, rc)
        assert b"signed_distance" in L.csu_last_error_string()
    assert L.csu_signed_distance(2, 3, 8, 9, 0, 0, q, 1.0, 1.0, -1.0, q, 1024, q, 3, 0, None) == -3


# ---- csu.train ---------------------------------------------------------------------------------

def test_train_model_applies_the_schedule_every_epoch():
    """train_model on the CPU, graph off, two epochs with linear_ramp: on_epoch runs before the first step of each
    epoch (the first epoch trains with 0.01, not with the constructor's weight); the other history keys are those
    of a MultiClassSegLoss run."""
    from csu.losses import ce_dice_boundary_loss, ce_dice_loss, linear_ramp
    from csu.train import make_optimizer, train_model
    g = torch.Generator().manual_seed(3)
    batches = [(torch.rand(2, 3, 12, 12, generator=g), label_maps(20 + i, (2, 12, 12), 3, ignore=0)) for i in range(3)]
    hs = []
    for crit in (ce_dice_boundary_loss(3, boundary=5.0, schedule=linear_ramp()), ce_dice_loss(3)):
        torch.manual_seed(0)
        m = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(8, 3, 1))
        if hasattr(crit, "on_epoch"):
            seen, run = [], crit._run
            crit._run = lambda *a, _c=crit, _r=run, **k: (seen.append(_c.boundary_weight), _r(*a, **k))[1]
        hs.append(train_model(m, batches[:2], batches[2:], crit, make_optimizer(m, lr=1e-2), None, "cpu", num_epochs=2,
                              verbose=False, graph=False))
    assert hs[0]["boundary_weight"] == [0.01, 0.02]
    assert seen == [0.01] * 3 + [0.02] * 3                     # two train steps and one evaluation per epoch
    assert set(hs[0]) == set(hs[1]) | {"boundary_weight"}
    assert all(len(v) == 2 for v in hs[0].values())
    assert np.isfinite(hs[0]["train_loss"]).all() and hs[0]["train_loss"] != hs[1]["train_loss"]
