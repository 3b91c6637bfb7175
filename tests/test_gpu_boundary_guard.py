"""Guard-band cases of the boundary loss (README "Testing"): csu_signed_distance and csu_seg_bd_* stay inside their
outputs and workspaces, write all of their outputs, initialise every workspace field they read (the workspace
payload is poisoned) and let nothing outside an input reach a result (the label map's guards hold a legal class,
the logits' and phi's guards and the logits' padding NaN)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from guard_alloc import GuardedAlloc
from test_boundary import COMBOS, SMOOTH, check_bd_grad, check_bd_loss, label_maps, make_criterion, make_phi, ref_bd_loss_grad
from test_gpu_boundary import check_maps
from test_gpu_guard_bands import _place_guarded, dev, finite, gin, guarded, mod, verify
from test_seg_ce import IGNORE, UPSTREAM, make_case


@pytest.mark.parametrize("clip", [None, 3.0], ids=["noclip", "clip3"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("spacing", [(1.0, 1.0), (0.7, 1.3)], ids=["unit", "0.7x1.3"])
def test_signed_distance_map(spacing, dtype, clip, monkeypatch):
    """(2, 5, 37, 53): every pixel of every plane is written (no NaN left), the two uint16 fields fill a workspace of
    exactly csu_signed_distance_workspace bytes, and a class read past the label map's edge (the guards hold class 1)
    would move the distances next to the edge."""
    boundary, L = mod("boundary"), mod("_lib").lib()
    d = dev()
    t = label_maps(53, (2, 37, 53), 5).to(dtype)
    want = boundary.reference_signed_distance_map(t, 5, spacing, clip)
    ga = GuardedAlloc()
    td = gin(ga, t, d, fill=1)
    with guarded(monkeypatch, "ops", "boundary", registry=ga):
        got = boundary.signed_distance_map(td, 5, spacing, clip)
    verify(ga, [got], ws=L.csu_signed_distance_workspace(2, 5, 37, 53))
    finite(got)
    check_maps(got, want, spacing)


@pytest.mark.parametrize("bg", [False, True], ids=["fg", "all"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_loss_forward_and_backward(dtype, bg, monkeypatch):
    """(2, 3, 7, 9) in the class-last padded layout, one Tversky row per image, phi passed as data between NaN
    guards: loss, terms, hard sums and dz (the padding included: zeros) are written whole, nothing else is."""
    L = mod("_lib").lib()
    d = dev()
    shape, combo = (2, 3, 7, 9), COMBOS[0]
    z, t = make_case(shape, dtype=dtype)
    phi = make_phi(shape)
    lref, gref, tref, scale, sref = ref_bd_loss_grad(z, t, phi, combo, bg, True)
    for lab in (torch.int64, torch.uint8):
        ga = GuardedAlloc()
        za = _place_guarded(ga, z, "class_last_padded", d)
        td, phid = gin(ga, t.to(lab), d, fill=77), gin(ga, phi, d)
        crit = make_criterion(3, combo, bg, True)
        crit(z.to(d), t.to(d), dist=phi.to(d))          # the weight's device scalar is made outside the guarded block
        with guarded(monkeypatch, "ops", "losses", registry=ga):
            loss, stats = crit.loss_stats(za, td, dist=phid)
            (loss * UPSTREAM).backward()
        verify(ga, [loss, stats, crit.last_terms], ws=L.csu_seg_bd_workspace(2, 3, 63))
        finite(loss, stats, crit.last_terms, za.grad)
        assert za.grad.dtype == dtype
        check_bd_loss(loss, crit.last_terms, lref, tref, scale, combo[2])
        check_bd_grad(za.grad, gref, bf16=dtype == torch.bfloat16)
        assert torch.equal(stats.cpu(), sref)


def test_criterion_makes_its_maps_between_guards(monkeypatch):
    """The whole criterion at (2, 5, 37, 53): maps from the guarded target, then the loss: both workspaces are seen
    at their claimed sizes and the result is the one computed with the reference's maps."""
    boundary, L = mod("boundary"), mod("_lib").lib()
    d = dev()
    shape = (2, 5, 37, 53)
    z, _ = make_case(shape)
    t = label_maps(54, (2, 37, 53), 5)
    phi = boundary.signed_distance_map(t, 5)
    lref, gref, tref, scale, sref = ref_bd_loss_grad(z, t, phi, COMBOS[0], False, False)
    ga = GuardedAlloc()
    za, td = gin(ga, z, d, grad=True), gin(ga, t, d, fill=1)
    crit = make_criterion(5, COMBOS[0], False, False)
    crit(z.to(d), t.to(d))
    with guarded(monkeypatch, "ops", "boundary", "losses", registry=ga):
        loss, stats = crit.loss_stats(za, td)
        (loss * UPSTREAM).backward()
    verify(ga, [loss, stats, crit.last_terms], ws=L.csu_seg_bd_workspace(2, 5, 37 * 53))
    assert ga.saw_workspace(L.csu_signed_distance_workspace(2, 5, 37, 53))
    finite(loss, stats, crit.last_terms, za.grad)
    check_bd_loss(loss, crit.last_terms, lref, tref, scale, COMBOS[0][2])
    check_bd_grad(za.grad, gref)
    assert torch.equal(stats.cpu(), sref)
