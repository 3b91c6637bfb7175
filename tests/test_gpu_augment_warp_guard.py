"""Guard-band case of csu.augment (README "Testing"): csu_augment_draw, csu_augment_mean and csu_augment_warp
stay inside their outputs and scratch, write all of their outputs, leave their inputs alone and let no byte
outside an input reach a result.  The second image of the batch starts at an odd byte offset, so the mean's
16-byte loads take their unaligned head and tail path next to the guards."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from csu import augment as A
from csu.augment import reference_augment
from guard_alloc import GuardedAlloc
from test_gpu_augment_warp import SPACING, TOL_WARP, compare, pair, snap_of
from test_gpu_guard_bands import dev, finite, gin, guarded, mod, verify
from test_augment_warp import full_augment

B, H, W = 2, 23, 37


@pytest.mark.parametrize("border,mask_mode,out", [("constant", "nearest", "labels"), ("replicate", "bilinear", "binary")])
def test_draw_mean_and_warp_between_guards(border, mask_mode, out, monkeypatch):
    ops = mod("ops")
    d = dev()
    img, lab = pair(B, H, W, 700)
    aug = full_augment(p_elastic=1.0)
    cfg = aug.config(H, W)
    snap = snap_of(d, 5, 2)
    table, ctrl = (t.cpu() for t in ops.augment_draw(cfg, B, H, W, snap, elastic=True))     # unguarded, to compare
    assert bool((table[:, A.T_ELASTIC] > 0).all())
    drawn = table.clone()
    table[:, A.T_SIGMA], table[:, A.T_GAMMA] = 0.0, 1.0      # parity: no noise; gamma has its own tolerance and test
    kw = dict(spacing=SPACING, border=border, image_fill=0.25, pad_label=255, mask_mode=mask_mode, out=out)
    want = reference_augment(img, lab, table, ctrl, **kw)
    sx, sy = A.reference_source_coords(table, ctrl, SPACING, H, W)
    near = lambda s: ((s + 0.5) - torch.round(s + 0.5)).abs() < 1e-3
    excluded = near(sx) | near(sy)
    assert float(excluded.double().mean()) <= 0.02
    ga = GuardedAlloc()
    imgd, labd = gin(ga, img, d, fill=255), gin(ga, lab, d, fill=200)
    tabd, ctrld, snapd = gin(ga, table, d), gin(ga, ctrl, d), gin(ga, snap.cpu(), d, fill=-1)
    with guarded(monkeypatch, "ops", registry=ga):
        t2, c2 = ops.augment_draw(cfg, B, H, W, snapd, elastic=True)
        mean = ops.augment_mean(imgd)
        got = ops.augment_warp(imgd, labd, tabd, ctrld, mean=mean, snap=snapd, **kw)
        noisy = ops.augment_warp(imgd, labd, t2, c2, snap=snapd, **kw)                      # the mean computed inside
    verify(ga, [t2, c2, mean, *got, *noisy])
    finite(t2, c2, mean, got[0], noisy[0], *(x for x in (got[1], noisy[1]) if x.is_floating_point()))
    assert torch.equal(c2.cpu(), ctrl) and torch.equal(t2.cpu(), drawn)
    assert torch.equal(mean.cpu(), (img.long().sum(dim=(1, 2, 3)).double() / (255.0 * H * W * 3)).float())
    compare(f"guarded {border} {mask_mode} {out}", got, want, excluded, mask_mode, TOL_WARP)
    assert float(noisy[0].min()) >= 0 and float(noisy[0].max()) <= 1
