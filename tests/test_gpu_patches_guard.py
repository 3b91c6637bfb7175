"""Guard-band case of csu.patches (README "Testing"): csu_patch_index, csu_patch_draw, csu_patch_locate and
csu_patch_warp stay inside their outputs, write all of them, leave the pool alone and let no byte outside it reach a
result.  The second image of the pool starts at an odd byte offset (the first has 7 x 5 pixels), and one patch hangs
over two edges of its image, so the clamped taps run along the pool's guards."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from csu import patches as P
from csu.augment import reference_source_coords
from csu.patches import PatchPool, reference_patch_draw, reference_patch_sample
from guard_alloc import GuardedAlloc
from test_gpu_augment_warp import SPACING, compare, snap_of
from test_gpu_guard_bands import dev, finite, gin, guarded, mod, verify
from test_gpu_patches import TOL_PATCH
from test_augment_warp import full_augment

SIZES = [(7, 5), (40, 52), (23, 61)]
K, B, Ph, Pw = 4, 4, 23, 37


@pytest.mark.parametrize("border,mask_mode,out", [("constant", "nearest", "labels"), ("replicate", "bilinear", "binary")])
def test_index_draw_locate_and_warp_between_guards(border, mask_mode, out, monkeypatch):
    ops = mod("ops")
    d = dev()
    g = np.random.default_rng(800)
    images = [g.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in SIZES]
    labels = [g.integers(0, K, (H, W), dtype=np.uint8) for H, W in SIZES]
    labels[1][g.random(SIZES[1]) < 0.1] = 255
    cpu = PatchPool(images, labels, K, "cpu", ignore_index=255)
    assert int(cpu.meta[1, 0]) % 2 == 1
    aug = full_augment(p_elastic=1.0)
    cfg = aug.config(Ph, Pw)
    snap = snap_of(d, 5, 2)
    table, ctrl = (t.cpu() for t in ops.augment_draw(cfg, B, Ph, Pw, snap, elastic=True))     # unguarded, to compare
    table[:, 10], table[:, 9] = 0.0, 1.0         # parity: no noise; gamma has its own tolerance and test (T_SIGMA, T_GAMMA)
    # slot 0 hangs over the top and the right edge of image 1, slot 1 covers the 7 x 5 image, 2 and 3 are drawn
    fixed = np.zeros((2, P.RECORD), dtype=np.int32)
    fixed[0, [P.R_N, P.R_OY, P.R_OX]] = (1, -9, 30)
    fixed[1, [P.R_N, P.R_OY, P.R_OX]] = (0, -8, -16)
    ga = GuardedAlloc()
    pool = types.SimpleNamespace(N=cpu.N, num_classes=K, pixels=gin(ga, cpu.pixels, d, fill=255), labels=gin(ga, cpu.labels, d, fill=200),
                                 meta=gin(ga, cpu.meta, d, fill=-1), mean=gin(ga, cpu.mean, d))
    tabd, ctrld, snapd = gin(ga, table, d), gin(ga, ctrl, d), gin(ga, snap.cpu(), d, fill=-1)
    qn, qc, qr = (gin(ga, torch.tensor(v, dtype=torch.int32), d, fill=-1) for v in ([1, 1, 2, 0], [1, 3, 2, 1], [0, 10 ** 6, 17, 3]))
    with guarded(monkeypatch, "ops", registry=ga):
        pool.rows = ops.patch_index(pool.labels, pool.meta, K, 40, cpu.rows.numel())
        drawn = ops.patch_draw(pool, Ph, Pw, B, snapd, fg_slots=3, p_fg=0.5)
        yx = ops.patch_locate(pool, qn, qc, qr)
        rec = torch.cat([torch.from_numpy(fixed).to(d), drawn[2:]])
        got = ops.patch_warp(pool, rec, Ph, Pw, tabd, ctrld, spacing=SPACING, snap=None, border=border, image_fill=0.25,
                             pad_label=255, mask_mode=mask_mode, out=out)
    verify(ga, [pool.rows, drawn, yx, *got])
    finite(got[0], *(x for x in (got[1],) if x.is_floating_point()))
    assert torch.equal(pool.rows.cpu(), cpu.rows)
    dr = drawn.cpu().numpy()
    assert np.array_equal(dr, reference_patch_draw(dr[:, 8:], cpu, Ph, Pw, fg_slots=3, p_fg=0.5))
    want_yx = [list(np.argwhere(labels[1] == 1)[0]), [-1, -1], list(np.argwhere(labels[2] == 2)[17]), list(np.argwhere(labels[0] == 1)[3])]
    assert yx.cpu().tolist() == [[int(v) for v in p] for p in want_yx]
    kw = dict(spacing=SPACING, border=border, image_fill=0.25, pad_label=255, mask_mode=mask_mode, out=out)
    want = reference_patch_sample(cpu, rec.cpu().numpy(), Ph, Pw, table, ctrl, **kw)
    sx, sy = reference_source_coords(table, ctrl, SPACING, Ph, Pw)
    near = lambda s: ((s + 0.5) - torch.round(s + 0.5)).abs() < 1e-3
    excluded = near(sx) | near(sy)
    assert float(excluded.double().mean()) <= 0.02
    compare(f"guarded patch_warp {border} {mask_mode} {out}", got, want, excluded, mask_mode, TOL_PATCH)
