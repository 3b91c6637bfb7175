"""CPU checks of csu.augment: the definitions (reference_augment), the table's folded inverse affine, the CPU
draw, the raw dataset output and the ctypes mirror of csu_augment_config.  No GPU."""
import ctypes
import itertools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from csu import augment as A
from csu.augment import SpatialAugment, identity_table, make_table, reference_augment
from csu.data import AugmentationTransform, SegmentationDataset

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pair(B, H, W, seed=0, classes=5):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    lab = torch.randint(0, classes, (B, H, W), dtype=torch.uint8, generator=g)
    return img, lab


def test_identity_table_changes_nothing():
    img, lab = pair(2, 9, 14)
    t = identity_table(2)
    for border in ("constant", "replicate"):
        o, m = reference_augment(img, lab, t, border=border, mask_mode="nearest", out="labels", pad_label=255)
        assert o.dtype == torch.float32 and m.dtype == torch.int64
        assert torch.equal(o, (img.float() / 255.0).permute(0, 3, 1, 2))
        assert torch.equal(m, lab.long())
        o2, mb = reference_augment(img, lab, t, border=border)
        assert torch.equal(o2, o) and torch.equal(mb, (lab.float() / 255.0)[:, None])
        _, mn = reference_augment(img, lab, t, border=border, mask_mode="nearest")
        assert torch.equal(mn, mb)


def test_flips_and_quarter_turns_match_the_host_transform():
    """Every (h, v, k) on a square equals AugmentationTransform.crop with a full crop; on a rectangle the flips."""
    img, lab = pair(1, 16, 16, seed=1)
    for h, v, k in itertools.product((0, 1), (0, 1), range(4)):
        t = make_table(16, 16, [dict(hflip=h, vflip=v, k=k)])
        o, m = reference_augment(img, lab, t, mask_mode="nearest", out="labels")
        ri, rm, _ = AugmentationTransform.crop(img[0].numpy(), lab[0].numpy(), (h, v, k, 0, 0, 16, 16))
        assert torch.equal(o[0], torch.from_numpy(np.ascontiguousarray(ri)).float().permute(2, 0, 1) / 255.0), (h, v, k)
        assert torch.equal(m[0], torch.from_numpy(np.ascontiguousarray(rm)).long()), (h, v, k)
    img, lab = pair(1, 12, 20, seed=2)
    for h, v in itertools.product((0, 1), (0, 1)):
        t = make_table(12, 20, [dict(hflip=h, vflip=v)])
        o, m = reference_augment(img, lab, t, mask_mode="nearest", out="labels")
        ri, rm, _ = AugmentationTransform.crop(img[0].numpy(), lab[0].numpy(), (h, v, 0, 0, 0, 12, 20))
        assert torch.equal(o[0], torch.from_numpy(np.ascontiguousarray(ri)).float().permute(2, 0, 1) / 255.0)
        assert torch.equal(m[0], torch.from_numpy(np.ascontiguousarray(rm)).long())


def shifted(x, tx, ty, fill, replicate):
    """x (..., H, W) with its content moved by (tx, ty) pixels; the vacated band holds `fill` or the edge."""
    H, W = x.shape[-2:]
    ys, xs = torch.arange(H) - ty, torch.arange(W) - tx
    out = x[..., ys.clamp(0, H - 1), :][..., xs.clamp(0, W - 1)]
    if not replicate:
        inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None]
        out = torch.where(inside, out, torch.full_like(out, fill))
    return out


@pytest.mark.parametrize("border", ["constant", "replicate"])
def test_integer_translation_is_exact(border):
    img, lab = pair(2, 11, 17, seed=3)
    want_i = (img.float() / 255.0).permute(0, 3, 1, 2)
    for tx, ty in ((3, -2), (-5, 4), (0, 6)):
        t = make_table(11, 17, [dict(tx=tx, ty=ty)] * 2)
        o, m = reference_augment(img, lab, t, border=border, image_fill=0.5, pad_label=255, mask_mode="nearest", out="labels")
        rep = border == "replicate"
        assert torch.equal(o, shifted(want_i, tx, ty, 0.5, rep))
        assert torch.equal(m, shifted(lab.long(), tx, ty, 255, rep))
        assert rep or bool((m == 255).any())


def test_constant_control_field_is_an_integer_translation():
    """The B-spline weights sum to one: a constant field (3, -2) displaces every output pixel by exactly (3, -2),
    i.e. moves the content by (-3, 2)."""
    H, W, sp = 13, 22, 8
    img, lab = pair(1, H, W, seed=4)
    t = make_table(H, W, [dict(elastic=3.0)])
    ctrl = torch.empty((1, 2) + A.control_grid(H, W, sp))
    ctrl[:, 0], ctrl[:, 1] = 3.0, -2.0
    o, m = reference_augment(img, lab, t, ctrl, spacing=sp, pad_label=9, mask_mode="nearest", out="labels")
    o2, m2 = reference_augment(img, lab, make_table(H, W, [dict(tx=-3, ty=2)]), pad_label=9, mask_mode="nearest", out="labels")
    assert torch.equal(o, o2) and torch.equal(m, m2)
    sx, sy = A.reference_source_coords(t, ctrl, sp, H, W)
    assert torch.equal(sx[0], (torch.arange(W, dtype=torch.float64) + 3.0).expand(H, W))
    assert torch.equal(sy[0], (torch.arange(H, dtype=torch.float64) - 2.0)[:, None].expand(H, W))


def compose_np(row, H, W):
    """The inverse of T(t) C R(angle) S(scale) Q(k) F(h, v) C^-1 with numpy matrices."""
    h, v, k, ang, s, tx, ty = (float(x) for x in row[:7])

    def m(a, b, c, d, e=0.0, f=0.0):
        return np.array([[a, b, e], [c, d, f], [0.0, 0.0, 1.0]])
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    Q = np.linalg.matrix_power(m(0, -1, 1, 0), int(k))
    M = (m(1, 0, 0, 1, tx, ty) @ m(1, 0, 0, 1, cx, cy) @ m(math.cos(ang), -math.sin(ang), math.sin(ang), math.cos(ang))
         @ m(s, 0, 0, s) @ Q @ m(-1 if h else 1, 0, 0, -1 if v else 1) @ m(1, 0, 0, 1, -cx, -cy))
    return np.linalg.inv(M)[:2].reshape(-1)


def full_augment(**kw):
    """Every transform on; the probabilities not given are the default 0.5."""
    args = dict(rotate=(-30, 30), p_rotate=0.7, scale=(0.6, 1.6), p_scale=0.6, translate=0.2, p_translate=0.8,
                flip_prob=0.5, rot90_prob=0.4, elastic=(8, 1.0, 4.0), brightness=(0.8, 1.2), contrast=(0.75, 1.25),
                gamma=(0.7, 1.5), noise=(0.0, 0.05))
    args.update(kw)
    return SpatialAugment(**args)


def test_cpu_drawn_rows_fold_their_raw_draws():
    H, W = 24, 37
    aug = full_augment()
    t, ctrl = aug.draw(64, H, W, "cpu", generator=torch.Generator().manual_seed(5))
    assert t.shape == (64, A.TABLE_P) and t.dtype == torch.float32 and ctrl.shape == (64, 2) + A.control_grid(H, W, 8)
    for b in range(64):
        want = compose_np(t[b].double().numpy(), H, W)
        got = t[b, A.T_A:A.T_A + 6].double().numpy()
        assert np.all(np.abs(got - want) <= 1e-6 * (1.0 + np.abs(want))), (b, got, want)
    assert len(set(t[:, A.T_ROT90].tolist())) == 4 and 0 < int((t[:, A.T_ANGLE] != 0).sum()) < 64
    assert bool((t[:, A.T_SCALE] >= 0.6).all()) and bool((t[:, A.T_SCALE] <= 1.6).all())
    assert bool((ctrl.abs().amax(dim=(1, 2, 3)) <= t[:, A.T_ELASTIC]).all())
    assert bool((ctrl[t[:, A.T_ELASTIC] == 0] == 0).all())
    # integer rows are exact: flips, turns and whole-pixel shifts give integers and half-integers
    ti = make_table(H, W, [dict(hflip=1, k=3, tx=4, ty=-7)])
    assert np.array_equal(ti[0, A.T_A:A.T_A + 6].double().numpy(), compose_np(ti[0].numpy(), H, W).round(1))


def test_cpu_end_to_end_keeps_labels():
    img, lab = pair(4, 33, 29, seed=6, classes=4)
    aug = full_augment(pad_label=255, mask_mode="nearest", out="labels")
    o, m = aug(img, lab, generator=torch.Generator().manual_seed(7))
    assert o.shape == (4, 3, 33, 29) and o.dtype == torch.float32 and float(o.min()) >= 0 and float(o.max()) <= 1
    assert m.shape == (4, 33, 29) and m.dtype == torch.int64
    assert set(m.unique().tolist()) <= set(lab.unique().tolist()) | {255}
    ob, mb = SpatialAugment(rotate=(-20, 20), p_rotate=1.0)(img, (lab > 1).to(torch.uint8) * 255,
                                                             generator=torch.Generator().manual_seed(8))
    assert mb.shape == (4, 1, 33, 29) and float(mb.min()) >= 0 and float(mb.max()) <= 1
    with pytest.raises(ValueError):
        SpatialAugment(mask_mode="bilinear", out="labels")
    with pytest.raises(ValueError):
        SpatialAugment(elastic=(2, 0.0, 1.0))


def test_raw_dataset(tmp_path):
    from PIL import Image
    (tmp_path / "img").mkdir()
    (tmp_path / "mask").mkdir()
    rng = np.random.default_rng(0)
    lab = rng.integers(0, 3, (40, 36)).astype(np.uint8)
    Image.fromarray(rng.integers(0, 256, (40, 36, 3), dtype=np.uint8)).save(tmp_path / "img" / "a.png")
    Image.fromarray(lab).save(tmp_path / "mask" / "a.png")
    dirs = (str(tmp_path / "img"), str(tmp_path / "mask"))
    ds = SegmentationDataset(*dirs, image_size=(32, 24), label_mode=True, raw=True, augment=True)
    x, m = ds[0]
    li, lm = ds.load(0)
    assert x.dtype == torch.uint8 and tuple(x.shape) == (24, 32, 3) and torch.equal(x, torch.from_numpy(li))
    assert m.dtype == torch.uint8 and tuple(m.shape) == (24, 32) and torch.equal(m, torch.from_numpy(lm))
    assert set(m.unique().tolist()) <= {0, 1, 2}
    with pytest.raises(ValueError):
        SegmentationDataset(*dirs, image_size=(32, 24), label_mode=True, device_augment=True)
    with pytest.raises(ValueError):
        SegmentationDataset(*dirs, image_size=(32, 24), label_mode=True, device_augment=True, raw=True)
    Image.fromarray(rng.integers(0, 256, (40, 36, 3), dtype=np.uint8)).save(tmp_path / "img" / "b.jpg")
    Image.fromarray(((rng.random((40, 36)) > 0.5) * 255).astype(np.uint8)).save(tmp_path / "mask" / "b.jpg")
    xb, mb = SegmentationDataset(*dirs, image_size=(32, 24), raw=True)[0]
    assert xb.dtype == torch.uint8 and mb.dtype == torch.uint8 and tuple(mb.shape) == (24, 32)
    Image.fromarray((lab.astype(np.uint16) * 200)).save(tmp_path / "mask" / "a.png")     # mode I;16: values up to 400
    with pytest.raises(ValueError, match="0..255"):
        SegmentationDataset(*dirs, image_size=(32, 24), label_mode=True, raw=True)[0]


def test_config_struct_matches_the_header(tmp_path):
    """The ctypes mirror of csu_augment_config has the C compiler's size and offsets, and CSU_AUGMENT_P is TABLE_P."""
    from csu import _lib, ops, rng
    fields = ["p_hflip", "rotate_hi", "translate_y", "gamma_lo", "elastic_hi", "spacing"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "csu.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(csu_augment_config));', 'printf("P %d\\n", CSU_AUGMENT_P);']
    lines += [f'printf("{f} %zu\\n", offsetof(csu_augment_config, {f}));' for f in fields] + ["return 0; }"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")],
                   check=True)
    got = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    assert ctypes.sizeof(_lib.AugmentConfig) == int(got["size"])
    assert int(got["P"]) == A.TABLE_P == ops.AUGMENT_P
    for f in fields:
        assert getattr(_lib.AugmentConfig, f).offset == int(got[f]), f
    sites = (rng.SITE_AUGMENT_DRAW, rng.SITE_AUGMENT_CTRL, rng.SITE_AUGMENT_NOISE)
    assert len(set(sites)) == 3 and all(rng.SITE_BASE + rng.SITE_STRIDE * 200 < s < 4096 for s in sites)
    c = full_augment().config(20, 40)
    assert c.spacing == 8 and abs(c.rotate_hi - math.radians(30)) < 1e-6 and c.translate_x == 8.0 and c.translate_y == 4.0
