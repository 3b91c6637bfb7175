"""csu.patches on the CPU: the numpy / fp64 references of the patch pool (row index, locate, the draw's origin rules
and its fall-back, the sample) against plain slicing and np.argwhere, a CPU pool end to end, the dataset at its
files' own sizes, and the header / library / ctypes agreement of the new entry points."""
import os
import re

import numpy as np
import pytest
import torch

from csu import patches as P
from csu.augment import SpatialAugment, identity_table, make_table
from csu.patches import (PatchLoader, PatchPool, PatchSampler, reference_locate, reference_origin, reference_patch_draw,
                         reference_patch_sample, reference_row_index)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case(H, W, seed, classes=4, ignore=None):
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    lab = g.integers(0, classes, (H, W), dtype=np.uint8)
    if ignore is not None:
        lab[g.random((H, W)) < 0.1] = ignore
    return img, lab


def pool_of(sizes, K=4, ignore=None, seed=0):
    cases = [case(H, W, seed + i, classes=K if K > 1 else 2, ignore=ignore) for i, (H, W) in enumerate(sizes)]
    if K == 1:
        cases = [(im, (lb * 255).astype(np.uint8)) for im, lb in cases]
    return PatchPool([c[0] for c in cases], [c[1] for c in cases], K, "cpu", ignore_index=ignore), cases


def record(rows):
    """int32 (B, 16) records of explicit (n, oy, ox)."""
    rec = np.zeros((len(rows), P.RECORD), dtype=np.int32)
    for b, (n, oy, ox) in enumerate(rows):
        rec[b, P.R_N], rec[b, P.R_OY], rec[b, P.R_OX] = n, oy, ox
    return rec


def test_identity_table_with_an_integer_origin_is_the_slice():
    pool, cases = pool_of([(40, 52), (33, 47)])
    Ph, Pw = 16, 21
    rows = [(0, 0, 0), (1, 17, 26), (0, 24, 31), (1, 5, 0)]          # the last two touch the far / near edges
    oi, ol = reference_patch_sample(pool, record(rows), Ph, Pw, identity_table(len(rows)), mask_mode="nearest", out="labels")
    for b, (n, oy, ox) in enumerate(rows):
        img, lab = cases[n]
        want = torch.from_numpy(img[oy:oy + Ph, ox:ox + Pw]).float() / 255.0
        assert torch.equal(oi[b], want.permute(2, 0, 1))
        assert torch.equal(ol[b], torch.from_numpy(lab[oy:oy + Ph, ox:ox + Pw].astype(np.int64)))


def test_a_smaller_image_is_centred_and_padded():
    pool, cases = pool_of([(9, 12)])
    Ph, Pw = 16, 17                                              # differences 7 (odd) and 5 (odd): origin -3, -2
    rec = reference_patch_draw(np.zeros((1, 8), dtype=np.int64), pool, Ph, Pw)
    assert tuple(rec[0, [P.R_OY, P.R_OX]]) == (-3, -2)
    oi, ol = reference_patch_sample(pool, rec, Ph, Pw, identity_table(1), image_fill=0.25, pad_label=255, mask_mode="nearest",
                                    out="labels")
    want_i = torch.full((3, Ph, Pw), 0.25)
    want_l = torch.full((Ph, Pw), 255, dtype=torch.int64)
    img, lab = cases[0]
    want_i[:, 3:12, 2:14] = (torch.from_numpy(img).float() / 255.0).permute(2, 0, 1)
    want_l[3:12, 2:14] = torch.from_numpy(lab.astype(np.int64))
    assert torch.equal(oi[0], want_i) and torch.equal(ol[0], want_l)


@pytest.mark.parametrize("K", [1, 4])
def test_reference_locate_is_argwhere_order(K):
    g = np.random.default_rng(5)
    lab = g.integers(0, 4, (13, 70), dtype=np.uint8)
    lab[3:6] = 0                                                 # rows that are empty before a hit
    lab[7] = 2                                                   # a class that fills a row
    lab[lab == 3] = 0                                            # an absent class
    lab[0, 5] = 200                                              # an ignore value: no class when K = 4
    rows = reference_row_index(lab, K)
    cls = P.class_map(lab, K)
    for c in range(P.num_index_classes(K)):
        want = np.argwhere(cls == c)
        assert rows[c, -1] == len(want)
        assert np.array_equal(rows[c], np.concatenate([[0], np.cumsum((cls == c).sum(1))]))
        for r in range(len(want)):
            assert reference_locate(lab, K, c, r) == tuple(want[r]), (c, r)
        assert reference_locate(lab, K, c, len(want)) == (-1, -1)
    if K == 4:
        assert rows[:, -1].sum() == lab.size - 1                 # the ignore pixel is in no class


def test_origin_rules_at_the_clamps():
    P_ = 8
    assert reference_origin(20, P_, True, 0, 0) == 0             # centre in the near corner
    assert reference_origin(20, P_, True, 19, 0) == 12           # and the far one: the patch stays inside
    assert reference_origin(20, P_, True, 10, 0) == 6            # free: centred on c
    assert reference_origin(8, P_, True, 5, 0) == 0 and reference_origin(8, P_, False, -1, 0xFFFFFFFF) == 0      # L == P
    assert reference_origin(9, P_, False, -1, 0) == 0 and reference_origin(9, P_, False, -1, 0xFFFFFFFF) == 1    # L == P + 1
    assert reference_origin(9, P_, True, 8, 0) == 1
    assert reference_origin(5, P_, True, 2, 123) == -1 and reference_origin(5, P_, False, -1, 123) == -1         # odd difference
    assert reference_origin(4, P_, False, -1, 123) == -2                                                          # even difference
    for c in range(20):                                          # a foreground patch contains its centre
        o = reference_origin(20, P_, True, c, 0)
        assert 0 <= o <= 12 and o <= c < o + P_
    assert all(0 <= P._pick(w, 13) < 13 for w in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF))
    assert P._pick(0xFFFFFFFF, 1 << 31) == (1 << 31) - 1         # no 24-bit ceiling on a count


def test_draw_centres_on_a_class_and_falls_back_without_one():
    pool, cases = pool_of([(30, 41), (25, 25)], K=4)
    cases[1][1][:] = 0                                           # case 1 holds background only
    pool = PatchPool([c[0] for c in cases], [c[1] for c in cases], 4, "cpu")
    g = np.random.default_rng(1)
    words = g.integers(0, 1 << 32, (64, 8), dtype=np.int64)
    idx = [b % 2 for b in range(64)]
    rec = reference_patch_draw(words, pool, 8, 8, fg_slots=64, indices=idx)
    assert np.array_equal(rec[:, 8:].view(np.uint32), words.astype(np.uint32))
    for b in range(64):
        n, cls, cy, cx, oy, ox, fg, count = rec[b, :8]
        assert n == idx[b]
        if n == 1:                                               # no eligible class present: a uniform slot
            assert (cls, cy, cx, fg, count) == (-1, -1, -1, 0, 0)
            assert oy == P._pick(words[b, 4], 25 - 8 + 1) and ox == P._pick(words[b, 5], 25 - 8 + 1)
        else:
            lab = cases[0][1]
            assert fg == 1 and 1 <= cls <= 3 and lab[cy, cx] == cls and count == int((lab == cls).sum())
            assert oy <= cy < oy + 8 and ox <= cx < ox + 8 and 0 <= oy <= 22 and 0 <= ox <= 33
    only0 = reference_patch_draw(words, pool, 8, 8, fg_slots=64, class_mask=1, indices=[1] * 64)
    assert (only0[:, P.R_CLS] == 0).all() and (only0[:, P.R_FG] == 1).all()      # class 0 when asked for
    uni = reference_patch_draw(words, pool, 8, 8, fg_slots=3, p_fg=0.0, indices=[0] * 64)
    assert uni[:3, P.R_FG].tolist() == [1, 1, 1] and not uni[3:, P.R_FG].any()


def test_cpu_pool_sampler_and_loader():
    pool, cases = pool_of([(40, 52), (33, 47), (10, 12)], K=3, ignore=255)
    assert len(pool) == 3 and pool.size(1) == (33, 47)
    assert np.array_equal(pool.image(1).numpy(), cases[1][0]) and np.array_equal(pool.label(2).numpy(), cases[2][1])
    assert pool.meta.tolist()[1] == [40 * 52, 33, 47, 3 * 41]
    want = torch.tensor([c[0].astype(np.float64).mean() / 255.0 for c in cases]).float()
    assert torch.equal(pool.mean, want)
    yx = pool.locate([0, 1, 2], [1, 2, 0], [0, 5, 10 ** 6])
    assert yx[0].tolist() == list(np.argwhere(cases[0][1] == 1)[0]) and yx[1].tolist() == list(np.argwhere(cases[1][1] == 2)[5])
    assert yx[2].tolist() == [-1, -1]
    pairs = list(pool.pairs())
    assert len(pairs) == 3 and tuple(pairs[1][0].shape) == (33, 47, 3) and tuple(pairs[1][1].shape) == (33, 47)
    aug = SpatialAugment(rotate=(-20, 20), p_rotate=1.0, flip_prob=0.5, elastic=(8, 1.0, 2.0), noise=(0.0, 0.05), pad_label=255,
                         mask_mode="nearest", out="labels")
    sampler = PatchSampler(pool, (16, 20), 6, foreground=0.5, augment=aug)
    assert sampler.fg_slots == 3 and sampler.p_fg == 0.0
    g = torch.Generator().manual_seed(3)
    x, y = sampler.sample(generator=g)
    assert tuple(x.shape) == (6, 3, 16, 20) and x.dtype == torch.float32 and tuple(y.shape) == (6, 16, 20) and y.dtype == torch.int64
    assert float(x.min()) >= 0 and float(x.max()) <= 1 and set(y.unique().tolist()) <= {0, 1, 2, 255}
    assert tuple(sampler.last_record.shape) == (6, 16) and sampler.last_record[:3, P.R_FG].tolist() == [1, 1, 1]
    x2, y2 = PatchSampler(pool, (16, 20), 6, foreground=0.5, augment=aug).sample(generator=torch.Generator().manual_seed(3))
    assert torch.equal(x, x2) and torch.equal(y, y2)
    loader = PatchLoader(PatchSampler(pool, 8, 2, foreground=1.0, foreground_mode="probability"), steps_per_epoch=3)
    assert len(loader) == 3 and len(list(loader)) == 3
    bp, _ = pool_of([(20, 20)], K=1)
    xb, mb = PatchSampler(bp, 8, 2).sample(generator=g)
    assert tuple(mb.shape) == (2, 1, 8, 8) and mb.dtype == torch.float32 and set(mb.unique().tolist()) <= {0.0, 1.0}
    with pytest.raises(ValueError):
        PatchPool([cases[0][0]], [cases[0][1][:5]], 3, "cpu")
    with pytest.raises(ValueError):
        PatchPool([cases[0][0]], [cases[0][1]], 3, "cpu", ignore_index=2)
    with pytest.raises(ValueError):
        PatchSampler(pool, 8, 2, classes=[3])


def test_a_rotated_patch_is_the_rotated_slice():
    """A quarter turn and a flip about the patch centre commute with the crop."""
    pool, cases = pool_of([(40, 52)])
    S = 15
    table = make_table(S, S, [dict(k=1), dict(hflip=1), dict(k=2, vflip=1)])
    rows = [(0, 3, 7), (0, 25, 37), (0, 11, 0)]
    oi, ol = reference_patch_sample(pool, record(rows), S, S, table, mask_mode="nearest", out="labels")
    plain = reference_patch_sample(pool, record(rows), S, S, identity_table(3), mask_mode="nearest", out="labels")
    assert torch.equal(oi[0], torch.rot90(plain[0][0], -1, (1, 2))) and torch.equal(ol[0], torch.rot90(plain[1][0], -1, (0, 1)))
    assert torch.equal(oi[1], plain[0][1].flip(2)) and torch.equal(ol[1], plain[1][1].flip(1))
    assert torch.equal(oi[2], plain[0][2].flip(2)) and torch.equal(ol[2], plain[1][2].flip(1))      # a half turn of a vflip


def test_dataset_returns_files_at_their_own_size(tmp_path):
    from PIL import Image
    from csu.data import SegmentationDataset
    (tmp_path / "img").mkdir()
    (tmp_path / "mask").mkdir()
    g = np.random.default_rng(0)
    sizes = [(40, 36), (25, 61)]
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / "img" / f"{i}.png")
        Image.fromarray(g.integers(0, 3, (h, w), dtype=np.uint8)).save(tmp_path / "mask" / f"{i}.png")
    ds = SegmentationDataset(str(tmp_path / "img"), str(tmp_path / "mask"), image_size=None, label_mode=True, raw=True)
    for i, (h, w) in enumerate(sizes):
        im, lb = ds[i]
        assert tuple(im.shape) == (h, w, 3) and im.dtype == torch.uint8 and tuple(lb.shape) == (h, w) and lb.dtype == torch.uint8
        assert np.array_equal(lb.numpy(), np.asarray(Image.open(tmp_path / "mask" / f"{i}.png")))
    pool = PatchPool.from_dataset(ds, 3, "cpu")
    assert [pool.size(i) for i in range(2)] == sizes and torch.equal(pool.label(1), ds[1][1])
    with pytest.raises(ValueError):
        SegmentationDataset(str(tmp_path / "img"), str(tmp_path / "mask"), image_size=None, label_mode=True)


def test_header_library_and_ctypes_agree_on_the_patch_entry_points():
    import ctypes
    from csu import _lib, ops, rng
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "csu.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ("csu_patch_index", "csu_patch_draw", "csu_patch_locate", "csu_patch_warp"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, name
        assert hasattr(L, name) and name in _lib._SIGS
        args = [a.strip() for a in m.group(1).split(",")]
        restype, argtypes = _lib._SIGS[name]
        assert restype is ctypes.c_int and len(argtypes) == len(args), name
        for a, t in zip(args, argtypes):
            want = (ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else
                    ctypes.c_uint if a.startswith("unsigned") else ctypes.c_int)
            assert t is want, (name, a, t)
    assert int(re.search(r"#define\s+CSU_PATCH_RECORD\s+(\d+)", src).group(1)) == ops.PATCH_RECORD == P.RECORD
    assert rng.SITE_PATCH_DRAW == 4083
    assert L.csu_patch_index(0, 4, 1, None, None, None, None) != 0 and b"patch_index" in L.csu_last_error_string()
