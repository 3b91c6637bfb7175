"""csu.patches on the MI355X: the row index, the wave select (exhaustively), the draw (recomputed exactly from its
own raw words by reference_patch_draw, its shares and purity), csu_patch_warp against csu_augment_warp (bitwise),
against reference_patch_sample (fp64, on the CPU) and against plain slices, graph capture and the loader.

Tolerances.  The patch warp evaluates the source position in the patch frame and adds the origin as an integer, so
the rounding boundaries of a label are the patch frame's: labels are exact wherever the fp64 coordinate is further
than EDGE = 1e-3 px from a rounding boundary (the mask of tests/test_gpu_augment_warp.py's mixed_inputs, whose tables
these cases use); the excluded share is asserted <= 2 % first.  Images and bilinear masks: 4 x the largest
deviation measured on the MI355X over these same cases, the value beside the constant; above 1e-3 is a bug whatever
the constants say.  Shares of the draw: 5 standard deviations of the binomial count, stated where they are used."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from csu import augment as A
from csu import patches as P
from csu.augment import SpatialAugment, identity_table, make_table
from csu.patches import PatchLoader, PatchPool, PatchSampler, reference_patch_draw, reference_patch_sample, reference_row_index
from test_gpu_augment_warp import BUG, MAX_EXCLUDED, MODES, SHAPES, SPACING, compare, dev, mixed_inputs, snap_of

MEASURED_PATCH = 9.060e-6     # largest |image - fp64 reference| over the cases below on the MI355X: the (70, 131) patches of
TOL_PATCH = 4 * MEASURED_PATCH    # the near / far test (8.106e-6 in test_warp_matches_reference); bilinear masks (0 .. 4 / 255)
                              # reach 1.835e-7, the guard case's (0 .. 255 / 255) 2.056e-6 (profiles/patch_sampler_timing.txt)

INDEX_SIZES = [(1, 1), (5, 3), (70, 131), (300, 64), (64, 257)]     # widths below, at and across the 64-label chunks of
IGNORE = 255                                                         # the wave's walk, heights across the 64-row scan


@functools.lru_cache(maxsize=None)
def index_cases(K):
    """The mixed-size cases: labels 0..3 (class 4 of K = 5 is absent), a row that class 2 fills, rows that hold
    class 0 only, 10 % ignore values; every case holds a class >= 1.  K = 1: the same maps as 0 / 255 masks."""
    g = np.random.default_rng(11)
    cases = []
    for H, W in INDEX_SIZES:
        img = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
        lab = g.integers(0, 4, (H, W), dtype=np.uint8)
        if H > 30:
            lab[10] = 2
            lab[20:26] = 0
            lab[g.random((H, W)) < 0.1] = IGNORE
            lab[10] = 2
        lab[H - 1, W - 1] = 1                                    # the last column of the last row
        if K == 1:
            lab = ((lab > 0) & (lab != IGNORE)).astype(np.uint8) * 255
        cases.append((img, lab))
    return cases


@functools.lru_cache(maxsize=None)
def index_pool(K, device):
    cases = index_cases(K)
    return PatchPool([c[0] for c in cases], [c[1] for c in cases], K, device, ignore_index=IGNORE if K > 1 else None)


@pytest.mark.parametrize("K", [5, 1], ids=["five-class", "binary"])
def test_row_index_is_numpys_exclusive_cumulative_count(K):
    d = dev()
    pool = index_pool(K, str(d))
    want = np.concatenate([reference_row_index(lab, K).reshape(-1) for _, lab in index_cases(K)])
    assert pool.rows.dtype == torch.int32 and np.array_equal(pool.rows.cpu().numpy(), want)
    assert torch.equal(pool.rows.cpu(), index_pool(K, "cpu").rows)
    assert torch.equal(pool.mean.cpu(), index_pool(K, "cpu").mean)          # the exact integer sum on both sides
    t = pool.row_table(2)
    if K == 5:
        assert t[4, -1] == 0 and t[2, 11] - t[2, 10] == 131 and (np.diff(t[1:, 20:27], axis=1) == 0).all()
        assert int(t[:, -1].sum()) < 70 * 131                                # ignore values are in no class


@pytest.mark.parametrize("K", [5, 1], ids=["five-class", "binary"])
def test_locate_is_exhaustively_the_argwhere_order(K):
    """Every (image, class, rank) of the pool, ranks 0 .. count (the last one past the end), in one launch."""
    d = dev()
    pool = index_pool(K, str(d))
    qn, qc, qr, want = [], [], [], []
    for n, (_, lab) in enumerate(index_cases(K)):
        cls = P.class_map(lab, K)
        for c in range(P.num_index_classes(K)):
            yx = np.argwhere(cls == c)
            m = len(yx) + 1
            qn.append(np.full(m, n)), qc.append(np.full(m, c)), qr.append(np.arange(m))
            want.append(np.concatenate([yx, [[-1, -1]]]))
    qn, qc, qr = (torch.from_numpy(np.concatenate(q).astype(np.int32)) for q in (qn, qc, qr))
    got = pool.locate(qn, qc, qr)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), np.concatenate(want))
    bad = pool.locate([-1, 5, 0, 0], [1, 1, -1, P.num_index_classes(K)], [0, 0, 0, 0])      # outside the pool
    assert bad.cpu().tolist() == [[-1, -1]] * 4


# ---------------------------------------------------------------------------------------------------------
# draw
# ---------------------------------------------------------------------------------------------------------
def check_records(rec, cases, K, Ph, Pw):
    for row in rec:
        n, cls, cy, cx, oy, ox, fg, count = row[:8].tolist()
        H, W = cases[n][1].shape
        if fg:
            assert P.class_map(cases[n][1], K)[cy, cx] == cls and count > 0
            assert oy <= cy < oy + Ph and ox <= cx < ox + Pw                 # the patch contains its centre
        else:
            assert (cls, cy, cx, count) == (-1, -1, -1, 0)
        for o, L, Pe in ((oy, H, Ph), (ox, W, Pw)):
            assert (0 <= o <= L - Pe) if L >= Pe else o == -((Pe - L) // 2)


@pytest.mark.parametrize("K", [5, 1], ids=["five-class", "binary"])
def test_draw_is_the_reference_of_its_own_words_and_pure(K):
    from csu import ops, rng
    d = dev()
    pool, cpu, cases = index_pool(K, str(d)), index_pool(K, "cpu"), index_cases(K)
    Ph, Pw = 23, 40                      # larger than two cases, one axis of a third
    snap = snap_of(d, 42, 5)
    kw = dict(fg_slots=9, p_fg=0.4)
    rec = ops.patch_draw(pool, Ph, Pw, 64, snap, **kw).cpu().numpy()
    assert np.array_equal(rec, reference_patch_draw(rec[:, 8:], cpu, Ph, Pw, **kw))
    check_records(rec, cases, K, Ph, Pw)
    assert rec[:9, P.R_FG].all() and 0 < rec[9:, P.R_FG].sum() < 55
    assert len(set(rec[:, P.R_N].tolist())) == 5
    # row b is a pure function of (seed, counter, site, b)
    assert np.array_equal(ops.patch_draw(pool, Ph, Pw, 7, snap, **kw).cpu().numpy(), rec[:7])
    assert np.array_equal(ops.patch_draw(pool, Ph, Pw, 64, snap_of(d, 42, 5), **kw).cpu().numpy(), rec)
    for other in (dict(snap=snap_of(d, 42, 6)), dict(snap=snap_of(d, 43, 5)), dict(snap=snap, site=rng.SITE_PATCH_DRAW - 5)):
        o = ops.patch_draw(pool, Ph, Pw, 64, other.pop("snap"), **kw, **other).cpu().numpy()
        assert (o[:, 8:] != rec[:, 8:]).mean() > 0.99 and (o[:, :6] != rec[:, :6]).mean() > 0.3
    # given images, other classes
    idx = torch.tensor([b % 5 for b in range(64)], dtype=torch.int32, device=d)
    mask = 0b1 if K == 1 else 0b1001                                         # class 0 (and 3)
    r2 = ops.patch_draw(pool, Ph, Pw, 64, snap, fg_slots=64, class_mask=mask, indices=idx).cpu().numpy()
    assert r2[:, P.R_N].tolist() == idx.cpu().tolist() and set(r2[:, P.R_CLS].tolist()) <= ({0, -1} if K == 1 else {0, 3, -1})
    assert np.array_equal(r2, reference_patch_draw(r2[:, 8:], cpu, Ph, Pw, fg_slots=64, class_mask=mask, indices=idx.cpu().tolist()))
    check_records(r2, cases, K, Ph, Pw)
    # no eligible class present: a uniform slot
    r3 = ops.patch_draw(pool, Ph, Pw, 16, snap, fg_slots=16, class_mask=0b10000 if K == 5 else 0).cpu().numpy()
    assert (r3[:, P.R_CLS] == -1).all() and not r3[:, P.R_FG].any()
    assert np.array_equal(r3, reference_patch_draw(r3[:, 8:], cpu, Ph, Pw, fg_slots=16, class_mask=0b10000 if K == 5 else 0))


def test_draw_shares():
    """B = 4096 slots: a count of successes of probability p is within 5 sqrt(B p (1 - p)) of B p (a 5.7e-7
    two-sided tail per check).  Every case of the pool holds a class >= 1, so a slot is foreground iff its uniform
    is below p_fg."""
    from csu import ops
    d = dev()
    K, B, p = 5, 4096, 0.3
    pool, cases = index_pool(K, str(d)), index_cases(K)
    assert all(((lab >= 1) & (lab < K)).any() for _, lab in cases)
    rec = ops.patch_draw(pool, 8, 8, B, snap_of(d, 7, 1), fg_slots=0, p_fg=p).cpu().numpy()

    def within(count, n, q, what):
        assert abs(count - n * q) <= 5 * math.sqrt(n * q * (1 - q)), (what, count, n * q)
    within(int(rec[:, P.R_FG].sum()), B, p, "foreground")
    for n in range(5):
        within(int((rec[:, P.R_N] == n).sum()), B, 1 / 5, f"image {n}")
    fg2 = rec[(rec[:, P.R_N] == 2) & (rec[:, P.R_FG] == 1)]                 # the 70 x 131 case holds classes 1, 2, 3
    for c in (1, 2, 3):
        within(int((fg2[:, P.R_CLS] == c).sum()), len(fg2), 1 / 3, f"class {c}")
    # the pixel: its rank is uniform over the class's count, so the centre's row is above the median row of the
    # class with probability (pixels of the class above it) / count
    lab = cases[3][1]
    sel = rec[(rec[:, P.R_N] == 3) & (rec[:, P.R_CLS] == 1)]
    within(int((sel[:, P.R_CY] < 150).sum()), len(sel), float((lab[:150] == 1).sum()) / float((lab == 1).sum()), "rank")
    forced = ops.patch_draw(pool, 8, 8, 16, snap_of(d, 7, 1), fg_slots=5, p_fg=0.0).cpu().numpy()
    assert forced[:, P.R_FG].tolist() == [1] * 5 + [0] * 11


# ---------------------------------------------------------------------------------------------------------
# warp
# ---------------------------------------------------------------------------------------------------------
def records(rows, d=None):
    rec = np.zeros((len(rows), P.RECORD), dtype=np.int32)
    for b, (n, oy, ox) in enumerate(rows):
        rec[b, P.R_N], rec[b, P.R_OY], rec[b, P.R_OX] = n, oy, ox
    return rec if d is None else torch.from_numpy(rec).to(d)


@pytest.mark.parametrize("m", range(len(MODES)), ids=["-".join(x) for x in MODES])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["x".join(map(str, s)) for s in SHAPES])
def test_warp_is_bitwise_the_batch_kernel(i, m):
    """A pool of B equal-size images, slot b reading image b at origin 0, patch = image: csu_augment_warp's
    arithmetic operation for operation, noise included."""
    from csu import ops
    d = dev()
    B, H, W = SHAPES[i]
    img, lab, table, ctrl, _ = mixed_inputs(i)
    table = table.clone()
    table[:, A.T_SIGMA], table[:, A.T_CONTRAST], table[:, A.T_GAMMA] = 0.03, 1.2, 0.8
    pool = PatchPool(list(img.numpy()), list(lab.numpy()), 5, d)
    border, mask_mode, out = MODES[m]
    kw = dict(spacing=SPACING, snap=snap_of(d, 77, 3), border=border, image_fill=0.25, pad_label=255, mask_mode=mask_mode, out=out)
    want = ops.augment_warp(img.to(d), lab.to(d), table.to(d), ctrl.to(d), **kw)
    got = ops.patch_warp(pool, records([(b, 0, 0) for b in range(B)], d), H, W, table.to(d), ctrl.to(d), **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[1].dtype == want[1].dtype
    quiet = ops.patch_warp(pool, records([(b, 0, 0) for b in range(B)], d), H, W, table.to(d), ctrl.to(d), **dict(kw, snap=None))
    assert B * H * W < 64 or not torch.equal(quiet[0], got[0])              # the noise was on


SOURCE_SIZES = [(90, 150), (100, 160), (10, 12), (3, 2), (40, 200)]
PATCH_SHAPES = [0, 3, 4]                  # of SHAPES: (3, 23, 23), (2, 70, 131), (1, 5, 3)
# per patch shape: slots inside larger images; slots past each edge, at negative origins and over smaller images
ORIGINS = {0: {"inside": [(0, 11, 7), (1, 70, 130), (4, 3, 60)], "edges": [(0, -9, -5), (1, 84, 147), (2, -6, -5)]},
           3: {"inside": [(1, 20, 25), (0, 20, 19)], "edges": [(1, -30, 90), (3, -33, -64)]},
           4: {"inside": [(2, 4, 8)], "edges": [(3, -1, 0)]}}


@functools.lru_cache(maxsize=None)
def source_cases():
    g = np.random.default_rng(21)
    return [(g.integers(0, 256, (H, W, 3), dtype=np.uint8), g.integers(0, 5, (H, W), dtype=np.uint8)) for H, W in SOURCE_SIZES]


@functools.lru_cache(maxsize=None)
def source_pool(device):
    cases = source_cases()
    return PatchPool([c[0] for c in cases], [c[1] for c in cases], 5, device)


@pytest.mark.parametrize("m", range(len(MODES)), ids=["-".join(x) for x in MODES])
@pytest.mark.parametrize("where", ["inside", "edges"])
@pytest.mark.parametrize("i", PATCH_SHAPES, ids=["x".join(map(str, SHAPES[s][1:])) for s in PATCH_SHAPES])
def test_warp_matches_reference(i, where, m):
    from csu import ops
    d = dev()
    B, Ph, Pw = SHAPES[i]
    _, _, table, ctrl, excluded = mixed_inputs(i)
    share = float(excluded.double().mean())
    assert share <= MAX_EXCLUDED, f"{share:.2%} of the pixels are within 1e-3 px of a rounding boundary"
    rows = ORIGINS[i][where]
    border, mask_mode, out = MODES[m]
    kw = dict(spacing=SPACING, border=border, image_fill=0.25, pad_label=255, mask_mode=mask_mode, out=out)
    want = reference_patch_sample(source_pool("cpu"), records(rows), Ph, Pw, table, ctrl, **kw)
    got = ops.patch_warp(source_pool(str(d)), records(rows, d), Ph, Pw, table.to(d), ctrl.to(d), **kw)
    compare(f"patch_warp {(Ph, Pw)} {where} {MODES[m]}", got, want, excluded, mask_mode, TOL_PATCH)


@functools.lru_cache(maxsize=None)
def far_cases():
    """A tall and a wide image, each a block of 100 rows / columns repeated: a patch at origin o and one at
    o + 100 k see the same content, as long as neither reaches the image's ends."""
    g = np.random.default_rng(31)
    tall = (np.tile(g.integers(0, 256, (100, 300, 3), dtype=np.uint8), (2005, 1, 1)),
            np.tile(g.integers(0, 5, (100, 300), dtype=np.uint8), (2005, 1)))
    wide = (np.tile(g.integers(0, 256, (300, 100, 3), dtype=np.uint8), (1, 605, 1)),
            np.tile(g.integers(0, 5, (300, 100), dtype=np.uint8), (1, 605)))
    return [tall, wide]


@pytest.mark.parametrize("m", [0, 2], ids=["-".join(MODES[x]) for x in (0, 2)])
def test_warp_far_from_the_image_origin_is_as_exact_as_near_it(m):
    """(70, 131) patches at (200000, 120) of a 200500 x 300 image and at (120, 59700) of a 300 x 60500 one (H W < 2^31
    bounds a case: the largest origins a few-second test affords; the warped patches reach at most 180 px from their
    centres, so none touches the far ends).  The origin is added as an integer, so the result
    is bit for bit that of the same content near the image's origin, and its deviation from the fp64 reference the
    same."""
    from csu import ops
    d = dev()
    i = 3
    B, Ph, Pw = SHAPES[i]
    _, _, table, ctrl, excluded = mixed_inputs(i)
    cases = far_cases()
    cpu = PatchPool([c[0] for c in cases], [c[1] for c in cases], 5, "cpu")
    pool = PatchPool([c[0] for c in cases], [c[1] for c in cases], 5, d)
    near, far = [(0, 500, 120), (1, 120, 700)], [(0, 200000, 120), (1, 120, 59700)]
    border, mask_mode, out = MODES[m]
    kw = dict(spacing=SPACING, border=border, image_fill=0.25, pad_label=255, mask_mode=mask_mode, out=out)
    got_near = ops.patch_warp(pool, records(near, d), Ph, Pw, table.to(d), ctrl.to(d), **kw)
    got_far = ops.patch_warp(pool, records(far, d), Ph, Pw, table.to(d), ctrl.to(d), **kw)
    want_near = reference_patch_sample(cpu, records(near), Ph, Pw, table, ctrl, **kw)
    want_far = reference_patch_sample(cpu, records(far), Ph, Pw, table, ctrl, **kw)
    # the same content: the references agree up to their own rounding (the fp64 sum o + s loses 2^-35 px at
    # o = 2e5, which can move an fp32 result by one ulp, 2^-24 below 1)
    ULP = 2.0 ** -24
    assert float((want_near[0].double() - want_far[0].double()).abs().max()) <= ULP
    e_near = compare(f"patch_warp near {MODES[m]}", got_near, want_near, excluded, mask_mode, TOL_PATCH)
    e_far = compare(f"patch_warp far {MODES[m]}", got_far, want_far, excluded, mask_mode, TOL_PATCH)
    assert e_far <= e_near + ULP and e_far <= MEASURED_PATCH         # no worse than near the origin
    assert torch.equal(got_far[0], got_near[0]) and torch.equal(got_far[1], got_near[1])


@pytest.mark.parametrize("m", range(len(MODES)), ids=["-".join(x) for x in MODES])
@pytest.mark.parametrize("i", PATCH_SHAPES, ids=["x".join(map(str, SHAPES[s][1:])) for s in PATCH_SHAPES])
def test_integer_tables_at_integer_origins_are_bit_exact(i, m):
    """Flips, quarter turns and whole-pixel shifts at arbitrary integer origins, inside and across every edge: every
    output equals the reference bit for bit; the identity table is the slice / 255."""
    from csu import ops
    d = dev()
    _, Ph, Pw = SHAPES[i]
    B = 8
    g = np.random.default_rng(300 + i)
    rows = [dict(hflip=int(g.integers(2)), vflip=int(g.integers(2)), k=int(g.integers(4)),
                 tx=int(g.integers(-(Pw // 3) - 1, Pw // 3 + 2)), ty=int(g.integers(-(Ph // 3) - 1, Ph // 3 + 2))) for _ in range(B)]
    table = make_table(Ph, Pw, rows)
    slots = []
    for b in range(B):
        n = int(g.integers(len(SOURCE_SIZES)))
        H, W = SOURCE_SIZES[n]
        slots.append((n, int(g.integers(-Ph, H + 1)), int(g.integers(-Pw, W + 1))))
    border, mask_mode, out = MODES[m]
    kw = dict(border=border, image_fill=0.25, pad_label=255, mask_mode=mask_mode, out=out)
    cpu, pool = source_pool("cpu"), source_pool(str(d))
    ri, rm = reference_patch_sample(cpu, records(slots), Ph, Pw, table, **kw)
    oi, om = ops.patch_warp(pool, records(slots, d), Ph, Pw, table.to(d), **kw)
    assert torch.equal(oi.cpu(), ri) and torch.equal(om.cpu(), rm)
    inside = [(n, int(g.integers(0, H - Ph + 1)), int(g.integers(0, W - Pw + 1))) for n, (H, W) in enumerate(SOURCE_SIZES)
              if H >= Ph and W >= Pw]
    ii, il = ops.patch_warp(pool, records(inside, d), Ph, Pw, identity_table(len(inside), d), mask_mode="nearest", out="labels")
    for b, (n, oy, ox) in enumerate(inside):
        img, lab = source_cases()[n]
        assert torch.equal(ii[b].cpu(), (torch.from_numpy(img[oy:oy + Ph, ox:ox + Pw]).float() / 255.0).permute(2, 0, 1))
        assert torch.equal(il[b].cpu(), torch.from_numpy(lab[oy:oy + Ph, ox:ox + Pw].astype(np.int64)))


# ---------------------------------------------------------------------------------------------------------
# graph capture and the loader
# ---------------------------------------------------------------------------------------------------------
def test_graph_replays_draw_fresh_patches_and_reproduce():
    """sample() captured with rng.advance inside: every replay draws new patches, two captures from the same seed
    replay bit for bit, and the foreground slots of every replay are centred on their class."""
    from csu import rng
    from test_augment_warp import full_augment
    d = dev()
    K, B, Ph, Pw = 5, 6, 40, 72
    pool, cases = index_pool(K, str(d)), index_cases(K)
    sampler = PatchSampler(pool, (Ph, Pw), B, foreground=0.5, augment=full_augment(pad_label=255, mask_mode="nearest", out="labels"))
    res = []
    for _ in range(2):
        rng.manual_seed(9, d)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            sampler.sample()                           # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = sampler.sample(snapshot=rng.advance(d))
            rec = sampler.last_record
        seq = []
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            seq.append([t.clone().cpu() for t in (rec,) + tuple(out)])
        res.append((seq, int(rng.state(d)[1].item())))
        del graph
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert not torch.equal(res[0][0][a][0], res[0][0][b][0]) and not torch.equal(res[0][0][a][1], res[0][0][b][1])
    assert res[0][1] == res[1][1] == 4                  # the warm-up and three replays
    for x, y in zip(res[0][0], res[1][0]):
        assert all(torch.equal(p, q) for p, q in zip(x, y))
    for r, img, lab in res[0][0]:
        check_records(r.numpy(), cases, K, Ph, Pw)
        assert r[:3, P.R_FG].tolist() == [1, 1, 1] and not r[3:, P.R_FG].any()
        assert tuple(img.shape) == (B, 3, Ph, Pw) and tuple(lab.shape) == (B, Ph, Pw) and lab.dtype == torch.int64
        assert not bool(torch.isnan(img).any()) and set(lab.unique().tolist()) <= {0, 1, 2, 3, 255}


def test_unaugmented_foreground_patch_holds_its_centre():
    """No augmentation: the patch is the slice at the drawn origin, so label[cy - oy, cx - ox] is the slot's class."""
    d = dev()
    K = 5
    pool, cases = index_pool(K, str(d)), index_cases(K)
    sampler = PatchSampler(pool, (16, 24), 32, foreground=1.0)
    idx = torch.tensor([2 + b % 3 for b in range(32)], dtype=torch.int32, device=d)      # the cases at least the patch's size
    img, lab = sampler.sample(snapshot=snap_of(d, 3, 3), indices=idx)
    rec = sampler.last_record.cpu().numpy()
    check_records(rec, cases, K, 16, 24)
    for b, row in enumerate(rec):
        n, cls, cy, cx, oy, ox = row[:6].tolist()
        assert int(lab[b, cy - oy, cx - ox]) == cls
        assert torch.equal(lab[b].cpu(), torch.from_numpy(cases[n][1][oy:oy + 16, ox:ox + 24].astype(np.int64)))
        assert torch.equal(img[b].cpu(), (torch.from_numpy(cases[n][0][oy:oy + 16, ox:ox + 24]).float() / 255.0).permute(2, 0, 1))


def test_loader_batches_go_through_the_loss():
    from csu import rng
    from csu.losses import ce_dice_loss
    d = dev()
    rng.manual_seed(3, d)
    K = 5
    pool = index_pool(K, str(d))
    aug = SpatialAugment(rotate=(-30, 30), p_rotate=1.0, scale=(0.7, 1.4), flip_prob=0.5, elastic=(8, 1.0, 3.0),
                         contrast=(0.75, 1.25), gamma=(0.7, 1.5), noise=(0.0, 0.05), pad_label=255, mask_mode="nearest", out="labels")
    loader = PatchLoader(PatchSampler(pool, 32, 4, foreground=0.5, augment=aug), steps_per_epoch=3)
    crit = ce_dice_loss(K, ignore_index=255)
    steps, seen = 0, set()
    for x, y in loader:
        steps += 1
        assert x.is_cuda and tuple(x.shape) == (4, 3, 32, 32) and x.dtype == torch.float32
        assert float(x.min()) >= 0 and float(x.max()) <= 1
        assert tuple(y.shape) == (4, 32, 32) and y.dtype == torch.int64
        seen |= set(y.unique().tolist())
        z = torch.randn(4, K, 32, 32, device=d, requires_grad=True)
        loss = crit(z, y)
        loss.backward()
        assert math.isfinite(float(loss)) and bool(torch.isfinite(z.grad).all()) and float(z.grad.abs().max()) > 0
    assert steps == len(loader) == 3 and seen <= {0, 1, 2, 3, 255} and 255 in seen and len(seen) >= 3
    # a binary pool yields masks as SpatialAugment does
    bpool = index_pool(1, str(d))
    xb, mb = PatchSampler(bpool, 16, 4).sample()
    assert tuple(mb.shape) == (4, 1, 16, 16) and mb.dtype == torch.float32 and set(mb.unique().tolist()) <= {0.0, 1.0}
