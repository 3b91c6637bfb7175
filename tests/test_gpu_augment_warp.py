"""csu.augment on the MI355X: csu_augment_warp against reference_augment (fp64, on the CPU) with explicit
tables, the device draw (ranges, shares, moments, purity of a row, the folded matrix), the Philox noise, graph
capture and the loader over a raw label-map dataset.

Tolerances.  Labels are exact wherever the fp64 source coordinate is further than EDGE = 1e-3 px from a rounding
boundary in both axes (the kernel's fp32 coordinates are within ~1e-4 px at these sizes); the excluded share is
capped at 2 % per case and counted on the CPU before anything is compared.  Images and bilinear masks: 4 x the
largest deviation measured on the MI355X over these same cases (fp32 coordinate rounding times an image gradient
of at most 1 per pixel: the images are uniform noise, the steepest there is); the measured values stand next to
the constants, and a deviation above 1e-3 is a bug whatever the constants say."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from csu import augment as A
from csu.augment import SpatialAugment, identity_table, make_table, reference_augment
from test_augment_warp import compose_np, full_augment

EDGE = 1e-3
MAX_EXCLUDED = 0.02
BUG = 1e-3
MEASURED_WARP = 8.598e-6    # largest |image - fp64 reference| over the cases below on the MI355X, at (2, 70, 131); the
TOL_WARP = 4 * MEASURED_WARP    # bilinear masks (0 .. 4 / 255) reach 1.406e-7 (profiles/augment_warp_timing.txt)
MEASURED_GAMMA = 1.192e-7   # largest deviation of the gamma rows of test_intensity_with_an_identity_warp, measured
TOL_GAMMA = 4 * MEASURED_GAMMA

# The fourth shape crosses the warp kernel's 64 x 4 output tile in both directions with a ragged last tile in
# each (131 = 2 * 64 + 3, 70 = 17 * 4 + 2); in the last the image is smaller than the control-grid spacing.
SHAPES = [(3, 23, 23), (2, 19, 37), (1, 1, 1), (2, 70, 131), (1, 5, 3)]
MODES = [("constant", "bilinear", "binary"), ("replicate", "nearest", "binary"), ("constant", "nearest", "labels")]
SPACING = 8


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def snap_of(d, seed, ctr):
    return torch.tensor([seed, ctr], dtype=torch.int64, device=d)


def pair(B, H, W, seed, classes=5):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    lab = torch.randint(0, classes, (B, H, W), dtype=torch.uint8, generator=g)
    return img, lab


@functools.lru_cache(maxsize=None)
def mixed_inputs(i):
    """Images, labels, a table mixing rotation, scale 0.6-1.6, shifts that push part of the image out, flips and
    turns, and an elastic field of spacing 8 and magnitude 1-4 px on every other row (seeded by the shape)."""
    B, H, W = SHAPES[i]
    g = np.random.default_rng(100 + i)
    rows = []
    for b in range(B):
        rows.append(dict(hflip=int(g.integers(2)), vflip=int(g.integers(2)), k=int(g.integers(4)),
                         angle=float(g.uniform(-math.pi, math.pi) if b % 2 == 0 else g.uniform(-0.5, 0.5)),
                         scale=float(np.exp(g.uniform(math.log(0.6), math.log(1.6)))),
                         tx=float(g.uniform(-0.4, 0.4) * W), ty=float(g.uniform(-0.4, 0.4) * H),
                         elastic=float(g.uniform(1.0, 4.0)) if (b + i) % 2 == 0 else 0.0))
    table = make_table(H, W, rows)
    mag = table[:, A.T_ELASTIC]
    ctrl = torch.from_numpy(g.uniform(-1.0, 1.0, (B, 2) + A.control_grid(H, W, SPACING))).float()
    ctrl = ctrl * torch.where(mag > 0, mag, torch.full_like(mag, 3.0))[:, None, None, None]   # magnitude 0: never read
    img, lab = pair(B, H, W, 200 + i)
    sx, sy = A.reference_source_coords(table, ctrl, SPACING, H, W)
    near = lambda s: ((s + 0.5) - torch.round(s + 0.5)).abs() < EDGE
    return img, lab, table, ctrl, near(sx) | near(sy)


@functools.lru_cache(maxsize=None)
def mixed_reference(i, m):
    img, lab, table, ctrl, _ = mixed_inputs(i)
    border, mask_mode, out = MODES[m]
    return reference_augment(img, lab, table, ctrl, spacing=SPACING, border=border, image_fill=0.25, pad_label=255,
                             mask_mode=mask_mode, out=out)


def compare(tag, got, want, excluded, mask_mode, tol):
    """Image (and a bilinear mask) within tol, a nearest mask exact off the rounding boundaries; the figures are
    printed first."""
    oi, om = (t.cpu() for t in got)
    ri, rm = want
    assert oi.shape == ri.shape and oi.dtype == torch.float32 and om.shape == rm.shape and om.dtype == rm.dtype
    assert not bool(torch.isnan(oi).any())
    ei = float((oi.double() - ri.double()).abs().max())
    line = f"augment_warp {tag}: max|d image| {ei:.3e}"
    if mask_mode == "bilinear":
        em = float((om.double() - rm.double()).abs().max())
        print(f"{line}, max|d mask| {em:.3e}")
        assert em < BUG and em <= tol, (tag, em)
    else:
        ex = excluded if om.dim() == 3 else excluded[:, None]
        bad = (om != rm) & ~ex
        print(f"{line}, labels differing off the boundaries {int(bad.sum())}, on them {int(((om != rm) & ex).sum())}"
              f" of {int(ex.sum())} excluded ({float(ex.double().mean()):.2%})")
        assert not bool(bad.any()), (tag, int(bad.sum()))
    assert ei < BUG and ei <= tol, (tag, ei)
    return ei


@pytest.mark.parametrize("m", range(len(MODES)), ids=["-".join(x) for x in MODES])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["x".join(map(str, s)) for s in SHAPES])
def test_warp_matches_reference(i, m):
    from csu import ops
    d = dev()
    img, lab, table, ctrl, excluded = mixed_inputs(i)
    share = float(excluded.double().mean())
    assert share <= MAX_EXCLUDED, f"{share:.2%} of the pixels are within {EDGE} px of a rounding boundary"
    border, mask_mode, out = MODES[m]
    got = ops.augment_warp(img.to(d), lab.to(d), table.to(d), ctrl.to(d), spacing=SPACING, border=border, image_fill=0.25,
                           pad_label=255, mask_mode=mask_mode, out=out)
    compare(f"{SHAPES[i]} {MODES[m]}", got, mixed_reference(i, m), excluded, mask_mode, TOL_WARP)


@pytest.mark.parametrize("m", range(len(MODES)), ids=["-".join(x) for x in MODES])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["x".join(map(str, s)) for s in SHAPES])
def test_integer_tables_are_bit_exact(i, m):
    """Flips, quarter turns and whole-pixel shifts (no elastic): every output equals the reference bit for bit."""
    from csu import ops
    d = dev()
    B, H, W = SHAPES[i]
    g = np.random.default_rng(300 + i)
    rows = [dict(hflip=int(g.integers(2)), vflip=int(g.integers(2)), k=int(g.integers(4)),
                 tx=int(g.integers(-(W // 3) - 1, W // 3 + 2)), ty=int(g.integers(-(H // 3) - 1, H // 3 + 2)))
            for _ in range(B)]
    table = make_table(H, W, rows)
    img, lab = pair(B, H, W, 400 + i)
    border, mask_mode, out = MODES[m]
    kw = dict(border=border, image_fill=0.25, pad_label=255, mask_mode=mask_mode, out=out)
    ri, rm = reference_augment(img, lab, table, **kw)
    oi, om = ops.augment_warp(img.to(d), lab.to(d), table.to(d), **kw)
    assert torch.equal(oi.cpu(), ri) and torch.equal(om.cpu(), rm)
    ident = ops.augment_warp(img.to(d), lab.to(d), identity_table(B, d), **kw)[0]
    assert torch.equal(ident.cpu(), (img.float() / 255.0).permute(0, 3, 1, 2))


def test_intensity_with_an_identity_warp():
    """Contrast and brightness within the warp tolerance, gamma (v_log_f32 / v_exp_f32) within its own."""
    from csu import ops
    d = dev()
    B, H, W = 4, 19, 37
    img, lab = pair(B, H, W, 500)
    mean = ops.augment_mean(img.to(d))
    assert torch.equal(mean.cpu(), (img.long().sum(dim=(1, 2, 3)).double() / (255.0 * H * W * 3)).float())   # exact sum
    lin = make_table(H, W, [dict(contrast=0.75, brightness=1.2), dict(contrast=1.25, brightness=0.8), dict(contrast=1.6),
                            dict(brightness=0.55)])
    gam = make_table(H, W, [dict(gamma=0.7), dict(gamma=1.5), dict(gamma=2.0, contrast=1.25, brightness=0.9),
                            dict(gamma=0.5, brightness=1.3)])
    for tag, table, tol in (("contrast / brightness", lin, TOL_WARP), ("gamma", gam, TOL_GAMMA)):
        want = reference_augment(img, lab, table, mask_mode="nearest", out="labels")
        got = ops.augment_warp(img.to(d), lab.to(d), table.to(d), mean=mean, mask_mode="nearest", out="labels")
        assert torch.equal(got[1].cpu(), lab.long())          # intensity steps never touch the mask
        compare(tag, got, want, torch.zeros(B, H, W, dtype=torch.bool), "nearest", tol)


# ---------------------------------------------------------------------------------------------------------
# draw
# ---------------------------------------------------------------------------------------------------------
def test_draw_ranges_shares_moments_and_purity():
    from csu import ops, rng
    d = dev()
    B, H, W = 4096, 64, 64
    aug = full_augment()
    cfg = aug.config(H, W)
    snap = snap_of(d, 1234, 7)
    table, ctrl = ops.augment_draw(cfg, B, H, W, snap, elastic=True)
    torch.cuda.synchronize()
    t, c = table.cpu().double(), ctrl.cpu().double()
    assert t.shape == (B, A.TABLE_P) and c.shape == (B, 2) + A.control_grid(H, W, 8) and not bool(torch.isnan(t).any())

    def share(col, identity, p, name):
        on = t[:, col] != identity
        sd = math.sqrt(p * (1 - p) / B)
        assert abs(float(on.double().mean()) - p) <= 5 * sd, (name, float(on.double().mean()), p)
        return on
    for col in (A.T_HFLIP, A.T_VFLIP):
        assert set(t[:, col].tolist()) == {0.0, 1.0}
        share(col, 0, 0.5, "flip")
    on = share(A.T_ROT90, 0, 0.4, "rot90")
    assert set(t[:, A.T_ROT90].tolist()) == {0.0, 1.0, 2.0, 3.0}
    for k in (1, 2, 3):      # each turn a third of the applied rows
        n = int(on.sum())
        assert abs(int((t[:, A.T_ROT90] == k).sum()) - n / 3) <= 5 * math.sqrt(n * 2 / 9)
    lo, hi = math.radians(-30), math.radians(30)
    on = share(A.T_ANGLE, 0, 0.7, "rotate")
    ang, n = t[on, A.T_ANGLE], int(on.sum())
    assert float(ang.min()) >= lo - 1e-7 and float(ang.max()) <= hi + 1e-7
    assert abs(float(ang.mean())) <= 5 * (hi - lo) / math.sqrt(12 * n)
    assert abs(float(ang.var()) - (hi - lo) ** 2 / 12) <= 5 * (hi - lo) ** 2 / math.sqrt(180 * n)
    on = share(A.T_SCALE, 1, 0.6, "scale")
    ls = torch.log(t[on, A.T_SCALE])
    assert float(ls.min()) >= math.log(0.6) - 1e-6 and float(ls.max()) <= math.log(1.6) + 1e-6
    assert abs(float(ls.mean()) - (math.log(0.6) + math.log(1.6)) / 2) <= 5 * math.log(1.6 / 0.6) / math.sqrt(12 * int(on.sum()))
    on = share(A.T_TX, 0, 0.8, "translate")
    assert bool(((t[:, A.T_TY] != 0) == on).all())
    assert float(t[:, A.T_TX].abs().max()) <= 0.2 * W and float(t[:, A.T_TY].abs().max()) <= 0.2 * H
    for col, ident, (a, b), name in ((A.T_CONTRAST, 1, (0.75, 1.25), "contrast"), (A.T_BRIGHTNESS, 1, (0.8, 1.2), "brightness"),
                                     (A.T_GAMMA, 1, (0.7, 1.5), "gamma"), (A.T_SIGMA, 0, (0.0, 0.05), "noise"),
                                     (A.T_ELASTIC, 0, (1.0, 4.0), "elastic")):
        on = share(col, ident, 0.5, name)
        v = t[on, col]
        assert float(v.min()) >= a - 1e-6 and float(v.max()) <= b + 1e-6, name
        assert abs(float(v.mean()) - (a + b) / 2) <= 5 * (b - a) / math.sqrt(12 * int(on.sum())), name
    assert bool((t[:, A.T_A + 6:] == 0).all())
    # the folded matrix: the fp64 composition of the row's own raw draws
    want = A.compose_affine(table.cpu(), H, W)
    got = t[:, A.T_A:A.T_A + 6]
    assert bool(((got - want).abs() <= 1e-5 * want.abs() + 1e-9).all()), float((got - want).abs().max())
    for b in range(32):
        w = compose_np(t[b].numpy(), H, W)
        assert np.all(np.abs(got[b].numpy() - w) <= 1e-5 * np.abs(w) + 1e-6), (b, got[b], w)
    # the control field: bounded by the row's magnitude, zero where elastic was not applied, and spread
    mag = t[:, A.T_ELASTIC]
    assert bool((c.abs().amax(dim=(1, 2, 3)) <= mag).all()) and bool((c[mag == 0] == 0).all())
    z = (c[mag > 0] / mag[mag > 0][:, None, None, None]).flatten()
    assert abs(float(z.mean())) <= 5 / math.sqrt(3 * z.numel()) and abs(float(z.var()) - 1 / 3) <= 5 * math.sqrt(4 / 45 / z.numel())
    # row b is a pure function of (seed, counter, site, b)
    t4, c4 = ops.augment_draw(cfg, 4, H, W, snap, elastic=True)
    assert torch.equal(t4, table[:4]) and torch.equal(c4, ctrl[:4])
    again = ops.augment_draw(cfg, B, H, W, snap_of(d, 1234, 7), elastic=True)
    assert torch.equal(again[0], table) and torch.equal(again[1], ctrl)
    for other in (dict(snap=snap_of(d, 1234, 8)), dict(snap=snap_of(d, 1235, 7)),
                  dict(snap=snap, site=rng.SITE_AUGMENT_DRAW - 1, site_ctrl=rng.SITE_AUGMENT_CTRL + 8)):
        to, co = ops.augment_draw(cfg, B, H, W, other.pop("snap"), elastic=True, **other)
        assert float((to[:, :12] != table[:, :12]).float().mean()) > 0.3 and float((co != ctrl).float().mean()) > 0.2
    # a transform that is off keeps its identity value in every row
    ti, ci = SpatialAugment().draw(64, H, W, d, snapshot=snap)
    assert ci is None and torch.equal(ti, identity_table(64, d))


# ---------------------------------------------------------------------------------------------------------
# noise
# ---------------------------------------------------------------------------------------------------------
def test_noise_is_standard_normal_and_reproducible():
    from csu import ops
    d = dev()
    B, H, W, sigma = 3, 64, 64, 0.05
    img = torch.full((B, H, W, 3), 128, dtype=torch.uint8, device=d)       # mid-grey: 10 sigma from either clamp
    lab = torch.zeros(B, H, W, dtype=torch.uint8, device=d)
    quiet, noisy = identity_table(B, d), identity_table(B, d)
    noisy[:, A.T_SIGMA] = sigma
    snap = snap_of(d, 77, 3)
    o0 = ops.augment_warp(img, lab, quiet, snap=snap)[0]
    o1 = ops.augment_warp(img, lab, noisy, snap=snap)[0]
    assert torch.equal(o0, torch.full_like(o0, 128 / 255))
    assert torch.equal(ops.augment_warp(img, lab, noisy)[0], o0)              # no snapshot: no noise
    z = ((o1.double() - o0.double()) / sigma).cpu()
    n = z.numel()
    assert abs(float(z.mean())) <= 5 / math.sqrt(n) and abs(float(z.var()) - 1) <= 5 * math.sqrt(2 / n)
    assert abs(float((z ** 4).mean()) - 3) <= 5 * math.sqrt(96 / n)
    corr = lambda a, b: float((a * b).mean())
    assert abs(corr(z[..., :-1], z[..., 1:])) <= 5 / math.sqrt(n)             # lag 1
    assert abs(corr(z[..., :-1, :], z[..., 1:, :])) <= 5 / math.sqrt(n)       # lag W
    for a, b in ((0, 1), (0, 2), (1, 2)):                                      # channels share a Philox call
        assert abs(corr(z[:, a], z[:, b])) <= 5 / math.sqrt(n / 3)
    assert abs(corr(z[:-1], z[1:])) <= 5 / math.sqrt(n)                       # images
    assert torch.equal(ops.augment_warp(img, lab, noisy, snap=snap_of(d, 77, 3))[0], o1)
    assert torch.equal(ops.augment_warp(img[:1], lab[:1], noisy[:1], snap=snap)[0], o1[:1])
    assert not torch.equal(ops.augment_warp(img, lab, noisy, snap=snap_of(d, 77, 4))[0], o1)


# ---------------------------------------------------------------------------------------------------------
# graph capture and the loader
# ---------------------------------------------------------------------------------------------------------
def test_graph_replays_draw_fresh_parameters_and_reproduce():
    """Draw + warp captured with rng.advance inside: every replay draws new parameters (the device counter moves
    inside the graph), and two captures from the same seed replay bit for bit."""
    from csu import rng
    d = dev()
    B, H, W = 2, 40, 72
    img, lab = (t.to(d) for t in pair(B, H, W, 600, classes=3))
    aug = full_augment(pad_label=255, mask_mode="nearest", out="labels")
    res = []
    for _ in range(2):
        rng.manual_seed(9, d)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            aug(img, lab)                              # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            snap = rng.advance(d)
            table, ctrl = aug.draw(B, H, W, d, snapshot=snap)
            out = aug.apply(img, lab, table, ctrl, snapshot=snap)
        seq = []
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            seq.append([t.clone().cpu() for t in (table, ctrl) + tuple(out)])
        res.append((seq, int(rng.state(d)[1].item())))
        del graph
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert not torch.equal(res[0][0][a][0], res[0][0][b][0]) and not torch.equal(res[0][0][a][2], res[0][0][b][2])
    assert res[0][1] == res[1][1] == 4                  # the warm-up and three replays
    for x, y in zip(res[0][0], res[1][0]):
        assert all(torch.equal(p, q) for p, q in zip(x, y))


def test_loader_yields_label_maps_the_loss_takes(tmp_path):
    from PIL import Image
    from csu.data import DeviceAugmentLoader, SegmentationDataset
    from csu import rng
    from csu.losses import ce_dice_loss
    d = dev()
    rng.manual_seed(3, d)
    (tmp_path / "img").mkdir()
    (tmp_path / "mask").mkdir()
    g = np.random.default_rng(0)
    for i in range(5):
        Image.fromarray(g.integers(0, 256, (40, 36, 3), dtype=np.uint8)).save(tmp_path / "img" / f"{i}.png")
        lab = np.zeros((40, 36), dtype=np.uint8)
        lab[8:30, 5:20], lab[15:38, 18:33] = 1, 2
        Image.fromarray(lab).save(tmp_path / "mask" / f"{i}.png")
    ds = SegmentationDataset(str(tmp_path / "img"), str(tmp_path / "mask"), image_size=(32, 32), label_mode=True, raw=True)
    aug = SpatialAugment(rotate=(-30, 30), p_rotate=1.0, scale=(0.7, 1.4), translate=0.1, flip_prob=0.5,
                         elastic=(8, 1.0, 3.0), contrast=(0.75, 1.25), gamma=(0.7, 1.5), noise=(0.0, 0.05), pad_label=255)
    loader = DeviceAugmentLoader(torch.utils.data.DataLoader(ds, batch_size=2), d, augment=aug)
    crit = ce_dice_loss(3, ignore_index=255)
    sizes, seen = [], set()
    for x, y in loader:
        B = x.shape[0]
        sizes.append(B)
        assert x.is_cuda and tuple(x.shape) == (B, 3, 32, 32) and x.dtype == torch.float32
        assert float(x.min()) >= 0 and float(x.max()) <= 1
        assert tuple(y.shape) == (B, 32, 32) and y.dtype == torch.int64
        seen |= set(y.unique().tolist())
        loss, stats = crit.loss_stats(torch.randn(B, 3, 32, 32, device=d), y)
        assert math.isfinite(float(loss)) and tuple(stats.shape) == (3, 3)
    assert sizes == [2, 2, 1] and len(loader) == 3
    assert seen <= {0, 1, 2, 255} and {1, 2} <= seen and 255 in seen
