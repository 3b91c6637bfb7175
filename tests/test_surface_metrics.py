"""Surface-distance metrics on the CPU: csu.metrics.reference_surface_metrics (the definitions in plain
torch ops, fp64) on hand cases and against medpy's formulas written with scipy.ndimage, the empty-mask
rules, the SurfaceMetrics accumulator and evaluate_full_res's optional third result."""
import math

import numpy as np
import pytest
import torch

import csu
from csu import metrics

NAN = float("nan")


def rnd_mask(rng, shape, p=0.08, grow=2):
    """Blobs: random seeds grown by `grow` 4-neighbour dilations (numpy only)."""
    m = rng.random(shape) < p
    for _ in range(grow):
        q = np.pad(m, 1)
        m = q[1:-1, 1:-1] | q[:-2, 1:-1] | q[2:, 1:-1] | q[1:-1, :-2] | q[1:-1, 2:]
    return m


def test_corner_pixels():
    p = torch.zeros(40, 70, dtype=torch.uint8)
    t = torch.zeros(40, 70, dtype=torch.int64)
    p[0, 0] = 1
    t[39, 69] = 3
    r = metrics.reference_surface_metrics(p, t)
    d = math.sqrt(39 ** 2 + 69 ** 2)
    assert r.shape == (1, 1, 6) and r.dtype == torch.float64
    assert r[0, 0].tolist() == [d, d, d, 0.0, 1.0, 1.0]
    assert csu.surface_metrics(p, t).equal(r)        # CPU tensors take the reference path


def test_identical_masks():
    m = torch.from_numpy(rnd_mask(np.random.default_rng(0), (23, 31)))
    r = metrics.reference_surface_metrics(m, m.clone(), spacing=(0.7, 1.3))
    assert r[0, 0, :4].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert r[0, 0, 4] == r[0, 0, 5] > 0


@pytest.mark.parametrize("H,W", [(5, 7), (2, 9), (1, 6), (12, 1)])
def test_full_mask_border_count(H, W):
    m = torch.ones(H, W, dtype=torch.uint8)
    r = metrics.reference_surface_metrics(m, m)
    want = 2 * (H + W) - 4 if min(H, W) > 1 else H * W
    assert r[0, 0, 4] == want and r[0, 0, 5] == want
    if (H, W) == (5, 7):
        assert want == 20


def test_one_row_image():
    p = torch.zeros(1, 64, dtype=torch.uint8)
    t = torch.zeros(1, 64, dtype=torch.uint8)
    p[0, 3:10] = 1        # every pixel of a one-row mask is a border pixel (rows beyond the image are outside)
    t[0, 5:20] = 1
    r = metrics.reference_surface_metrics(p, t, spacing=(1.0, 2.0), tolerance=3.0)[0, 0]
    d1 = [2 * max(5 - x, 0) for x in range(3, 10)]
    d2 = [2 * max(x - 9, 0) for x in range(5, 20)]
    assert r[4] == 7 and r[5] == 15
    assert r[0] == 20.0
    assert r[1] == pytest.approx(np.percentile(d1 + d2, 95), rel=1e-12)
    assert r[2] == pytest.approx((np.mean(d1) + np.mean(d2)) / 2, rel=1e-12)
    assert r[3] == pytest.approx(sum(v <= 3.0 for v in d1 + d2) / 22, rel=1e-12)


def test_multiclass_classes_and_batch():
    rng = np.random.default_rng(1)
    p = torch.from_numpy(rng.integers(0, 4, (2, 17, 19)))
    t = torch.from_numpy(rng.integers(0, 4, (2, 17, 19)).astype(np.uint8))
    r = metrics.reference_surface_metrics(p, t, num_classes=4)
    assert r.shape == (2, 3, 6)
    rb = metrics.reference_surface_metrics(p, t, num_classes=4, include_background=True)
    assert rb.shape == (2, 4, 6) and rb[:, 1:].equal(r)
    one = metrics.reference_surface_metrics(p[1] == 2, t[1] == 2)
    assert one[0, 0].equal(r[1, 1])


def test_empty_masks_give_nan_and_keep_counts():
    z = torch.zeros(9, 11, dtype=torch.uint8)
    m = z.clone()
    m[2:6, 3:8] = 1
    n = 2 * (4 + 5) - 4
    for p, t, cp, ct in ((z, m, 0, n), (m, z, n, 0), (z, z, 0, 0)):
        r = metrics.reference_surface_metrics(p, t)[0, 0]
        assert torch.isnan(r[:4]).all()
        assert r[4] == cp and r[5] == ct


def test_accumulator_leaves_empty_pairs_out():
    acc = csu.SurfaceMetrics(num_classes=3, tolerance=1.0)
    p = torch.zeros(2, 12, 12, dtype=torch.int64)
    t = torch.zeros(2, 12, 12, dtype=torch.int64)
    p[0, 2:6, 2:6] = 1
    t[0, 3:7, 2:6] = 1          # image 0: class 1 on both sides, class 2 nowhere
    p[1, 1:4, 1:4] = 2
    t[1, 1:4, 1:5] = 2          # image 1: class 2 on both sides; class 1 only predicted
    p[1, 8:10, 8:10] = 1
    rows = acc.update(p, t)
    assert rows.shape == (2, 2, 6)
    acc.update(p[0], t[0])       # a single (H, W) pair
    res = acc.compute()
    assert res["valid"] == 3
    r = metrics.reference_surface_metrics(p, t, num_classes=3)
    for k, j in (("hd", 0), ("hd95", 1), ("assd", 2), ("nsd", 3)):
        c1, c2 = float(r[0, 0, j]), float(r[1, 1, j])
        assert res["class_" + k] == pytest.approx([c1, c2], rel=1e-12)
        assert res[k] == pytest.approx((c1 + c2) / 2, rel=1e-12)
    empty = csu.SurfaceMetrics(num_classes=3)
    empty.update(torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8))
    res = empty.compute()
    assert res["valid"] == 0 and math.isnan(res["hd95"]) and all(math.isnan(v) for v in res["class_nsd"])


def test_argument_checks():
    m = torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="at most 32 classes"):
        csu.surface_metrics(m, m, num_classes=33, include_background=True)
    assert csu.surface_metrics(m, m, num_classes=33).shape == (1, 32, 6)
    with pytest.raises(ValueError, match="spacing"):
        csu.surface_metrics(m, m, spacing=(0.0, 1.0))
    with pytest.raises(ValueError, match="percentile"):
        csu.surface_metrics(m, m, percentile=101.0)
    with pytest.raises(ValueError, match="shape"):
        csu.surface_metrics(m, torch.zeros(4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="integer or bool"):
        csu.surface_metrics(m.float(), m)


# ---- against scipy.ndimage (medpy's formulas) ---------------------------------------------------
def medpy_formulas(ndi, P, T, spacing, tau, q):
    st = ndi.generate_binary_structure(2, 1)
    bp, bt = P ^ ndi.binary_erosion(P, st), T ^ ndi.binary_erosion(T, st)
    d1 = ndi.distance_transform_edt(~bt, sampling=spacing)[bp]
    d2 = ndi.distance_transform_edt(~bp, sampling=spacing)[bt]
    pool = np.concatenate([d1, d2])
    return [max(d1.max(), d2.max()), np.percentile(pool, q), (d1.mean() + d2.mean()) / 2,
            ((d1 <= tau).sum() + (d2 <= tau).sum()) / pool.size, bp.sum(), bt.sum()]


@pytest.mark.parametrize("shape", [(37, 53), (9, 1100)])
@pytest.mark.parametrize("spacing", [(1.0, 1.0), (0.7, 1.3)])
def test_reference_matches_scipy(shape, spacing):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(shape[0] * 7 + int(spacing[0] * 10))
    P, T = rnd_mask(rng, shape), rnd_mask(rng, shape)
    want = np.asarray(medpy_formulas(ndi, P, T, spacing, 2.0, 95.0), dtype=np.float64)
    got = metrics.reference_surface_metrics(torch.from_numpy(P), torch.from_numpy(T), 1, spacing, 2.0, 95.0)[0, 0].numpy()
    assert got[4] == want[4] > 0 and got[5] == want[5] > 0
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("shape", [(37, 53), (9, 1100)])
@pytest.mark.parametrize("spacing", [(1.0, 1.0), (0.7, 1.3)])
def test_edt_matches_scipy(shape, spacing):
    """The CPU path computes in fp64 (compared at 1e-12) and returns it rounded to fp32, which is then
    scipy's result rounded to fp32."""
    ndi = pytest.importorskip("scipy.ndimage")
    m = rnd_mask(np.random.default_rng(5 + shape[0]), shape, p=0.15)
    want = ndi.distance_transform_edt(m, sampling=spacing)
    got64 = metrics.reference_distance_transform_edt(torch.from_numpy(m), spacing)
    np.testing.assert_allclose(got64.numpy(), want, rtol=1e-12, atol=0)
    got = csu.distance_transform_edt(torch.from_numpy(m), spacing)
    assert got.dtype == torch.float32 and got.shape == m.shape
    np.testing.assert_allclose(got.numpy(), want.astype(np.float32), rtol=1e-12, atol=0)
    b = csu.distance_transform_edt(torch.from_numpy(np.stack([m, ~m])).to(torch.int64), spacing)
    assert b.shape == (2,) + m.shape and b[0].equal(got)


def test_edt_without_a_zero_pixel_is_inf():
    e = csu.distance_transform_edt(torch.ones(3, 5, dtype=torch.uint8))
    assert e.dtype == torch.float32 and torch.isinf(e).all()
    assert csu.distance_transform_edt(torch.zeros(3, 5)).eq(0).all()


# ---- evaluate_full_res ---------------------------------------------------------------------------
class StubPredictor:
    """predict(image) = the image's first channel as a label map."""

    def predict(self, image):
        return torch.as_tensor(image)[..., 0].to(torch.uint8)


@pytest.mark.parametrize("K", [1, 3])
def test_evaluate_full_res_surface_argument(K):
    rng = np.random.default_rng(3)
    pairs = []
    for _ in range(2):
        lab = rng.integers(0, max(K, 2), (20, 24)).astype(np.uint8)
        tgt = rng.integers(0, max(K, 2), (20, 24)).astype(np.int64)
        pairs.append((np.repeat(lab[..., None], 3, 2), tgt))
    two = csu.evaluate_full_res(StubPredictor(), pairs, num_classes=K)
    assert isinstance(two, tuple) and len(two) == 2
    acc = csu.SurfaceMetrics(num_classes=K, tolerance=1.0)
    three = csu.evaluate_full_res(StubPredictor(), pairs, num_classes=K, surface=acc)
    assert len(three) == 3 and three[:2] == two
    rows = torch.cat([metrics.reference_surface_metrics(torch.from_numpy(i[..., 0]), torch.from_numpy(t), K) for i, t in pairs])
    assert three[2]["valid"] == int((~torch.isnan(rows[:, :, 0])).sum())
    assert three[2]["hd95"] == pytest.approx(float(rows[:, :, 1].mean(0).mean()), rel=1e-12)
