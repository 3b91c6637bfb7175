"""Surface-distance metrics and the distance transform on the MI355X (csrc/surface.hip) against
csu.metrics.reference_surface_metrics' fp64 brute force on the CPU.

Unit and dyadic spacing ((1, 1), (2, 2), (1.5, 0.75)): every squared distance is exact in the kernels'
arithmetic (int32 index distances; fp32 sums of multiples of 1/16 below 2^24 / 16 at these sizes), so the
border counts, hd and hd95 agree (1e-12 relative admits nothing but the fp64 interpolation) and assd / nsd
agree to 1e-12 relative (fp64 sums in another order).  Tolerances 1.5, 3.0 and 2.0: no squared distance
ties with tau^2 (a + b = 2.25 has no integer solution; 36 a + 9 b = 64 none either).

Spacing (0.7, 1.3) (fp32 path): hd, hd95 and assd within 4e-7 relative.  sy^2 and sx^2 are rounded to
fp32, then two products and a sum: at most about 3 * 2^-24 relative in d^2, so 1.5 * 2^-24 in d, plus one
fp32 -> fp64 square root: about 1.5e-7, taken with a factor of a little over two.  nsd with tolerance 2.0 is
equal: 0.49 a + 1.69 b = 4 has no solution in squares; the test asserts on the reference that no border
distance lies within 1e-5 relative of the tolerance."""
import numpy as np
import pytest
import torch

import csu
from csu import metrics

pytestmark = pytest.mark.gpu

EXACT_RTOL = 1e-12
F32_RTOL = 4e-7
# spacing -> tolerance
SPACINGS = {(1.0, 1.0): 1.5, (2.0, 2.0): 3.0, (1.5, 0.75): 2.0, (0.7, 1.3): 2.0}
_CASES = {}
_REFS = {}


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def blobs(rng, shape, p=0.08, grow=2):
    m = rng.random(shape) < p
    for _ in range(grow):
        q = np.pad(m, ((0, 0), (1, 1), (1, 1)))
        m = q[:, 1:-1, 1:-1] | q[:, :-2, 1:-1] | q[:, 2:, 1:-1] | q[:, 1:-1, :-2] | q[:, 1:-1, 2:]
    return torch.from_numpy(m.astype(np.uint8))


def build_cases():
    """name -> (pred, target, num_classes, include_background), CPU tensors, made once and left unchanged."""
    if _CASES:
        return _CASES
    rng = np.random.default_rng(2024)
    c = _CASES
    c["batch_odd"] = (blobs(rng, (3, 37, 53)), blobs(rng, (3, 37, 53)), 1, False)
    c["wide"] = (blobs(rng, (1, 9, 1100), 0.03), blobs(rng, (1, 9, 1100), 0.03), 1, False)    # rows longer than a block
    c["tall"] = (blobs(rng, (1, 300, 5), 0.05, 1), blobs(rng, (1, 300, 5), 0.05, 1), 1, False)   # several column segments
    c["one_row"] = (blobs(rng, (1, 1, 64), 0.2, 1), blobs(rng, (1, 1, 64), 0.2, 1), 1, False)
    c["one_col"] = (blobs(rng, (1, 64, 1), 0.2, 1), blobs(rng, (1, 64, 1), 0.2, 1), 1, False)
    from csu.data import ellipse_batch
    _, t = ellipse_batch(np.random.default_rng(7), 2, 64, 5)      # int64; classes 1 and 4 / 2 absent: NaN rows
    _, p = ellipse_batch(np.random.default_rng(8), 2, 64, 5)
    c["ellipses"] = (p, t, 5, False)
    yy, xx = np.mgrid[0:40, 0:40]
    t33 = torch.from_numpy(((yy // 5) * 8 + xx // 5) % 33)
    p33 = torch.from_numpy((((yy + 2) // 5) * 8 + (xx + 1) // 5) % 33)
    c["k33"] = (p33[None].to(torch.uint8), t33[None], 33, False)  # 32 classes in one call
    frame = torch.ones(1, 30, 45, dtype=torch.uint8)
    frame[:, 4:26, 5:40] = 0                                       # a frame on all four image edges ...
    inner = torch.zeros(1, 30, 45, dtype=torch.uint8)
    inner[:, 0:30, 20:25] = 1                                      # ... against a bar from the top edge to the bottom
    inner[:, 13:17, 0:45] = 1
    c["edges"] = (frame, inner, 1, False)
    a, b = torch.zeros(1, 40, 70, dtype=torch.uint8), torch.zeros(1, 40, 70, dtype=torch.uint8)
    a[0, 0, 0] = 1
    b[0, 39, 69] = 1
    c["corners"] = (a, b, 1, False)                                # the longest possible search
    one = torch.zeros(1, 20, 30, dtype=torch.uint8)
    one[0, 7, 11] = 1
    c["full_vs_pixel"] = (torch.ones(1, 20, 30, dtype=torch.uint8), one, 1, False)
    c["max_width"] = (blobs(rng, (1, 2, 32767), 0.01, 1), blobs(rng, (1, 2, 32767), 0.01, 1), 1, False)    # 64 KiB of LDS a row
    c["max_height"] = (blobs(rng, (1, 32767, 2), 0.01, 1), blobs(rng, (1, 32767, 2), 0.01, 1), 1, False)  # 16 segments of 2048 rows
    c["mixed_dtype"] = (torch.from_numpy(rng.integers(0, 3, (2, 21, 33)).astype(np.uint8)) * blobs(rng, (2, 21, 33), 0.1),
                        torch.from_numpy(rng.integers(0, 3, (2, 21, 33))) * blobs(rng, (2, 21, 33), 0.1).long(), 3, True)
    return c


CASE_NAMES = ["batch_odd", "wide", "tall", "one_row", "one_col", "ellipses", "k33", "edges", "corners", "full_vs_pixel",
              "max_width", "max_height", "mixed_dtype"]


def reference(name, spacing):
    key = (name, spacing)
    if key not in _REFS:
        p, t, K, bg = build_cases()[name]
        _REFS[key] = metrics.reference_surface_metrics(p, t, K, spacing, SPACINGS[spacing], 95.0, bg)
    return _REFS[key]


def border_distances(name, spacing):
    """Every d1 and d2 of the case, from the reference's own pieces."""
    p, t, K, bg = build_cases()[name]
    binary, values = metrics._class_values(K, bg)
    out = []
    for b in range(p.shape[0]):
        for v in values:
            mp, mt = metrics._masks(p[b], t[b], binary, v)
            bp, bt = metrics._border(mp).nonzero().double(), metrics._border(mt).nonzero().double()
            if len(bp) and len(bt):
                out += [metrics._nearest(bp, bt, *spacing), metrics._nearest(bt, bp, *spacing)]
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.float64)


def bits(t):
    return t.contiguous().view(torch.int64)


def test_cases_are_what_they_claim():
    c = build_cases()
    assert set(CASE_NAMES) == set(c)
    assert c["ellipses"][1].dtype == torch.int64 and c["mixed_dtype"][0].dtype == torch.uint8
    assert c["mixed_dtype"][1].dtype == torch.int64
    nan = torch.isnan(reference("ellipses", (1.0, 1.0))[:, :, 0])
    assert nan.any() and not nan.all()
    assert reference("k33", (1.0, 1.0)).shape == (1, 32, 6) and not torch.isnan(reference("k33", (1.0, 1.0))).any()
    assert reference("corners", (1.0, 1.0))[0, 0, 0] == (39 ** 2 + 69 ** 2) ** 0.5


@pytest.mark.parametrize("spacing", list(SPACINGS), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", CASE_NAMES)
def test_kernels_match_the_reference(name, spacing):
    d = dev()
    p, t, K, bg = build_cases()[name]
    want = reference(name, spacing)
    tau = SPACINGS[spacing]
    got = csu.surface_metrics(p.to(d), t.to(d), K, spacing, tau, 95.0, bg)
    assert got.dtype == torch.float64 and got.device.type == "cuda" and got.shape == want.shape
    got = got.cpu()
    print(name, spacing, "max rel err", float(((got - want).abs() / want.abs().clamp_min(1e-300)).nan_to_num(0).max()))
    assert torch.equal(got[:, :, 4:], want[:, :, 4:]), "border counts"
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want[:, :, 0])
    exact = spacing != (0.7, 1.3)
    if not exact:
        dist = border_distances(name, spacing)
        assert not ((dist - tau).abs() <= 1e-5 * tau).any(), "a border distance ties with the tolerance"
    rtol = EXACT_RTOL if exact else F32_RTOL
    for j in (0, 1, 2):
        torch.testing.assert_close(got[:, :, j][ok], want[:, :, j][ok], rtol=rtol, atol=0)
    if exact:
        torch.testing.assert_close(got[:, :, 3][ok], want[:, :, 3][ok], rtol=EXACT_RTOL, atol=0)
    else:
        assert torch.equal(got[:, :, 3][ok], want[:, :, 3][ok]), "nsd"


@pytest.mark.parametrize("spacing", [(1.0, 1.0), (0.7, 1.3)], ids=["int", "fp32"])
def test_repeatable_and_independent_of_batching(spacing, monkeypatch):
    d = dev()
    p, t, K, bg = build_cases()["ellipses"]
    p, t = p.to(d), t.to(d)
    a = csu.surface_metrics(p, t, K, spacing, 1.5)
    assert torch.equal(bits(a), bits(csu.surface_metrics(p, t, K, spacing, 1.5)))
    for i in range(p.shape[0]):           # image i of a batch = that image alone
        assert torch.equal(bits(csu.surface_metrics(p[i], t[i], K, spacing, 1.5)), bits(a[i:i + 1]))
    # class c does not depend on how many classes were asked for, nor on the chunks they go in
    assert torch.equal(bits(csu.surface_metrics(p, t, 3, spacing, 1.5)), bits(a[:, :2]))
    assert torch.equal(bits(csu.surface_metrics(p, t, K, spacing, 1.5, include_background=True)[:, 1:]), bits(a))
    monkeypatch.setattr(metrics, "WORKSPACE_BUDGET", 3 * 12 * 64 * 64)      # three (image, class) pairs per call
    assert torch.equal(bits(csu.surface_metrics(p, t, K, spacing, 1.5)), bits(a))
    monkeypatch.setattr(metrics, "WORKSPACE_BUDGET", 9 * 12 * 64 * 64)      # both images' four classes in one call
    assert torch.equal(bits(csu.surface_metrics(p, t, K, spacing, 1.5)), bits(a))
    b3 = csu.surface_metrics(build_cases()["batch_odd"][0].to(d), build_cases()["batch_odd"][1].to(d), 1, spacing, 1.5)
    monkeypatch.setattr(metrics, "WORKSPACE_BUDGET", 2 * 12 * 37 * 53)      # images in chunks of two
    assert torch.equal(bits(csu.surface_metrics(build_cases()["batch_odd"][0].to(d), build_cases()["batch_odd"][1].to(d), 1,
                                                spacing, 1.5)), bits(b3))


def test_percentiles():
    """q = 0, 50 and 100 select the smallest, the middle and the largest pooled distance."""
    d = dev()
    p, t, K, bg = build_cases()["batch_odd"]
    for q in (0.0, 50.0, 100.0):
        want = metrics.reference_surface_metrics(p, t, K, (1.0, 1.0), 1.5, q)
        got = csu.surface_metrics(p.to(d), t.to(d), K, (1.0, 1.0), 1.5, q).cpu()
        torch.testing.assert_close(got, want, rtol=EXACT_RTOL, atol=0, equal_nan=True)
    assert torch.equal(got[:, :, 0], got[:, :, 1])     # q = 100: hd95 is hd


def test_too_many_classes_and_bad_arguments():
    from csu._lib import lib, ptr
    d = dev()
    m = torch.zeros(1, 40, 40, dtype=torch.uint8, device=d)
    with pytest.raises(ValueError, match="at most 32 classes"):
        csu.surface_metrics(m, m, 33, include_background=True)
    L = lib()
    out = torch.zeros(1, 33, 6, dtype=torch.float64, device=d)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=d)
    args = lambda C, H=40, W=40, mode=0, dt=0, sy=1.0, nbytes=ws.numel(): L.csu_surface_metrics(  # noqa: E731
        1, C, H, W, mode, 0, dt, ptr(m), 0, ptr(m), sy, 1.0, 1.0, 95.0, ptr(ws), nbytes, ptr(out), 33, 0, None)
    assert L.csu_surface_workspace(1, 33, 40, 40) == 0 and L.csu_surface_workspace(1, 1, 40, 40) > 12 * 40 * 40
    for kw, text in ((dict(C=33), "1 <= C <= 32"), (dict(C=1, H=40000), "32767"), (dict(C=2, mode=1), "binary form"),
                     (dict(C=1, dt=7), "CSU_SURFACE_U8"), (dict(C=1, sy=0.0), "spacing"), (dict(C=1, nbytes=16), "workspace")):
        assert args(**kw) != 0 and text in L.csu_last_error_string().decode()
    assert L.csu_edt(1, 40, 40, 3, ptr(m), 1.0, 1.0, ptr(ws), ws.numel(), ptr(out), None) != 0
    torch.cuda.synchronize()


def test_target_on_the_host_follows_the_prediction():
    d = dev()
    p, t, K, bg = build_cases()["mixed_dtype"]
    assert torch.equal(bits(csu.surface_metrics(p.to(d), t, K)), bits(csu.surface_metrics(p.to(d), t.to(d), K)))


# ---- the distance transform ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 53), (9, 1100)])
def test_edt(shape):
    d = dev()
    rng = np.random.default_rng(shape[1])
    m = blobs(rng, (2,) + shape, 0.15)
    ref1 = metrics.reference_distance_transform_edt(m, (1.0, 1.0))
    got1 = csu.distance_transform_edt(m.to(d))
    assert got1.dtype == torch.float32 and got1.shape == m.shape
    assert torch.equal(got1.cpu(), ref1.float()), "unit spacing is exact"
    assert torch.equal(csu.distance_transform_edt(m[1].bool().to(d)), got1[1])          # (H, W), another dtype
    assert torch.equal(csu.distance_transform_edt(m.long().to(d) * 5), got1)
    ref2 = metrics.reference_distance_transform_edt(m, (0.7, 1.3))
    got2 = csu.distance_transform_edt(m.float().to(d), (0.7, 1.3)).cpu().double()
    assert torch.equal(got2 == 0, ref2 == 0)
    torch.testing.assert_close(got2, ref2, rtol=F32_RTOL, atol=0)
    assert torch.isinf(csu.distance_transform_edt(torch.ones(shape, dtype=torch.uint8, device=d))).all()
    both = torch.stack([torch.ones(shape, dtype=torch.uint8), m[0]]).to(d)              # inf stays inside its image
    e = csu.distance_transform_edt(both)
    assert torch.isinf(e[0]).all() and torch.equal(e[1], got1[0])


def test_edt_longest_row():
    d = dev()
    m = torch.from_numpy((np.random.default_rng(9).random((2, 32767)) > 0.005).astype(np.uint8))     # ~330 zero pixels
    want = metrics.reference_distance_transform_edt(m, (1.0, 1.0))
    assert torch.equal(csu.distance_transform_edt(m.to(d)).cpu(), want.float())
    want = metrics.reference_distance_transform_edt(m, (0.7, 1.3))
    torch.testing.assert_close(csu.distance_transform_edt(m.to(d), (0.7, 1.3)).cpu().double(), want, rtol=F32_RTOL, atol=0)


# ---- end to end ---------------------------------------------------------------------------------
def test_evaluate_full_res_with_an_accumulator():
    from csu import infer
    from csu.model import CSWinTransformer
    d = dev()
    torch.manual_seed(11)
    m = CSWinTransformer(img_size=64, split_size=[1, 2, 2, 2], num_classes=3).set_head("logits")
    with torch.no_grad():     # the initial head puts every pixel in one class (tests/test_gpu_infer.py)
        m.output.weight.copy_(4.0 * torch.randn(m.output.weight.shape, generator=torch.Generator().manual_seed(100)))
    m = m.to(d).eval()
    g = torch.Generator().manual_seed(31)
    pairs = [(torch.randint(0, 256, (100, 90, 3), dtype=torch.uint8, generator=g),
              (torch.arange(100)[:, None] // 34 + torch.arange(90)[None, :] // 45) % 3) for _ in range(2)]
    p = infer.SlidingWindowPredictor(m, overlap=0.5, batch_size=8)
    two = infer.evaluate_full_res(p, pairs, 3)
    acc = csu.SurfaceMetrics(num_classes=3, spacing=(1.0, 1.0), tolerance=1.5)
    dice, iou, surf = infer.evaluate_full_res(p, pairs, 3, surface=acc)
    assert (dice, iou) == two
    rows = torch.cat([metrics.reference_surface_metrics(p.predict(img).cpu(), t, 3, (1.0, 1.0), 1.5) for img, t in pairs])
    ok = ~torch.isnan(rows[:, :, 0])
    assert surf["valid"] == int(ok.sum()) and surf["valid"] > 0
    for j, k in enumerate(("hd", "hd95", "assd", "nsd")):
        per = [float(rows[:, c, j][ok[:, c]].mean()) if ok[:, c].any() else float("nan") for c in range(2)]
        assert surf["class_" + k] == pytest.approx(per, rel=EXACT_RTOL, nan_ok=True)
        have = [v for v in per if v == v]
        assert surf[k] == pytest.approx(sum(have) / len(have), rel=EXACT_RTOL)


def test_capturable():
    d = dev()
    p, t, K, bg = build_cases()["ellipses"]
    p, t = p.to(d), t.to(d)
    eager = csu.surface_metrics(p, t, K, (0.7, 1.3), 2.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = csu.surface_metrics(p, t, K, (0.7, 1.3), 2.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(eager))
