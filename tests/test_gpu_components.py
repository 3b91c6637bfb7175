"""csu_ccl / csu_cc_filter on the MI355X against the numpy reference of csu.components: every
comparison is exact integer equality.  The cases are built once on the CPU and their references are
computed once per (case, connectivity); both dtypes and all tests share them.

T = 64 is the tile edge of csrc/components.hip: the shapes sit on, one below, one above and several
times T, ragged on both axes, and the thin 32767-long ones check the index arithmetic at the limit."""
import functools

import numpy as np
import pytest
import torch

import csu
from csu import components as cc
from csu import infer
from csu.components import (PostProcess, connected_components, postprocess_labels, reference_connected_components,
                            reference_postprocess_labels)
from csu.data import ellipse_batch

pytestmark = pytest.mark.gpu

T = 64
SMALL = [(1, 1), (1, T + 3), (T + 3, 1), (7, 5), (T, T), (T + 1, T - 1), (2 * T + 2, 3 * T + 5), (3, 1100), (1100, 3)]
LIMIT = [(2, 32767), (32767, 2)]
MULTI = (2 * T + 2, 3 * T + 5)
DTYPES = {"u8": torch.uint8, "i64": torch.int64}


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---- patterns (uint8 numpy maps) ----------------------------------------------------------------------
def checkerboard(H, W):
    y, x = np.mgrid[:H, :W]
    return ((y + x) % 2 == 0).astype(np.uint8)


def serpentine(H, W):
    """One-pixel-wide snake: every other row full, joined alternately at the right and the left end."""
    m = np.zeros((H, W), np.uint8)
    m[0::2] = 1
    for i, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if i % 2 == 0 else 0] = 1
    return m


def spiral(H, W):
    """A one-pixel-wide path from (0, 0) inwards: straight on while the cell ahead and the one after it are
    free, else a right turn."""
    m = np.zeros((H, W), np.uint8)
    free = lambda y, x: not (0 <= y < H and 0 <= x < W) or m[y, x] == 0
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1
    moved = True
    while moved:
        moved = False
        for _ in range(2):
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and m[ny, nx] == 0 and free(ny + dy, nx + dx):
                y, x, moved = ny, nx, True
                m[y, x] = 1
                break
            dy, dx = dx, -dy
    return m


def diagonals(H, W):
    """Diagonal lines laid through the four-tile corners, in both directions: (63, 63) -> (64, 64) and
    (63, 64) -> (64, 63), and the same one tile to the right."""
    m = np.zeros((H, W), np.uint8)
    for off in (0, T):
        for i in range(H):
            if 0 <= i + off < W:
                m[i, i + off] = 1
            x = 2 * T - 1 - i + off
            if 0 <= x < W:
                m[i, x] = 2
    return m


def comb(H, W):
    """Teeth in every other column that join only in the last row: the root is far from most pixels."""
    m = np.zeros((H, W), np.uint8)
    m[:, 0::2] = 1
    m[H - 1] = 1
    return m


def noisy_ellipses(seed, batch, size, salt):
    rng = np.random.default_rng(seed)
    m = ellipse_batch(rng, batch, size, 5)[1].numpy().astype(np.uint8)
    hit = rng.random(m.shape) < salt
    m[hit] = rng.integers(0, 5, size=int(hit.sum()))
    return m


@functools.lru_cache(maxsize=None)
def build_cases():
    cases = {}
    rng = np.random.default_rng(2024)
    for H, W in SMALL + LIMIT:
        tag = f"{H}x{W}"
        cases[f"zeros_{tag}"] = np.zeros((H, W), np.uint8)
        cases[f"ones_{tag}"] = np.ones((H, W), np.uint8)
        for p in (0.3, 0.5, 0.593):
            cases[f"random{p}_{tag}"] = (rng.random((H, W)) < p).astype(np.uint8)
    for H, W in [(T, T), (T + 1, T - 1), MULTI, (2, 32767), (32767, 2)]:
        cases[f"checker_{H}x{W}"] = checkerboard(H, W)
    for H, W in [(T + 1, T - 1), MULTI, (3, 1100), (1100, 3)]:
        tag = f"{H}x{W}"
        cases[f"serpentine_{tag}"] = serpentine(H, W)
        cases[f"serpentineT_{tag}"] = np.ascontiguousarray(serpentine(W, H).T)
        cases[f"spiral_{tag}"] = spiral(H, W)
        cases[f"comb_{tag}"] = comb(H, W)
    cases["diagonals"] = diagonals(*MULTI)
    cases["ellipses"] = noisy_ellipses(7, 2, 160, 0.0)
    cases["ellipses_salt"] = noisy_ellipses(8, 2, 160, 0.02)
    m = noisy_ellipses(9, 1, 150, 0.01)[0]
    m[m == 4] = 255                                   # an ignore value, in regions and as salt
    m[10:30, 100:140] = 255
    cases["ignore255"] = m
    # three classes of random salt: many values, many tiny components, across every seam
    cases["random_classes"] = rng.integers(0, 4, MULTI).astype(np.uint8)
    return cases


CASE_NAMES = sorted(build_cases())


@functools.lru_cache(maxsize=None)
def reference(name, conn):
    return reference_connected_components(torch.from_numpy(build_cases()[name]), conn, return_areas=True)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_ccl_equals_reference(name, conn, dtype):
    d = dev()
    m = torch.from_numpy(build_cases()[name])
    want = reference(name, conn)
    got = connected_components(m.to(DTYPES[dtype]).to(d), conn, return_areas=True)
    for g, w, what in zip(got, want, ("comp", "count", "area")):
        assert g.dtype == torch.int32 and g.device.type == "cuda" and g.shape == w.shape
        assert torch.equal(g.cpu(), w), what


def test_expected_counts_of_the_patterns():
    """The reference itself gives what the patterns were laid out for."""
    for name, m in build_cases().items():
        H, W = m.shape[-2:]
        n4, n8 = int(reference(name, 4)[1].sum()), int(reference(name, 8)[1].sum())
        if name.startswith("zeros"):
            assert (n4, n8) == (0, 0)
        elif name.startswith("ones"):
            assert (n4, n8) == (1, 1) and bool((reference(name, 8)[2] == H * W).all())
        elif name.startswith("checker"):
            assert n4 == (H * W + 1) // 2 == int(m.sum()) and n8 == 1      # every pixel of its own at 4
        elif name.startswith(("serpentine", "spiral", "comb")):
            assert (n4, n8) == (1, 1)
    assert int(reference("diagonals", 8)[1]) == 4           # two lines of 1 and two of 2, crossing between the pixels
    assert int(reference("diagonals", 4)[1]) == int((build_cases()["diagonals"] > 0).sum())


def test_batch_equals_single_images_and_runs_repeat():
    d = dev()
    names = ["random0.593_130x197", "serpentine_130x197", "random_classes"]
    x = torch.stack([torch.from_numpy(build_cases()[n]) for n in names]).to(d)
    for conn in (4, 8):
        a = connected_components(x, conn, return_areas=True)
        b = connected_components(x, conn, return_areas=True)
        for i, n in enumerate(names):
            one = connected_components(x[i], conn, return_areas=True)
            for u, v, w, r in zip(a, b, one, reference(n, conn)):
                assert torch.equal(u, v) and torch.equal(u[i], w) and torch.equal(w.cpu(), r)


def test_non_contiguous_input_and_other_integer_types():
    d = dev()
    m = torch.from_numpy(build_cases()["random_classes"])
    wide = torch.zeros(MULTI[0], 2 * MULTI[1], dtype=torch.uint8)
    wide[:, ::2] = m
    view = wide.to(d)[:, ::2]
    assert not view.is_contiguous()
    got = connected_components(view, 8, return_areas=True)
    for g, w in zip(got, reference("random_classes", 8)):
        assert torch.equal(g.cpu(), w)
    got = connected_components(m.to(torch.int32).to(d).t(), 4)
    want = reference_connected_components(m.t(), 4)
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
    b = (m > 1)
    assert torch.equal(connected_components(b.to(d), 8)[0].cpu(), reference_connected_components(b, 8)[0])
    out = postprocess_labels(view, 4, keep_largest=True, fill_holes=True)
    assert torch.equal(out.cpu(), reference_postprocess_labels(m, 4, keep_largest=True, fill_holes=True))


@pytest.mark.parametrize("outs", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)])
def test_each_output_may_be_omitted(outs):
    d = dev()
    comp, area, count = (bool(v) for v in outs)
    x = torch.from_numpy(build_cases()["random0.5_130x197"]).to(d).unsqueeze(0)
    c, n, a = cc._device_ccl(x, 8, comp=comp, area=area, count=count)
    wc, wn, wa = reference("random0.5_130x197", 8)
    assert (c is None) == (not comp) and (a is None) == (not area) and (n is None) == (not count)
    if comp:
        assert torch.equal(c[0].cpu(), wc)
    if area:
        assert torch.equal(a[0].cpu(), wa)
    if count:
        assert int(n[0]) == int(wn)


# ---- the rules ----------------------------------------------------------------------------------
RULES = {
    "keep": dict(keep_largest=True),
    "small": dict(min_size=9),
    "fill": dict(fill_holes=True),
    "all": dict(keep_largest=True, min_size=9, fill_holes=True),
    "max_hole": dict(fill_holes=True, max_hole_size=3),
    "max_hole_all": dict(keep_largest=True, min_size=4, fill_holes=True, max_hole_size=40),
}
RULES5 = dict(RULES, per_class=dict(min_size=[0, 3, 0, 30, 7], fill_holes=True), subset=dict(keep_largest=[2, 4], min_size=2))
FILTER_MAPS = ["ellipses_salt", "ignore255", "random_classes", "random0.593_130x197", "diagonals", "random0.5_65x63",
               "checker_65x63", "random0.3_1x67"]


@functools.lru_cache(maxsize=None)
def filter_reference(name, K, rule, conn):
    kw = (RULES5 if K == 5 else RULES)[rule]
    return reference_postprocess_labels(torch.from_numpy(build_cases()[name]), K, connectivity=conn, **kw)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("K,rule", [(1, r) for r in RULES] + [(5, r) for r in RULES5])
def test_postprocess_equals_reference(K, rule, conn, dtype):
    d = dev()
    kw = (RULES5 if K == 5 else RULES)[rule]
    changed = 0
    for name in FILTER_MAPS:
        m = torch.from_numpy(build_cases()[name]).to(DTYPES[dtype])
        want = filter_reference(name, K, rule, conn)
        got = postprocess_labels(m.to(d), K, connectivity=conn, **kw)
        assert got.dtype == m.dtype and got.shape == m.shape
        assert torch.equal(got.cpu(), want.to(m.dtype)), name
        changed += int((want.to(m.dtype) != (m if K > 1 else (m > 0).to(m.dtype))).sum())
    assert changed > 0


def test_postprocess_batch_in_place_and_nothing_to_do():
    d = dev()
    m = torch.from_numpy(build_cases()["ellipses_salt"])                      # (2, 160, 160)
    x = m.to(d)
    kw = dict(keep_largest=[1, 3], min_size=5, fill_holes=True)
    want = reference_postprocess_labels(m, 5, **kw)
    got = postprocess_labels(x, 5, **kw)
    assert torch.equal(got.cpu(), want) and torch.equal(x.cpu(), m)
    for i in range(2):
        assert torch.equal(postprocess_labels(x[i], 5, **kw), got[i])
    assert torch.equal(postprocess_labels(x, 5, **kw), got)
    assert torch.equal(postprocess_labels(x, 5).cpu(), m)
    assert torch.equal(postprocess_labels(x, 1).cpu(), (m > 0).to(m.dtype))
    # csu_cc_filter with out == labels
    ru = cc._Rules(5, [1, 3], 5, True, None, 8)
    y = x.clone()
    assert cc._device_postprocess(y, ru, out=y) is y
    assert torch.equal(y.cpu(), want)


def test_capture_and_replay():
    """connected_components + postprocess_labels captured once on one stream and replayed."""
    d = dev()
    H, W = T + 1, T - 1
    rng = np.random.default_rng(5)
    a = torch.from_numpy(rng.integers(0, 4, (H, W)).astype(np.uint8) * (rng.random((H, W)) < 0.7))
    b = torch.from_numpy(rng.integers(0, 4, (H, W)).astype(np.uint8) * (rng.random((H, W)) < 0.55))
    x = a.to(d)
    kw = dict(keep_largest=True, min_size=3, fill_holes=True)
    eager = connected_components(x, 8, return_areas=True) + (postprocess_labels(x, 4, **kw),)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = connected_components(x, 8, return_areas=True) + (postprocess_labels(x, 4, **kw),)
    graph.replay()
    torch.cuda.synchronize()
    for g, e in zip(out, eager):
        assert torch.equal(g, e)
    x.copy_(b.to(d))                      # the replay reads the new map
    graph.replay()
    torch.cuda.synchronize()
    want = reference_connected_components(b, 8, return_areas=True) + (reference_postprocess_labels(b, 4, **kw),)
    for g, w in zip(out, want):
        assert torch.equal(g.cpu(), w)


# ---- SlidingWindowPredictor / evaluate_full_res ---------------------------------------------------------
class Stub(torch.nn.Module):
    """Logits that turn channel 0 of the image (= class / 4) back into the class."""

    def __init__(self):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        k = torch.arange(5, dtype=x.dtype, device=x.device).view(1, -1, 1, 1)
        return -50 * (x[:, :1].float() * 4 - k) ** 2


def test_predictor_and_evaluate_full_res():
    from csu.metrics import SurfaceMetrics
    d = dev()
    H, W = 70, 90
    maps = torch.from_numpy(noisy_ellipses(31, 2, 96, 0.04)[:, :H, :W].astype(np.int64))
    pairs = [(torch.stack([m.float() / 4] * 3), m) for m in maps]
    post = PostProcess(5, keep_largest=True, min_size=4, fill_holes=True)
    stub = Stub().to(d)
    plain = infer.SlidingWindowPredictor(stub, tile=32, overlap=0.5, batch_size=7)
    cleaned = infer.SlidingWindowPredictor(stub, tile=32, overlap=0.5, batch_size=7, postprocess=post)
    raws = []
    for img, m in pairs:
        raw = plain.predict(img)
        assert raw.is_cuda and torch.equal(raw.cpu().long(), m)
        want = postprocess_labels(raw, 5, keep_largest=True, min_size=4, fill_holes=True)
        assert torch.equal(want.cpu(), reference_postprocess_labels(raw.cpu(), 5, True, 4, True)) and not torch.equal(want, raw)
        got, prob = cleaned.predict(img, return_prob=True)
        assert got.dtype == torch.uint8 and torch.equal(got, want)
        assert torch.equal(prob, plain.predict(img, return_prob=True)[1])
        raws.append(want)

    class Fixed:
        def __init__(self):
            self.it = iter(raws)

        def predict(self, image):
            return next(self.it)

    by_hand = infer.evaluate_full_res(Fixed(), pairs, 5, surface=SurfaceMetrics(5))
    # repr: the per-class lists may hold NaN, and NaN != NaN
    assert repr(infer.evaluate_full_res(plain, pairs, 5, surface=SurfaceMetrics(5), postprocess=post)) == repr(by_hand)
    assert repr(infer.evaluate_full_res(cleaned, pairs, 5, surface=SurfaceMetrics(5))) == repr(by_hand)
    assert infer.evaluate_full_res(plain, pairs, 5) != by_hand[:2]
