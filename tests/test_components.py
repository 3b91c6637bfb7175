"""csu.components on the CPU: the numpy reference against hand-written cases and scipy.ndimage, the
argument checks of the Python side and of the C ABI (no device is touched), and the post-processing
plumbing of SlidingWindowPredictor / evaluate_full_res."""
import ctypes

import numpy as np
import pytest
import torch

import csu
from csu import components as cc
from csu import infer
from csu.components import (PostProcess, connected_components, postprocess_labels, reference_connected_components,
                            reference_postprocess_labels)
from csu.data import ellipse_batch


def grid(*rows):
    """A uint8 map from strings of digits ('.' = 0)."""
    return torch.tensor([[0 if ch == "." else int(ch) for ch in r] for r in rows], dtype=torch.uint8)


def noisy_ellipses(seed, batch, size, classes=5, salt=0.02):
    """int64 (B, S, S) ellipse label maps with `salt` of the pixels set to a random class."""
    rng = np.random.default_rng(seed)
    m = ellipse_batch(rng, batch, size, classes)[1].numpy().copy()
    hit = rng.random(m.shape) < salt
    m[hit] = rng.integers(0, classes, size=int(hit.sum()))
    return torch.from_numpy(m)


# ---- the reference against hand-written cases -------------------------------------------------------
def test_diagonal_blobs_join_at_8_only():
    m = grid("11..",
             "11..",
             "..11",
             "..11")
    comp, count = reference_connected_components(m, 8)
    assert int(count) == 1 and torch.equal(comp, (m > 0).int())
    comp, count, area = reference_connected_components(m, 4, return_areas=True)
    assert int(count) == 2
    assert torch.equal(comp, torch.tensor([[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 2, 2], [0, 0, 2, 2]], dtype=torch.int32))
    # the background is 4-connected whatever the connectivity: two components of 4 pixels each
    assert torch.equal(area, torch.full((4, 4), 4, dtype=torch.int32))
    assert comp.dtype == torch.int32 and count.dtype == torch.int32 and area.dtype == torch.int32


def test_numbers_follow_the_first_pixel_in_raster_order():
    m = grid("..2.1",
             "3.2.1",
             "3...1",
             "3.111")
    comp, count, area = reference_connected_components(m, 4, return_areas=True)
    assert int(count) == 3
    assert torch.equal(comp, torch.tensor([[0, 0, 1, 0, 2], [3, 0, 1, 0, 2], [3, 0, 0, 0, 2], [3, 0, 2, 2, 2]],
                                          dtype=torch.int32))
    assert torch.equal(area, torch.tensor([[9, 9, 2, 9, 6], [3, 9, 2, 9, 6], [3, 9, 9, 9, 6], [3, 9, 6, 6, 6]],
                                          dtype=torch.int32))


def test_ring_with_a_hole():
    m = grid(".....",
             ".111.",
             ".1.1.",
             ".111.",
             ".....")
    for conn in (4, 8):
        out = reference_postprocess_labels(m, 1, fill_holes=True, connectivity=conn)
        want = m.clone()
        want[2, 2] = 1
        assert torch.equal(out, want) and out.dtype == m.dtype
    # the hole is background-4-connected: at connectivity 8 a diagonal gap in the ring does not open it
    m[1, 1] = 0
    out = reference_postprocess_labels(m, 1, fill_holes=True, connectivity=8)
    assert int(out[2, 2]) == 1 and int(out[1, 1]) == 0


def test_ring_at_the_border_is_a_hole_unless_open_to_it():
    closed = grid("111",
                  "1.1",
                  "111")
    assert int(reference_postprocess_labels(closed, 1, fill_holes=True)[1, 1]) == 1
    opened = grid("1.1",
                  "1.1",
                  "111")
    assert torch.equal(reference_postprocess_labels(opened, 1, fill_holes=True), opened)
    # max_hole_size: a hole of 2 pixels stays at 1, goes at 2
    two = grid("1111",
               "1..1",
               "1111")
    assert torch.equal(reference_postprocess_labels(two, 1, fill_holes=True, max_hole_size=1), two)
    assert torch.equal(reference_postprocess_labels(two, 1, fill_holes=True, max_hole_size=2), (two >= 0).to(torch.uint8))


def test_hole_between_two_classes_takes_its_left_neighbour():
    m = grid("22211",
             "2..11",
             "2.111",
             "22211")
    out = reference_postprocess_labels(m, 3, fill_holes=True)
    want = m.clone()
    want[1, 1] = want[1, 2] = want[2, 1] = 2      # first pixel (1, 1): left of it is a 2
    assert torch.equal(out, want)
    # an ignore value left of the hole's first pixel: not filled; and 255 is never a hole itself
    m = grid("99911",
             "9..11",
             "9.111",
             "99911")
    m[m == 9] = 255
    assert torch.equal(reference_postprocess_labels(m, 3, fill_holes=True), m)


def test_filling_joins_components_before_the_size_rule():
    m = grid("......",
             ".1111.",
             ".1..1.",
             ".2222.",
             "......")
    # class 1 has one component (6 pixels); the hole (2 pixels) takes the 1 to its left: 8 pixels
    assert torch.equal(reference_postprocess_labels(m, 3, min_size=7), grid("......", "......", "......", "......", "......"))
    out = reference_postprocess_labels(m, 3, min_size=[0, 7, 0], fill_holes=True)
    assert torch.equal(out, grid("......", ".1111.", ".1111.", ".2222.", "......"))
    # two components of one class that only the filled hole joins (connectivity 4)
    m = grid(".......",
             ".11211.",
             ".1...1.",
             ".22222.",
             ".......")
    assert int(reference_connected_components((m == 1).to(torch.uint8), 4)[1]) == 2
    gone = reference_postprocess_labels(m, 3, min_size=[0, 4, 0], connectivity=4)
    assert not bool((gone == 1).any())                    # each arm has 3 pixels
    out = reference_postprocess_labels(m, 3, min_size=[0, 4, 0], fill_holes=True, connectivity=4)
    assert torch.equal(out, grid(".......", ".11211.", ".11111.", ".22222.", "......."))


def test_keep_largest_and_its_tie():
    m = grid("11..2",
             "11..2",
             ".....",
             "11.22",
             "11.22")
    out = reference_postprocess_labels(m, 3, keep_largest=True)
    assert torch.equal(out, grid("11...", "11...", ".....", "...22", "...22"))      # class 1: a tie, the first wins
    out = reference_postprocess_labels(m, 3, keep_largest=[2])
    assert torch.equal(out, grid("11...", "11...", ".....", "11.22", "11.22"))
    # the size rule comes first: the largest of what is left
    out = reference_postprocess_labels(m, 3, keep_largest=True, min_size=[0, 5, 3])
    assert torch.equal(out, grid(".....", ".....", ".....", "...22", "...22"))
    # binary form: everything > 0 is the one class
    out = reference_postprocess_labels(m, 1, keep_largest=True, connectivity=4)
    assert torch.equal(out, grid("11...", "11...", ".....", ".....", "....."))


def test_shapes_dtypes_and_the_cpu_path():
    m = noisy_ellipses(3, 2, 40)
    for t in (m, m.to(torch.uint8), m.to(torch.int32), m.numpy()):
        comp, count, area = connected_components(t, 8, return_areas=True)
        r = reference_connected_components(m, 8, return_areas=True)
        assert all(torch.equal(a, b) for a, b in zip((comp, count, area), r))
        assert tuple(comp.shape) == (2, 40, 40) and tuple(count.shape) == (2,)
    comp, count = connected_components(m[1], 4)
    assert tuple(comp.shape) == (40, 40) and count.dim() == 0
    assert torch.equal(comp, reference_connected_components(m, 4)[0][1])
    b = m > 2
    out = postprocess_labels(b, 1, keep_largest=True)
    assert out.dtype == torch.bool and tuple(out.shape) == (2, 40, 40)
    assert torch.equal(out, reference_postprocess_labels(b.to(torch.uint8), 1, keep_largest=True).bool())
    out = postprocess_labels(m.to(torch.int32)[0], 5, min_size=3)
    assert out.dtype == torch.int32 and tuple(out.shape) == (40, 40)
    assert torch.equal(out.long(), reference_postprocess_labels(m[0], 5, min_size=3))
    # every rule off: the map itself (binarised for one class)
    assert torch.equal(postprocess_labels(m, 5), m)
    assert torch.equal(postprocess_labels(m, 1), (m > 0).long())
    # a batch is its images
    full = reference_postprocess_labels(m, 5, True, 4, True)
    for i in range(2):
        assert torch.equal(full[i], reference_postprocess_labels(m[i], 5, True, 4, True))
    for name in ("connected_components", "postprocess_labels", "PostProcess", "reference_connected_components",
                 "reference_postprocess_labels"):
        assert getattr(csu, name) is getattr(cc, name) and name in csu.__all__


# ---- the reference against scipy ------------------------------------------------------------------
SHAPES = [(1, 1), (1, 7), (9, 1), (2, 2), (5, 8), (17, 13), (40, 40), (33, 40)]
STRUCT = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: [[1, 1, 1]] * 3}


def random_maps():
    rng = np.random.default_rng(11)
    return [(rng.random(s) < p).astype(np.uint8) for s in SHAPES for p in (0.3, 0.5, 0.6)]


@pytest.mark.parametrize("conn", [4, 8])
def test_reference_equals_scipy_label(conn):
    ndi = pytest.importorskip("scipy.ndimage")
    for m in random_maps():
        want, n = ndi.label(m, structure=STRUCT[conn])
        comp, count, area = reference_connected_components(m, conn, return_areas=True)
        assert int(count) == n and np.array_equal(comp.numpy(), want)
        sizes = np.bincount(want.ravel())
        assert np.array_equal(area.numpy()[m > 0], sizes[want[m > 0]])


def test_reference_equals_scipy_fill_holes():
    ndi = pytest.importorskip("scipy.ndimage")
    for conn in (4, 8):
        for m in random_maps():
            out = reference_postprocess_labels(m, 1, fill_holes=True, connectivity=conn)
            assert np.array_equal(out.numpy(), ndi.binary_fill_holes(m).astype(np.uint8))


def scipy_postprocess(a, K, keep, min_size, fill, max_hole, conn):
    """The three steps restated literally with scipy.ndimage, class by class."""
    import scipy.ndimage as ndi
    a = a.copy()
    H, W = a.shape
    if fill:
        lab, n = ndi.label(a == 0, structure=STRUCT[4])
        new = a.copy()
        for i in range(1, n + 1):
            ys, xs = np.nonzero(lab == i)
            if ys.min() == 0 or xs.min() == 0 or ys.max() == H - 1 or xs.max() == W - 1:
                continue
            if max_hole is not None and len(ys) > max_hole:
                continue
            v = a[ys[0], xs[0] - 1]           # nonzero() is in raster order
            if v < K:
                new[lab == i] = v
        a = new
    for c in range(1, K):
        lab, n = ndi.label(a == c, structure=STRUCT[conn])
        sizes = np.bincount(lab.ravel(), minlength=n + 1)
        a[(lab > 0) & (sizes[lab] < min_size[c])] = 0
    for c in keep:
        lab, n = ndi.label(a == c, structure=STRUCT[conn])
        if n:
            sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
            a[(lab > 0) & (lab != int(np.argmax(sizes)) + 1)] = 0     # argmax: the first of equals
    return a


@pytest.mark.parametrize("conn", [4, 8])
def test_reference_postprocess_equals_scipy_restatement(conn):
    pytest.importorskip("scipy.ndimage")
    maps = noisy_ellipses(5, 3, 64, salt=0.04)
    maps[2][maps[2] == 4] = 255          # an ignore value
    cfgs = [dict(keep=[1, 2, 3, 4], min_size=[0] * 5, fill=False, max_hole=None),
            dict(keep=[], min_size=[0, 6, 2, 9, 4], fill=False, max_hole=None),
            dict(keep=[], min_size=[0] * 5, fill=True, max_hole=None),
            dict(keep=[2, 4], min_size=[0, 3, 3, 3, 3], fill=True, max_hole=5),
            dict(keep=[1, 2, 3, 4], min_size=[0, 8, 8, 8, 8], fill=True, max_hole=None)]
    for cfg in cfgs:
        got = reference_postprocess_labels(maps, 5, cfg["keep"], cfg["min_size"], cfg["fill"], cfg["max_hole"], conn)
        for b in range(3):
            want = scipy_postprocess(maps[b].numpy(), 5, cfg["keep"], cfg["min_size"], cfg["fill"], cfg["max_hole"], conn)
            assert np.array_equal(got[b].numpy(), want), (cfg, b)


# ---- arguments ----------------------------------------------------------------------------------
def test_python_side_argument_checks():
    m = torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="connectivity"):
        connected_components(m, 6)
    with pytest.raises(ValueError, match="label map"):
        connected_components(torch.zeros(4))
    with pytest.raises(ValueError, match="integer or bool"):
        connected_components(torch.zeros(4, 4))
    with pytest.raises(TypeError):
        connected_components([[0, 1]])
    for kw in (dict(num_classes=0), dict(num_classes=33), dict(min_size=-1), dict(num_classes=3, min_size=[0, 1]),
               dict(num_classes=3, min_size=[0, -1, 2]), dict(num_classes=3, keep_largest=[3]),
               dict(num_classes=3, keep_largest=[0]), dict(max_hole_size=-1), dict(connectivity=5)):
        with pytest.raises(ValueError):
            postprocess_labels(m, **kw)
        with pytest.raises(ValueError):
            PostProcess(**kw)
    assert "keep_largest=[1, 2]" in repr(PostProcess(3, keep_largest=True))
    arr, mask = cc._Rules(4, [1, 3], [9, 5, 6, 7], False, None, 8).tables()
    assert list(arr) == [0, 5, 6, 7] and mask == 0b1010
    arr, mask = cc._Rules(1, True, 12, False, None, 8).tables()
    assert list(arr) == [12] and mask == 1


def test_abi_rejects_bad_arguments_on_the_host():
    """Bad arguments are refused with CSU_E_ARG / CSU_E_WORKSPACE and a message before any launch (the
    pointers are dummies a launch would fault on)."""
    from csu import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40
    ok = dict(B=2, H=5, W=7, dtype=0, conn=8)
    bad = [dict(B=0), dict(H=0), dict(W=0), dict(H=32768), dict(W=32768), dict(B=65536), dict(B=40, H=32767, W=32767),
           dict(conn=6), dict(conn=0), dict(dtype=2), dict(dtype=-1)]
    for b in bad:
        a = dict(ok, **b)
        assert L.csu_ccl(a["B"], a["H"], a["W"], a["dtype"], q, a["conn"], q, big, q, q, q, None) == -1, b     # CSU_E_ARG
        assert b"ccl:" in L.csu_last_error_string()
        assert L.csu_cc_filter(a["B"], a["H"], a["W"], a["dtype"], q, a["conn"], 3, None, 0, 0, -1, q, big, q, None) == -1, b
        assert b"cc_filter:" in L.csu_last_error_string()
        if "conn" not in b and "dtype" not in b:
            assert L.csu_ccl_workspace(a["B"], a["H"], a["W"]) == 0 and L.csu_cc_filter_workspace(a["B"], a["H"], a["W"]) == 0
    assert L.csu_ccl(2, 5, 7, 0, q, 8, q, big, None, None, None, None) == -1           # no output at all
    assert L.csu_ccl(2, 5, 7, 0, None, 8, q, big, q, q, q, None) == -1
    assert L.csu_ccl(2, 5, 7, 0, q, 8, None, big, q, q, q, None) == -1
    neg, fine = (ctypes.c_int * 3)(0, -1, 0), (ctypes.c_int * 3)(0, 4, 0)
    for K, ms, hole in ((0, None, -1), (33, None, -1), (3, neg, -1), (3, fine, -2)):
        assert L.csu_cc_filter(2, 5, 7, 0, q, 8, K, ms, 0, 0, hole, q, big, q, None) == -1, (K, hole)
    assert L.csu_cc_filter(2, 5, 7, 0, None, 8, 3, fine, 0, 0, -1, q, big, q, None) == -1
    assert L.csu_cc_filter(2, 5, 7, 0, q, 8, 3, fine, 0, 0, -1, q, big, None, None) == -1
    # the workspace formulas of include/csu.h, and CSU_E_WORKSPACE one byte below them
    up = lambda n: (n + 255) // 256 * 256
    for B, H, W in ((2, 5, 7), (1, 65, 63), (3, 130, 197), (1, 32767, 2)):
        n = L.csu_ccl_workspace(B, H, W)
        assert n == 3 * up(4 * B * H * W) + up(4 * B * -(-H * W // 4096))
        f = L.csu_cc_filter_workspace(B, H, W)
        assert f == 2 * up(4 * B * H * W) + up(256 * B)
        assert L.csu_ccl(B, H, W, 0, q, 8, q, n - 1, q, q, q, None) == -3
        assert L.csu_cc_filter(B, H, W, 0, q, 8, 3, fine, 0, 0, -1, q, f - 1, q, None) == -3
        assert b"workspace" in L.csu_last_error_string()


# ---- SlidingWindowPredictor / evaluate_full_res ---------------------------------------------------------
class Stub(torch.nn.Module):
    """Logits that turn channel 0 of the image (= class / 4) back into the class."""

    def __init__(self, K):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))
        self.K = K

    def forward(self, x):
        if self.K == 1:
            return (x[:, :1] - 0.5) * 40
        k = torch.arange(self.K, dtype=x.dtype, device=x.device).view(1, -1, 1, 1)
        return -50 * (x[:, :1] * 4 - k) ** 2


def stub_pairs(K, n=2, size=44):
    maps = noisy_ellipses(21, n, size, 5 if K > 1 else 2, salt=0.05)
    return [(torch.stack([m.float() / (4 if K > 1 else 1)] * 3), m) for m in maps]


@pytest.mark.parametrize("K", [1, 5])
def test_predictor_and_evaluate_plumbing_on_the_cpu(K):
    from csu.metrics import SurfaceMetrics
    pairs = stub_pairs(K)
    post = PostProcess(K, keep_largest=True, min_size=3, fill_holes=True)
    plain = infer.SlidingWindowPredictor(Stub(K), tile=16, overlap=0.5, batch_size=5)
    cleaned = infer.SlidingWindowPredictor(Stub(K), tile=16, overlap=0.5, batch_size=5, postprocess=post)
    for img, m in pairs:
        raw = plain.predict(img)
        assert torch.equal(raw.long(), m if K > 1 else (m > 0).long())         # the stub reproduces the map
        assert torch.equal(plain.predict(img, postprocess=None), raw)
        want = reference_postprocess_labels(raw, K, True, 3, True)
        assert not torch.equal(want, raw)
        got, prob = cleaned.predict(img, return_prob=True)
        assert got.dtype == torch.uint8 and torch.equal(got, want)
        assert torch.equal(prob, plain.predict(img, return_prob=True)[1])
        assert torch.equal(cleaned.predict(img, postprocess=None), raw)
        assert torch.equal(plain.predict(img, postprocess=post), want)

    class Fixed:       # a predictor of the already cleaned maps
        def __init__(self):
            self.it = iter([reference_postprocess_labels(plain.predict(img), K, True, 3, True) for img, _ in pairs])

        def predict(self, image):
            return next(self.it)

    sm = lambda: SurfaceMetrics(K)
    by_hand = infer.evaluate_full_res(Fixed(), pairs, K, surface=sm())
    # repr: the per-class lists hold NaN for a class without a valid pair, and NaN != NaN
    assert repr(infer.evaluate_full_res(plain, pairs, K, surface=sm(), postprocess=post)) == repr(by_hand)
    assert repr(infer.evaluate_full_res(cleaned, pairs, K, surface=sm())) == repr(by_hand)
    # the call's setting replaces the predictor's own
    other = PostProcess(K, min_size=2)
    ref_other = infer.evaluate_full_res(plain, pairs, K, postprocess=other)
    assert infer.evaluate_full_res(cleaned, pairs, K, postprocess=other) == ref_other
    assert ref_other != by_hand[:2]
    assert infer.evaluate_full_res(plain, pairs, K) != by_hand[:2]
