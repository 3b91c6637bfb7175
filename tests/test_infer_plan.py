"""Tiled whole-image inference, host side (csu.infer): the tile plan, the separable weight sum, the TTA
variants and reference_predict's un-flip and edge clamp.  No GPU."""
import itertools

import numpy as np
import pytest
import torch

from csu import infer

S = 32
LENGTHS = [1, 20, 32, 33, 63, 64, 80, 95]
OVERLAPS = [0.0, 0.25, 0.5, 0.75]
IMAGES = [(80, 72), (20, 40)]


@pytest.mark.parametrize("L,overlap", list(itertools.product(LENGTHS, OVERLAPS)))
def test_plan_axis_covers_and_stays_inside(L, overlap):
    pos = infer.plan_axis(L, S, overlap)
    covered = np.zeros(max(L, S), dtype=bool)
    for p in pos:
        assert 0 <= p and p + S <= max(L, S)
        covered[p:p + S] = True
    assert covered[:L].all()
    assert pos[0] == 0
    if L <= S:
        assert pos == [0]
    else:
        stride = max(1, S - int(round(S * overlap)))
        n = -(-(L - S) // stride) + 1
        assert len(pos) == n and pos[-1] == L - S
        assert pos == [min(i * stride, L - S) for i in range(n)]
        assert all(b - a <= stride for a, b in zip(pos, pos[1:]))


def test_plan_tiles_order_is_row_major_with_tta_innermost():
    t = infer.plan_tiles(80, 72, S, 0.5, "d4")
    ys, xs = infer.plan_axis(80, S, 0.5), infer.plan_axis(72, S, 0.5)
    assert t.dtype == np.int32 and t.shape == (len(ys) * len(xs) * 8, 6) and (t[:, 5] == 1).all()
    want = [(y, x) + infer.TTA_VARIANTS[n] for y in ys for x in xs for n in infer.D4]
    assert [tuple(r[:5]) for r in t.tolist()] == want
    assert infer.parse_tta([(1, 1, 2), "rot90"]) == [(1, 1, 2), (0, 0, 1)]
    assert infer.parse_tta(("identity",)) == [(0, 0, 0)] and len(infer.parse_tta("d4")) == 8
    with pytest.raises(ValueError):
        infer.parse_tta(["diagonal"])
    with pytest.raises(ValueError):
        infer.parse_tta([(0, 0, 4)])


def test_window():
    assert (infer.window_1d(S, "uniform") == 1.0).all()
    g = infer.window_1d(S, "gaussian")
    i = np.arange(S)
    assert np.array_equal(g, np.exp(-0.5 * ((i - (S - 1) / 2) / (0.125 * S)) ** 2))
    assert (g > 0).all() and np.array_equal(g, g[::-1])
    with pytest.raises(ValueError):
        infer.window_1d(S, "hann")


@pytest.mark.parametrize("H,W", IMAGES + [(33, 95), (64, 64)])
@pytest.mark.parametrize("overlap", OVERLAPS)
@pytest.mark.parametrize("kind", ["gaussian", "uniform"])
def test_separable_weight_sum_equals_brute_force(H, W, overlap, kind):
    w1 = infer.window_1d(S, kind)
    w2 = np.outer(w1, w1)
    table = infer.plan_tiles(H, W, S, overlap, "d4")
    acc = np.zeros((H, W))
    for y0, x0, *_ in table.tolist():
        hh, ww = min(S, H - y0), min(S, W - x0)
        acc[y0:y0 + hh, x0:x0 + ww] += w2[:hh, :ww]
    sep = np.outer(infer.axis_weight(H, S, overlap, w1), infer.axis_weight(W, S, overlap, w1)) * 8
    assert (sep > 0).all()
    assert np.abs(sep - acc).max() <= 1e-12 * acc.max()
    assert (np.abs(sep - acc) <= 1e-12 * acc).all()


def test_variant_names_are_the_eight_symmetries():
    """Each named variant's forward view is the torch op of that name; all eight differ."""
    t = torch.arange(S * S, dtype=torch.float64).reshape(1, S, S)
    want = {"identity": t, "hflip": t.flip(-1), "vflip": t.flip(-2), "rot90": torch.rot90(t, -1, (-2, -1)),
            "rot180": torch.rot90(t, 2, (-2, -1)), "rot270": torch.rot90(t, 1, (-2, -1)),
            "transpose": t.transpose(-2, -1), "antitranspose": t.flip(-1).flip(-2).transpose(-2, -1)}
    seen = []
    for name, (h, v, r) in infer.TTA_VARIANTS.items():
        f = infer._forward_view(t, h, v, r)
        assert torch.equal(f, want[name]), name
        assert torch.equal(infer._backward_view(f, h, v, r), t), name
        assert not any(torch.equal(f, s) for s in seen)
        seen.append(f)


def test_forward_view_is_the_augmentation_oracles():
    """(hflip, vflip, rot) mean what they mean to the training augmentation (oracle.augment_ref)."""
    from oracle import augment_ref as A
    src = np.random.default_rng(0).integers(0, 256, (S, S, 3), dtype=np.uint8)
    for h, v, r in itertools.product((0, 1), (0, 1), range(4)):
        got = infer._forward_view(torch.from_numpy(src).permute(2, 0, 1), h, v, r).permute(1, 2, 0).numpy()
        assert np.array_equal(got, A.geometry(src, (h, v, r, 0, 0, S, S))), (h, v, r)


@pytest.mark.parametrize("H,W", IMAGES)
@pytest.mark.parametrize("src", ["u8", "f32"])
@pytest.mark.parametrize("window", ["gaussian", "uniform"])
def test_reference_predict_identity_fn_returns_the_image(H, W, src, window):
    """fn returns channel 0 of its input as the probability: whatever the variant, the blended result
    is the image's channel 0 at every pixel -- the un-flip inverts the flip for all eight variants and
    the pixels a clamped tile replicates past the edge are dropped."""
    g = torch.Generator().manual_seed(H * 100 + W)
    if src == "u8":
        img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g)
        want = img[:, :, 0].double() / 255.0
    else:
        img = torch.rand(3, H, W, generator=g)
        want = img[0].double()
    calls = []

    def fn(x):
        assert x.dtype == torch.float32 and tuple(x.shape[1:]) == (3, S, S)
        calls.append(x.shape[0])
        return x[:, :1]

    for tta in (infer.D4, ("antitranspose",), ("rot90", "hflip")):
        labels, prob = infer.reference_predict(fn, img, S, 0.5, window, tta, batch_size=5, output="prob", return_prob=True)
        assert prob.dtype == torch.float64 and tuple(prob.shape) == (1, H, W)
        # float32 image values, fp64 arithmetic: the weighted mean of equal numbers
        assert (prob[0] - want.float().double()).abs().max() <= 1e-12
        assert labels.dtype == torch.uint8 and torch.equal(labels, (prob[0] > 0.5).to(torch.uint8))
    n = len(infer.plan_tiles(H, W, S, 0.5, ("rot90", "hflip")))
    assert sum(calls[-(-(-n // 5)):]) == n and max(calls) <= 5


def test_reference_predict_position_dependent_fn_pins_orientation():
    """A model that is NOT equivariant (it adds a ramp in its own frame) separates a correct un-flip
    from a forgotten one: the expectation is computed per variant from the named torch ops."""
    H, W = 32, 32
    img = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3))
    ramp = torch.linspace(0, 1, S).view(1, 1, S, 1) * 0.25 + torch.linspace(0, 1, S).view(1, 1, 1, S) * 0.5

    def fn(x):
        return x[:, :1] * 0.25 + ramp

    for name, (h, v, r) in infer.TTA_VARIANTS.items():
        _, prob = infer.reference_predict(fn, img, S, 0.5, "uniform", (name,), output="prob", return_prob=True)
        want = img[:1].double() * 0.25 + infer._backward_view(ramp[0].double(), h, v, r)
        assert (prob - want).abs().max() <= 1e-7, name     # fn computes in fp32


def test_reference_predict_logits_forms():
    H, W = 40, 36
    img = torch.rand(3, H, W, generator=torch.Generator().manual_seed(5))
    w = torch.randn(4, 3, generator=torch.Generator().manual_seed(6))

    def fn(x):
        return torch.einsum("kc,bchw->bkhw", w, x)

    labels, prob = infer.reference_predict(fn, img, S, 0.25, "gaussian", "d4", output="logits", return_prob=True)
    want = torch.softmax(torch.einsum("kc,chw->khw", w.double(), img.double()), 0)    # pointwise model: exact
    assert (prob - want).abs().max() <= 1e-6
    assert (prob.sum(0) - 1).abs().max() <= 1e-12
    assert torch.equal(labels, prob.argmax(0).to(torch.uint8))
    _, p1 = infer.reference_predict(lambda x: fn(x)[:, :1], img, S, 0.25, "gaussian", ("vflip",), output="logits",
                                    return_prob=True)
    assert (p1[0] - torch.sigmoid((w[0].double().view(3, 1, 1) * img.double()).sum(0))).abs().max() <= 1e-6


def test_predictor_on_the_cpu_uses_the_torch_path():
    class Pointwise(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c = torch.nn.Conv2d(3, 3, 1)

        def forward(self, x):
            return self.c(x)

    m = Pointwise()
    img = torch.randint(0, 256, (50, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(7))
    p = infer.SlidingWindowPredictor(m, tile=S, overlap=0.5, tta=("identity", "hflip"), batch_size=3)
    labels, prob = p.predict(img.numpy(), return_prob=True)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (50, 70)
    assert prob.dtype == torch.float32 and tuple(prob.shape) == (3, 50, 70)
    with torch.no_grad():
        want = torch.softmax(m(img.permute(2, 0, 1).float()[None] / 255.0)[0].double(), 0)
    assert (prob.double() - want).abs().max() <= 1e-6
    with pytest.raises(ValueError):
        infer.SlidingWindowPredictor(m)                  # no img_size and no tile
    with pytest.raises(ValueError):
        infer.SlidingWindowPredictor(m, tile=S, batch_size=129)


def test_evaluate_full_res_on_the_cpu():
    class Thresh(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.dummy = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            return (x[:, :1] - 0.5) * 20

    pairs = []
    g = torch.Generator().manual_seed(9)
    for _ in range(2):
        img = torch.rand(3, 45, 52, generator=g)
        pairs.append((img, (torch.rand(45, 52, generator=g) > 0.5).float()))
    p = infer.SlidingWindowPredictor(Thresh(), tile=S)
    dice, iou = infer.evaluate_full_res(p, pairs, 1)
    d, u = [], []
    for img, t in pairs:
        pred = (img[0] > 0.5).double().numpy()
        tt = t.double().numpy()
        inter = (pred * tt).sum()
        d.append((2 * inter + 1e-6) / (pred.sum() + tt.sum() + 1e-6))
        u.append((inter + 1e-6) / (pred.sum() + tt.sum() - inter + 1e-6))
    assert abs(dice - np.mean(d)) <= 1e-12 and abs(iou - np.mean(u)) <= 1e-12
