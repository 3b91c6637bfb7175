"""Tiled whole-image inference on the MI355X: csu_tile_gather / csu_tile_blend / csu_tile_finish against
csu.infer.reference_predict's fp64 arithmetic on synthetic model outputs, and SlidingWindowPredictor end
to end against reference_predict fed by the same network.

Probabilities: max abs error <= 4e-6.  At most 32 positive fp32 terms of at most 1, each a few ulp off,
give about (32 + 4) 2^-24 = 2.1e-6 in the worst case; doubling that admits a 2-ulp device exp.
Labels: equal to the reference's wherever the fp64 reference's decision margin (top-two probability gap,
|p - 0.5| for one class) is >= 1e-5; the pixels excluded that way are at most 0.1 % of the image."""
import copy

import numpy as np
import pytest
import torch

from csu import infer

pytestmark = pytest.mark.gpu

PROB_TOL = 4e-6
MARGIN = 1e-5
EXCLUDED_CAP = 1e-3

# (H, W, S, overlap, K, dtype, layout)
CASES = [
    (80, 72, 32, 0.5, 3, torch.float32, "nchw"),
    (80, 72, 32, 0.25, 5, torch.bfloat16, "class_last_padded"),     # pitch 8, pad_ok
    (20, 40, 32, 0.5, 2, torch.float32, "class_last_dense"),
    (33, 95, 32, 0.5, 1, torch.float32, "prob"),
    (33, 95, 32, 0.5, 1, torch.bfloat16, "nchw"),
    (64, 64, 32, 0.5, 32, torch.bfloat16, "class_last_dense"),
]
_REFS = {}


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def case_ref(case, window="gaussian"):
    """(table, outputs (N, K, S, S) in the tested dtype, fp64 labels, fp64 prob) on the CPU, made once per
    case and left unchanged.  All eight variants."""
    key = (CASES.index(case), window)
    if key not in _REFS:
        H, W, S, overlap, K, dtype, layout = case
        table = infer.plan_tiles(H, W, S, overlap, "d4")
        g = torch.Generator().manual_seed(1000 + CASES.index(case))
        z = 2.0 * torch.randn(len(table), K, S, S, generator=g)
        if layout == "prob":
            z = torch.sigmoid(z)
        z = z.to(dtype)                      # rounded before either side sees it
        chunks = iter(torch.split(z.double(), 16))
        labels, prob = infer.reference_predict(lambda x: next(chunks), torch.zeros(3, H, W), S, overlap, window, "d4", 16,
                                               "prob" if layout == "prob" else "logits", True)
        _REFS[key] = (table, z, labels, prob)
    return _REFS[key]


def place(z, layout, d):
    """Model outputs (B, K, S, S) on the device in a memory layout."""
    B, K, H, W = z.shape
    if layout in ("nchw", "prob"):
        return z.to(d).contiguous()
    pitch = (K + 7) // 8 * 8 if layout == "class_last_padded" else K
    buf = torch.full((B, H * W, pitch), float("nan"), dtype=z.dtype, device=d)     # the padding is never used
    buf[..., :K] = z.to(d).reshape(B, K, H * W).transpose(1, 2)
    v = buf[..., :K].transpose(1, 2).reshape(B, K, H, W)
    assert v.data_ptr() == buf.data_ptr() and v.stride()[1:] == (1, W * pitch, pitch)
    return v


def run_kernels(case, table, z, window, batch, d):
    """canvas, labels, prob of the three kernels with the table cut into batches of ``batch``."""
    H, W, S, overlap, K, dtype, layout = case
    w1 = infer.window_1d(S, window)
    w1d = torch.from_numpy(w1.astype(np.float32)).to(d)
    ry = torch.from_numpy(infer.axis_weight(H, S, overlap, w1).astype(np.float32)).to(d)
    rx = torch.from_numpy(infer.axis_weight(W, S, overlap, w1).astype(np.float32)).to(d)
    N = len(table)
    nb = -(-N // batch)
    pad = np.zeros((nb * batch, 6), dtype=np.int32)
    pad[:N] = table
    tab = torch.from_numpy(pad).to(d)
    canvas = torch.zeros(K, H, W, device=d)
    for i in range(nb):
        zb = torch.full((batch, K, S, S), 7.0, dtype=z.dtype)          # padding slots: finite junk that must not count
        n = min(batch, N - i * batch)
        zb[:n] = z[i * batch:i * batch + n]
        region = infer.tile_region(pad[i * batch:(i + 1) * batch], S, H, W) if i % 2 else None      # both spellings
        infer.tile_blend(place(zb, layout, d), tab[i * batch:(i + 1) * batch], w1d, canvas, "prob" if layout == "prob" else "logits",
                         region)
    labels, prob = infer.tile_finish(canvas, ry, rx, 8, return_prob=True)
    return canvas, labels, prob


def check_against_reference(labels, prob, ref_labels, ref_prob, what):
    """The file's two bounds; prints each figure before asserting."""
    p = prob.double().cpu()
    err = float((p - ref_prob).abs().max())
    if ref_prob.shape[0] == 1:
        margin = (ref_prob[0] - 0.5).abs()
    else:
        top = ref_prob.topk(2, 0).values
        margin = top[0] - top[1]
    sure = margin >= MARGIN
    excluded = 1.0 - float(sure.double().mean())
    wrong = int((labels.cpu()[sure] != ref_labels[sure]).sum())
    print(f"{what}: max|dprob| {err:.3e}, excluded {100 * excluded:.4f} %, wrong labels {wrong}, "
          f"nonzero labels {100 * float((ref_labels != 0).double().mean()):.1f} %")
    assert err <= PROB_TOL
    assert excluded <= EXCLUDED_CAP
    assert wrong == 0
    assert labels.dtype == torch.uint8 and prob.dtype == torch.float32


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}-K{c[4]}-{str(c[5]).split('.')[-1]}-{c[6]}")
def test_blend_and_finish_match_the_fp64_reference(case):
    d = dev()
    table, z, ref_labels, ref_prob = case_ref(case)
    _, labels, prob = run_kernels(case, table, z, "gaussian", 16, d)
    check_against_reference(labels, prob, ref_labels, ref_prob, "gaussian")


def test_uniform_window():
    d = dev()
    case = CASES[1]
    table, z, ref_labels, ref_prob = case_ref(case, "uniform")
    _, labels, prob = run_kernels(case, table, z, "uniform", 16, d)
    check_against_reference(labels, prob, ref_labels, ref_prob, "uniform")


def test_finish_outputs_are_optional():
    d = dev()
    case = CASES[0]
    table, z, _, _ = case_ref(case)
    canvas, labels, prob = run_kernels(case, table, z, "gaussian", 16, d)
    H, W, S, overlap = case[:4]
    w1 = infer.window_1d(S, "gaussian")
    ry = torch.from_numpy(infer.axis_weight(H, S, overlap, w1).astype(np.float32)).to(d)
    rx = torch.from_numpy(infer.axis_weight(W, S, overlap, w1).astype(np.float32)).to(d)
    l2, p2 = infer.tile_finish(canvas, ry, rx, 8, return_prob=False)
    assert p2 is None and torch.equal(l2, labels)
    l3, p3 = infer.tile_finish(canvas, ry, rx, 8, return_prob=True, return_labels=False)
    assert l3 is None and torch.equal(p3, prob)
    # argmax: the lowest index wins a tie
    tie = torch.zeros(3, 4, 5, device=d)
    tie[1:] = 2.0
    one = torch.ones(5, device=d)
    lt, _ = infer.tile_finish(tie, one[:4].contiguous(), one, 1)
    assert (lt == 1).all()


def torch_gather(img, kind, table, S):
    """crop with edge clamp, / 255, then flip and rotate -- on the CPU, IEEE division by numpy."""
    if kind == 0:
        chw = torch.from_numpy(img.numpy().astype(np.float32) / np.float32(255.0)).permute(2, 0, 1)
    else:
        chw = img
    H, W = chw.shape[1:]
    ar = torch.arange(S)
    out = []
    for y0, x0, h, v, r, on in table.tolist():
        if not on:
            y0, x0, h, v, r, _ = table[0].tolist()
        crop = chw[:, (y0 + ar).clamp(0, H - 1)][:, :, (x0 + ar).clamp(0, W - 1)]
        if h:
            crop = crop.flip(-1)
        if v:
            crop = crop.flip(-2)
        out.append(torch.rot90(crop, -r, (-2, -1)))
    return torch.stack(out)


@pytest.mark.parametrize("H,W", [(80, 72), (20, 40), (33, 95)])
@pytest.mark.parametrize("kind", [0, 1], ids=["u8_hwc", "f32_chw"])
def test_gather_is_bitwise_the_torch_restatement(H, W, kind):
    d = dev()
    S = 32
    g = torch.Generator().manual_seed(H + W + kind)
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g) if kind == 0 else torch.rand(3, H, W, generator=g)
    table = infer.plan_tiles(H, W, S, 0.5, "d4")
    table = np.concatenate([table, np.zeros((3, 6), dtype=np.int32)])          # three padding slots
    table[-2] = (5, 7, 1, 1, 3, 0)                                             # inactive whatever else it says
    want = torch_gather(img, kind, torch.from_numpy(table), S)
    got = infer.tile_gather(img.to(d), torch.from_numpy(table).to(d), S)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(table), 3, S, S)
    assert torch.equal(got.cpu(), want)


def test_batch_independence_and_repeatability():
    """The 128 records of the 80x72 K = 3 case cut into batches of 1, 7 (ragged: inactive slots) and 128
    (one launch): bitwise equal canvases and label maps; the same call twice: bitwise equal."""
    d = dev()
    case = CASES[0]
    table, z, _, _ = case_ref(case)
    assert len(table) == 128
    runs = {}
    for batch in (1, 7, 128):
        runs[batch] = run_kernels(case, table, z, "gaussian", batch, d)
    again = run_kernels(case, table, z, "gaussian", 7, d)
    for batch in (1, 128):
        for a, b in zip(runs[batch], runs[7]):
            assert torch.equal(a, b), batch
    for a, b in zip(again, runs[7]):
        assert torch.equal(a, b)


def test_bad_arguments_raise_without_launching():
    from csu._lib import CSU_F32, CsuError, lib, ptr
    d = dev()
    S = 8
    tab = torch.from_numpy(infer.plan_tiles(8, 8, S, 0.5)).to(d)
    w1 = torch.ones(S, device=d)
    canvas = torch.zeros(33, 8, 8, device=d)
    z = torch.zeros(1, 33, S, S, device=d)
    L = lib()
    before = canvas.clone()
    with pytest.raises(CsuError, match="K <= 32"):
        infer.tile_blend(z, tab, w1, canvas)
    with pytest.raises(CsuError, match="K <= 32"):
        infer.tile_finish(canvas, w1, w1, 1)
    args = lambda S_, tab_: (1, S_, 8, 8, 2, 1, CSU_F32, ptr(z), 2 * S * S, S * S, 1, 0, tab_, ptr(w1), ptr(canvas), 0, 0, 8, 8,
                            None)  # noqa: E731
    assert L.csu_tile_blend(*args(0, ptr(tab))) == -1 and b"S, H and W" in L.csu_last_error_string()
    assert L.csu_tile_blend(*args(S, None)) == -1 and b"null" in L.csu_last_error_string()
    assert L.csu_tile_gather(1, 0, 8, 8, 1, ptr(z), ptr(tab), ptr(z), None) == -1
    assert L.csu_tile_gather(1, S, 8, 8, 1, ptr(z), None, ptr(z), None) == -1
    assert L.csu_tile_gather(1, S, 8, 8, 2, ptr(z), ptr(tab), ptr(z), None) == -1
    assert L.csu_tile_blend(129, S, 8, 8, 2, 1, CSU_F32, ptr(z), 2 * S * S, S * S, 1, 0, ptr(tab), ptr(w1), ptr(canvas), 0, 0, 8, 8,
                            None) == -1
    assert L.csu_tile_blend(1, S, 8, 8, 1, 0, 1, ptr(z), S * S, S * S, 1, 0, ptr(tab), ptr(w1), ptr(canvas), 0, 0, 8, 8, None) == -1   # bf16 PROB
    for region in ((0, 0, 9, 8), (4, 0, 4, 8), (-1, 0, 8, 8)):
        with pytest.raises(CsuError, match="region"):
            infer.tile_blend(z[:, :2], tab, w1, canvas[:2].contiguous(), "logits", region)
    assert L.csu_tile_finish(2, 8, 8, ptr(canvas), ptr(w1), ptr(w1), 1.0, None, None, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(canvas, before)


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
E2E = dict(overlap=0.5, tta=("identity", "hflip", "rot90"), batch_size=4)
_MODELS = {}


def e2e_model(head, d):
    from csu.model import CSWinTransformer
    if head not in _MODELS:
        torch.manual_seed(11)
        if head == "sigmoid":
            m = CSWinTransformer(img_size=64, split_size=[1, 2, 2, 2])
        else:
            m = CSWinTransformer(img_size=64, split_size=[1, 2, 2, 2], num_classes=3).set_head("logits")
        with torch.no_grad():
            # the initial head leaves every pixel on one side of the decision (logits -0.41 +- 0.08 at one class);
            # these weights give about 3/4 foreground at one class and a 28 / 72 % split of two of the three classes
            m.output.weight.copy_(4.0 * torch.randn(m.output.weight.shape, generator=torch.Generator().manual_seed(100)))
        _MODELS[head] = m.to(d).eval()
    return _MODELS[head]


def e2e_image():
    return torch.randint(0, 256, (160, 112, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(21))


@pytest.mark.parametrize("amp", [None, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("head", ["sigmoid", "logits"])
def test_predictor_matches_reference_predict(head, amp):
    d = dev()
    m = e2e_model(head, d)
    img = e2e_image().to(d)

    def fwd(x):
        with torch.no_grad(), torch.autocast("cuda", dtype=amp or torch.float32, enabled=amp is not None):
            return m(x)

    ref_labels, ref_prob = infer.reference_predict(fwd, img, 64, output="prob" if head == "sigmoid" else "logits",
                                                   return_prob=True, **E2E)
    pg = infer.SlidingWindowPredictor(m, amp_dtype=amp, graph=True, **E2E)
    labels, prob = pg.predict(img, return_prob=True)
    assert tuple(prob.shape) == ((1 if head == "sigmoid" else 3), 160, 112) and tuple(labels.shape) == (160, 112)
    check_against_reference(labels, prob, ref_labels.cpu(), ref_prob.cpu(), f"{head} {amp}")
    pe = infer.SlidingWindowPredictor(m, amp_dtype=amp, graph=False, **E2E)
    l2, p2 = pe.predict(img.cpu().numpy(), return_prob=True)          # numpy HWC in, eager forward
    assert torch.equal(l2, labels) and torch.equal(p2, prob)
    assert torch.equal(pg.predict(img), labels)                       # the cached graph replays; labels alone


@pytest.mark.parametrize("amp", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_one_tile_uniform_window_is_the_plain_forward_bitwise(amp):
    d = dev()
    m = e2e_model("sigmoid", d)
    img = torch.randint(0, 256, (64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(22)).to(d)
    x = torch.from_numpy(img.cpu().numpy().astype(np.float32) / np.float32(255.0)).permute(2, 0, 1)[None].contiguous().to(d)
    with torch.no_grad(), torch.autocast("cuda", dtype=amp or torch.float32, enabled=amp is not None):
        want = m(x)
    for graph in (True, False):
        p = infer.SlidingWindowPredictor(m, window="uniform", tta=("identity",), amp_dtype=amp, graph=graph)
        labels, prob = p.predict(img, return_prob=True)
        assert torch.equal(prob, want[0])
        assert torch.equal(labels, (want[0, 0] > 0.5).to(torch.uint8))
    # the fp32 CHW form of the same image gathers the same tile
    assert torch.equal(p.predict(x[0], return_prob=True)[1], want[0])


@pytest.mark.parametrize("K", [1, 3])
def test_evaluate_full_res_equals_numpy(K):
    from csu.data import SyntheticSegmentation
    d = dev()
    m = e2e_model("sigmoid" if K == 1 else "logits", d)
    ds = SyntheticSegmentation(2, 96, seed=5, num_classes=K)
    pairs = [ds[i] for i in range(2)]
    p = infer.SlidingWindowPredictor(m, overlap=0.5, tta=("identity", "vflip"), batch_size=8)
    dice, iou = infer.evaluate_full_res(p, pairs, K)
    sm = 1e-6
    if K == 1:
        ds_, us = [], []
        for img, t in pairs:
            pred = p.predict(img).cpu().numpy().astype(np.float64).reshape(-1)
            tt = (t.numpy().reshape(-1) > 0.5).astype(np.float64)
            inter = (pred * tt).sum()
            ds_.append((2 * inter + sm) / (pred.sum() + tt.sum() + sm))
            us.append((inter + sm) / (pred.sum() + tt.sum() - inter + sm))
        want = (np.mean(ds_), np.mean(us))
    else:
        I, P, T = np.zeros(K), np.zeros(K), np.zeros(K)
        for img, t in pairs:
            pred = p.predict(img).cpu().numpy().reshape(-1)
            tt = t.numpy().reshape(-1)
            for c in range(K):
                I[c] += ((pred == c) & (tt == c)).sum()
                P[c] += (pred == c).sum()
                T[c] += (tt == c).sum()
        seen = P + T > 0
        want = (((2 * I + sm) / (P + T + sm))[seen].mean(), ((I + sm) / (P + T - I + sm))[seen].mean())
    print("full-res dice/iou", (dice, iou), "numpy", want)
    assert abs(dice - want[0]) <= 1e-12 and abs(iou - want[1]) <= 1e-12


def test_predict_inside_ema_applied():
    """Inside opt.ema.applied() the (captured) predictor sees the averaged weights: bitwise the result of a
    second instance loaded with ema.model_state_dict(); afterwards the raw weights' result again."""
    from csu.model import CSWinTransformer
    from csu.train import bce_loss, make_optimizer, train_step
    d = dev()
    m = copy.deepcopy(e2e_model("sigmoid", d)).train()
    opt = make_optimizer(m, lr=1e-3, ema_decay=0.5, ema_warmup=False)
    g = torch.Generator().manual_seed(31)
    for _ in range(2):
        x = torch.rand(2, 3, 64, 64, generator=g).to(d)
        t = (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float().to(d)
        train_step(m, x, t, bce_loss, opt, amp_dtype=torch.bfloat16)
    img = e2e_image()[:100, :90].contiguous()
    p = infer.SlidingWindowPredictor(m, amp_dtype=torch.bfloat16, tta=("identity", "transpose"), batch_size=4)
    raw = p.predict(img, return_prob=True)[1]
    with opt.ema.applied():
        got = p.predict(img, return_prob=True)[1]
    back = p.predict(img, return_prob=True)[1]
    m2 = CSWinTransformer(img_size=64, split_size=[1, 2, 2, 2]).to(d)
    m2.load_state_dict(opt.ema.model_state_dict())
    want = infer.SlidingWindowPredictor(m2, amp_dtype=torch.bfloat16, tta=("identity", "transpose"), batch_size=4).predict(
        img, return_prob=True)[1]
    assert torch.equal(got, want)
    assert torch.equal(back, raw) and not torch.equal(got, raw)
