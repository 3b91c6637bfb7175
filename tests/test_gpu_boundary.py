"""The boundary loss on the MI355X: csu_signed_distance against csu.boundary's fp64 reference, csu_seg_bd_* against
the fp64 restatement of tests/test_boundary.py (loss, terms, gradient under a non-unit upstream factor, exact hard
sums) in every layout, logits dtype and label dtype, the exact equalities with csu_seg_ce_*, and BoundarySegLoss end
to end: against the CPU path, inside a captured graph whose weight changes between replays, and in train_model.

Distance maps.  Unit spacing: squared index distances are exact in int32 and the kernel takes the square root and
the difference min(sy, sx) - d in fp64 as the reference does, so the maps equal the reference rounded to fp32.
Spacing (0.7, 1.3) (fp32 path): d is within test_gpu_surface_metrics.py's F32_RTOL = 4e-7 of the reference (its
docstring: about 1.5e-7, taken with a factor of a little over two); inside a class phi = 0.7 - d, and the smallest
d above 0.7 is 1.3, so the cancellation costs at most a factor 1.3 / 0.6 < 2.2 on 1.5e-7: still inside F32_RTOL.
The inner border (d = 0.7 exactly) must be 0 in both: the zero sets are compared as sets.

Loss tolerances are those of tests/test_boundary.py (ten times torch's own fp32 error against fp64, measured at
these shapes; bf16 gradients get one bf16 rounding, rtol 2**-8, on top)."""
import copy

import numpy as np
import pytest
import torch

from test_boundary import (BD_LOSS_TOL, COMBOS, SHAPES, SMOOTH, check_bd_grad, check_bd_loss, label_maps, make_criterion,
                           make_phi, ref_bd_loss_grad)
from test_gpu_seg_ce import LAYOUTS, _multiclass_setup, dev, place
from test_gpu_surface_metrics import F32_RTOL
from test_seg_ce import IGNORE, UPSTREAM, make_case

pytestmark = pytest.mark.gpu

K = 5
SPACINGS = [(1.0, 1.0), (0.7, 1.3)]
# name -> (B, H, W): degenerate; ragged, under one column block, a single-class image; rows longer than the block's
# stride; 16 column segments with carries between them; the LDS limit (two rows of 16383 uint16 each)
MAP_CASES = {"one_pixel": (2, 1, 1), "ragged": (3, 37, 53), "wide": (1, 9, 1100), "tall": (1, 1100, 9),
             "lds_limit": (1, 2, 16383)}
_MAPS, _MAP_REFS, _REFS = {}, {}, {}


def labels_of(name):
    if name not in _MAPS:
        _MAPS[name] = label_maps(len(name) + MAP_CASES[name][2], MAP_CASES[name], K)
    return _MAPS[name]


def map_ref(name, spacing, clip=None):
    """The fp64 reference of a case, made once and left unchanged."""
    key = (name, spacing, clip)
    if key not in _MAP_REFS:
        from csu.boundary import reference_signed_distance_map
        _MAP_REFS[key] = reference_signed_distance_map(labels_of(name), K, spacing, clip)
    return _MAP_REFS[key]


def check_maps(got, want, spacing):
    assert got.dtype == torch.float32 and got.shape == want.shape
    got = got.cpu()
    if spacing[0] == spacing[1]:
        assert torch.equal(got, want.float())
    else:
        assert torch.equal(got == 0, want == 0)
        torch.testing.assert_close(got.double(), want, rtol=F32_RTOL, atol=0)


def test_map_cases_are_what_they_claim():
    t = labels_of("ragged")
    assert t.dtype == torch.int64 and int((t == IGNORE).sum()) > 0 and int((t == K - 1).sum()) == 0      # class 4 absent
    assert int((t[0] == t[0, 0, 0]).sum()) == 37 * 53                                                    # one class fills image 0
    r = map_ref("ragged", (1.0, 1.0))
    assert float(r[0].abs().max()) == 0.0 and float(r[:, 4].abs().max()) == 0.0
    assert float(r[1:, :4].min()) < -1.0 and float(r[1:, :4].max()) > 1.0
    assert sorted(labels_of("lds_limit").unique().tolist()) == [0, 1, 2, 3, IGNORE]


@pytest.mark.parametrize("spacing", SPACINGS, ids=["unit", "0.7x1.3"])
@pytest.mark.parametrize("name", list(MAP_CASES))
def test_signed_distance_map_vs_reference(name, spacing):
    from csu.boundary import signed_distance_map
    d = dev()
    t = labels_of(name)
    want = map_ref(name, spacing)
    for lab in (torch.int64, torch.uint8):
        got = signed_distance_map(t.to(d).to(lab), K, spacing)
        err = float(((got.cpu().double() - want).abs() / want.abs().clamp(min=1e-300)).max())
        print(f"{name} {spacing} {lab}: max rel err {err:.2e}, range [{float(want.min()):.3f}, {float(want.max()):.3f}]")
        check_maps(got, want, spacing)
    one = signed_distance_map(t[0].to(d), K, spacing)                 # an (H, W) map
    assert one.shape == (K,) + tuple(t.shape[1:]) and torch.equal(one, got[0])


@pytest.mark.parametrize("spacing", SPACINGS, ids=["unit", "0.7x1.3"])
def test_clip_and_class_chunks(spacing, monkeypatch):
    from csu import boundary
    d = dev()
    t = labels_of("ragged").to(d)
    full = boundary.signed_distance_map(t, K, spacing)
    for clip in (0.6, 3.0):        # under one step of the coarser axis; a few pixels
        got = boundary.signed_distance_map(t, K, spacing, clip=clip)
        check_maps(got, map_ref("ragged", spacing, clip), spacing)
        assert torch.equal(got, full.clamp(-clip, clip)) and float(got.abs().max()) == np.float32(clip)
    # classes passed in chunks, by the caller and by the workspace budget
    assert torch.equal(boundary.signed_distance_map(t, K, spacing, classes=(1, 4)), full[:, 1:4])
    assert torch.equal(boundary.signed_distance_map(t, K, spacing, classes=(4, 5)), full[:, 4:])
    for pairs in (1, 2, 7, 10):        # one class a call; two; all five of one image; of two images
        monkeypatch.setattr(boundary, "WORKSPACE_BUDGET", pairs * 4 * 37 * 53)
        assert torch.equal(boundary.signed_distance_map(t, K, spacing), full), pairs


def test_maps_bitwise_repeatable_and_independent_of_the_batching():
    from csu.boundary import signed_distance_map
    d = dev()
    for name in ("ragged", "tall"):
        t = labels_of(name).to(d)
        for spacing in SPACINGS:
            a = signed_distance_map(t, K, spacing, clip=None)
            assert torch.equal(a, signed_distance_map(t, K, spacing))
            parts = [signed_distance_map(t[i:i + 1], K, spacing) for i in range(t.shape[0])]
            assert torch.equal(a, torch.cat(parts))
            if t.shape[0] > 2:
                assert torch.equal(a, torch.cat([signed_distance_map(t[:2], K, spacing), parts[2]]))


def test_sizes_past_the_lds_limit_raise():
    from csu import ops
    from csu._lib import CsuError, lib
    from csu.boundary import signed_distance_map
    d = dev()
    for shape in ((1, 1, 16384), (1, 16384, 1)):
        t = torch.zeros(shape, dtype=torch.uint8, device=d)
        with pytest.raises(ValueError, match="16383"):
            signed_distance_map(t, 2)
        with pytest.raises(ValueError, match="16383"):
            ops.signed_distance(t, 0, 2, torch.empty(1, 2, *shape[1:], device=d))
        assert lib().csu_signed_distance_workspace(1, 2, shape[1], shape[2]) == 0
    with pytest.raises(CsuError):
        ops.signed_distance(torch.zeros(1, 4, 4, dtype=torch.uint8), 0, 2, torch.empty(1, 2, 4, 4))
    with pytest.raises(CsuError, match="clip"):         # refused by the C entry point before any launch
        ops.signed_distance(torch.zeros(1, 4, 4, dtype=torch.uint8, device=d), 0, 2, torch.empty(1, 2, 4, 4, device=d), clip=0.0)


# ---- the fused loss ----------------------------------------------------------------------------

def ref(shape, dtype, combo, bg, per_sample):
    """(z, t, phi, loss, grad, terms, A, stats) on the CPU, made once per case and left unchanged."""
    key = (shape, dtype, COMBOS.index(combo), bg, per_sample)
    if key not in _REFS:
        z, t = make_case(shape, dtype=dtype)
        phi = make_phi(shape)
        _REFS[key] = (z, t, phi) + ref_bd_loss_grad(z, t, phi, combo, bg, per_sample)
    return _REFS[key]


def run_seg_bd(za, t, phi, combo, bg, per_sample, d):
    from csu import ops
    w = torch.full((1,), combo[2], dtype=torch.float32, device=d)
    rows = za.shape[0] if per_sample else 1
    return ops.seg_bd(za, t, phi, w, (combo[0], combo[1], 0.5, 0.5, SMOOTH), None, IGNORE, rows, True, bg, True)


@pytest.mark.parametrize("per_sample", [False, True], ids=["rows1", "rowsB"])
@pytest.mark.parametrize("bg", [False, True], ids=["fg", "all"])
@pytest.mark.parametrize("combo", COMBOS, ids=["ce_dice_bd", "bd_alone", "w_bd_0"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_seg_bd_vs_fp64(shape, layout, dtype, combo, bg, per_sample):
    d = dev()
    z, t, phi, lref, gref, tref, scale, sref = ref(shape, dtype, combo, bg, per_sample)
    phid = phi.to(d)
    for lab in (torch.int64, torch.uint8):
        za = place(z, layout, d)
        loss, terms, stats = run_seg_bd(za, t.to(d).to(lab), phid, combo, bg, per_sample, d)
        (loss * UPSTREAM).backward()
        g = za.grad.double().cpu()
        print(f"{lab}: loss {float(loss):.9g} ref {float(lref):.9g}  BD {float(terms[1]):.9g} ref {float(tref[1]):.9g} "
              f"A {scale:.4g}  grad err / max|g_ref| {float((g - gref).abs().max() / gref.abs().max()):.2e}")
        assert za.grad.dtype == dtype and terms.dtype == torch.float32 and not terms.requires_grad
        check_bd_loss(loss, terms, lref, tref, scale, combo[2])
        check_bd_grad(za.grad, gref, bf16=dtype == torch.bfloat16)
        assert stats.dtype == torch.float64 and torch.equal(stats.cpu(), sref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (3, 5, 37, 41), (2, 32, 8, 8), (2, 6, 300, 333)])
def test_zero_weight_equals_seg_ce(shape, layout, dtype):
    """w_bd = 0 and finite phi: the loss and dz are those of csu_seg_ce_* on the same inputs, bit for bit."""
    from csu import ops
    d = dev()
    z, t = make_case(shape, dtype=dtype)
    phid, td = make_phi(shape).to(d), t.to(d)
    prm = (0.5, 1.0, 0.3, 0.7, SMOOTH)
    for rows in (1, shape[0]):
        for bg in (False, True):
            za, zb = place(z, layout, d), place(z, layout, d)
            la, sa = ops.seg_ce(za, td, prm, None, IGNORE, rows, False, True)
            lb, terms, sb = ops.seg_bd(zb, td, phid, torch.zeros(1, device=d), prm, None, IGNORE, rows, False, bg, True)
            (la * UPSTREAM).backward()
            (lb * UPSTREAM).backward()
            assert torch.equal(la, lb) and torch.equal(terms[0], la) and torch.equal(sa, sb)
            assert torch.equal(za.grad, zb.grad)
            assert bool(torch.isfinite(terms[1])) and float(terms[1]) != 0.0


def test_all_ignored_batch_is_zero_not_nan():
    d = dev()
    z, _ = make_case((2, 3, 7, 9))
    t = torch.full((2, 7, 9), IGNORE, dtype=torch.int64, device=d)
    phid = make_phi((2, 3, 7, 9)).to(d)
    for combo in COMBOS:
        for layout in LAYOUTS:
            za = place(z, layout, d)
            loss, terms, stats = run_seg_bd(za, t, phid, combo, False, False, d)
            loss.backward()
            assert float(loss.detach()) == 0.0 and float(terms.abs().max()) == 0.0 and float(stats.abs().max()) == 0.0
            assert float(za.grad.abs().max()) == 0.0 and not bool(torch.isnan(za.grad).any())


def test_seg_bd_bitwise_repeatable():
    d = dev()
    shape = (2, 6, 300, 333)
    z, t = make_case(shape)
    phid, td = make_phi(shape).to(d), t.to(d)
    for layout in LAYOUTS:
        res = []
        for _ in range(2):
            za = place(z, layout, d)
            loss, terms, stats = run_seg_bd(za, td, phid, COMBOS[0], False, True, d)
            (loss * UPSTREAM).backward()
            res.append((loss.detach(), terms, stats, za.grad))
        for a, b in zip(*res):
            assert torch.equal(a, b)


def test_ops_seg_bd_argument_checks():
    from csu import ops
    from csu._lib import CsuError
    d = dev()
    z = torch.randn(2, 3, 4, 4, device=d)
    t = torch.zeros(2, 4, 4, dtype=torch.int64, device=d)
    phi, w = torch.zeros(2, 3, 4, 4, device=d), torch.ones(1, device=d)
    prm = (1.0, 1.0, 0.5, 0.5, 0.5)
    with pytest.raises(CsuError):
        ops.seg_bd(z.cpu(), t.cpu(), phi.cpu(), w.cpu(), prm)
    for a, b, p, v, q, kw in ((z.double(), t, phi, w, prm, {}), (z, t.float(), phi, w, prm, {}), (z, t[:1], phi, w, prm, {}),
                              (z, t, phi[:, :2], w, prm, {}), (z, t, phi.double(), w, prm, {}), (z, t, phi, w.double(), prm, {}),
                              (z, t, phi, torch.ones(2, device=d), prm, {}), (z, t, phi, w, prm[:4], {}),
                              (z, t, phi, w, prm, dict(rows=3)), (z[:, :1], t, phi[:, :1], w, prm, {})):
        with pytest.raises(ValueError):
            ops.seg_bd(a, b, p, v, q, **kw)
    with pytest.raises(CsuError, match="smooth"):
        ops.seg_bd(z, t, phi, w, (1.0, 1.0, 0.5, 0.5, 0.0))
    with pytest.raises(ValueError):
        ops.seg_bd(torch.randn(2, 33, 4, 4, device=d), t, torch.zeros(2, 33, 4, 4, device=d), w, prm)


# ---- end to end --------------------------------------------------------------------------------

@pytest.mark.parametrize("spacing,clip", [((1.0, 1.0), None), ((0.7, 1.3), 4.0)], ids=["unit", "0.7x1.3_clip4"])
def test_criterion_vs_cpu_path(spacing, clip):
    """BoundarySegLoss with maps made from the target at (3,5,37,41), GPU against the CPU path: the maps agree as in
    check_maps; both losses are within the tolerance of the fp64 restatement on the CPU maps, so within twice that
    of each other; the gradients likewise.  (With spacing (0.7, 1.3) the GPU's maps are within F32_RTOL = 4e-7 of the
    CPU's, a quarter of BD_LOSS_TOL relative to the same sum of |p phi|.)"""
    d = dev()
    shape = (3, 5, 37, 41)
    z, _ = make_case(shape)
    t = label_maps(11, (3, 37, 41), 5)
    from csu.boundary import reference_signed_distance_map, signed_distance_map
    check_maps(signed_distance_map(t.to(d), 5, spacing, clip), reference_signed_distance_map(t, 5, spacing, clip), spacing)
    for combo, bg, per_sample in ((COMBOS[0], False, False), (COMBOS[1], True, True)):
        out = []
        for dv in (torch.device("cpu"), d):
            crit = make_criterion(5, combo, bg, per_sample, spacing=spacing, clip=clip)
            za = z.detach().clone().to(dv).requires_grad_(True)
            loss, stats = crit.loss_stats(za, t.to(dv))
            (loss * UPSTREAM).backward()
            out.append((loss.detach().cpu(), crit.last_terms.cpu(), stats.cpu(), za.grad.cpu()))
        phi = signed_distance_map(t, 5, spacing, clip)
        lref, gref, tref, scale, sref = ref_bd_loss_grad(z, t, phi, combo, bg, per_sample)
        for loss, terms, stats, grad in out:
            check_bd_loss(loss, terms, lref, tref, scale, combo[2])
            check_bd_grad(grad, gref)
            assert torch.equal(stats, sref)
        torch.testing.assert_close(out[0][0], out[1][0], rtol=0, atol=2 * BD_LOSS_TOL * (abs(float(tref[0])) + combo[2] * scale))


def test_33_classes_take_the_torch_route_on_the_device():
    d = dev()
    shape = (2, 33, 9, 11)
    z, t = make_case(shape)
    phi = make_phi(shape)
    lref, gref, tref, scale, sref = ref_bd_loss_grad(z, t, phi, COMBOS[0], False, False)
    crit = make_criterion(33, COMBOS[0], False, False)
    za = z.to(d).requires_grad_(True)
    loss, stats = crit.loss_stats(za, t.to(d), dist=phi.to(d))
    (loss * UPSTREAM).backward()
    assert loss.is_cuda and crit.last_terms.is_cuda
    check_bd_loss(loss, crit.last_terms, lref, tref, scale, COMBOS[0][2])
    check_bd_grad(za.grad, gref)
    assert torch.equal(stats.cpu(), sref)
    maps = crit(za.detach(), t.to(d))                                  # 33 maps: two class chunks of the kernel
    assert bool(torch.isfinite(maps))


def test_captured_graph_follows_the_weight():
    """Maps + loss + backward captured once; after set_boundary_weight the replay equals the eager result with that
    weight bit for bit (the kernels are deterministic and read the weight from the device)."""
    d = dev()
    shape = (3, 5, 37, 41)
    z, _ = make_case(shape, dtype=torch.bfloat16)
    labels = [label_maps(30 + i, (3, 37, 41), 5).to(d) for i in range(2)]
    crit = make_criterion(5, COMBOS[0], False, False, clip=6.0)

    def step(zs, ts):
        loss = crit(zs, ts)
        (g,) = torch.autograd.grad(loss * UPSTREAM, zs)
        return loss.detach(), g, crit.last_terms

    zs = place(z, "class_last_padded", d)
    ts = labels[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(zs, ts)                                                   # warm-up: the weight's device scalar exists
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(zs, ts)
    for w, lab in ((0.5, labels[0]), (0.05, labels[1]), (2.0, labels[0])):
        crit.set_boundary_weight(w)
        ts.copy_(lab)
        graph.replay()
        got = [v.clone() for v in captured]
        want = step(zs, lab)
        for a, b in zip(got, want):
            assert torch.equal(a, b), w
        torch.testing.assert_close(got[0], got[2][0] + w * got[2][1], rtol=1e-5, atol=1e-5)
    assert crit.boundary_weight == 2.0


def test_train_model_graphed_equals_eager_with_a_ramp():
    """train_model on test_gpu_seg_ce's 3-class setup with ce_dice_boundary_loss and a ramp over two epochs: the
    captured step (maps, loss and per-class sums inside the graph, the weight changed between epochs without a
    re-capture) == graph=False, the boundary_weight history included (that test's tolerances)."""
    from csu.losses import ce_dice_boundary_loss, linear_ramp
    from csu.train import _graph_cache, make_optimizer, train_model
    d, m0, train, test = _multiclass_setup()
    hs, ps = [], []
    for graph in (True, False):
        m = copy.deepcopy(m0).to(d)
        opt = make_optimizer(m)
        crit = ce_dice_boundary_loss(3, schedule=linear_ramp(0.2, 0.5, 1.0), clip=8.0)
        hs.append(train_model(m, train, test, crit, opt, None, d, num_epochs=2, verbose=False, amp_dtype=torch.bfloat16,
                              graph=graph))
        ps.append([p.detach().clone() for p in m.parameters()])
        if graph:
            keys = [k for k in _graph_cache(m) if k[0] == "train"]
            assert len(keys) == 1 and keys[0][4] is crit          # one captured step served both weights
    assert hs[0]["boundary_weight"] == [0.2, 0.7] and set(hs[0]) == set(hs[1])
    for k in hs[0]:
        np.testing.assert_allclose(hs[0][k], hs[1][k], rtol=1e-5, atol=1e-6, err_msg=k)
    assert np.isfinite(hs[0]["train_loss"]).all() and hs[0]["train_loss"][0] != hs[0]["train_loss"][1]
    for a, b in zip(*ps):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
