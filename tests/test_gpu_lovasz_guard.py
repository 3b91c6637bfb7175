"""Guard-band cases of the Lovasz-Softmax loss (README "Testing"): csu_sort_pairs and csu_seg_lovasz_* stay inside
their outputs, the sorted keys / values / psi buffers and workspaces of exactly the claimed sizes, write all of their
outputs, initialise every workspace field they read (the payloads are poisoned) and let nothing outside an input
reach a result: the label map is filled with 254 around its payload (neither a class nor ignore_index), the logits'
guards and padding hold NaN."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from guard_alloc import GuardedAlloc
from test_gpu_guard_bands import _place_guarded, dev, finite, gin, guarded, mod, verify
from test_gpu_lovasz import check_order_and_psi, class_list, pixel_errors, run_debug
from test_gpu_seg_ce import LAYOUTS
from test_gpu_sort_pairs import reference
from test_lovasz import CLASS_MODES, LV_PARAM_SETS, check_grad, check_loss, ref_lovasz_loss_grad
from test_seg_ce import IGNORE, UPSTREAM, make_case


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (2, 5, 33, 33)])
def test_forward_and_backward(shape, layout, dtype, per_image, monkeypatch):
    L = mod("_lib").lib()
    d = dev()
    B, K, H, W = shape
    ps = LV_PARAM_SETS[1]
    z, t = make_case(shape, dtype=dtype)
    for mode, lab in zip(CLASS_MODES, (torch.int64, torch.uint8, torch.int64)):
        cls = class_list(mode, K)
        lref, gref, sref, _ = ref_lovasz_loss_grad(z, t, ps, per_image, mode, per_image)
        e64, e32 = pixel_errors(z.double(), t, cls), pixel_errors(z.float(), t, cls)
        live = (t != IGNORE).reshape(1, B, -1).expand_as(e64)
        e_tol = 10.0 * float((e32.double() - e64)[live].abs().max())
        ga = GuardedAlloc()
        za = _place_guarded(ga, z, layout, d)
        td = gin(ga, t.to(lab), d, fill=254)
        with guarded(monkeypatch, "ops", "losses", registry=ga):
            loss, terms, stats, skeys, svals, psi = run_debug(za, td, ps, mode, per_image, K, d)
            (loss * UPSTREAM).backward()
        mask = sum(1 << c for c in cls)
        verify(ga, [loss, terms, stats, skeys, svals, psi], ws=L.csu_seg_lovasz_workspace(B, K, H * W, mask, int(per_image)))
        assert ga.sizes(torch.int32).count(4 * len(cls) * B * H * W) == 2, "sorted keys and values: one word per (class, pixel)"
        finite(loss, terms, stats, psi, za.grad)
        assert za.grad.dtype == dtype
        check_order_and_psi(skeys, svals, psi, t, cls, mode, per_image, e64.numpy(), e_tol)
        check_loss(loss, lref)
        check_grad(za.grad, gref, shape, bf16=dtype == torch.bfloat16)
        assert torch.equal(stats.cpu(), sref)


@pytest.mark.parametrize("bits", [9, 31, 32])
@pytest.mark.parametrize("n,segments", [(1, 1), (257, 3), (4099, 2)])
def test_sort_pairs(n, segments, bits, monkeypatch):
    ops, L = mod("ops"), mod("_lib").lib()
    d = dev()
    g = torch.Generator().manual_seed(n)
    keys = torch.randint(-(1 << 31), 1 << 31, (n * segments,), generator=g).to(torch.int32)
    vals = torch.arange(n * segments, dtype=torch.int32)
    ga = GuardedAlloc()
    kd, vd = gin(ga, keys, d, fill=-1), gin(ga, vals, d, fill=-1)
    with guarded(monkeypatch, "ops", registry=ga):
        ko, vo = ops.sort_pairs(kd, vd, segments, bits)
    verify(ga, [ko, vo], ws=L.csu_sort_pairs_workspace(segments, n))
    wk, wv = reference(keys.numpy().view(np.uint32), vals.numpy().view(np.uint32), segments, bits)
    assert np.array_equal(ko.cpu().numpy().view(np.uint32), wk) and np.array_equal(vo.cpu().numpy().view(np.uint32), wv)
