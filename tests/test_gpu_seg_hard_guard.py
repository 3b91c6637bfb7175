"""Guard-band cases of the hard-example loss (README "Testing"): csu_seg_hard_* with a selection and csu_kth_largest
stay inside their outputs, the keys buffer and a workspace of exactly the claimed size, write all of their outputs,
initialise every workspace field they read (the payloads are poisoned) and let nothing outside an input reach a
result: the label map is filled with 254 around its payload (neither a class nor ignore_index), the logits' guards
and padding hold NaN."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from guard_alloc import GuardedAlloc
from test_gpu_guard_bands import _place_guarded, dev, finite, gin, guarded, mod, verify
from test_gpu_seg_ce import LAYOUTS
from test_seg_ce import UPSTREAM, make_case
from test_seg_hard import (HARD_PARAM_SETS, MARGIN, check_grad, check_loss, check_tau, make_hard_criterion, ref_hard_loss_grad,
                           selection_margin)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(2, 5, 33, 33), (3, 5, 37, 41)])
def test_forward_and_backward_with_a_selection(shape, layout, dtype, monkeypatch):
    L = mod("_lib").lib()
    d = dev()
    B, K, H, W = shape
    ps, gamma, rho = HARD_PARAM_SETS[1], 2.0, 0.3
    z, t = make_case(shape, dtype=dtype)
    assert selection_margin(z, t, ps[4], gamma, rho) >= MARGIN
    lref, gref, sref, info = ref_hard_loss_grad(z, t, ps, True, gamma, rho)
    for lab in (torch.int64, torch.uint8):
        ga = GuardedAlloc()
        za = _place_guarded(ga, z, layout, d)
        td = gin(ga, t.to(lab), d, fill=254)
        crit = make_hard_criterion(K, ps, True, gamma, rho)
        crit(z.to(d), t.to(d))          # the fraction's device scalar and the class weights are made outside the guarded block
        with guarded(monkeypatch, "ops", "losses", registry=ga):
            loss, stats = crit.loss_stats(za, td)
            (loss * UPSTREAM).backward()
        verify(ga, [loss, stats, crit.last_terms], ws=L.csu_seg_hard_workspace(B, K, H * W))
        assert 4 * B * H * W in ga.sizes(torch.float32), "the keys buffer: one float per pixel"
        finite(loss, stats, crit.last_terms, za.grad)
        assert za.grad.dtype == dtype
        check_loss(loss, lref)
        check_grad(za.grad, gref, bf16=dtype == torch.bfloat16)
        check_tau(crit.last_terms[2], info)
        assert float(crit.last_terms[3]) == info["k"] and torch.equal(stats.cpu(), sref)


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_kth_largest(n, monkeypatch):
    ops, L = mod("ops"), mod("_lib").lib()
    d = dev()
    g = torch.Generator().manual_seed(n)
    keys = torch.rand(n, generator=g)
    keys[::5] = -1.0
    ga = GuardedAlloc()
    kd, rho = gin(ga, keys, d), gin(ga, torch.tensor([0.4]), d)
    with guarded(monkeypatch, "ops", registry=ga):
        out = ops.kth_largest(kd, rho)
    verify(ga, [out], ws=L.csu_kth_largest_workspace(n))
    finite(out)
    live = keys[keys >= 0]
    k = max(1, int(float(torch.tensor(0.4)) * live.numel() // 1)) if live.numel() else 0
    want = float(torch.sort(live, descending=True).values[k - 1]) if k else 0.0
    assert float(out[0]) == want and int(out[3]) == k and int(out[4]) == live.numel()
