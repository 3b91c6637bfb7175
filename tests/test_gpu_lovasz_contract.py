"""csu.ops.seg_lovasz (_SegLovaszFn) under the call patterns autograd allows -- the patterns of
tests/test_gpu_autograd_contract.py for an op with one differentiable input and no parameters (the table of
tests/contract_cases.py is fixed, so the op is covered here): strided and offset logits; an expanded, a
non-contiguous and a cast upstream gradient; torch.autograd.grad; a second backward with retain_graph; an existing
.grad; micro-batches; a no_grad forward between; a user stream; create_graph=True (first-order values, as
_SegCEFn); and no deferred state left behind (the autouse fixture of the contract file, imported)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_autograd_contract import no_state_left_behind  # noqa: F401  (autouse: pattern J)
from test_gpu_seg_ce import LAYOUTS, dev, place
from test_lovasz import LV_PARAM_SETS, check_grad as _check_grad, check_loss, ref_lovasz_loss_grad
from test_seg_ce import IGNORE, SMOOTH, UPSTREAM, class_weights, make_case

SHAPE, MODE, PS = (2, 3, 7, 9), "present", LV_PARAM_SETS[1]
_CASES = {}


def check_grad(g, g_ref):
    _check_grad(g, g_ref, SHAPE)


def case(seed=0):
    """(z, t, fp64 loss, fp64 gradient under UPSTREAM) of one seed, made once."""
    if seed not in _CASES:
        z, t = make_case(SHAPE, seed=3100 + seed)
        _CASES[seed] = (z, t) + ref_lovasz_loss_grad(z, t, PS, False, MODE, False)[:2]
    return _CASES[seed]


def call(za, t, stats=False):
    from csu import ops
    d = za.device
    ce, tv, alpha, beta, _, bg, lv = PS
    w = torch.full((1,), lv, device=d)
    cw = torch.tensor(class_weights(SHAPE[1]), device=d)
    return ops.seg_lovasz(za, t.to(d), w, (ce, tv, alpha, beta, SMOOTH), None, True, False, cw, IGNORE, 1, bg,
                          with_stats=stats)


def plain(seed=0):
    """The anchor: one plain forward / backward; (loss, grad)."""
    z, t, _, _ = case(seed)
    za = place(z, "nchw", dev())
    loss = call(za, t)[0]
    (loss * UPSTREAM).backward()
    return loss.detach(), za.grad.clone()


def test_plain_matches_the_reference_and_terms_do_not_require_grad():
    z, t, lref, gref = case()
    loss, g = plain()
    check_loss(loss, lref)
    check_grad(g, gref)
    za = place(z, "nchw", dev())
    out = call(za, t, stats=True)
    assert out[0].requires_grad and not out[1].requires_grad and not out[2].requires_grad


@pytest.mark.parametrize("layout", LAYOUTS + ["offset", "sliced_batch"])
def test_strided_and_offset_logits(layout):
    d = dev()
    z, t, lref, gref = case()
    if layout == "offset":
        buf = torch.zeros(z.numel() + 3, device=d)
        za = buf[3:].view(SHAPE).copy_(z).detach().requires_grad_(True)
    elif layout == "sliced_batch":      # every other image of a larger batch: a batch stride twice the dense one
        big = torch.zeros((4,) + SHAPE[1:], device=d)
        big[::2] = z.to(d)
        za = big[::2].detach().requires_grad_(True)
        assert not za.is_contiguous()
    else:
        za = place(z, layout, d)
    loss = call(za, t)[0]
    (loss * UPSTREAM).backward()
    check_loss(loss, lref)
    check_grad(za.grad, gref)
    assert za.grad.shape == za.shape


@pytest.mark.parametrize("kind", ["expanded", "noncontig", "float64", "bfloat16"])
def test_upstream_gradient_forms(kind):
    d = dev()
    z, t, _, _ = case()
    loss0, g0 = plain()
    za = place(z, "nchw", d)
    loss = call(za, t)[0]
    up = {"expanded": torch.tensor([UPSTREAM], device=d).expand(4)[2],
          "noncontig": torch.tensor([[UPSTREAM, 7.0], [5.0, 3.0]], device=d).t()[0, 0],
          "float64": torch.tensor(UPSTREAM, device=d, dtype=torch.float64),
          "bfloat16": torch.tensor(UPSTREAM, device=d, dtype=torch.bfloat16)}[kind]
    if kind in ("expanded", "noncontig", "float64"):
        loss.backward(up.to(loss.dtype) if kind == "float64" else up)
        assert torch.equal(za.grad, g0)
    else:       # the gradient of the other float dtype reaches the op through a cast of the loss
        (loss.to(torch.bfloat16) * up).backward()
        # the three terms of dz cancel in its small elements, so another upstream factor rounds them differently:
        # the gradient tolerance of the op's own test, absolute against the largest element
        check_grad(za.grad, (g0 * (float(up) / UPSTREAM)).double().cpu())


def test_autograd_grad_equals_backward():
    z, t, _, _ = case()
    _, g0 = plain()
    za = place(z, "nchw", dev())
    (g,) = torch.autograd.grad(call(za, t)[0] * UPSTREAM, za)
    assert torch.equal(g, g0) and za.grad is None


def test_second_backward_with_retain_graph_and_an_existing_grad():
    z, t, _, _ = case()
    _, g0 = plain()
    za = place(z, "nchw", dev())
    loss = call(za, t)[0] * UPSTREAM
    loss.backward(retain_graph=True)
    assert torch.equal(za.grad, g0)
    loss.backward()                      # onto the existing .grad
    assert torch.equal(za.grad, g0 + g0)
    zb = place(z, "nchw", dev())
    zb.grad = torch.full_like(zb, 0.25)
    (call(zb, t)[0] * UPSTREAM).backward()
    assert torch.equal(zb.grad, torch.full_like(zb, 0.25) + g0)


def test_micro_batches_and_a_no_grad_forward_between():
    d = dev()
    (z0, t0, _, _), (z1, t1, _, _) = case(0), case(1)
    _, g0 = plain(0)
    za = place(z0, "nchw", d)
    loss = call(za, t0)[0]
    with torch.no_grad():                # another forward of the op before the backward: no state is shared
        other = call(place(z1, "nchw", d), t1)[0]
    assert not other.requires_grad
    (loss * UPSTREAM).backward()
    assert torch.equal(za.grad, g0)
    (call(za, t0)[0] * UPSTREAM).backward()      # the second micro-batch accumulates
    assert torch.equal(za.grad, g0 + g0)


def test_user_stream():
    d = dev()
    z, t, _, _ = case()
    loss0, g0 = plain()
    za = place(z, "nchw", d)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        loss = call(za, t)[0]
        (loss * UPSTREAM).backward()
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(loss.detach(), loss0) and torch.equal(za.grad, g0)


def test_create_graph_gives_the_first_order_values():
    z, t, _, _ = case()
    _, g0 = plain()
    za = place(z, "nchw", dev())
    (call(za, t)[0] * UPSTREAM).backward(create_graph=True)
    assert torch.equal(za.grad.detach(), g0)
    za.grad = None
