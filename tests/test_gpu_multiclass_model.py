"""The logits head (``set_head("logits")``) and the K-class head GEMM of the CSWin-UNet on the
MI355X against the fp64 oracle (oracle.cswin_ref.cswin_forward, which returns sigmoid
probabilities: the logits compared here are ``logit()`` of them), the default head pinned against
it, the UNet's logits head, and a CE + Dice step's ``output.weight`` gradient.

Forward tolerance, the way __graft_entry__.smoke measures its own: smoke allows the fp32 model
1e-4 on the oracle's probabilities at this configuration (img 64, fp32).  A probability error dp is a
logit error dp / (p (1 - p)), so the logits are allowed 1e-4 / min(p (1 - p)) over the oracle's
probabilities (4e-4 where they stay near 0.5), and the default head's probabilities smoke's 1e-4.
The gradient tolerance is smoke's: 1e-3 of the largest reference gradient entry."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PROB_TOL = 1e-4
GRAD_TOL_REL = 1e-3
_CACHE = {}


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def setup(nc):
    """(cfg, params, x, oracle probabilities fp64 (grad-enabled params)), made once per class count."""
    from oracle import cswin_ref as O
    if nc not in _CACHE:
        cfg = O.CSWinConfig(img_size=64, num_classes=nc, split_size=(1, 2, 2, 2))
        p = O.recipe_params(cfg, seed=0)
        x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(0))
        pref = {k: v.double().requires_grad_(True) for k, v in p.items()}
        _CACHE[nc] = (cfg, p, x, pref, O.cswin_forward(pref, x.double(), cfg))
    return _CACHE[nc]


def model(nc, p, d):
    from csu.model import CSWinTransformer
    m = CSWinTransformer(img_size=64, split_size=[1, 2, 2, 2], num_classes=nc).to(d)
    m.load_state_dict(p)
    return m


@pytest.mark.parametrize("nc", [1, 3])
def test_logits_head_vs_oracle_and_default_head_pinned(nc):
    d = dev()
    cfg, p, x, _, yr = setup(nc)
    yr = yr.detach()
    m = model(nc, p, d).eval()
    keys = list(m.state_dict())
    with torch.no_grad():
        prob = m(x.to(d))
        assert m.set_head("logits") is m
        z = m(x.to(d))
        prob2 = m.set_head("sigmoid")(x.to(d))
    assert list(m.state_dict()) == keys
    assert z.shape == (2, nc, 64, 64) and z.dtype == torch.float32 and prob.shape == z.shape
    # a view of the class-last token GEMM output (pitch 8): nothing was copied
    assert z.stride()[2:] == (64 * 8, 8) and (nc == 1 or z.stride()[:2] == (64 * 64 * 8, 1))
    tol = PROB_TOL / float((yr * (1 - yr)).min())
    err = float((z.double().cpu() - torch.logit(yr)).abs().max())
    perr = float((prob.double().cpu() - yr).abs().max())
    print(f"logits err {err:.2e} (tol {tol:.2e}), default-head prob err {perr:.2e}")
    assert err < tol
    assert perr < PROB_TOL
    assert torch.equal(prob, prob2)
    if nc == 1:     # the fused CARAFE + sigmoid head against the token GEMM's logits
        assert float((torch.sigmoid(z) - prob).abs().max()) < PROB_TOL
    else:           # the existing num_classes != 1 branch: sigmoid of exactly these logits
        assert torch.equal(prob, torch.sigmoid(z.float()))
    with pytest.raises(ValueError):
        m.set_head("softmax")


def ce_dice_ref(nc=3):
    """(criterion, labels, fp64 loss, fp64 d loss / d output.weight) of a CE + Dice step through the
    oracle (the criterion's own formula on logit() of its probabilities), made once."""
    from csu.losses import ce_dice_loss
    if "ref" not in _CACHE:
        cfg, p, x, pref, yr = setup(nc)
        t = torch.randint(0, nc, (2, 64, 64), generator=torch.Generator().manual_seed(1))
        crit = ce_dice_loss(nc)
        lref = crit._torch(torch.logit(yr), t)
        (gref,) = torch.autograd.grad(lref, pref["output.weight"], retain_graph=True)
        _CACHE["ref"] = (crit, t, lref.detach(), gref)
    return _CACHE["ref"]


def test_ce_dice_step_output_weight_grad_vs_oracle():
    d = dev()
    nc = 3
    cfg, p, x, pref, yr = setup(nc)
    crit, t, lref, gref = ce_dice_ref(nc)
    m = model(nc, p, d).set_head("logits")
    loss = crit(m(x.to(d)), t.to(d))
    loss.backward()
    g = m.output.weight.grad.double().cpu()
    gerr, gscale = float((g - gref).abs().max()), float(gref.abs().max())
    print(f"loss {float(loss.detach()):.7f} vs {float(lref):.7f}, output.weight grad err {gerr:.2e} (scale {gscale:.2e})")
    assert abs(float(loss.detach()) - float(lref)) < 1e-5 * max(1.0, abs(float(lref)))
    assert gerr < GRAD_TOL_REL * max(gscale, 1e-6)


def test_ce_dice_step_output_weight_grad_bf16():
    """The same step under bf16 autocast (the head GEMM's padded weight is computed in the graph: its
    gradient must be complete when the padding's backward reads it, not deferred to the end of
    backward or left on the side stream) to the project's bf16 standard (tests/test_gpu_model.py):
    loss within 1e-2 relative, gradient relative L2 error <= 5e-2; logits in bf16, a view again."""
    d = dev()
    nc = 3
    cfg, p, x, pref, yr = setup(nc)
    crit, t, lref, gref = ce_dice_ref(nc)
    m = model(nc, p, d).set_head("logits")
    for _ in range(2):           # twice: the second backward meets the first one's .grad
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            z = m(x.to(d))
        assert z.dtype == torch.bfloat16 and z.stride()[1:] == (1, 64 * 8, 8)
        loss = crit(z, t.to(d))
        loss.backward()
        g = m.output.weight.grad.double().cpu()
        rel = float((g - gref).norm() / gref.norm())
        print(f"bf16 loss {float(loss.detach()):.6f} vs {float(lref):.6f}, output.weight grad rel-L2 {rel:.2e}")
        assert abs(float(loss.detach()) - float(lref)) < 1e-2 * abs(float(lref))
        assert rel <= 5e-2


def test_unet_logits_head():
    from csu.unet import UNet
    d = dev()
    torch.manual_seed(0)
    m = UNet(3, 3).to(d).eval()
    x = torch.rand(2, 3, 32, 32, device=d)
    with torch.no_grad():
        prob = m(x)
        z = m.set_head("logits")(x)
        assert torch.equal(m.set_head("sigmoid")(x), prob)
    assert z.shape == (2, 3, 32, 32) and z.stride(1) == 1          # class-last: a view of outc's NHWC output
    assert torch.equal(torch.sigmoid(z.float()), prob)
    with pytest.raises(ValueError):
        m.set_head("softmax")
