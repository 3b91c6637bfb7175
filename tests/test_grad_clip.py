"""Global-norm gradient clipping, CPU side: the C ABI exports and their ctypes mirrors, argument
validation, make_optimizer / train_step / train_model with ``max_grad_norm`` on a CPU module (where
torch's clip_grad_norm_ does the work) against a hand-written loop."""
import copy

import pytest
import torch

NEW_SYMBOLS = ["csu_grad_norm_workspace", "csu_grad_sumsq", "csu_grad_norm_finish", "csu_grad_scale", "csu_adamw_step_ex"]


def _net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(4, 1, 1),
                               torch.nn.Sigmoid())


def _batches(n, b=2, s=8, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(b, 3, s, s, generator=g), (torch.rand(b, 1, s, s, generator=g) > 0.5).float()) for _ in range(n)]


def test_library_exports_grad_clip_symbols():
    from csu import _lib
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert n in _lib._SIGS, n
    assert L.csu_grad_norm_workspace(10) == 80 and L.csu_grad_norm_workspace(0) == 0
    # argument errors are reported before any device work
    assert L.csu_grad_sumsq(None, 0, 0, None, None) != 0
    assert L.csu_grad_norm_finish(None, 0, 1.0, None, None) != 0
    assert L.csu_grad_scale(None, 0, 0, None, None) != 0
    assert L.csu_adamw_step_ex(None, 0, 0, None, 0.0, 0.9, 0.999, 1e-8, 0.0, None, 1.0, None, 0, 0, None) != 0


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan")])
def test_fused_adamw_rejects_bad_max_grad_norm(bad):
    from csu.optim import FusedAdam, FusedAdamW
    p = [torch.nn.Parameter(torch.zeros(3))]
    for cls in (FusedAdamW, FusedAdam):
        with pytest.raises(ValueError):
            cls(p, max_grad_norm=bad)
        o = cls(p, max_grad_norm=2.0, skip_nonfinite=True)
        assert o.max_grad_norm == 2.0 and o.skip_nonfinite is True
        # plain attributes: the state_dict keeps torch.optim.AdamW's format
        assert "max_grad_norm" not in o.defaults and "max_grad_norm" not in o.param_groups[0]
        assert set(o.state_dict()) == {"state", "param_groups"}
        assert set(o.state_dict()["param_groups"][0]) == set(cls(p).state_dict()["param_groups"][0])


def test_make_optimizer_cpu_sets_attribute_and_refuses_skip():
    from csu.train import make_optimizer
    m = _net()
    o = make_optimizer(m, max_grad_norm=0.5)
    assert isinstance(o, torch.optim.AdamW) and o.max_grad_norm == 0.5
    assert make_optimizer(m).max_grad_norm is None
    with pytest.raises(ValueError):
        make_optimizer(m, skip_nonfinite=True)
    with pytest.raises(ValueError):
        make_optimizer(m, max_grad_norm=0)


def test_train_step_cpu_clip_equals_handwritten_loop():
    """train_step with max_grad_norm == backward, clip_grad_norm_, AdamW.step over 3 steps, bitwise;
    optimizer.grad_norm is torch's returned (pre-clip) norm."""
    from csu.train import bce_loss, make_optimizer, train_step
    m1 = _net()
    m2 = copy.deepcopy(m1)
    batches = _batches(3)
    # a clip value that bites: half the first step's norm
    mp = copy.deepcopy(m1)
    bce_loss(mp(batches[0][0]), batches[0][1]).backward()
    c = 0.5 * float(torch.nn.utils.clip_grad_norm_(mp.parameters(), float("inf")))
    assert c > 0
    o1 = make_optimizer(m1, lr=1e-2, max_grad_norm=c)
    o2 = torch.optim.AdamW(m2.parameters(), lr=1e-2, weight_decay=1e-4)
    clipped = 0
    for x, t in batches:
        train_step(m1, x, t, bce_loss, o1)
        o2.zero_grad(set_to_none=True)
        bce_loss(m2(x), t).backward()
        norm = torch.nn.utils.clip_grad_norm_(m2.parameters(), c)
        o2.step()
        assert torch.equal(o1.grad_norm, norm)
        clipped += float(norm) > c
    assert clipped >= 1
    for a, b in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(a, b)
    # and clipping changed the trajectory
    m3 = copy.deepcopy(_net())
    o3 = make_optimizer(m3, lr=1e-2)
    for x, t in batches:
        train_step(m3, x, t, bce_loss, o3)
    assert not all(torch.equal(a, b) for a, b in zip(m1.parameters(), m3.parameters()))
    assert not hasattr(o3, "grad_norm")


def test_train_model_cpu_history_keys_only_when_asked():
    from csu.train import bce_loss, make_optimizer, train_model
    base = {"train_loss", "train_dice", "train_iou", "test_loss", "test_dice", "test_iou", "learning_rates"}
    train, test = _batches(3), _batches(1, seed=6)
    m = _net()
    h = train_model(m, train, test, bce_loss, make_optimizer(m), None, "cpu", num_epochs=2, verbose=False)
    assert set(h) == base
    m = _net()
    h = train_model(m, train, test, bce_loss, make_optimizer(m, max_grad_norm=0.05), None, "cpu", num_epochs=2,
                    verbose=False)
    assert set(h) == base | {"grad_norm", "skipped_steps"}
    assert all(len(v) == 2 for v in h.values())
    assert h["skipped_steps"] == [0, 0]
    # the per-epoch mean of the per-step pre-clip norms of the same run done by hand
    m2 = _net()
    o2 = torch.optim.AdamW(m2.parameters(), lr=1e-4, weight_decay=1e-4)
    for e in range(2):
        norms = []
        for x, t in train:
            o2.zero_grad(set_to_none=True)
            bce_loss(m2(x), t).backward()
            norms.append(float(torch.nn.utils.clip_grad_norm_(m2.parameters(), 0.05).double()))
            o2.step()
        assert h["grad_norm"][e] == pytest.approx(sum(norms) / len(norms), rel=1e-12)


def test_train_model_resume_restores_clip_history(tmp_path):
    from csu.train import bce_loss, make_optimizer, train_model
    train, test = _batches(2), _batches(1, seed=6)
    ck = str(tmp_path / "ck.pt")
    m = _net()
    h1 = train_model(m, train, test, bce_loss, make_optimizer(m, max_grad_norm=0.05), None, "cpu", num_epochs=1,
                     verbose=False, checkpoint_path=ck)
    m = _net()
    h2 = train_model(m, train, test, bce_loss, make_optimizer(m, max_grad_norm=0.05), None, "cpu", num_epochs=2,
                     verbose=False, resume_from=ck)
    assert h2["grad_norm"][:1] == h1["grad_norm"] and len(h2["grad_norm"]) == 2 and h2["skipped_steps"] == [0, 0]


def test_standalone_helpers_forward_to_torch_on_cpu():
    from csu.optim import clip_grad_norm_, grad_norm
    g = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in [(5, 3), (7,), (2, 2, 2)]]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for p, q in zip(ps, qs):
        p.grad = torch.randn(p.shape, generator=g)
        q.grad = p.grad.clone()
    want = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ps))
    torch.testing.assert_close(grad_norm(ps).double(), want, rtol=1e-6, atol=0)
    n1 = clip_grad_norm_(ps, 0.5)
    n2 = torch.nn.utils.clip_grad_norm_(qs, 0.5)
    assert torch.equal(n1, n2)
    for p, q in zip(ps, qs):
        assert torch.equal(p.grad, q.grad)
