"""Weight EMA on the MI355X: csu_adamw_step_ema (the update fused into FusedAdamW's step),
csu_ema_update (stand-alone) and csu_ema_swap through csu.ema.WeightEMA, the captured step,
train_model and the fp8 weight format.

Kernel-level tensor set (the shape of the AdamW / gradient-clipping tests' sets): with a CastCache
alive the optimizer's table has tile items (192 x 64: three whole tiles; 96 x 72: ragged tiles in both
directions on the 16-B path; 70 x 33: cols % 4 != 0, the scalar path), conv-scatter items (3 x 3 with
both layouts; 7 x 7 over 3 channels whose OHWI layout is channel-padded, cols_pad > cols, and has no
IHWO) and flat items with a bf16 copy (numel 1 and 4097: one element, and two chunks with a ragged
tail); outside the cache plain flat items of numel 3 and 2 * 4096, and a parameter that never gets a
gradient.

Everything that compares two ways of computing the same thing is bitwise (torch.equal).  Against
fp64: one update e + w (p - e) makes two fp32 roundings, each at most 2^-24 relative to values of at
most 2 max(|p|, |e|); over 8 updates that is about 1.5e-6 max, so |e - e64| <= 4e-6 max(|p|, |e|)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class _Holder(torch.nn.Module):
    """A module over a list of parameters (WeightEMA takes a model)."""

    def __init__(self, ps):
        super().__init__()
        self.ps = torch.nn.ParameterList(ps)


def _set(d, seed=4):
    """(cached linear-like params, cached convs, uncached flat params, a parameter without a gradient,
    the CastCache)."""
    from csu import ops
    g = torch.Generator(device=d).manual_seed(seed)
    r = lambda *s: torch.nn.Parameter(torch.randn(*s, device=d, generator=g))   # noqa: E731
    ps = [r(192, 64), r(96, 72), r(70, 33), r(16, 64, 1, 1), r(1), r(4097)]
    convs = [r(36, 16, 3, 3), r(64, 3, 7, 7)]
    flat = [r(3), r(2 * 4096)]
    nograd = r(33)
    c = ops.CastCache()
    c.refresh(ps, torch.bfloat16, convs)
    return ps, convs, flat, nograd, c


def _twin_set(src):
    """An independent copy of a _set with its own CastCache."""
    from csu import ops
    ps, convs, flat, nograd, _ = src
    cp = lambda xs: [torch.nn.Parameter(x.detach().clone()) for x in xs]   # noqa: E731
    ps2, convs2, flat2, ng2 = cp(ps), cp(convs), cp(flat), cp([nograd])[0]
    c = ops.CastCache()
    c.refresh(ps2, torch.bfloat16, convs2)
    return ps2, convs2, flat2, ng2, c


def _stepped(s):
    return s[0] + s[1] + s[2]


def _all(s):
    return _stepped(s) + [s[3]]


def _raw_shadows(s):
    """Every bf16 layout the cache keeps, as it is in memory (no refresh: what the kernels wrote)."""
    c = s[4]
    out = list(c.shadow) + [t for t in c.shadow_t if t is not None] + list(c.conv_o) + [t for t in c.conv_i if t is not None]
    assert len(out) >= len(s[0]) + len(s[1])
    return out


def _set_grads(ps, seed, scale=1.0):
    g = torch.Generator(device=ps[0].device).manual_seed(seed)
    for p in ps:
        p.grad = torch.randn(p.shape, device=p.device, generator=g) * scale


def _copy_grads(a, b):
    for p, q in zip(a, b):
        q.grad = p.grad.clone()


def _ref_norm(ps):
    return torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ps if p.grad is not None))


def _state(opt, ps):
    return [opt.state[p][k] for p in ps if p in opt.state and opt.state[p] for k in ("exp_avg", "exp_avg_sq")]


def _eq(xs, ys):
    xs, ys = [x.detach() for x in xs], [y.detach() for y in ys]
    return len(xs) == len(ys) and len(xs) > 0 and all(torch.equal(a, b) for a, b in zip(xs, ys))


def _table_kinds(opt):
    """The optimizer's table really has tile, conv and flat items (the cache is alive)."""
    from csu.ops import shadow_spec
    specs = [shadow_spec(p) for g in opt.param_groups for p in g["params"]]
    tiled = sum(1 for s in specs if s and s[0] and s[1] and s[4] == 0)
    conv = sum(1 for s in specs if s and s[4] > 0)
    padded = sum(1 for s in specs if s and s[4] > 0 and s[5] > s[3])
    return tiled, conv, padded


# ------------------------------------------------------------------------- kernel level


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("l2", [False, True])
def test_fused_equals_step_then_update_bitwise(l2, clip):
    """Three steps of FusedAdamW / FusedAdam(ema=...) == the plain step followed by ema.update():
    parameters, moments, every shadow, every EMA tensor and the update count torch.equal."""
    from csu.ema import WeightEMA
    from csu.optim import FusedAdam, FusedAdamW
    cls = FusedAdam if l2 else FusedAdamW
    d = dev()
    A = _set(d)
    B = _twin_set(A)
    ea = WeightEMA(_Holder(_all(A)), decay=0.9, warmup=True)
    eb = WeightEMA(_Holder(_all(B)), decay=0.9, warmup=True)
    _set_grads(_stepped(A), 100)
    kw = dict(lr=1e-2, weight_decay=1e-2)
    if clip:
        kw["max_grad_norm"] = 0.5 * float(_ref_norm(_stepped(A)))
    oa = cls(_all(A), ema=ea, **kw)
    ob = cls(_all(B), **kw)
    assert _table_kinds(oa) == (4, 2, 1)
    for it in range(3):
        _set_grads(_stepped(A), 100 + it, scale=1.0 + 0.3 * it)
        _copy_grads(_stepped(A), _stepped(B))
        oa.step()
        ob.step()
        eb.update()
        if clip:
            assert float(oa._ctl[1]) < 1.0
    assert _eq(_all(A), _all(B))
    assert _eq(_state(oa, _all(A)), _state(ob, _all(B)))
    assert _eq(_raw_shadows(A), _raw_shadows(B))
    assert _eq(ea.tensors, eb.tensors)
    assert float(ea.num_updates) == float(eb.num_updates) == 3.0
    # the averages moved, except the one of the parameter without a gradient
    assert not any(torch.equal(e, p.detach()) for e, p in zip(ea.tensors[:-1], _stepped(A)))
    assert torch.equal(ea.tensors[-1], A[3].detach()) and A[3] not in oa.state
    for p, sh in zip(A[0], A[4].shadow):             # and the shadows are the bf16 image of the weights
        assert torch.equal(sh, p.detach().bfloat16())


def test_ema_does_not_perturb_the_step():
    """With and without an EMA attached (clipping and skip_nonfinite on): parameters, moments and
    shadows torch.equal after three steps."""
    from csu.ema import WeightEMA
    from csu.optim import FusedAdamW
    d = dev()
    A = _set(d)
    B = _twin_set(A)
    _set_grads(_stepped(A), 7)
    kw = dict(lr=1e-2, weight_decay=1e-2, max_grad_norm=0.5 * float(_ref_norm(_stepped(A))), skip_nonfinite=True)
    oa = FusedAdamW(_all(A), ema=WeightEMA(_Holder(_all(A)), decay=0.99), **kw)
    ob = FusedAdamW(_all(B), **kw)
    for it in range(3):
        _set_grads(_stepped(A), 7 + it)
        _copy_grads(_stepped(A), _stepped(B))
        oa.step()
        ob.step()
    assert _eq(_all(A), _all(B))
    assert _eq(_state(oa, _all(A)), _state(ob, _all(B)))
    assert _eq(_raw_shadows(A), _raw_shadows(B))
    assert float(oa.state[A[0][0]]["step"]) == float(ob.state[B[0][0]]["step"]) == 3.0


def test_ema_against_fp64_recurrence():
    """8 fused steps at decay 0.9, warmup off, against the fp64 recurrence over the recorded fp32
    parameter sequence: |e - e64| <= 4e-6 max(|p|, |e|) over the run, elementwise (module docstring)."""
    from csu.ema import WeightEMA
    from csu.optim import FusedAdamW
    d = dev()
    A = _set(d)
    ps = _stepped(A)
    ema = WeightEMA(_Holder(_all(A)), decay=0.9, warmup=False)
    opt = FusedAdamW(_all(A), lr=5e-2, weight_decay=1e-2, ema=ema)
    dd = float(np.float32(0.9))
    ref = [p.detach().double().clone() for p in ps]
    big = [p.detach().abs().double() for p in ps]
    for it in range(8):
        _set_grads(ps, 30 + it)
        opt.step()
        for r, b, p in zip(ref, big, ps):
            r.mul_(dd).add_(p.detach().double(), alpha=1 - dd)
            torch.maximum(b, torch.maximum(p.detach().abs().double(), r.abs()), out=b)
    worst = 0.0
    for e, r, b in zip(ema.tensors, ref, big):
        err = ((e.double() - r).abs() / b.clamp(min=1e-30)).max()
        worst = max(worst, float(err))
        assert bool(((e.double() - r).abs() <= 4e-6 * b).all())
    print(f"max |e - e64| / max(|p|, |e|) over the set: {worst:.3e} (bound 4e-6)")
    assert float(ema.num_updates) == 8.0


def test_warmup_schedule_on_device():
    """12 fused steps at decay 0.999 with warmup: d_n = min(0.999, n / (n + 9)), recovered from a
    tensor that holds 0 when the EMA is made and 1 afterwards (lr = 0 keeps it there exactly): e_n =
    1 - prod d_k.  One update's absolute error on values <= 1: d, w = 1 - d, p - e and the fma each round
    at <= 2^-24, so <= 2.5e-7 per update, n of them on e_n; the ratio of two consecutive 1 - e
    amplifies that by 1 / (1 - e_(n-1)) and is checked while that keeps it below 1e-3."""
    from csu.ema import WeightEMA
    from csu.optim import FusedAdamW
    d = dev()
    ps = [torch.nn.Parameter(torch.zeros(s, device=d)) for s in [(96, 72), (4097,), (3,)]]
    ema = WeightEMA(_Holder(ps), decay=0.999, warmup=True)
    with torch.no_grad():
        for p in ps:
            p.fill_(1.0)
    opt = FusedAdamW(ps, lr=0.0, weight_decay=0.0, ema=ema)
    prev, prod = 0.0, 1.0
    for n in range(1, 13):
        _set_grads(ps, n)
        opt.step()
        want = min(0.999, n / (n + 9))
        prod *= want
        for p, e in zip(ps, ema.tensors):
            assert bool((p.detach() == 1.0).all())
            assert float(e.min()) == float(e.max())                    # every element took the same path
        e = float(ema.tensors[0].view(-1)[0])
        assert all(float(t.view(-1)[-1]) == e for t in ema.tensors)
        assert abs((1.0 - e) - prod) <= n * 2.5e-7, n
        if 1.0 - prev > 1e-3:
            dn = (1.0 - e) / (1.0 - prev)
            print(f"n {n}: d {dn:.7f} want {want:.7f}")
            assert abs(dn - want) <= 2 * n * 2.5e-7 / (1.0 - prev), n
        prev = e
    assert float(ema.num_updates) == 12.0
    assert ema.current_decay() == pytest.approx(13 / 22, rel=1e-6)


def test_skip_nonfinite_leaves_the_ema_untouched():
    """One inf gradient element with skip_nonfinite=True: EMA tensors and num_updates bitwise unchanged,
    skipped_steps == 1; the next finite step advances num_updates by 1."""
    from csu.ema import WeightEMA
    from csu.optim import FusedAdamW
    d = dev()
    A = _set(d)
    ps = _stepped(A)
    ema = WeightEMA(_Holder(_all(A)), decay=0.9, warmup=True)
    _set_grads(ps, 60)
    opt = FusedAdamW(_all(A), lr=1e-2, weight_decay=1e-2, max_grad_norm=0.5 * float(_ref_norm(ps)), skip_nonfinite=True,
                     ema=ema)
    opt.step()
    snap = [e.clone() for e in ema.tensors]
    n0 = ema.num_updates.clone()
    assert float(n0) == 1.0
    psnap = [p.detach().clone() for p in ps]
    _set_grads(ps, 61)
    ps[1].grad.view(-1)[1234] = float("inf")            # inside the ragged-tile matrix 96 x 72
    opt.step()
    assert float(opt._ctl[2]) == 0.0 and int(opt.skipped_steps) == 1
    assert _eq(snap, ema.tensors) and torch.equal(ema.num_updates, n0)
    assert _eq(psnap, ps)
    _set_grads(ps, 62)
    opt.step()
    assert int(opt.skipped_steps) == 1 and float(ema.num_updates) == 2.0
    assert not any(torch.equal(a, b) for a, b in zip(snap[:-1], ema.tensors[:-1]))


def test_swap_exchanges_and_rewrites_every_shadow():
    """swap(): parameters <- old EMA, EMA <- old parameters, every shadow bitwise what a fresh
    CastCache casts from the now-live parameters; a second swap() restores parameters, EMA and shadows
    bitwise; applied() restores on an exception; nested use raises."""
    from csu.ema import WeightEMA
    from csu.optim import FusedAdamW
    d = dev()
    A = _set(d)
    ps = _stepped(A)
    ema = WeightEMA(_Holder(_all(A)), decay=0.5, warmup=False)
    opt = FusedAdamW(_all(A), lr=5e-2, weight_decay=1e-2, ema=ema)
    for it in range(2):
        _set_grads(ps, 90 + it)
        opt.step()
    p0 = [p.detach().clone() for p in _all(A)]
    e0 = [e.clone() for e in ema.tensors]
    s0 = [s.clone() for s in _raw_shadows(A)]
    assert not any(torch.equal(a, b) for a, b in zip(p0[:-1], e0[:-1]))
    ema.swap()
    assert ema.swapped
    assert _eq(_all(A), e0) and _eq(ema.tensors, p0)
    assert A[4]._fresh()                                  # the next forward launches no cast
    B = _twin_set(A)                                      # a fresh cache's cast of the now-live parameters
    B[4].ensure_fresh()
    assert _eq(_raw_shadows(A), _raw_shadows(B))
    assert not _eq(_raw_shadows(A), s0)
    with pytest.raises(RuntimeError):
        opt.step()                                        # no training on the averaged weights
    ema.swap()
    assert not ema.swapped
    assert _eq(_all(A), p0) and _eq(ema.tensors, e0) and _eq(_raw_shadows(A), s0)
    with pytest.raises(KeyError):
        with ema.applied():
            assert _eq(_all(A), e0)
            with pytest.raises(RuntimeError):
                with ema.applied():
                    pass
            raise KeyError("boom")
    assert not ema.swapped
    assert _eq(_all(A), p0) and _eq(ema.tensors, e0) and _eq(_raw_shadows(A), s0)


# ----------------------------------------------------------------------------- model level


def _model_and_batches(d, n, seed=1, batch=4):
    from csu.data import ellipse_batch
    from csu.model import CSWinTransformer
    torch.manual_seed(0)
    m0 = CSWinTransformer(img_size=128, split_size=[1, 2, 4, 4])
    rng = np.random.default_rng(seed)
    return m0, [tuple(t.to(d) for t in ellipse_batch(rng, batch, 128)) for _ in range(n)]


def _snap(m, ema):
    return [p.detach().clone() for p in m.parameters()] + [e.clone() for e in ema.tensors] + [ema.num_updates.clone()]


def test_captured_step_carries_the_ema(monkeypatch):
    """Three eager and four replayed GraphedTrainStep steps with an EMA == seven eager steps
    (parameters, EMA tensors and update count torch.equal); two identical captured runs are bitwise
    equal; load_state_dict of model, optimizer and EMA after the capture, followed by replays, equals
    the uninterrupted run.
    ops.SIDE_WGRAD is off for all three runs: with it an eager backward launches every Linear weight
    gradient on its own on a side stream, where a capture defers them to one grouped launch that sums
    in another order -- eager and replayed steps then agree to rounding only, EMA or not
    (test_train_model_graphed_equals_eager); without it both run the same kernels."""
    from csu import ops
    from csu.train import GraphedTrainStep, bce_loss, make_optimizer
    monkeypatch.setattr(ops, "SIDE_WGRAD", False)
    d = dev()
    m0, b = _model_and_batches(d, 5)

    def run(capture, rewind):
        m = copy.deepcopy(m0).to(d)
        opt = make_optimizer(m, capturable=True, ema_decay=0.9)
        gs = GraphedTrainStep(m, opt, bce_loss, b[0][0], b[0][1], torch.bfloat16, warmup=3, capture=capture)
        assert float(opt.ema.num_updates) == 3.0
        gs(*b[1])
        gs(*b[2])
        if rewind:
            sd = copy.deepcopy((m.state_dict(), opt.state_dict(), opt.ema.state_dict()))
            ptrs = [e.data_ptr() for e in opt.ema.tensors]
        gs(*b[3])
        gs(*b[4])
        out = _snap(m, opt.ema)
        if rewind:
            m.load_state_dict(sd[0])
            opt.load_state_dict(sd[1])
            opt.ema.load_state_dict(sd[2])
            assert [e.data_ptr() for e in opt.ema.tensors] == ptrs and float(opt.ema.num_updates) == 5.0
            gs(*b[3])
            gs(*b[4])
            assert _eq(out, _snap(m, opt.ema))
        torch.cuda.synchronize()
        assert float(opt.ema.num_updates) == 7.0
        assert not any(torch.equal(e, p.detach()) for e, p in zip(opt.ema.tensors, m.parameters()))
        return out

    g1 = run(True, False)
    g2 = run(True, True)
    eager = run(False, False)
    assert _eq(g1, g2)
    names = [n for n, _ in m0.named_parameters()]
    names = names + ["ema." + n for n in names] + ["num_updates"]
    diff = [(n, float((x - y).abs().max())) for n, x, y in zip(names, g1, eager) if not torch.equal(x, y)]
    print("captured vs eager: tensors that differ:", len(diff), diff[:5])
    assert not diff, (len(diff), diff[:5])


def _loaders(n_train=12, n_test=4):
    from csu.data import SyntheticSegmentation
    mk = lambda n, seed: torch.utils.data.DataLoader(SyntheticSegmentation(n, 128, seed=seed), batch_size=4)   # noqa: E731
    return mk(n_train, 1234), mk(n_test, 99)


def test_train_model_evaluates_the_ema_in_place():
    """Two epochs with make_optimizer(model, ema_decay=0.9): ema_test_* keys with one value per epoch;
    the last triple equals evaluate_model on a second instance loaded with ema.model_state_dict(); the
    trained weights are torch.equal to the same run without an EMA (whose history has no new key)."""
    from csu.model import CSWinTransformer
    from csu.train import bce_loss, evaluate_model, make_optimizer, train_model
    d = dev()
    m0, _ = _model_and_batches(d, 0)
    train, test = _loaders()
    base = {"train_loss", "train_dice", "train_iou", "test_loss", "test_dice", "test_iou", "learning_rates"}
    m = copy.deepcopy(m0).to(d)
    opt = make_optimizer(m, ema_decay=0.9)
    h = train_model(m, train, test, bce_loss, opt, None, d, num_epochs=2, verbose=False, amp_dtype=torch.bfloat16)
    assert set(h) == base | {"ema_test_loss", "ema_test_dice", "ema_test_iou"}
    assert all(len(v) == 2 for v in h.values())
    assert not opt.ema.swapped and float(opt.ema.num_updates) == 6.0
    m2 = CSWinTransformer(img_size=128, split_size=[1, 2, 4, 4]).to(d)
    m2.load_state_dict(opt.ema.model_state_dict())
    want = evaluate_model(m2, test, bce_loss, d, amp_dtype=torch.bfloat16)
    got = (h["ema_test_loss"][-1], h["ema_test_dice"][-1], h["ema_test_iou"][-1])
    print("ema eval", got, "second instance", want, "raw", h["test_loss"][-1])
    assert got == want
    assert h["ema_test_loss"][-1] != h["test_loss"][-1]
    m3 = copy.deepcopy(m0).to(d)
    h3 = train_model(m3, train, test, bce_loss, make_optimizer(m3), None, d, num_epochs=2, verbose=False,
                     amp_dtype=torch.bfloat16)
    assert set(h3) == base
    assert _eq(list(m.parameters()), list(m3.parameters()))
    assert all(h3[k] == h[k] for k in base)


def test_train_model_resume_restores_the_ema(tmp_path):
    """Stop after one epoch with checkpoint_path, resume into fresh objects: EMA, weights and history
    equal the uninterrupted run's (graph=False: a resumed run would otherwise begin its second epoch with
    eager warm-up steps where the uninterrupted one replays)."""
    from csu.train import bce_loss, make_optimizer, train_model
    d = dev()
    m0, _ = _model_and_batches(d, 0)
    train, test = _loaders(8, 4)
    kw = dict(verbose=False, amp_dtype=torch.bfloat16, graph=False)
    m = copy.deepcopy(m0).to(d)
    opt = make_optimizer(m, ema_decay=0.9)
    h = train_model(m, train, test, bce_loss, opt, None, d, num_epochs=2, **kw)
    ck = str(tmp_path / "ck.pt")
    m1 = copy.deepcopy(m0).to(d)
    train_model(m1, train, test, bce_loss, make_optimizer(m1, ema_decay=0.9), None, d, num_epochs=1, checkpoint_path=ck, **kw)
    assert "ema" in torch.load(ck, weights_only=True)
    m2 = copy.deepcopy(m0).to(d)
    o2 = make_optimizer(m2, ema_decay=0.9)
    h2 = train_model(m2, train, test, bce_loss, o2, None, d, num_epochs=2, resume_from=ck, **kw)
    assert h2 == h
    assert _eq(o2.ema.tensors, opt.ema.tensors) and float(o2.ema.num_updates) == float(opt.ema.num_updates) == 4.0
    assert _eq(list(m2.parameters()), list(m.parameters()))


def test_fp8_weight_format_under_applied():
    """set_weight_format("fp8_e4m3") with bf16 autocast: the eval output under applied() equals bitwise
    that of a second instance loaded with model_state_dict() (the swap writes fp32 parameters and bf16
    shadows; the quantiser re-quantises on every forward)."""
    from csu.model import CSWinTransformer
    from csu.train import bce_loss, make_optimizer, train_step
    d = dev()
    m0, b = _model_and_batches(d, 2)
    m = copy.deepcopy(m0).to(d).set_weight_format("fp8_e4m3")
    opt = make_optimizer(m, lr=1e-3, ema_decay=0.5, ema_warmup=False)
    for x, t in b:
        train_step(m, x, t, bce_loss, opt, amp_dtype=torch.bfloat16)
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        raw = m(b[0][0]).clone()
        with opt.ema.applied():
            got = m(b[0][0]).clone()
        back = m(b[0][0]).clone()
    m2 = CSWinTransformer(img_size=128, split_size=[1, 2, 4, 4]).to(d).set_weight_format("fp8_e4m3")
    m2.load_state_dict(opt.ema.model_state_dict())
    m2.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        want = m2(b[0][0])
    assert torch.equal(got, want)
    assert torch.equal(back, raw) and not torch.equal(got, raw)
