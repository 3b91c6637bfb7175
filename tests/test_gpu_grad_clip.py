"""Fused global-norm gradient clipping on the MI355X: csu_grad_sumsq / csu_grad_norm_finish /
csu_grad_scale / csu_adamw_step_ex through csu.optim.FusedAdamW(max_grad_norm, skip_nonfinite),
csu.optim.clip_grad_norm_ and the captured training step.

Tensor sets are those of the AdamW tests (tests/test_gpu_kernels.py), which reach every path of the
item table: flat chunks with ragged tails and a parameter without a gradient; with a CastCache the
64 x 64 tile items (ragged tiles, cols % 4 != 0) and the conv-scatter items; plus a 2048 x 2048
matrix so that the partial count exceeds the finish workgroup (1024 threads) and its strided loop
runs.

Tolerances: the norm is summed in fp64 from the element on, so the only fp32 rounding is the final
cast (2^-24 ~ 6e-8 relative): rtol 1e-6 leaves room for nothing but that.  Everything that compares
the fused clip with "scale the gradient, then the plain step" is bitwise (torch.equal).  Against
torch.optim.AdamW the tolerances are those of test_fused_adamw_matches_torch."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLAT = [(256, 64), (64,), (3, 7, 11), (1,), (4099,), (512, 2048)]


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _flat_params(d, seed=0, extra=()):
    """The flat set + one parameter that never gets a gradient (last)."""
    g = torch.Generator(device=d).manual_seed(seed)
    ps = [torch.randn(s, device=d, generator=g).requires_grad_(True) for s in list(FLAT) + list(extra)]
    return ps, torch.randn(33, device=d, generator=g).requires_grad_(True)


def _cast_set(d, seed=4):
    """The CastCache set of test_fused_adamw_writes_cast_cache_shadows: (linear-like params, convs,
    cache).  With the cache alive FusedAdamW's table has tile, ragged-tile and conv-scatter items."""
    from csu import ops
    g = torch.Generator(device=d).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=d, generator=g).requires_grad_(True)   # noqa: E731
    ps = [r(192, 64), r(70), r(16, 64, 1, 1), r(130, 333), r(5), r(512, 2048)]
    convs = [r(36, 16, 3, 3), r(64, 3, 7, 7), r(256, 128, 3, 3)]
    c = ops.CastCache()
    c.refresh(ps, torch.bfloat16, convs)
    return ps, convs, c


def _shadows(c, ps, convs):
    """Every bf16 layout the cache keeps, as a flat list of tensors."""
    c.refresh(ps, torch.bfloat16, convs)
    out = []
    for p in ps:
        out.append(c.get(p, torch.bfloat16))
        if p.dim() > 1:
            out.append(c.get_t(p.detach().reshape(p.shape[0], -1), torch.bfloat16))
    for w in convs:
        out.extend(t for t in c.get_conv(w, torch.bfloat16) if t is not None)
    return out


def _set_grads(ps, seed, scale=1.0):
    g = torch.Generator(device=ps[0].device).manual_seed(seed)
    for p in ps:
        p.grad = torch.randn(p.shape, device=p.device, generator=g) * scale


def _ref_norm(ps):
    return torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ps if p.grad is not None))


def _coef32(c, norm):
    """min(1, c / (norm + 1e-6)) in IEEE fp32 on the host, from the returned fp32 norm."""
    q = np.float32(c) / (np.float32(float(norm)) + np.float32(1e-6))
    return float(q) if q < 1 else 1.0


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def _state(opt, ps):
    return [opt.state[p][k].clone() for p in ps if p in opt.state and opt.state[p] for k in ("exp_avg", "exp_avg_sq")]


def _all_equal(xs, ys):
    xs, ys = list(xs), list(ys)
    return len(xs) == len(ys) and all(torch.equal(a, b) for a, b in zip(xs, ys))


# ------------------------------------------------------------------------------------- the norm


@pytest.mark.parametrize("which", ["flat", "cast", "big"])
def test_grad_norm_matches_fp64_and_repeats_bitwise(which):
    """opt.grad_norm == sqrt(sum g.double()^2) at rtol 1e-6 on the flat set (+ a parameter without a
    gradient), the CastCache set (tile / ragged-tile / conv items) and the flat set + 2048 x 2048
    (more partials than finish threads); the same gradients again give the bitwise same norm."""
    from csu.optim import FusedAdamW, grad_norm
    d = dev()
    if which == "cast":
        ps, convs, cache = _cast_set(d)
        allp = ps + convs
    else:
        allp, nograd = _flat_params(d, extra=[(2048, 2048)] if which == "big" else [])
    _set_grads(allp, 11)
    if which != "cast":
        allp = allp + [nograd]
    opt = FusedAdamW(allp, lr=1e-3, max_grad_norm=1.0)
    opt.step()
    n1 = opt.grad_norm.clone()
    want = _ref_norm(allp)
    print(f"{which}: norm {float(n1):.9g} fp64 {float(want):.12g} rel err {_rel(n1, want):.3e}")
    torch.testing.assert_close(n1.double(), want, rtol=1e-6, atol=0)
    opt.step()                                     # the fused path leaves p.grad unscaled: same input
    assert torch.equal(opt.grad_norm, n1)
    # the stand-alone norm (flat items over the same gradients)
    a, b = grad_norm(allp), grad_norm(allp)
    torch.testing.assert_close(a.double(), want, rtol=1e-6, atol=0)
    assert torch.equal(a, b)
    if which == "big":
        chunk = 4096
        assert sum(-(-p.numel() // chunk) for p in allp if p.grad is not None) > 1024


@pytest.mark.parametrize("fill", [1e-30, 1e25])
def test_grad_norm_of_tiny_and_huge_gradients(fill):
    """fp32 squares of 1e-30 underflow to 0 and of 1e25 overflow to inf: the element goes to fp64
    before it is squared, on the flat, tile and conv paths."""
    from csu.optim import FusedAdamW, grad_norm
    d = dev()
    ps, convs, cache = _cast_set(d)
    allp = ps + convs
    for p in allp:
        p.grad = torch.full_like(p, fill)
    want = _ref_norm(allp)
    opt = FusedAdamW(allp, lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True)
    opt.step()
    print(f"fill {fill}: norm {float(opt.grad_norm):.9g} fp64 {float(want):.12g}")
    torch.testing.assert_close(opt.grad_norm.double(), want, rtol=1e-6, atol=0)
    assert int(opt.skipped_steps) == 0 and float(opt._ctl[2]) == 1.0
    torch.testing.assert_close(grad_norm(allp).double(), want, rtol=1e-6, atol=0)


def test_finish_sums_many_partials_in_fp64():
    """csu_grad_norm_finish over n = 5000 partials (several rounds of the strided loop, its 4-deep
    part included) and n = 1, 63, 1025: norm vs torch's fp64 sum, and the ctl layout."""
    from csu._lib import check, lib, stream_ptr
    d = dev()
    g = torch.Generator(device=d).manual_seed(2)
    for n in (1, 63, 1025, 5000):
        part = torch.rand(n, device=d, generator=g, dtype=torch.float64) * 10
        ctl = torch.full((4,), -1.0, device=d)
        check(lib().csu_grad_norm_finish(part.data_ptr(), n, 2.0, ctl.data_ptr(), stream_ptr(d)), "finish")
        want = torch.sqrt(part.sum())
        torch.testing.assert_close(ctl[0].double(), want, rtol=1e-6, atol=0)
        assert float(ctl[1]) == _coef32(2.0, ctl[0]) and float(ctl[2]) == 1.0 and float(ctl[3]) == 0.0
    # norm-only modes: max_norm <= 0 or infinite -> coefficient exactly 1
    for mx in (0.0, -1.0, float("inf")):
        check(lib().csu_grad_norm_finish(part.data_ptr(), n, mx, ctl.data_ptr(), stream_ptr(d)), "finish")
        assert float(ctl[1]) == 1.0
    part[17] = float("inf")
    check(lib().csu_grad_norm_finish(part.data_ptr(), n, 2.0, ctl.data_ptr(), stream_ptr(d)), "finish")
    assert float(ctl[2]) == 0.0 and float(ctl[0]) == float("inf") and float(ctl[1]) == 0.0


def test_clip_coefficient_formula():
    """ctl's coefficient == min(1, c / (norm + 1e-6)) in fp32 from the returned norm; exactly 1.0
    when c exceeds the norm."""
    from csu.optim import FusedAdamW
    d = dev()
    allp, _ = _flat_params(d)
    _set_grads(allp, 3)
    norm = float(_ref_norm(allp))
    for c in (0.5 * norm, 1e-3, 0.999 * norm, 1.001 * norm, 10 * norm):
        opt = FusedAdamW(allp, lr=0.0, weight_decay=0.0, max_grad_norm=c)
        opt.step()
        want = _coef32(c, opt.grad_norm)
        assert float(opt._ctl[1]) == want, (c, float(opt._ctl[1]), want)
        if c > 1.0005 * norm:
            assert float(opt._ctl[1]) == 1.0
        else:
            assert float(opt._ctl[1]) < 1.0


# ------------------------------------------------------------- fused clip == scale, then step


def _twin(ps):
    return [p.detach().clone().requires_grad_(True) for p in ps]


def test_fused_clip_is_bitwise_scale_then_step_cast_set():
    """3 steps of FusedAdamW(max_grad_norm = c ~ half the norm) on the CastCache set == plain
    FusedAdamW fed g * coef (coef read back from the first optimizer each step): parameters, both
    moments and every bf16 shadow torch.equal."""
    from csu import ops
    from csu.optim import FusedAdamW
    d = dev()
    ps, convs, c1 = _cast_set(d)
    ps2, convs2 = _twin(ps), _twin(convs)
    c2 = ops.CastCache()
    c2.refresh(ps2, torch.bfloat16, convs2)
    a, b = ps + convs, ps2 + convs2
    _set_grads(a, 100)
    cval = 0.5 * float(_ref_norm(a))
    o1 = FusedAdamW(a, lr=1e-2, weight_decay=1e-2, max_grad_norm=cval)
    o2 = FusedAdamW(b, lr=1e-2, weight_decay=1e-2)
    for it in range(3):
        _set_grads(a, 100 + it, scale=1.0 + 0.3 * it)
        o1.step()
        coef = o1._ctl[1].clone()
        assert float(coef) < 1.0
        for p, q in zip(a, b):
            q.grad = p.grad * coef
        o2.step()
        _shadows(c1, ps, convs), _shadows(c2, ps2, convs2)
    assert _all_equal((p.detach() for p in a), (q.detach() for q in b))
    assert _all_equal(_state(o1, a), _state(o2, b))
    s1, s2 = _shadows(c1, ps, convs), _shadows(c2, ps2, convs2)
    assert len(s1) >= len(ps) + len(convs) and _all_equal(s1, s2)
    for p in ps:                                     # and the shadows are the bf16 image of the weights
        assert torch.equal(c1.get(p, torch.bfloat16), p.detach().bfloat16())


@pytest.mark.parametrize("l2", [False, True])
def test_fused_clip_is_bitwise_scale_then_step_flat(l2):
    """The same on the flat set (ragged tails, a parameter without a gradient) for FusedAdamW and for
    FusedAdam with a non-zero weight_decay (the product must not be contracted into the L2 fmaf)."""
    from csu.optim import FusedAdam, FusedAdamW
    cls = FusedAdam if l2 else FusedAdamW
    d = dev()
    a, na = _flat_params(d)
    b, nb = _twin(a), None
    _set_grads(a, 7)
    cval = 0.5 * float(_ref_norm(a))
    o1 = cls(a + [na], lr=1e-2, weight_decay=0.05, max_grad_norm=cval)
    o2 = cls(b, lr=1e-2, weight_decay=0.05)
    for it in range(3):
        _set_grads(a, 7 + it)
        o1.step()
        coef = o1._ctl[1].clone()
        assert float(coef) < 1.0
        for p, q in zip(a, b):
            q.grad = p.grad * coef
        o2.step()
    assert _all_equal((p.detach() for p in a), (q.detach() for q in b))
    assert _all_equal(_state(o1, a), _state(o2, b))
    assert na not in o1.state or not o1.state[na]


def test_clip_above_norm_equals_unclipped():
    """c above the norm: coefficient exactly 1, the result torch.equal to the unclipped optimizer."""
    from csu import ops
    from csu.optim import FusedAdamW
    d = dev()
    ps, convs, c1 = _cast_set(d)
    ps2, convs2 = _twin(ps), _twin(convs)
    c2 = ops.CastCache()
    c2.refresh(ps2, torch.bfloat16, convs2)
    a, b = ps + convs, ps2 + convs2
    o1 = FusedAdamW(a, lr=1e-2, weight_decay=1e-2, max_grad_norm=1e9)
    o2 = FusedAdamW(b, lr=1e-2, weight_decay=1e-2)
    for it in range(3):
        _set_grads(a, 40 + it)
        for p, q in zip(a, b):
            q.grad = p.grad.clone()
        o1.step()
        o2.step()
        assert float(o1._ctl[1]) == 1.0
    assert _all_equal((p.detach() for p in a), (q.detach() for q in b))
    assert _all_equal(_state(o1, a), _state(o2, b))
    assert _all_equal(_shadows(c1, ps, convs), _shadows(c2, ps2, convs2))


# ------------------------------------------------------------------------------- against torch


@pytest.mark.parametrize("capturable", [False, True])
def test_fused_clip_matches_torch_clip_then_adamw(capturable):
    """6 steps of clip_grad_norm_ + torch.optim.AdamW(foreach=False) vs FusedAdamW(max_grad_norm) at
    the tolerances of test_fused_adamw_matches_torch (incl. its lr change)."""
    from csu.optim import FusedAdamW
    d = dev()
    g = torch.Generator(device=d).manual_seed(0)
    ps = [torch.randn(s, device=d, generator=g) for s in FLAT]
    ref = [p.clone().requires_grad_(True) for p in ps]
    mine = [p.clone().requires_grad_(True) for p in ps]
    cval = 0.5 * float(sum(p.numel() for p in ps)) ** 0.5       # half the expected norm of N(0, 1) gradients
    o_ref = torch.optim.AdamW(ref, lr=1e-3, weight_decay=1e-2, foreach=False)
    o_mine = FusedAdamW(mine, lr=1e-3, weight_decay=1e-2, capturable=capturable, max_grad_norm=cval)
    for it in range(6):
        if it == 3:
            for o in (o_ref, o_mine):
                o.param_groups[0]["lr"] = 5e-4
            o_mine.sync_lr()
        grads = [torch.randn(s, device=d, generator=g) for s in FLAT]
        for p, q, gr in zip(ref, mine, grads):
            p.grad, q.grad = gr.clone(), gr.clone()
        tn = torch.nn.utils.clip_grad_norm_(ref, cval)
        o_ref.step()
        o_mine.step()
        assert float(tn) > cval
        torch.testing.assert_close(o_mine.grad_norm.double(), _ref_norm(mine), rtol=1e-6, atol=0)
    for p, q in zip(ref, mine):
        torch.testing.assert_close(q.detach(), p.detach(), rtol=1e-5, atol=1e-6)
    for p, q in zip(ref, mine):
        torch.testing.assert_close(o_mine.state[q]["exp_avg"], o_ref.state[p]["exp_avg"], rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(o_mine.state[q]["exp_avg_sq"], o_ref.state[p]["exp_avg_sq"], rtol=5e-5, atol=1e-9)
    assert float(o_mine.state[mine[0]]["step"]) == 6.0


def test_standalone_clip_grad_norm_matches_torch():
    """csu.optim.clip_grad_norm_ vs torch.nn.utils.clip_grad_norm_: returned norm and the gradients
    afterwards at rtol 1e-6 (a gradient buffer off a 16-B boundary and a parameter without a
    gradient included); c above the norm leaves the gradients bitwise alone."""
    from csu.optim import clip_grad_norm_
    d = dev()
    a, na = _flat_params(d)
    _set_grads(a, 21)
    buf = torch.randn(4 * 1000 + 1, device=d)
    buf0 = buf.clone()
    a[4].grad = torch.randn(4100, device=d)[1:]          # 4099 elements starting 4 B into an allocation
    odd = torch.zeros(4000, device=d).requires_grad_(True)
    odd.grad = buf[1:]                                    # numel % 4 == 0 but off a 16-B boundary
    assert odd.grad.data_ptr() % 16 == 4 and odd.grad.is_contiguous()
    a = a + [odd, na]
    b = _twin(a)
    for p, q in zip(a, b):
        q.grad = None if p.grad is None else p.grad.clone()
    before = [p.grad.clone() for p in a if p.grad is not None]
    norm = float(_ref_norm(a))
    n1 = clip_grad_norm_(a, 0.5 * norm)
    n2 = torch.nn.utils.clip_grad_norm_(b, 0.5 * norm)
    assert n1.is_cuda and n1.dim() == 0
    assert _rel(n1, norm) < 1e-6
    torch.testing.assert_close(n1, n2, rtol=1e-6, atol=0)
    for p, q, g0 in zip([p for p in a if p.grad is not None], [q for q in b if q.grad is not None], before):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-6, atol=0)
        assert not torch.equal(p.grad, g0)
    assert na.grad is None
    now = [p.grad.clone() for p in a if p.grad is not None]
    clip_grad_norm_(a, 10 * norm)
    assert _all_equal(now, [p.grad for p in a if p.grad is not None])
    assert torch.equal(buf[0], buf0[0])              # the element in front of the view is untouched


# ---------------------------------------------------------------------------- non-finite steps


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_skip_nonfinite_leaves_everything_untouched(bad):
    """One gradient element inf / NaN with skip_nonfinite=True: parameters, moments, shadows and the
    step count bitwise unchanged, skipped_steps == 1, and the next clean step equals the step of a
    twin that never saw the bad gradient."""
    from csu import ops
    from csu.optim import FusedAdamW
    d = dev()
    ps, convs, c1 = _cast_set(d)
    ps2, convs2 = _twin(ps), _twin(convs)
    c2 = ops.CastCache()
    c2.refresh(ps2, torch.bfloat16, convs2)
    a, b = ps + convs, ps2 + convs2
    _set_grads(a, 60)
    cval = 0.5 * float(_ref_norm(a))
    o1 = FusedAdamW(a, lr=1e-2, weight_decay=1e-2, max_grad_norm=cval, skip_nonfinite=True)
    o2 = FusedAdamW(b, lr=1e-2, weight_decay=1e-2, max_grad_norm=cval, skip_nonfinite=True)

    def both(seed):
        _set_grads(a, seed)
        for p, q in zip(a, b):
            q.grad = p.grad.clone()
        o1.step()
        o2.step()

    both(60)
    snap = [p.detach().clone() for p in a] + _state(o1, a) + [s.clone() for s in _shadows(c1, ps, convs)]
    _set_grads(a, 61)
    a[3].grad.view(-1)[12345] = bad                  # inside the ragged-tile matrix 130 x 333
    o1.step()
    assert float(o1._ctl[2]) == 0.0 and int(o1.skipped_steps) == 1
    assert not bool(torch.isfinite(o1.grad_norm))
    after = [p.detach() for p in a] + _state(o1, a) + _shadows(c1, ps, convs)
    assert _all_equal(snap, after)
    assert all(float(o1.state[p]["step"]) == 1.0 for p in a)
    both(62)
    assert int(o1.skipped_steps) == 1 and int(o2.skipped_steps) == 0
    assert all(float(o1.state[p]["step"]) == 2.0 for p in a)
    assert _all_equal((p.detach() for p in a), (q.detach() for q in b))
    assert _all_equal(_state(o1, a), _state(o2, b))
    assert _all_equal(_shadows(c1, ps, convs), _shadows(c2, ps2, convs2))


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_without_skip_behaves_as_torch(bad):
    """skip_nonfinite=False: ordinary arithmetic on the inf / NaN values -- the same parameters
    become non-finite as with clip_grad_norm_ + torch.optim.AdamW (inf: norm inf, coefficient 0,
    inf * 0 = NaN at the bad element only; NaN: the coefficient is NaN, everything is)."""
    from csu.optim import FusedAdamW
    d = dev()
    a, na = _flat_params(d)
    b = _twin(a)
    _set_grads(a, 80)
    a[4].grad[4098] = bad
    for p, q in zip(a, b):
        q.grad = p.grad.clone()
    o1 = FusedAdamW(a + [na], lr=1e-2, weight_decay=1e-2, max_grad_norm=1.0)
    o2 = torch.optim.AdamW(b, lr=1e-2, weight_decay=1e-2, foreach=False)
    o1.step()
    torch.nn.utils.clip_grad_norm_(b, 1.0)
    o2.step()
    assert not bool(torch.isfinite(a[4].detach()).all())
    for p, q in zip(a, b):
        assert torch.equal(torch.isfinite(p.detach()), torch.isfinite(q.detach()))
    assert bool(torch.isfinite(na.detach()).all()) and int(o1.skipped_steps) == 0
    assert float(o1.state[a[0]]["step"]) == 1.0


# ----------------------------------------------------------------------------- the captured step


def _model_and_batches(d, n, seed=1, batch=4):
    from csu.data import ellipse_batch
    from csu.model import CSWinTransformer
    torch.manual_seed(0)
    m0 = CSWinTransformer(img_size=128, split_size=[1, 2, 4, 4])
    rng = np.random.default_rng(seed)
    return m0, [tuple(t.to(d) for t in ellipse_batch(rng, batch, 128)) for _ in range(n)]


def _probe_norm(m0, batch, d):
    """Pre-clip gradient norm of one eager bf16 step of a copy of the model."""
    from csu.optim import grad_norm
    from csu.train import bce_loss
    m = copy.deepcopy(m0).to(d)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(batch[0])
    bce_loss(out, batch[1]).backward()
    n = float(grad_norm(list(m.parameters())))
    assert np.isfinite(n) and n > 0
    return n


def test_graph_replays_with_clip_bitwise_reproducible():
    """Two independent captures of the bf16 train step with max_grad_norm set (clipping active)
    replay to bitwise-equal losses, parameters and grad_norm values."""
    from csu.train import GraphedTrainStep, bce_loss, make_optimizer
    d = dev()
    m0, batches = _model_and_batches(d, 2)
    # the norm falls several-fold over the first steps (the replays follow two warm-up steps): a
    # small fraction of the first step's norm keeps the clip active in the replays
    cval = 0.05 * _probe_norm(m0, batches[0], d)
    res = []
    for _ in range(2):
        m = copy.deepcopy(m0).to(d)
        opt = make_optimizer(m, capturable=True, max_grad_norm=cval)
        gs = GraphedTrainStep(m, opt, bce_loss, batches[0][0], batches[0][1], torch.bfloat16, warmup=2)
        gn_ptr = opt.grad_norm.data_ptr()
        losses, norms, coefs = [], [], []
        for i in range(5):
            losses.append(float(gs(*batches[i % 2])[0].item()))
            norms.append(float(opt.grad_norm))
            coefs.append(float(opt._ctl[1]))
        torch.cuda.synchronize()
        assert opt.grad_norm.data_ptr() == gn_ptr         # same storage across replays
        assert min(coefs) < 1.0 and max(norms) > cval, (coefs, norms, cval)   # the clip is active
        res.append((losses, norms, [p.detach().clone() for p in m.parameters()]))
        del gs, opt
    assert res[0][0] == res[1][0]
    assert res[0][1] == res[1][1]
    names = [n for n, _ in m0.named_parameters()]
    diff = [(n, float((a - b).abs().max())) for n, a, b in zip(names, res[0][2], res[1][2]) if not torch.equal(a, b)]
    assert not diff, diff


def test_clip_acts_inside_the_graph():
    """With c tiny (1e-3) the parameter change of one replay is smaller than without clipping (the
    clipped gradients fall towards AdamW's eps, which then damps the normalised update)."""
    from csu.train import GraphedTrainStep, bce_loss, make_optimizer
    d = dev()
    m0, batches = _model_and_batches(d, 1)
    delta = {}
    for c in (None, 1e-3):
        m = copy.deepcopy(m0).to(d)
        opt = make_optimizer(m, capturable=True, max_grad_norm=c)
        gs = GraphedTrainStep(m, opt, bce_loss, batches[0][0], batches[0][1], torch.bfloat16, warmup=1)
        before = [p.detach().clone() for p in m.parameters()]
        gs(*batches[0])
        torch.cuda.synchronize()
        delta[c] = sum(float((p.detach() - q).abs().sum()) for p, q in zip(m.parameters(), before))
        if c is not None:
            assert float(opt._ctl[1]) < 1.0 and float(opt.grad_norm) > c
        del gs, opt
    print(f"sum |dp| of one replay: unclipped {delta[None]:.6g}, max_grad_norm 1e-3 {delta[1e-3]:.6g}")
    assert 0 < delta[1e-3] < delta[None]


def test_train_model_graphed_equals_eager_with_clip():
    """train_model graph=None (two eager steps, then replays; a ragged last batch eager) == graph=False
    with clipping on, at the tolerances of test_train_model_graphed_equals_eager, history["grad_norm"]
    and history["skipped_steps"] included."""
    from csu.data import ellipse_batch
    from csu.train import bce_loss, make_optimizer, train_model
    d = dev()
    m0, _ = _model_and_batches(d, 0)
    rng = np.random.default_rng(8)
    train = [ellipse_batch(rng, 4, 128) for _ in range(5)] + [ellipse_batch(rng, 2, 128)]
    test = [ellipse_batch(rng, 4, 128), ellipse_batch(rng, 3, 128)]
    cval = 0.05 * _probe_norm(m0, tuple(t.to(d) for t in train[0]), d)   # active beyond the first steps too
    hs, ps = [], []
    for graph in (None, False):
        m = copy.deepcopy(m0).to(d)
        opt = make_optimizer(m, max_grad_norm=cval, skip_nonfinite=True)
        hs.append(train_model(m, train, test, bce_loss, opt, None, d, num_epochs=2, verbose=False, graph=graph))
        ps.append([p.detach().clone() for p in m.parameters()])
    assert set(hs[0]) == set(hs[1]) and {"grad_norm", "skipped_steps"} <= set(hs[0])
    assert hs[0]["skipped_steps"] == [0, 0] and max(hs[0]["grad_norm"]) > cval
    for k in hs[0]:
        np.testing.assert_allclose(hs[0][k], hs[1][k], rtol=1e-5, atol=1e-6, err_msg=k)
    for a, b in zip(*ps):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
