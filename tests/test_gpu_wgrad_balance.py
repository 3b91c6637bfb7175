"""Grouped weight gradients launched with the group-aware plan (csu_linear_wgrad_group_plan_all +
csu_linear_wgrad_group_planned + csu_wslab_reduce_batch) against the per-Linear kernel
(ops.linear_wgrad: fp32 sums in another chunk order, relative Frobenius error < 1e-5, the bound of
test_linear_wgrad_grouped) and against themselves (bitwise).  cus = 2 in the plan so that the small
token counts still come out in several chunks."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MIXED = [(100, 64, 64), (4097, 256, 128), (2112, 128, 128), (1536, 128, 64), (1536, 64, 128), (8192, 768, 256),
         (3000, 256, 256)]
FIFTY = [(2112 + 64 * (i % 5), 64, 64) for i in range(50)]   # more than one launch of <= 48 items


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _inputs(shapes, seed):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return [((torch.randn(M, N, device=dev(), generator=g) * 0.1).bfloat16(), torch.randn(M, K, device=dev(), generator=g).bfloat16())
            for M, N, K in shapes]


def _plan(shapes, cus):
    from csu import _lib
    n = len(shapes)
    items = (_lib.WgradGroupItem * n)(*[_lib.WgradGroupItem(None, None, None, None, *s) for s in shapes])
    plans = (_lib.WgradGroupPlan * n)()
    assert _lib.lib().csu_linear_wgrad_group_plan_all(items, n, cus, plans) == 0
    return plans


def _run(shapes, ins, plans, reduce=True):
    """The planned launches + the batched slab sums; outputs pre-filled with NaN."""
    from csu import _lib
    L, d, n = _lib.lib(), dev(), len(shapes)
    outs = [torch.full((N * K + N,), float("nan"), device=d) for _, N, K in shapes]
    slabs = [torch.empty(p.slab_bytes // 4, device=d) if p.slab_bytes else None for p in plans]
    items = (_lib.WgradGroupItem * n)(*[
        _lib.WgradGroupItem(dy.data_ptr(), x.data_ptr(), o.data_ptr(), sl.data_ptr() if sl is not None else None, *s)
        for s, (dy, x), o, sl in zip(shapes, ins, outs, slabs)])
    st = torch.cuda.current_stream().cuda_stream
    assert L.csu_linear_wgrad_group_planned(items, plans, n, st) == 0, L.csu_last_error_string()
    if reduce:
        multi = [i for i in range(n) if plans[i].chunks > 1]
        if multi:
            ws = (_lib.WslabItem * len(multi))(*[
                _lib.WslabItem(slabs[i].data_ptr(), outs[i].data_ptr(), shapes[i][1], shapes[i][2], plans[i].tn, plans[i].tk,
                               plans[i].chunks, 0) for i in multi])
            assert L.csu_wslab_reduce_batch(ws, len(multi), st) == 0
    torch.cuda.synchronize()
    return outs


def _check(shapes, ins, outs):
    from csu import ops
    for (M, N, K), (dy, x), o in zip(shapes, ins, outs):
        dw, db = ops.linear_wgrad(dy, x)
        for got, want in ((o[:N * K].view(N, K), dw), (o[N * K:], db)):
            err = float((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-30))
            print(f"({M}, {N}, {K}): rel {err:.2e}")
            assert err < 1e-5, (M, N, K, err)


@pytest.mark.parametrize("name,shapes", [("mixed", MIXED), ("fifty", FIFTY)])
def test_planned_group_matches_per_linear_kernel(name, shapes):
    ins = _inputs(shapes, 11)
    plans = _plan(shapes, 2)
    if name == "mixed":
        assert max(p.chunks for p in plans) > 1 and min(p.chunks for p in plans) == 1
    else:
        assert len({p.launch for p in plans}) >= 2
    a = _run(shapes, ins, plans)
    b = _run(shapes, ins, plans)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    _check(shapes, ins, a)


def test_one_chunk_items_write_their_result_directly():
    """chunks == 1: no slab (slab_bytes 0, a null slab pointer is accepted) and dw_db complete after
    the tile launch alone; through ops, only the items with chunks > 1 queue a slab sum."""
    from csu import ops
    ins = _inputs(MIXED, 12)
    plans = _plan(MIXED, 2)
    outs = _run(MIXED, ins, plans, reduce=False)
    ones = [i for i, p in enumerate(plans) if p.chunks == 1]
    assert ones and all(plans[i].slab_bytes == 0 for i in ones)
    _check([MIXED[i] for i in ones], [ins[i] for i in ones], [outs[i] for i in ones])

    class Recorder(list):
        seen = 0

        def append(self, v):
            Recorder.seen += 1
            list.append(self, v)
    old = ops._WG_PENDING
    ops._WG_PENDING = Recorder()
    try:
        assert ops.BALANCE_WGRAD
        res = [ops.linear_wgrad(dy, x, defer=True) for dy, x in ins]
        ops._wgrad_flush()
        torch.cuda.synchronize()
    finally:
        ops._WG_PENDING = old
    assert Recorder.seen == sum(p.chunks > 1 for p in _plan(MIXED, 0))
    _check(MIXED, ins, [torch.cat([w.reshape(-1), b]) for w, b in res])


def test_forced_plans_one_token_last_chunk():
    """The launch entry with hand-made plans: a last chunk of ONE token on the 8-wave 256 x 128 tile
    and on the 64 x 64 tile, beside whole chunks; a plan that does not cover the tokens is refused."""
    from csu import _lib
    shapes = [(4097, 256, 128), (4097, 256, 128), (2049, 64, 64)]
    rpcs = [2048, 4096, 1024]
    ins = _inputs(shapes, 13)
    plans = _plan(shapes, 2)
    for i, ((M, N, K), r) in enumerate(zip(shapes, rpcs)):
        p = plans[i]
        p.rpc, p.chunks = r, -(-M // r)
        p.slab_bytes = (-(-N // p.tn) * -(-K // p.tk) * p.tn * p.tk + -(-N // p.tn) * p.tn) * p.chunks * 4
        p.launch, p.pos = (0 if p.tn == 256 else 1), i
    _check(shapes, ins, _run(shapes, ins, plans))
    plans[0].chunks = 2
    n = len(shapes)
    dummy = torch.zeros(1 << 20, device=dev())
    items = (_lib.WgradGroupItem * n)(*[_lib.WgradGroupItem(dy.data_ptr(), x.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), *s)
                                        for s, (dy, x) in zip(shapes, ins)])
    assert _lib.lib().csu_linear_wgrad_group_planned(items, plans, n, torch.cuda.current_stream().cuda_stream) != 0
    torch.cuda.synchronize()


def test_captured_step_reproduces_with_and_without_balance(monkeypatch):
    """One captured bf16 step of the 128 x 128 model (tools/launch_trace.py's), balance on and off:
    each setting reproduces itself bitwise over two independent captures."""
    from csu import ops
    from csu.data import ellipse_batch
    from csu.model import CSWinTransformer
    from csu.train import GraphedTrainStep, bce_loss, make_optimizer
    d = dev()
    torch.manual_seed(0)
    m0 = CSWinTransformer(img_size=128, split_size=[1, 2, 4, 4])
    x, t = (v.to(d) for v in ellipse_batch(np.random.default_rng(1), 4, 128))
    for on in (True, False):
        monkeypatch.setattr(ops, "BALANCE_WGRAD", on)
        res = []
        for _ in range(2):
            m = copy.deepcopy(m0).to(d)
            opt = make_optimizer(m, capturable=True)
            gs = GraphedTrainStep(m, opt, bce_loss, x, t, torch.bfloat16, warmup=1)
            loss = float(gs(x, t)[0].item())
            torch.cuda.synchronize()
            res.append((loss, [p.detach().clone() for p in m.parameters()]))
            del gs, opt
        assert res[0][0] == res[1][0], on
        assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1])), on
