"""Weight EMA, CPU side: csu.ema.WeightEMA on a CPU module against the fp64 recurrence, the warmup
schedule, applied() / swap(), the state_dict round trip, make_optimizer / train_step / train_model
with ``ema_decay`` on a CPU module, checkpoints with and without the ``"ema"`` entry, and the three
C ABI exports with their argument validation.

Tolerance of the recurrence tests: one update e + w (p - e) makes two fp32 roundings, each at most
2^-24 relative to values of at most 2 max(|p|, |e|); over 8 updates that is about 1.5e-6 max, so
|e - e64| <= 4e-6 max(|p|, |e|) has margin and nothing else."""
import copy

import numpy as np
import pytest
import torch

NEW_SYMBOLS = ["csu_adamw_step_ema", "csu_ema_update", "csu_ema_swap"]


def _net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, padding=1), torch.nn.BatchNorm2d(4), torch.nn.ReLU(),
                               torch.nn.Conv2d(4, 1, 1), torch.nn.Sigmoid())


def _batches(n, b=2, s=8, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(b, 3, s, s, generator=g), (torch.rand(b, 1, s, s, generator=g) > 0.5).float()) for _ in range(n)]


def _perturb(m, g):
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.1)


def test_library_exports_ema_symbols():
    from csu import _lib
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert n in _lib._SIGS, n
    # argument errors are reported before any device work
    assert L.csu_ema_update(None, None, 0, 0, None, 0.9, 0, None) != 0
    assert L.csu_ema_swap(None, None, 0, 0, None) != 0
    assert L.csu_adamw_step_ema(None, 0, 0, None, 0.0, 0.9, 0.999, 1e-8, 0.0, None, 1.0, None, 0, 0, None, None, 0.9, 0,
                                None) != 0


def test_cpu_ema_matches_fp64_recurrence():
    from csu.ema import WeightEMA
    m = _net()
    ema = WeightEMA(m, decay=0.9, warmup=False)
    assert len(ema.tensors) == len(list(m.parameters()))
    assert all(torch.equal(e, p.detach()) and e.data_ptr() != p.data_ptr() for e, p in zip(ema.tensors, m.parameters()))
    ref = [p.detach().double().clone() for p in m.parameters()]
    big = [p.detach().abs().double() for p in m.parameters()]
    g = torch.Generator().manual_seed(0)
    d = float(np.float32(0.9))
    for _ in range(8):
        _perturb(m, g)
        ema.update()
        for r, b, p in zip(ref, big, m.parameters()):
            r.mul_(d).add_(p.detach().double(), alpha=1 - d)
            torch.maximum(b, torch.maximum(p.detach().abs().double(), r.abs()), out=b)
    assert ema.num_updates == 8
    for e, r, b in zip(ema.tensors, ref, big):
        assert bool(((e.double() - r).abs() <= 4e-6 * b).all())
    # buffers are not averaged
    assert not any(n.endswith("running_mean") for n in ema.names)


def test_warmup_schedule():
    """A parameter held at 0 before and 1 after: e_n = 1 - prod d_k, so d_n is recovered from two
    consecutive values; d_n = min(decay, n / (n + 9)), i.e. (1 + t) / (10 + t) for t = n - 1."""
    from csu.ema import WeightEMA
    lin = torch.nn.Linear(4, 4, bias=False)
    with torch.no_grad():
        lin.weight.zero_()
    ema = WeightEMA(lin, decay=0.5, warmup=True)
    with torch.no_grad():
        lin.weight.fill_(1.0)
    prev, prod = 0.0, 1.0
    for n in range(1, 14):
        want = min(0.5, n / (n + 9))
        assert ema.current_decay() == pytest.approx(want, rel=1e-6)
        ema.update()
        e = float(ema.tensors[0][0, 0])
        # one update's absolute error on values <= 1: d, w = 1 - d, p - e and the fma each round at
        # <= 2^-24 -> <= 2.5e-7 per update, n of them on e; dividing by 1 - prev amplifies it
        prod *= want
        assert abs((1.0 - e) - prod) <= n * 2.5e-7, n
        if 1.0 - prev > 1e-3:
            d = (1.0 - e) / (1.0 - prev)          # e = d prev + (1 - d) 1
            assert abs(d - want) <= 2 * n * 2.5e-7 / (1.0 - prev), n
        prev = e
    assert min(0.5, 9 / 18) == 0.5 and ema.current_decay() == pytest.approx(0.5, rel=1e-6)   # capped from n = 9 on
    with pytest.raises(ValueError):
        WeightEMA(lin, decay=1.5)


def test_applied_swaps_and_restores_also_on_exception():
    from csu.ema import WeightEMA
    m = _net()
    ema = WeightEMA(m, decay=0.5, warmup=False)
    _perturb(m, torch.Generator().manual_seed(1))
    ema.update()
    p0 = [p.detach().clone() for p in m.parameters()]
    e0 = [e.clone() for e in ema.tensors]
    bn0 = m[1].running_mean.clone()
    assert not any(torch.equal(a, b) for a, b in zip(p0, e0))
    with ema.applied():
        assert ema.swapped
        assert all(torch.equal(p.detach(), e) for p, e in zip(m.parameters(), e0))
        assert all(torch.equal(e, p) for e, p in zip(ema.tensors, p0))
        assert torch.equal(m[1].running_mean, bn0)          # the live buffers are used
        with pytest.raises(RuntimeError):
            with ema.applied():                             # nested use
                pass
        with pytest.raises(RuntimeError):
            ema.update()
        sd_in = ema.model_state_dict()
    assert not ema.swapped
    assert all(torch.equal(p.detach(), q) for p, q in zip(m.parameters(), p0))
    assert all(torch.equal(e, q) for e, q in zip(ema.tensors, e0))
    with pytest.raises(KeyError):
        with ema.applied():
            raise KeyError("boom")
    assert not ema.swapped
    assert all(torch.equal(p.detach(), q) for p, q in zip(m.parameters(), p0))
    assert all(torch.equal(e, q) for e, q in zip(ema.tensors, e0))
    # model_state_dict: the averages under the parameter names, buffers as they are, whichever side is live
    sd = ema.model_state_dict()
    assert list(sd) == list(m.state_dict())
    for n, e in zip(ema.names, e0):
        assert torch.equal(sd[n], e) and torch.equal(sd_in[n], e)
    assert torch.equal(sd["1.running_mean"], bn0)
    m2 = _net()
    m2.load_state_dict(sd)
    assert all(torch.equal(p.detach(), e) for p, e in zip(m2.parameters(), e0))


def test_state_dict_round_trip_keeps_tensors_in_place():
    from csu.ema import WeightEMA
    m = _net()
    ema = WeightEMA(m, decay=0.75, warmup=True)
    g = torch.Generator().manual_seed(2)
    for _ in range(3):
        _perturb(m, g)
        ema.update()
    sd = ema.state_dict()
    assert set(sd) == {"decay", "warmup", "num_updates", "ema"} and sd["num_updates"] == 3
    assert list(sd["ema"]) == ema.names
    assert all(v.data_ptr() != e.data_ptr() for v, e in zip(sd["ema"].values(), ema.tensors))
    ema2 = WeightEMA(_net(), decay=0.1, warmup=False)
    ptrs = [e.data_ptr() for e in ema2.tensors]
    ema2.load_state_dict(sd)
    assert [e.data_ptr() for e in ema2.tensors] == ptrs
    assert (ema2.decay, ema2.warmup, ema2.num_updates) == (0.75, True, 3)
    assert all(torch.equal(a, b) for a, b in zip(ema.tensors, ema2.tensors))
    # and both continue identically
    for e_, m_ in ((ema, m), (ema2, ema2.model)):
        with torch.no_grad():
            for p in m_.parameters():
                p.fill_(0.25)
        e_.update()
    assert all(torch.equal(a, b) for a, b in zip(ema.tensors, ema2.tensors))
    bad = dict(sd, ema={k + "x": v for k, v in sd["ema"].items()})
    with pytest.raises(KeyError):
        ema2.load_state_dict(bad)


def test_make_optimizer_cpu_attaches_ema_and_train_step_updates_it():
    from csu.ema import WeightEMA
    from csu.train import bce_loss, make_optimizer, train_step
    m = _net()
    o = make_optimizer(m, lr=1e-2, ema_decay=0.9, ema_warmup=False)
    assert isinstance(o, torch.optim.AdamW) and isinstance(o.ema, WeightEMA)
    assert (o.ema.decay, o.ema.warmup, o.ema.num_updates) == (float(0.9), False, 0)
    assert make_optimizer(m).ema is None
    # by hand: the same steps on a copy, ema.update() after each
    m2 = copy.deepcopy(m)
    o2 = torch.optim.AdamW(m2.parameters(), lr=1e-2, weight_decay=1e-4)
    ema2 = WeightEMA(m2, decay=0.9, warmup=False)
    for x, t in _batches(3):
        train_step(m, x, t, bce_loss, o)
        o2.zero_grad(set_to_none=True)
        bce_loss(m2(x), t).backward()
        o2.step()
        ema2.update()
    assert o.ema.num_updates == 3
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(m.parameters(), m2.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(o.ema.tensors, ema2.tensors))
    assert not all(torch.equal(e, p.detach()) for e, p in zip(o.ema.tensors, m.parameters()))


def test_train_model_cpu_ema_history_and_resume(tmp_path):
    from csu.train import bce_loss, evaluate_model, make_optimizer, train_model
    base = {"train_loss", "train_dice", "train_iou", "test_loss", "test_dice", "test_iou", "learning_rates"}
    train, test = _batches(3), _batches(1, seed=6)
    m = _net()
    opt = make_optimizer(m, lr=1e-2, ema_decay=0.9)
    h = train_model(m, train, test, bce_loss, opt, None, "cpu", num_epochs=2, verbose=False)
    assert set(h) == base | {"ema_test_loss", "ema_test_dice", "ema_test_iou"}
    assert all(len(v) == 2 for v in h.values())
    assert not opt.ema.swapped and opt.ema.num_updates == 6
    # the last ema_test_* triple is the evaluation of a second instance loaded with the averaged weights
    m2 = _net()
    m2.load_state_dict(opt.ema.model_state_dict())
    want = evaluate_model(m2, test, bce_loss, "cpu")
    assert (h["ema_test_loss"][-1], h["ema_test_dice"][-1], h["ema_test_iou"][-1]) == want
    assert h["ema_test_loss"][-1] != h["test_loss"][-1]
    # the trained weights are those of the same run without an EMA
    m3 = _net()
    h3 = train_model(m3, train, test, bce_loss, make_optimizer(m3, lr=1e-2), None, "cpu", num_epochs=2, verbose=False)
    assert set(h3) == base
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(m.parameters(), m3.parameters()))
    assert h3["test_loss"] == h["test_loss"]
    # stop after one epoch, resume: EMA and history of the uninterrupted run
    ck = str(tmp_path / "ck.pt")
    m4 = _net()
    train_model(m4, train, test, bce_loss, make_optimizer(m4, lr=1e-2, ema_decay=0.9), None, "cpu", num_epochs=1,
                verbose=False, checkpoint_path=ck)
    m5 = _net()
    o5 = make_optimizer(m5, lr=1e-2, ema_decay=0.9)
    h5 = train_model(m5, train, test, bce_loss, o5, None, "cpu", num_epochs=2, verbose=False, resume_from=ck)
    assert h5 == h and o5.ema.num_updates == 6
    assert all(torch.equal(a, b) for a, b in zip(o5.ema.tensors, opt.ema.tensors))


def test_train_model_takes_an_ema_for_a_plain_optimizer():
    """train_model(ema=...) with an optimizer that carries none: it is attached and updated every step."""
    from csu.ema import WeightEMA
    from csu.train import bce_loss, train_model
    m = _net()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    ema = WeightEMA(m, decay=0.9)
    h = train_model(m, _batches(3), _batches(1, seed=6), bce_loss, opt, None, "cpu", num_epochs=1, verbose=False, ema=ema)
    assert opt.ema is ema and ema.num_updates == 3 and len(h["ema_test_loss"]) == 1
    assert not all(torch.equal(e, p.detach()) for e, p in zip(ema.tensors, m.parameters()))


def test_checkpoint_with_and_without_ema_entry(tmp_path):
    from csu.ema import WeightEMA
    from csu.report import load_checkpoint, save_checkpoint
    m = _net()
    ema = WeightEMA(m, decay=0.8, warmup=True)
    _perturb(m, torch.Generator().manual_seed(4))
    ema.update()
    with_e, without = str(tmp_path / "a.pt"), str(tmp_path / "b.pt")
    save_checkpoint(with_e, m, epoch=3, history={"train_loss": [1.0]}, ema=ema)
    save_checkpoint(without, m, epoch=3, history={"train_loss": [1.0]})
    ck = torch.load(with_e, weights_only=True)         # tensors, numbers and booleans only
    assert set(ck["ema"]) == {"decay", "warmup", "num_updates", "ema"}
    assert "ema" not in torch.load(without, weights_only=True)
    m2 = _net()
    ema2 = WeightEMA(m2, decay=0.1, warmup=False)
    assert load_checkpoint(with_e, m2, ema=ema2) == (3, {"train_loss": [1.0]})
    assert (ema2.decay, ema2.warmup, ema2.num_updates) == (0.8, True, 1)
    assert all(torch.equal(a, b) for a, b in zip(ema.tensors, ema2.tensors))
    # a file without the entry loads as before and leaves a passed EMA alone
    m3 = _net()
    ema3 = WeightEMA(m3, decay=0.1, warmup=False)
    keep = [e.clone() for e in ema3.tensors]
    assert load_checkpoint(without, m3, ema=ema3)[0] == 3
    assert (ema3.decay, ema3.num_updates) == (0.1, 0) and all(torch.equal(a, b) for a, b in zip(keep, ema3.tensors))
    assert load_checkpoint(with_e, _net())[0] == 3         # and a file with it loads without an EMA object
