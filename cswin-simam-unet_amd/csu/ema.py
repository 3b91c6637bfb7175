"""Exponential moving average (EMA) of a model's weights, for evaluation and for the exported
checkpoint.

On the GPU the update rides in csu's optimizer step (``FusedAdamW(ema=...)`` / ``make_optimizer(model,
ema_decay=...)``: csu_adamw_step_ema updates the average from the parameter it has just computed, 8 B
per parameter of extra traffic and no extra launch, so it is captured with the step), and
evaluating on the averaged weights is an in-place exchange, ``swap()`` / ``applied()``: one
csu_ema_swap launch exchanges parameter and average and re-makes every bf16 shadow layout the
forward reads, so no second model, no load_state_dict round trip, no re-cast, and every pointer a
captured graph holds stays valid.  ``update()`` is the stand-alone form (csu_ema_update, one launch)
for other optimizers; the fused update equals it bit for bit."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from ._lib import lib, stream_ptr
from .ledger import launch


def _decay32(decay, warmup, n):
    """The decay in effect at the n-th update, in fp32 as the kernels compute it."""
    d = np.float32(decay)
    if warmup:
        n = np.float32(n)
        d = min(d, n / (n + np.float32(9.0)))
    return d


class WeightEMA:
    """``ema <- ema + (1 - d) (param - ema)`` after every optimizer step, one contiguous fp32 tensor per
    parameter of ``model`` (initialised to the parameter's current value).  ``d = min(decay, n / (n + 9))``
    with ``warmup`` (n = number of updates so far, this one included: (1 + t) / (10 + t) for t = n - 1),
    else ``decay``.  Buffers (BatchNorm running statistics) are not averaged: under a swap the live
    ones are used.

    ``num_updates`` is a device fp32 scalar on a GPU (incremented on the device: the update can live in
    a HIP graph) and a Python int on the CPU.

    Data parallel: every rank steps on the same all-reduced gradients from the same weights, so every
    rank computes the same average; nothing is communicated.

    After a HIP-graph capture of a step with this EMA the graph holds the EMA tensors' and
    ``num_updates``' pointers (load_state_dict copies into them) and the decay / warmup values of the
    capture."""

    def __init__(self, model, decay=0.999, warmup=True):
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"invalid EMA decay {decay}")
        self.model = model.module if isinstance(model, torch.nn.parallel.DistributedDataParallel) else model
        self.decay, self.warmup = float(decay), bool(warmup)
        named = list(self.model.named_parameters())
        if not named:
            raise ValueError("WeightEMA: the model has no parameters")
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        devs = {p.device for p in self.params}
        if len(devs) != 1:
            raise ValueError("WeightEMA: every parameter on one device")
        self.device = devs.pop()
        self.cuda = self.device.type == "cuda"
        if self.cuda and any(p.dtype != torch.float32 or not p.is_contiguous() for p in self.params):
            raise RuntimeError("WeightEMA: contiguous fp32 parameters only on the GPU")
        with torch.no_grad():
            self.tensors = [p.detach().float().clone(memory_format=torch.contiguous_format) for p in self.params]
        self._of = {id(p): e for p, e in zip(self.params, self.tensors)}
        self.num_updates = torch.zeros((), dtype=torch.float32, device=self.device) if self.cuda else 0
        self._swapped = False
        self._tables = {}        # "flat" (update) / "shadow" (swap) -> (key, host, dev, count, chunks, shadowed)
        self._captured, self._retired = False, []

    # ------------------------------------------------------------------ lookups

    def tensor_for(self, p):
        """The EMA tensor of parameter ``p`` (None: not a parameter of the model)."""
        return self._of.get(id(p))

    @property
    def swapped(self) -> bool:
        """The parameters currently hold the averaged weights (between two swap() calls)."""
        return self._swapped

    def current_decay(self) -> float:
        """The decay the next update will use (host sync on a GPU)."""
        return float(_decay32(self.decay, self.warmup, int(self.num_updates) + 1))

    # ------------------------------------------------------------------ device tables

    def _table(self, kind):
        """Device csu_adamw_item table over every parameter + the parallel EMA pointer array behind
        it in the same buffer.  "flat": plain chunks (csu_ema_update reads only param / numel / chunk0);
        "shadow": with the bf16 shadow layouts the model's cast cache keeps (csu_ema_swap writes them),
        rebuilt when those move.  Built outside a capture (pinned host memory cannot be allocated
        while capturing): prepare_capture() or one eager call builds them."""
        from .optim import _ITEM, _NO_SHADOW, _chunks
        specs = [_NO_SHADOW] * len(self.params)
        if kind == "shadow":
            from .ops import shadow_spec
            specs = [shadow_spec(p) or _NO_SHADOW for p in self.params]
        key = tuple((p.data_ptr(), e.data_ptr()) + tuple(s) for p, e, s in zip(self.params, self.tensors, specs))
        t = self._tables.get(kind)
        capturing = torch.cuda.is_current_stream_capturing()
        if t is not None and t[0] == key:
            self._captured |= capturing
            return t
        if capturing:
            raise RuntimeError("WeightEMA: no device table for this capture (call prepare_capture(), or run the "
                               "call once eagerly, before capturing)")
        chunk = lib().csu_adamw_chunk_elems()
        rec = np.zeros(len(self.params), dtype=_ITEM)
        c0 = 0
        for i, (p, s) in enumerate(zip(self.params, specs)):
            rec[i] = (p.data_ptr(), 0, 0, 0, p.numel(), c0) + tuple(s)
            c0 += max(1, _chunks(p.numel(), s, chunk))
        ptrs = np.array([e.data_ptr() for e in self.tensors], dtype="<u8")
        raw = np.frombuffer(rec.tobytes() + ptrs.tobytes(), dtype=np.uint8)
        host = torch.empty(raw.size, dtype=torch.uint8, pin_memory=True)
        host.numpy()[:] = raw
        dev = torch.empty(raw.size, dtype=torch.uint8, device=self.device)
        dev.copy_(host, non_blocking=True)
        if t is not None and self._captured:
            self._retired.append(t)          # a captured launch keeps reading the old table
        shadowed = [p for p, s in zip(self.params, specs) if s[0]]
        t = self._tables[kind] = (key, host, dev, len(self.params), c0, shadowed)
        return t

    def prepare_capture(self):
        """Build the device tables of update() and swap() now, outside a HIP-graph capture."""
        if self.cuda:
            self._table("flat")
            self._table("shadow")

    # ------------------------------------------------------------------ update / swap

    @torch.no_grad()
    def update(self):
        """One EMA update from the model's current parameters: the stand-alone form, to be called
        after ``optimizer.step()`` of an optimizer that does not carry the EMA itself.  GPU: one
        csu_ema_update launch, no host sync; CPU: the same recurrence in torch ops."""
        if self._swapped:
            raise RuntimeError("WeightEMA.update() while the averaged weights are swapped in")
        if not self.cuda:
            self.num_updates += 1
            w = float(np.float32(1.0) - _decay32(self.decay, self.warmup, self.num_updates))
            torch._foreach_lerp_(self.tensors, [p.detach() for p in self.params], w)
            return
        self.num_updates += 1
        _, _, dev, n, chunks, _ = self._table("flat")
        from .optim import _ITEM
        items, ema = dev.data_ptr(), dev.data_ptr() + n * _ITEM.itemsize
        numel = sum(e.numel() for e in self.tensors)
        launch("ema_update", lambda: lib().csu_ema_update(items, ema, n, chunks, self.num_updates.data_ptr(), self.decay,
                                                          int(self.warmup), stream_ptr(self.device)),
               3 * numel, 12 * numel, idem=False, prec="f32")

    @torch.no_grad()
    def swap(self):
        """Exchange parameters and averages in place.  GPU: one csu_ema_swap launch that also
        re-makes every bf16 shadow layout of the model's cast cache from the now-live values, so the
        next forward (eager or a captured graph's replay) launches no cast.  A second swap() restores
        parameters, averages and shadows bit for bit."""
        if not self.cuda:
            for p, e in zip(self.params, self.tensors):
                tmp = p.detach().clone()
                p.detach().copy_(e)
                e.copy_(tmp)
            self._swapped = not self._swapped
            return
        _, _, dev, n, chunks, shadowed = self._table("shadow")
        from .ops import shadows_written
        from .optim import _ITEM
        items, ema = dev.data_ptr(), dev.data_ptr() + n * _ITEM.itemsize
        numel = sum(e.numel() for e in self.tensors)
        launch("ema_swap", lambda: lib().csu_ema_swap(items, ema, n, chunks, stream_ptr(self.device)),
               0, 16 * numel + sum(2 * p.numel() for p in shadowed), idem=False, prec="f32")
        shadows_written(shadowed)
        self._swapped = not self._swapped

    @contextlib.contextmanager
    def applied(self):
        """``with ema.applied(): evaluate(model)``: the averaged weights are live inside the block and
        the trained ones are back after it, also when the block raises.  Not re-entrant."""
        if self._swapped:
            raise RuntimeError("WeightEMA.applied(): the averaged weights are already swapped in")
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    # ------------------------------------------------------------------ state

    def model_state_dict(self):
        """The model's state_dict with the averaged values in place of the parameters (buffers as they
        are): what gets exported and loads into a plain model instance."""
        sd = self.model.state_dict()
        out = {k: v.detach().clone() for k, v in sd.items()}
        if not self._swapped:            # swapped in: the parameters ARE the averages
            for n, p, e in zip(self.names, self.params, self.tensors):
                out[n] = e.detach().clone().to(p.dtype)
        return out

    def state_dict(self):
        """Tensors, numbers and booleans only (loads with ``torch.load(weights_only=True)``)."""
        if self._swapped:
            raise RuntimeError("WeightEMA.state_dict() while the averaged weights are swapped in")
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": int(self.num_updates),
                "ema": {n: e.detach().clone() for n, e in zip(self.names, self.tensors)}}

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Copies INTO the existing EMA tensors and update counter, so the pointers a captured step
        holds stay valid (as FusedAdamW.load_state_dict does after a capture)."""
        if self._swapped:
            raise RuntimeError("WeightEMA.load_state_dict() while the averaged weights are swapped in")
        ema = sd["ema"]
        if set(ema) != set(self.names):
            raise KeyError(f"WeightEMA.load_state_dict: parameter names differ "
                           f"({sorted(set(ema) ^ set(self.names))[:4]} ...)")
        for n, e in zip(self.names, self.tensors):
            if tuple(ema[n].shape) != tuple(e.shape):
                raise ValueError(f"WeightEMA.load_state_dict: shape of {n}")
            e.copy_(ema[n])
        self.decay, self.warmup = float(sd["decay"]), bool(sd["warmup"])
        if self.cuda:
            self.num_updates.fill_(float(sd["num_updates"]))
        else:
            self.num_updates = int(sd["num_updates"])
