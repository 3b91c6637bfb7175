"""Fused AdamW on the csu_adamw_step kernel (the optimizer of cswin:937-941).

The same pass writes the bf16 shadow copies of the updated weights that the model's cast cache
keeps for the next forward (csu.ops.shadow_spec: W, W^T, conv OHWI / IHWO), so no separate cast
launch re-reads the fp32 weights.

Drop-in for ``torch.optim.AdamW`` (same constructor arguments, param_groups, state keys
``step`` / ``exp_avg`` / ``exp_avg_sq`` and state_dict format, ReduceLROnPlateau works on it): one
kernel launch updates every parameter of a group from a device table of pointers.  The table is
rebuilt only when the set of (param, grad) buffers changes, from a pinned host buffer, so the step
can also be captured into a HIP graph (lr and the step count then live in device tensors that are
updated in place: ``capturable=True``).

Gradient clipping (``max_grad_norm``, ``skip_nonfinite``): the global L2 norm of all gradients of all
param groups is reduced on the device over the same tables (csu_grad_sumsq + csu_grad_norm_finish),
and the step kernel multiplies every gradient element by the resulting coefficient while it holds
it in registers (csu_adamw_step_ex) -- ``torch.nn.utils.clip_grad_norm_`` + ``step()`` without a
host sync, so it is captured with the step.  ``p.grad`` itself is left UNSCALED by this fused path
(only the update sees the clipped value); ``csu.optim.clip_grad_norm_`` is the stand-alone,
in-place form for other optimizers.

Weight EMA (``ema=``, a csu.ema.WeightEMA): the same launch also updates the exponential moving
average of every parameter it steps (csu_adamw_step_ema), from the updated value in registers -- 8 B
per parameter more, no launch after the step, captured with it."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import lib, stream_ptr
from .ledger import launch

_ITEM = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("numel", "<i8"),
                  ("chunk0", "<i8"), ("shadow", "<u8"), ("shadow_t", "<u8"), ("rows", "<i4"), ("cols", "<i4"),
                  ("taps", "<i4"), ("cols_pad", "<i4")])
_NO_SHADOW = (0, 0, 0, 0, 0, 0)
_TABLE_REC = _ITEM.itemsize + 8     # bytes reserved per parameter: its item + its EMA pointer


def _chunks(n, spec, chunk):
    """Chunk (workgroup) count of one item: 64 x 64 tiles for a matrix with a transposed shadow,
    else ceil(numel / chunk) (csu.h, csu_adamw_item)."""
    sh, sht, rows, cols, taps, _ = spec
    if sh and sht and taps == 0:
        return -(-rows // 64) * -(-cols // 64)
    return -(-n // chunk)


class FusedAdamW(torch.optim.Optimizer):
    _L2 = False   # FusedAdam: coupled L2 weight decay (torch.optim.Adam)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, capturable=False,
                 max_grad_norm=None, skip_nonfinite=False, ema=None):
        """``max_grad_norm``: clip the global L2 norm of all gradients (all param groups together, as
        ``clip_grad_norm_(model.parameters(), max_grad_norm)``) before the update; ``skip_nonfinite``:
        a step whose gradient norm is inf / NaN changes nothing (parameters, moments, shadows and
        the step count keep their values; ``skipped_steps`` counts it).  Both are plain attributes,
        not param-group entries: state_dict() keeps torch.optim.AdamW's format.
        ``ema``: a csu.ema.WeightEMA of the model these parameters belong to; step() then updates it in
        the same launch (csu_adamw_step_ema), from every updated parameter while it is in registers.
        A parameter without a gradient is not stepped and its average stays as it is; a skipped
        non-finite step leaves the averages and their update count alone."""
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError("invalid AdamW hyper-parameter")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas {betas}")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"invalid max_grad_norm {max_grad_norm} (None: no clipping)")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema = ema
        # device scalars of the norm pass, allocated HERE, outside any capture (see _capture_dev below):
        # _ctl = (norm, clip coefficient, finite flag, 0) written by csu_grad_norm_finish
        dev0 = next((p.device for g in self.param_groups for p in g["params"] if p.is_cuda), None)
        self._ctl = self.grad_norm = self.skipped_steps = self._partial = None
        self._retired = []
        if dev0 is not None:
            self._ctl = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float32, device=dev0)
            self.grad_norm = self._ctl[0]          # pre-clip norm of the last step; same storage at every replay
            self.skipped_steps = torch.zeros((), dtype=torch.int32, device=dev0)
            if self._clipping():
                self._reserve_partial(self._chunk_bound())
        self._tables = {}
        self._gstate = {}
        self._deferred = []
        self._captured = []
        # one pinned table buffer per group, reserved for a HIP-graph capture of step(): the items and,
        # behind them, the parallel EMA pointer array (8 B per item; built, cached, frozen and copied
        # with the table under the same key)
        self._pinned = {gi: torch.empty(max(1, len(g["params"])) * _TABLE_REC, dtype=torch.uint8, pin_memory=True)
                        for gi, g in enumerate(self.param_groups)} if torch.cuda.is_available() else {}
        # ... and its device image, allocated HERE, outside any capture: a buffer allocated inside the
        # capture comes from the graph's private pool, where it may alias memory an earlier captured
        # kernel writes on every replay -- fine for buffers the graph itself fills, fatal for one
        # filled once after the capture (finish_capture)
        self._capture_dev = {gi: torch.empty(max(1, len(g["params"])) * _TABLE_REC, dtype=torch.uint8,
                                             device=g["params"][0].device)
                             for gi, g in enumerate(self.param_groups) if g["params"] and g["params"][0].is_cuda}

    def prepare_capture(self):
        """Reserve the table buffers of one more capture (outside any graph pool; each captured graph
        keeps its own).  GraphedTrainStep calls it before capturing; the first capture's buffers
        come from the constructor.  A later capture re-fills the eager-side table cache only: the
        graphs captured before keep their own tables."""
        for gi, g in enumerate(self.param_groups):
            if g["params"] and g["params"][0].is_cuda and (gi not in self._pinned or gi not in self._capture_dev):
                n = max(1, len(g["params"])) * _TABLE_REC
                self._pinned[gi] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
                self._capture_dev[gi] = torch.empty(n, dtype=torch.uint8, device=g["params"][0].device)
        if self._ctl is not None and self._clipping():
            self._reserve_partial(self._chunk_bound())

    def _clipping(self):
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _chunk_bound(self):
        """Upper bound of the chunk count of all groups' tables, whichever shadow layouts the
        parameters have by the time they step (flat chunks, or 64 x 64 tiles of [shape[0], rest])."""
        chunk = lib().csu_adamw_chunk_elems()
        n = 0
        for g in self.param_groups:
            for p in g["params"]:
                flat = -(-p.numel() // chunk)
                tiles = -(-p.shape[0] // 64) * -(-(p.numel() // p.shape[0]) // 64) if p.dim() >= 2 and p.numel() else 0
                n += max(flat, tiles, 1)
        return n

    def _reserve_partial(self, chunks):
        """The fp64 partial-sum buffer of the norm pass (one per chunk of every group's table),
        allocated outside any capture for the same reason as the table images above."""
        if self._partial is not None and self._partial.numel() >= chunks:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamW: the gradient-norm workspace is too small for this capture (call "
                               "prepare_capture() before capturing)")
        if self._partial is not None and self._captured:
            self._retired.append(self._partial)      # a captured graph keeps writing the old buffer
        self._partial = torch.empty(max(1, chunks), dtype=torch.float64, device=self._ctl.device)

    def _norm_pass(self, work):
        """csu_grad_sumsq of every group's table into its slice of the partial buffer, then ONE
        csu_grad_norm_finish over all of them -> self._ctl (norm, coefficient, finite flag)."""
        total = sum(w["table"][4] for w in work)
        self._reserve_partial(total)
        dev = self._ctl.device
        if any(w["dev"] != dev for w in work):
            raise RuntimeError("FusedAdamW: gradient clipping needs every param group on one device")
        L, off = lib(), 0
        for w in work:
            _, _, table, n, chunks = w["table"]
            part = self._partial.data_ptr() + 8 * off
            numel = sum(it[4] for it in w["items"])
            launch("grad_norm", lambda: L.csu_grad_sumsq(table.data_ptr(), n, chunks, part, stream_ptr(dev)),
                   0, 4 * numel, prec="f32")       # algorithmic: every gradient read once
            off += chunks
        mx = self.max_grad_norm if self.max_grad_norm is not None else 0.0
        launch("grad_norm", lambda: L.csu_grad_norm_finish(self._partial.data_ptr(), total, float(mx),
                                                           self._ctl.data_ptr(), stream_ptr(dev)),
               0, 0, prec="f32")

    def _table(self, gi, items, device, ema=None):
        """Device item table for the current (param, grad) buffers, rebuilt when they change
        (e.g. every step under zero_grad(set_to_none=True) when the allocator hands out other grad
        buffers).  Eager: an asynchronous copy from a fresh pinned buffer (no host sync; the
        caching host allocator keeps it alive until the copy has run).  Under HIP-graph capture:
        the host image goes to a pinned buffer reserved for that capture (pinned memory cannot be
        allocated while capturing) and is copied ONCE after the capture (finish_capture) into a
        device buffer allocated outside the graph's memory pool and kept for the optimizer's
        lifetime -- no copy node in the replayed graph.
        ``ema``: the EMA tensor address of every item (0: none), laid out as a uint64 array behind the
        items in the same buffers -- the ``float* const* ema`` of csu_adamw_step_ema, at byte offset
        len(items) * sizeof(csu_adamw_item)."""
        key = (gi,) + tuple(v for it in items for v in it[:4] + it[5]) + (tuple(ema) if ema is not None else ())
        t = self._tables.get(gi)
        if t is not None and t[0] == key:
            return t
        chunk = lib().csu_adamw_chunk_elems()
        rec = np.zeros(len(items), dtype=_ITEM)
        c0 = 0
        for i, (p, g, m, v, n, spec) in enumerate(items):
            rec[i] = (p, g, m, v, n, c0) + tuple(spec)
            c0 += _chunks(n, spec, chunk)
        tail = np.array(ema, dtype="<u8").tobytes() if ema is not None else b""
        raw = np.frombuffer(rec.tobytes() + tail, dtype=np.uint8)
        if torch.cuda.is_current_stream_capturing():
            host = self._pinned.get(gi)
            dev = self._capture_dev.get(gi)
            if host is None or dev is None or host.numel() < raw.size:
                raise RuntimeError("FusedAdamW: no pinned table buffer for this capture (call prepare_capture() before capturing)")
            del self._pinned[gi]                      # frozen: owned by the captured graph from now on
            del self._capture_dev[gi]
            host[:raw.size].numpy()[:] = raw
            dev = dev[:raw.size]
            # the captured kernel reads this buffer on every replay: keep it (and its host image)
            # alive for the optimizer's lifetime, whatever later eager steps put into _tables
            self._captured.append((host, dev))
            # the table is constant over replays: copied once after the capture (finish_capture)
            # instead of by a copy node on every replay
            self._deferred.append((dev, host[:raw.size]))
        else:
            host = torch.empty(raw.size, dtype=torch.uint8, pin_memory=True)
            host.numpy()[:] = raw
            dev = torch.empty(raw.size, dtype=torch.uint8, device=device)
            dev.copy_(host, non_blocking=True)
        t = (key, host, dev, len(items), c0)
        self._tables[gi] = t
        return t

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        from .ops import shadow_spec, shadows_written
        clip = self._clipping()
        ema = self.ema
        if ema is not None and ema.swapped:
            raise RuntimeError("FusedAdamW.step() while the EMA weights are swapped in (inside WeightEMA.applied())")
        work = []
        for gi, group in enumerate(self.param_groups):
            items, dev, keep, shadowed, eptr, enumel = [], None, [], [], [], 0
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse or p.dtype != torch.float32 or not p.is_cuda:
                    raise RuntimeError("FusedAdamW: dense fp32 CUDA parameters only")
                st = self.state[p]
                if not st:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                keep.append(g)          # a contiguous temporary must outlive the launch below
                if not p.is_contiguous():
                    raise RuntimeError("FusedAdamW: contiguous parameters only")
                # the bf16 copies the next forward reads (a CastCache's layouts of p), written by the
                # same pass from the updated value
                spec = shadow_spec(p)
                if spec is not None:
                    shadowed.append(p)
                items.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                              p.numel(), spec or _NO_SHADOW))
                dev = p.device
                if ema is not None:
                    e = ema.tensor_for(p)
                    eptr.append(0 if e is None else e.data_ptr())
                    enumel += 0 if e is None else p.numel()
            if not items:
                continue
            work.append({"gi": gi, "group": group, "items": items, "dev": dev, "keep": keep, "shadowed": shadowed,
                         "ema": eptr if ema is not None else None, "ema_numel": enumel})
        if clip and work:
            # one norm over all param groups, ordered before the step-count adds and the step kernels
            for w in work:
                w["table"] = self._table(w["gi"], w["items"], w["dev"], w["ema"])
            self._norm_pass(work)
            if self.skip_nonfinite:
                self.skipped_steps += self._ctl[2] == 0
        if ema is not None and work:
            # one EMA update per step() whatever the number of groups; a skipped step does not count
            if clip and self.skip_nonfinite:
                ema.num_updates += self._ctl[2]
            else:
                ema.num_updates += 1
        for w in work:
            gi, group, items, dev, shadowed = w["gi"], w["group"], w["items"], w["dev"], w["shadowed"]
            gs = self._gstate.get(gi)
            if gs is None:
                # one device step count per group (every parameter of a group steps together);
                # resumes from a loaded state_dict's per-parameter step
                st0 = next((self.state[p]["step"] for p in group["params"] if "step" in self.state[p]
                            and self.state[p]["step"] is not None), None)
                step0 = float(st0) if st0 is not None else 0.0
                gs = self._gstate[gi] = {"step": torch.full((), step0, dtype=torch.float32, device=dev),
                                         "lr": torch.full((), group["lr"], dtype=torch.float32, device=dev)}
            if clip and self.skip_nonfinite:
                gs["step"] += self._ctl[2]       # a skipped step does not count: + 1 only when the norm is finite
            else:
                gs["step"] += 1
            for p in group["params"]:
                if p.grad is not None:
                    self.state[p]["step"] = gs["step"]
            _, _, table, n, chunks = self._table(gi, items, dev, w["ema"])
            lr_ptr = gs["lr"].data_ptr() if group["capturable"] else None
            b1, b2 = group["betas"]
            numel = sum(it[4] for it in items)
            args = (table.data_ptr(), n, chunks, lr_ptr, float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                    float(group["weight_decay"]), gs["step"].data_ptr(), 0.0)
            nema = 0
            if ema is not None:
                fn = lib().csu_adamw_step_ema
                args += (self._ctl.data_ptr() if clip else None, int(self.skip_nonfinite), int(self._L2),
                         table.data_ptr() + n * _ITEM.itemsize, ema.num_updates.data_ptr(), float(ema.decay),
                         int(ema.warmup))
                nema = 8 * w["ema_numel"]       # algorithmic: the EMA value read and written once
            elif clip:
                fn = lib().csu_adamw_step_ex
                args += (self._ctl.data_ptr(), int(self.skip_nonfinite), int(self._L2))
            else:
                fn = lib().csu_adam_l2_step if self._L2 else lib().csu_adamw_step
            nsh = sum(2 * it[4] * (1 + (it[5][1] != 0)) for it in items if it[5][0])
            launch("adamw", lambda: fn(*args, stream_ptr(dev)), 12 * numel, 28 * numel + nsh + nema, idem=False,
                   prec="f32")
            # (a skipped step leaves the shadows as they are: still the bf16 image of the unchanged weights)
            shadows_written(shadowed)
        return loss

    def state_dict(self):
        """torch.optim.AdamW format with a separate ``step`` tensor per parameter (the live state
        shares one device step tensor per group), so the checkpoint also loads into
        torch.optim.AdamW, whose per-parameter steps would otherwise advance once per parameter."""
        sd = super().state_dict()
        for st in sd["state"].values():
            if isinstance(st.get("step"), torch.Tensor):
                st["step"] = st["step"].detach().clone()
        return sd

    def load_state_dict(self, state_dict):
        """Load an AdamW / FusedAdamW state; the device step / lr of every group and the pointer
        tables are rebuilt from it on the next step().  Once a step has been captured into a HIP
        graph, the graph keeps reading the current state tensors (step, lr, exp_avg, exp_avg_sq):
        the loaded values are then copied INTO them, so the captured pointers stay valid."""
        if not self._captured:
            super().load_state_dict(state_dict)
            self._gstate = {}
            self._tables = {}
            return
        old = {p: dict(self.state[p]) for g in self.param_groups for p in g["params"] if self.state.get(p)}
        super().load_state_dict(state_dict)
        with torch.no_grad():
            for gi, g in enumerate(self.param_groups):
                gs = self._gstate.get(gi)
                for p in g["params"]:
                    st, o = self.state.get(p), old.get(p)
                    if not st:
                        if o is not None:
                            # the captured step keeps updating this parameter with its old moments
                            # and the group's step count: a "fresh" loaded state cannot be honoured
                            raise RuntimeError("FusedAdamW.load_state_dict after a capture: the loaded state "
                                               "has no state for a parameter the captured step updates")
                        continue
                    if o is None:
                        raise RuntimeError("FusedAdamW.load_state_dict after a capture: the loaded state has a "
                                           "parameter the captured step has no state for")
                    for k in ("exp_avg", "exp_avg_sq"):
                        o[k].copy_(st[k])
                        st[k] = o[k]
                    if gs is not None:
                        gs["step"].fill_(float(st["step"]))
                        st["step"] = gs["step"]
                if gs is not None:
                    gs["lr"].fill_(g["lr"])

    def finish_capture(self):
        """After a HIP-graph capture of step(): fill the device tables the captured kernel reads
        (their host images were frozen during the capture).  Synchronous, once per capture."""
        for dev, host in self._deferred:
            dev.copy_(host)
        self._deferred = []
        torch.cuda.synchronize()

    def sync_lr(self):
        """Copy the host lr of every group into its device tensor (capturable groups read it at
        replay time): call after a scheduler step, outside graph replay."""
        for gi, g in enumerate(self.param_groups):
            if gi in self._gstate:
                self._gstate[gi]["lr"].fill_(g["lr"])


class FusedAdam(FusedAdamW):
    """Drop-in for ``torch.optim.Adam`` (coupled L2 weight decay: g += weight_decay * param before the
    moments) on the same one-launch kernel: the plain UNet's optimizer (unet:486-490)."""
    _L2 = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False,
                 max_grad_norm=None, skip_nonfinite=False, ema=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, ema=ema)


def _grads_of(parameters):
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    return [p.grad for p in parameters if p.grad is not None]


def _device_norm(grads, max_norm, scale):
    """(norm, coef, finite, 0) device tensor of dense fp32 GPU gradients: a flat-item table of the
    gradients (csu_adamw_item with only grad / numel / chunk0 set), csu_grad_sumsq +
    csu_grad_norm_finish, and csu_grad_scale in place when ``scale``.  No host sync."""
    dev = grads[0].device
    for g in grads:
        if g.is_sparse or g.dtype != torch.float32 or g.device != dev or not g.is_contiguous():
            raise RuntimeError("csu.optim gradient norm: dense contiguous fp32 gradients on one GPU only")
    L = lib()
    chunk = L.csu_adamw_chunk_elems()
    rec = np.zeros(len(grads), dtype=_ITEM)
    c0 = 0
    for i, g in enumerate(grads):
        rec[i] = (0, g.data_ptr(), 0, 0, g.numel(), c0) + _NO_SHADOW
        c0 += max(1, -(-g.numel() // chunk))
    host = torch.empty(rec.nbytes, dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = np.frombuffer(rec.tobytes(), dtype=np.uint8)
    table = torch.empty(rec.nbytes, dtype=torch.uint8, device=dev)
    table.copy_(host, non_blocking=True)
    partial = torch.empty(c0, dtype=torch.float64, device=dev)
    ctl = torch.empty(4, dtype=torch.float32, device=dev)
    numel = sum(g.numel() for g in grads)
    st = stream_ptr(dev)
    launch("grad_norm", lambda: L.csu_grad_sumsq(table.data_ptr(), len(grads), c0, partial.data_ptr(), st),
           0, 4 * numel, prec="f32")
    launch("grad_norm", lambda: L.csu_grad_norm_finish(partial.data_ptr(), c0, float(max_norm), ctl.data_ptr(), st),
           0, 0, prec="f32")
    if scale:
        launch("grad_scale", lambda: L.csu_grad_scale(table.data_ptr(), len(grads), c0, ctl.data_ptr() + 4, st),
               numel, 8 * numel, idem=False, prec="f32")
    return ctl


def grad_norm(parameters) -> torch.Tensor:
    """Global L2 norm of the gradients of ``parameters`` (a 0-dim tensor on their device; no host
    sync on the GPU): the value ``clip_grad_norm_`` returns, without clipping."""
    grads = _grads_of(parameters)
    if not grads:
        return torch.tensor(0.0)
    if not grads[0].is_cuda:
        return torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
    return _device_norm([g if g.is_contiguous() else g.contiguous() for g in grads], 0.0, False)[0]


def clip_grad_norm_(parameters, max_norm) -> torch.Tensor:
    """Drop-in for ``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` (L2 norm) for users with
    another optimizer: three launches over one table of all gradients instead of ~2 small torch
    kernels per tensor, scaling ``p.grad`` in place by min(1, max_norm / (norm + 1e-6)).  Dense fp32
    GPU gradients; returns the total norm as a device tensor without a host sync.  Eager only
    (FusedAdamW(max_grad_norm=...) is the form a captured step uses).  CPU gradients go to torch."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    grads = _grads_of(parameters)
    if not grads:
        return torch.tensor(0.0)
    if not grads[0].is_cuda:
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm)
    if not float(max_norm) > 0.0:
        raise ValueError(f"invalid max_norm {max_norm}")
    return _device_norm(grads, max_norm, True)[0]
