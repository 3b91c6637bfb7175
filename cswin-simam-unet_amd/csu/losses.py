"""Training criteria beyond nn.BCELoss: soft Dice, BCE + Dice, Tversky (binary, ``SegLoss``) and softmax
cross-entropy + per-class Dice / Tversky on integer label maps (``MultiClassSegLoss``), that with the boundary
loss of signed distance maps on top (``BoundarySegLoss``), and that with a focal or top-k cross-entropy in the
place of the plain one (``HardExampleSegLoss``), or with the Lovasz-Softmax surrogate of the IoU on top
(``LovaszSegLoss``, at the end).

One family, ``SegLoss``:  ``bce * BCE + tversky * mean_r(1 - TI_r)`` on probabilities ``p`` and
targets ``t`` viewed as rows (one row for the whole batch, or one per image), with

    TP = sum p t,  P = sum p,  T = sum t,
    TI = (TP + smooth) / ((1 - alpha - beta) TP + alpha P + beta T + smooth),
    BCE = mean -(pos_weight t max(log p, -100) + (1 - t) max(log1p(-p), -100)).

Soft Dice is ``alpha = beta = 0.5``; with ``smooth = s / 2`` it is ``1 - csu.train._dice_t(p, t, s)``,
the reference's batch-flattened Dice (cswin:692-698) on probabilities.  On the GPU the loss, its
gradient and the per-step thresholded Dice / IoU sums come from the fused csu_seg_loss kernels
(two reads forward, two reads and one write backward -- what bce_loss costs); a criterion with a
``loss_stats`` method takes csu.train's graph-captured loss-plus-metrics route.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


class SegLoss:
    """``criterion(prob, target) -> loss``;  ``criterion.loss_stats(prob, target) -> (loss, stats)``
    with stats = (sum(pred * t), sum(pred), sum(t)) of pred = prob > 0.5 over the whole batch.

    bce, tversky: the two weights (>= 0, not both 0); alpha, beta: Tversky's weights of sum p and
    sum t (>= 0; false positives / false negatives); smooth > 0; pos_weight >= 0 scales the target
    term of the BCE; per_sample: one Tversky index per image (rows = prob.shape[0]) instead of one
    over the flattened batch.  Always fp32, autocast disabled.  Hashable by identity."""

    def __init__(self, bce: float = 1.0, tversky: float = 1.0, alpha: float = 0.5, beta: float = 0.5,
                 smooth: float = 0.5, pos_weight: float = 1.0, per_sample: bool = False):
        vals = {"bce": bce, "tversky": tversky, "alpha": alpha, "beta": beta, "pos_weight": pos_weight}
        for k, v in vals.items():
            if not float(v) >= 0.0 or float(v) == float("inf"):
                raise ValueError(f"SegLoss: {k} must be a finite number >= 0 (got {v!r})")
        if not 0.0 < float(smooth) < float("inf"):
            raise ValueError(f"SegLoss: smooth must be > 0 (got {smooth!r})")
        if float(bce) == 0.0 and float(tversky) == 0.0:
            raise ValueError("SegLoss: bce and tversky are both zero")
        self.bce, self.tversky, self.alpha, self.beta = float(bce), float(tversky), float(alpha), float(beta)
        self.smooth, self.pos_weight, self.per_sample = float(smooth), float(pos_weight), bool(per_sample)

    @property
    def params(self):
        """(w_bce, pos_weight, w_tversky, alpha, beta, smooth): the scalar arguments of csu_seg_loss_fwd."""
        return (self.bce, self.pos_weight, self.tversky, self.alpha, self.beta, self.smooth)

    def __repr__(self):
        return (f"SegLoss(bce={self.bce}, tversky={self.tversky}, alpha={self.alpha}, beta={self.beta}, "
                f"smooth={self.smooth}, pos_weight={self.pos_weight}, per_sample={self.per_sample})")

    def _rows(self, prob):
        return prob.shape[0] if self.per_sample and prob.dim() > 0 else 1

    def _torch(self, p, t):
        """The same formula in torch ops (CPU tensors), ATen's BCE clamps included."""
        rows = self._rows(p)
        pr, tr = p.reshape(rows, -1), t.reshape(rows, -1)
        tp, ps, ts = (pr * tr).sum(1), pr.sum(1), tr.sum(1)
        den = (1.0 - self.alpha - self.beta) * tp + self.alpha * ps + self.beta * ts + self.smooth
        loss = self.tversky * (1.0 - (tp + self.smooth) / den).mean()
        if self.bce != 0.0:
            # -(pos_weight t log p) and -((1 - t) log1p(-p)) as two weighted ATen BCE sums: its forward
            # clamp (log >= -100) and its backward clamp (p (1 - p) >= 1e-12), as the kernels apply them
            tgt = F.binary_cross_entropy(pr, torch.ones_like(pr), weight=self.pos_weight * tr, reduction="sum")
            bkg = F.binary_cross_entropy(pr, torch.zeros_like(pr), weight=1.0 - tr, reduction="sum")
            loss = loss + self.bce * ((tgt + bkg) / pr.numel())
        return loss

    def _run(self, prob, target, with_stats):
        if prob.shape != target.shape:
            raise ValueError("SegLoss: probabilities and targets of one shape")
        with torch.autocast(prob.device.type, enabled=False):
            p, t = prob.float(), target.float()
            if prob.is_cuda:
                from . import ops
                return ops.seg_loss(p, t, self.params, self._rows(p), with_stats)
            loss = self._torch(p, t)
            if not with_stats:
                return loss
            pred = (p > 0.5).float()
            return loss, torch.stack([(pred * t).sum(), pred.sum(), t.sum()]).detach()

    def __call__(self, prob: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return self._run(prob, target, False)

    def loss_stats(self, prob: torch.Tensor, target: torch.Tensor):
        """The loss and the per-step segmentation sums (cswin:789-795) of the same pass."""
        return self._run(prob, target, True)


def dice_loss(smooth: float = 1e-6, per_sample: bool = False) -> SegLoss:
    """Soft Dice loss 1 - (2 sum p t + smooth) / (sum p + sum t + smooth)."""
    return SegLoss(bce=0.0, tversky=1.0, alpha=0.5, beta=0.5, smooth=smooth / 2, per_sample=per_sample)


def bce_dice_loss(bce: float = 1.0, dice: float = 1.0, smooth: float = 1.0, pos_weight: float = 1.0,
                  per_sample: bool = False) -> SegLoss:
    """bce * BCE + dice * (1 - Dice); smooth is Dice's (numerator and denominator)."""
    return SegLoss(bce=bce, tversky=dice, alpha=0.5, beta=0.5, smooth=smooth / 2, pos_weight=pos_weight,
                   per_sample=per_sample)


def tversky_loss(alpha: float = 0.3, beta: float = 0.7, smooth: float = 1.0, per_sample: bool = False) -> SegLoss:
    """1 - Tversky index; alpha weighs sum p (false positives), beta sum t (false negatives)."""
    return SegLoss(bce=0.0, tversky=1.0, alpha=alpha, beta=beta, smooth=smooth, per_sample=per_sample)


class MultiClassSegLoss:
    """``criterion(logits, target) -> loss``;  ``criterion.loss_stats(logits, target) -> (loss, stats)``
    for K-class segmentation: softmax cross-entropy plus a per-class soft Tversky / Dice term,

        p = softmax_k(z),
        CE = sum_pix w[t] (logsumexp(z) - z_t) / sum_pix w[t]                     (whole batch),
        TP_rc = sum p_c [t = c],  P_rc = sum p_c,  T_rc = sum [t = c]              (row r, class c),
        TI_rc = (TP + smooth) / ((1 - alpha - beta) TP + alpha P + beta T + smooth),
        loss = ce * CE + tversky * mean_r mean_{c in C} (1 - TI_rc),

    rows r = the whole batch, or one per image with ``per_sample``; C = all classes, or 1 .. K-1 with
    ``include_background=False``.  Pixels whose label is ``ignore_index`` contribute to no sum and get
    a zero gradient.  stats is an fp64 (3, K) tensor [I; Pr; T] of the hard prediction pred = argmax_k z
    (the lowest index wins a tie) over the batch: I_c = sum [pred = c][t = c], Pr_c = sum [pred = c],
    T_c = sum [t = c] -- what csu.train turns into per-class and macro Dice / IoU.

    logits: (B, K, H, W), fp32 or bf16 (bf16 goes to the kernel as it is and is upcast in registers;
    the arithmetic is fp32 with autocast disabled); either memory layout a csu model produces is read
    in place.  target: (B, H, W) or (B, 1, H, W), int64 or uint8.  A label outside [0, K) that is not
    ``ignore_index`` is a caller error: it is not checked (a check would synchronise the host) and
    matches no class.

    The one deliberate difference from ``F.cross_entropy``: when every pixel is ignored (sum w[t] = 0)
    the CE term and its gradient are 0, not NaN, so a captured training run survives such a batch.

    ce, tversky: the two weights (>= 0, not both 0); alpha, beta >= 0; smooth > 0; class_weight: K
    weights >= 0 of the CE term or None.  On the GPU with 2 <= K <= 32 the loss, its gradient and the
    stats come from the fused csu_seg_ce kernels; more classes take the same formula in torch ops on
    the device.  Hashable by identity."""

    _other_terms = False      # a subclass with a term of its own may have ce = tversky = 0

    def __init__(self, num_classes: int, ce: float = 1.0, tversky: float = 1.0, alpha: float = 0.5, beta: float = 0.5,
                 smooth: float = 0.5, class_weight=None, ignore_index: int = -100, per_sample: bool = False,
                 include_background: bool = True):
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes < 2:
            raise ValueError(f"MultiClassSegLoss: num_classes must be an integer >= 2 (got {num_classes!r})")
        for k, v in {"ce": ce, "tversky": tversky, "alpha": alpha, "beta": beta}.items():
            if not float(v) >= 0.0 or float(v) == float("inf"):
                raise ValueError(f"MultiClassSegLoss: {k} must be a finite number >= 0 (got {v!r})")
        if not 0.0 < float(smooth) < float("inf"):
            raise ValueError(f"MultiClassSegLoss: smooth must be > 0 (got {smooth!r})")
        if float(ce) == 0.0 and float(tversky) == 0.0 and not self._other_terms:
            raise ValueError("MultiClassSegLoss: ce and tversky are both zero")
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, int):
            raise ValueError(f"MultiClassSegLoss: ignore_index must be an integer (got {ignore_index!r})")
        if class_weight is not None:
            cw = torch.as_tensor(class_weight, dtype=torch.float32).detach().reshape(-1).cpu().clone()
            if cw.numel() != num_classes or not bool(torch.isfinite(cw).all()) or bool((cw < 0).any()):
                raise ValueError("MultiClassSegLoss: class_weight must hold num_classes finite weights >= 0")
            class_weight = cw
        self.num_classes = num_classes
        self.ce, self.tversky, self.alpha, self.beta = float(ce), float(tversky), float(alpha), float(beta)
        self.smooth, self.class_weight, self.ignore_index = float(smooth), class_weight, ignore_index
        self.per_sample, self.include_background = bool(per_sample), bool(include_background)
        self._cw = {}

    @property
    def params(self):
        """(w_ce, w_tversky, alpha, beta, smooth): the scalar arguments of csu_seg_ce_fwd."""
        return (self.ce, self.tversky, self.alpha, self.beta, self.smooth)

    def __repr__(self):
        return (f"MultiClassSegLoss(num_classes={self.num_classes}, ce={self.ce}, tversky={self.tversky}, "
                f"alpha={self.alpha}, beta={self.beta}, smooth={self.smooth}, class_weight="
                f"{None if self.class_weight is None else self.class_weight.tolist()}, ignore_index={self.ignore_index}, "
                f"per_sample={self.per_sample}, include_background={self.include_background})")

    def _weight(self, device):
        if self.class_weight is None:
            return None
        w = self._cw.get(device)
        if w is None:
            w = self._cw[device] = self.class_weight.to(device)
        return w

    def _torch(self, z, t):
        """The same formula in torch ops, in z's floating dtype: z (B, K, *), t (B, *) int64."""
        ce, tv = self._terms_torch(z, t)
        return self.ce * ce + self.tversky * tv

    def _terms_torch(self, z, t):
        """(CE, mean_r mean_{c in C} (1 - TI_rc)) of _torch."""
        B, K = z.shape[0], z.shape[1]
        rows = B if self.per_sample else 1
        z2 = z.reshape(B, K, -1)
        t2 = t.reshape(B, -1)
        live = t2 != self.ignore_index
        tc = torch.where(live, t2, torch.zeros_like(t2))
        w = self._weight(z.device)
        w = torch.ones(K, dtype=z.dtype, device=z.device) if w is None else w.to(z.dtype)
        lsm = torch.log_softmax(z2, 1)
        wt = w[tc] * live.to(z.dtype)
        sw = wt.sum()
        ce = -(lsm.gather(1, tc.unsqueeze(1)).squeeze(1) * wt).sum()
        ce = torch.where(sw > 0, ce / torch.where(sw > 0, sw, torch.ones_like(sw)), ce * 0.0)
        lv = live.to(z.dtype).unsqueeze(1)
        p = lsm.exp() * lv
        oh = F.one_hot(tc, K).permute(0, 2, 1).to(z.dtype) * lv

        def rk(x):   # (B, K, n) -> (rows, K, n')
            return x if rows == B else x.permute(1, 0, 2).reshape(1, K, -1)

        p, oh = rk(p), rk(oh)
        tp, ps, ts = (p * oh).sum(-1), p.sum(-1), oh.sum(-1)
        den = (1.0 - self.alpha - self.beta) * tp + self.alpha * ps + self.beta * ts + self.smooth
        one_minus = 1.0 - (tp + self.smooth) / den
        if not self.include_background:
            one_minus = one_minus[:, 1:]
        return ce, one_minus.mean()

    def hard_stats(self, z, t):
        """fp64 (3, K) [I; Pr; T] in torch ops; the first maximum is the prediction."""
        K = z.shape[1]
        z2 = z.reshape(z.shape[0], K, -1)
        t2 = t.reshape(z.shape[0], -1)
        live = t2 != self.ignore_index
        m = z2.max(1, keepdim=True).values
        ar = torch.arange(K, device=z.device).view(1, K, 1)
        pred = torch.where(z2 == m, ar, torch.full_like(ar, K)).min(1).values     # lowest index of the maximum
        cls = torch.arange(K, device=z.device).view(K, 1, 1)
        pm = (pred.unsqueeze(0) == cls) & live.unsqueeze(0)
        tm = (t2.unsqueeze(0) == cls) & live.unsqueeze(0)
        f = torch.float64
        return torch.stack([(pm & tm).sum((1, 2)).to(f), pm.sum((1, 2)).to(f), tm.sum((1, 2)).to(f)])

    def _label_map(self, logits, target):
        """The target as a (B, *spatial) label map, after the shape and dtype checks."""
        K = self.num_classes
        if logits.dim() < 3 or logits.shape[1] != K:
            raise ValueError(f"MultiClassSegLoss: logits (B, {K}, H, W) (got {tuple(logits.shape)})")
        if target.dim() == logits.dim() and target.shape[1] == 1:
            target = target[:, 0]
        if target.dtype not in (torch.int64, torch.uint8) or \
                tuple(target.shape) != (logits.shape[0],) + tuple(logits.shape[2:]):
            raise ValueError("MultiClassSegLoss: an int64 or uint8 label map (B, H, W) or (B, 1, H, W) of the logits' size")
        return target

    def _run(self, logits, target, with_stats):
        K = self.num_classes
        target = self._label_map(logits, target)
        with torch.autocast(logits.device.type, enabled=False):
            if logits.is_cuda and K <= 32:
                from . import ops
                z = logits if logits.dtype in (torch.float32, torch.bfloat16) else logits.float()
                rows = logits.shape[0] if self.per_sample else 1
                return ops.seg_ce(z, target, self.params, self._weight(logits.device), self.ignore_index, rows,
                                  self.include_background, with_stats)
            z, t = logits.float(), target.long()
            loss = self._torch(z, t)
            if not with_stats:
                return loss
            return loss, self.hard_stats(z.detach(), t)

    def __call__(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return self._run(logits, target, False)

    def loss_stats(self, logits: torch.Tensor, target: torch.Tensor):
        """The loss and the hard per-class sums (3, K) fp64 of the same pass."""
        return self._run(logits, target, True)


def ce_loss(num_classes: int, class_weight=None, ignore_index: int = -100) -> MultiClassSegLoss:
    """Softmax cross-entropy (F.cross_entropy's weighted mean) with the per-class metrics of MultiClassSegLoss."""
    return MultiClassSegLoss(num_classes, ce=1.0, tversky=0.0, class_weight=class_weight, ignore_index=ignore_index)


def ce_dice_loss(num_classes: int, ce: float = 1.0, dice: float = 1.0, smooth: float = 1.0, class_weight=None,
                 ignore_index: int = -100, per_sample: bool = False, include_background: bool = True) -> MultiClassSegLoss:
    """ce * CE + dice * mean over classes of (1 - Dice_c); smooth is Dice's (numerator and denominator)."""
    return MultiClassSegLoss(num_classes, ce=ce, tversky=dice, alpha=0.5, beta=0.5, smooth=smooth / 2,
                             class_weight=class_weight, ignore_index=ignore_index, per_sample=per_sample,
                             include_background=include_background)


def multiclass_dice_loss(num_classes: int, smooth: float = 1e-6, ignore_index: int = -100, per_sample: bool = False,
                         include_background: bool = True) -> MultiClassSegLoss:
    """Mean over classes of the soft Dice loss 1 - (2 sum p_c [t = c] + smooth) / (sum p_c + sum [t = c] + smooth)."""
    return MultiClassSegLoss(num_classes, ce=0.0, tversky=1.0, alpha=0.5, beta=0.5, smooth=smooth / 2,
                             ignore_index=ignore_index, per_sample=per_sample, include_background=include_background)


class BoundarySegLoss(MultiClassSegLoss):
    """``MultiClassSegLoss`` plus the boundary loss of Kervadec et al. ("Boundary loss for highly unbalanced
    segmentation", 2019), the term that moves HD95 where CE + Dice move the overlap:

        n  = sum_c T_c                                      (live pixels whose label is a class, whole batch),
        BD = (1 / (n |Cb|)) sum over live pixels, c in Cb of softmax(z)_c phi_c      (0 when n = 0),
        loss = ce * CE + tversky * mean_r mean_{c in C} (1 - TI_rc) + boundary_weight * BD,

    phi_c = the signed distance of the pixel to the border of class c in the target, negative inside the
    class (``csu.boundary.signed_distance_map``: ``spacing`` and ``clip`` go there); Cb = classes 1 .. K-1, or
    all with ``boundary_background``.  ``ce = tversky = 0`` is legal here (the boundary term alone).

    ``criterion(logits, target, dist=None)`` and ``criterion.loss_stats(logits, target, dist=None)``: without
    ``dist`` (fp32 (B, K, H, W) maps made beforehand) the maps are made from ``target`` in the same call, on
    its device -- on the GPU by csu_signed_distance with no host synchronisation, so labels that were
    augmented on the device this step are fine and the whole call can be captured in a graph.  On the GPU
    with K <= 32 the loss and its gradient come from the fused csu_seg_bd kernels; CPU tensors and more
    classes take the same formula in torch ops.

    The weight lives in a one-element device tensor the kernels read: ``set_boundary_weight(w)`` fills it in
    place, so a captured graph follows a schedule without a re-capture; ``boundary_weight`` is the host
    copy.  ``schedule``: a callable epoch -> weight (``linear_ramp`` is the authors' rebalancing), applied by
    ``on_epoch(epoch)``, which csu.train.train_model calls at the start of every epoch.  ``last_terms``: the
    (2,) device tensor (loss without the boundary term, BD) of the last call."""

    _other_terms = True

    def __init__(self, num_classes: int, ce: float = 1.0, tversky: float = 1.0, alpha: float = 0.5, beta: float = 0.5,
                 smooth: float = 0.5, class_weight=None, ignore_index: int = -100, per_sample: bool = False,
                 include_background: bool = True, boundary: float = 1.0, boundary_background: bool = False,
                 spacing=(1.0, 1.0), clip=None, schedule=None):
        super().__init__(num_classes, ce, tversky, alpha, beta, smooth, class_weight, ignore_index, per_sample,
                         include_background)
        if not float(boundary) >= 0.0 or float(boundary) == float("inf"):
            raise ValueError(f"BoundarySegLoss: boundary must be a finite number >= 0 (got {boundary!r})")
        try:
            sy, sx = (float(v) for v in spacing)
        except (TypeError, ValueError):
            raise ValueError(f"BoundarySegLoss: spacing = (sy, sx) (got {spacing!r})") from None
        if not (0.0 < sy < float("inf") and 0.0 < sx < float("inf")):
            raise ValueError(f"BoundarySegLoss: spacing must be positive and finite (got {spacing!r})")
        if clip is not None and not 0.0 < float(clip) < float("inf"):
            raise ValueError(f"BoundarySegLoss: clip must be positive and finite, or None (got {clip!r})")
        if schedule is not None and not callable(schedule):
            raise ValueError("BoundarySegLoss: schedule is a callable epoch -> weight, or None")
        self.boundary_background, self.spacing = bool(boundary_background), (sy, sx)
        self.clip, self.schedule = None if clip is None else float(clip), schedule
        self._w, self._wbd = float(boundary), {}
        self.last_terms = None

    def __repr__(self):
        return (f"BoundarySegLoss({super().__repr__()[len('MultiClassSegLoss('):-1]}, boundary={self._w}, "
                f"boundary_background={self.boundary_background}, spacing={self.spacing}, clip={self.clip}, "
                f"schedule={self.schedule!r})")

    @property
    def boundary_weight(self) -> float:
        """The current weight of the boundary term (the host copy of the device scalar)."""
        return self._w

    def set_boundary_weight(self, w: float) -> None:
        """Set the weight; every device's scalar is filled in place (no re-capture, no synchronisation)."""
        if not float(w) >= 0.0 or float(w) == float("inf"):
            raise ValueError(f"BoundarySegLoss: the boundary weight must be a finite number >= 0 (got {w!r})")
        self._w = float(w)
        for t in self._wbd.values():
            t.fill_(self._w)

    def on_epoch(self, epoch: int) -> None:
        """Apply the schedule, if there is one, for the epoch that starts (0-based)."""
        if self.schedule is not None:
            self.set_boundary_weight(self.schedule(int(epoch)))

    def _scalar(self, device):
        t = self._wbd.get(device)
        if t is None:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("BoundarySegLoss: call the criterion once on this device before capturing it in a "
                                   "graph (the weight's device scalar is made at the first call)")
            t = self._wbd[device] = torch.full((1,), self._w, dtype=torch.float32, device=device)
        return t

    def _boundary_torch(self, z, t, phi):
        """BD in torch ops, in z's floating dtype: z, phi (B, K, *), t (B, *) int64."""
        K = z.shape[1]
        live = t != self.ignore_index
        n = (live & (t >= 0) & (t < K)).sum().to(z.dtype)
        first = 0 if self.boundary_background else 1
        p = torch.softmax(z, 1) * live.unsqueeze(1).to(z.dtype)
        s = (p[:, first:] * phi[:, first:].to(z.dtype)).sum()
        den = n * (K - first)
        return torch.where(n > 0, s / torch.where(n > 0, den, torch.ones_like(den)), s * 0.0)

    def _run(self, logits, target, with_stats, dist=None):
        K = self.num_classes
        target = self._label_map(logits, target)
        with torch.autocast(logits.device.type, enabled=False):
            if dist is None:
                from .boundary import signed_distance_map
                if target.dim() != 3:
                    raise ValueError("BoundarySegLoss: distance maps are made of (B, H, W) label maps; pass dist= otherwise")
                dist = signed_distance_map(target, K, self.spacing, self.clip)
            elif not isinstance(dist, torch.Tensor) or not dist.is_floating_point() or dist.shape != logits.shape \
                    or dist.device != logits.device:
                raise ValueError("BoundarySegLoss: dist is a floating-point tensor of the logits' shape on their device")
            dist = dist.detach().float()
            w = self._scalar(logits.device)
            if logits.is_cuda and K <= 32:
                from . import ops
                z = logits if logits.dtype in (torch.float32, torch.bfloat16) else logits.float()
                rows = logits.shape[0] if self.per_sample else 1
                res = ops.seg_bd(z, target, dist, w, self.params, self._weight(logits.device), self.ignore_index, rows,
                                 self.include_background, self.boundary_background, with_stats)
                self.last_terms = res[1]
                return (res[0], res[2]) if with_stats else res[0]
            z, t = logits.float(), target.long()
            base, bd = self._torch(z, t), self._boundary_torch(z, t, dist)
            self.last_terms = torch.stack([base.detach(), bd.detach()])
            loss = base + w[0] * bd
            if not with_stats:
                return loss
            return loss, self.hard_stats(z.detach(), t)

    def __call__(self, logits: torch.Tensor, target: torch.Tensor, dist: torch.Tensor = None) -> torch.Tensor:
        return self._run(logits, target, False, dist)

    def loss_stats(self, logits: torch.Tensor, target: torch.Tensor, dist: torch.Tensor = None):
        """The loss and the hard per-class sums (3, K) fp64 of the same pass."""
        return self._run(logits, target, True, dist)


def linear_ramp(start: float = 0.01, step: float = 0.01, stop: float = 1.0):
    """The boundary weight of epoch e (0-based): start + step * e, at most ``stop`` -- Kervadec's rebalancing,
    which lets the region terms shape the prediction first.  For ``BoundarySegLoss(schedule=...)``."""
    start, step, stop = float(start), float(step), float(stop)
    if not (0.0 <= start <= stop < float("inf")) or not 0.0 <= step < float("inf"):
        raise ValueError("linear_ramp: 0 <= start <= stop and step >= 0, all finite")

    def weight(epoch: int) -> float:
        return min(stop, start + step * int(epoch))

    return weight


def boundary_loss(num_classes: int, ignore_index: int = -100, boundary_background: bool = False, spacing=(1.0, 1.0),
                  clip=None, schedule=None) -> BoundarySegLoss:
    """The boundary term alone (weight 1), with the per-class metrics of MultiClassSegLoss."""
    return BoundarySegLoss(num_classes, ce=0.0, tversky=0.0, ignore_index=ignore_index, boundary=1.0,
                           boundary_background=boundary_background, spacing=spacing, clip=clip, schedule=schedule)


def ce_dice_boundary_loss(num_classes: int, ce: float = 1.0, dice: float = 1.0, boundary: float = 1.0, smooth: float = 1.0,
                          class_weight=None, ignore_index: int = -100, per_sample: bool = False,
                          include_background: bool = True, boundary_background: bool = False, spacing=(1.0, 1.0),
                          clip=None, schedule=None) -> BoundarySegLoss:
    """ce * CE + dice * mean over classes of (1 - Dice_c) + boundary * BD; smooth is Dice's, as in ce_dice_loss."""
    return BoundarySegLoss(num_classes, ce=ce, tversky=dice, alpha=0.5, beta=0.5, smooth=smooth / 2,
                           class_weight=class_weight, ignore_index=ignore_index, per_sample=per_sample,
                           include_background=include_background, boundary=boundary,
                           boundary_background=boundary_background, spacing=spacing, clip=clip, schedule=schedule)


class HardExampleSegLoss(MultiClassSegLoss):
    """``MultiClassSegLoss`` whose CE term weighs the pixels by how hard they are: the focal loss (Lin et al. 2017,
    ``gamma``), the top-k / OHEM cross-entropy over the batch (nnU-Net's ``TopKLoss``, ``top_k``), or both.  For a
    live pixel i (label t in [0, K), not ``ignore_index``) with p = softmax(z_i):

        q = p_t,   u = sum_{k != t} p_k  (1 - q without its cancellation),   L = logsumexp(z_i) - z_{i,t},
        l_i = w[t] u^gamma L                                                  (u^gamma = 1 at gamma = 0; l_i >= +0),
        n = the live pixels of the batch,
        top_k = None:  HCE = sum_i l_i / sum_i w[t_i]                         (0 when the denominator is 0),
        top_k = rho:   k = max(1, floor(double(float32(rho)) n)),  tau = the k-th largest l_i (as fp32 values),
                       n_gt = #{l_i > tau},  n_eq = #{l_i = tau},  f = (k - n_gt) / n_eq,
                       m_i = 1 (l_i > tau), f (l_i = tau), 0 (l_i < tau),
                       HCE = sum_i m_i l_i / sum_i m_i w[t_i]                 (0 when the denominator is 0; n = 0: 0),
        loss = ce * HCE + tversky * mean_r mean_{c in C} (1 - TI_rc).

    The values tied at the threshold share the remaining places equally, so the loss does not depend on the order
    of the pixels and the gradient, dHCE/dz_{i,k} = m_i w[t] (p_k - [k = t]) (u^gamma + gamma q u^(gamma-1) L) / W
    with W the denominator of HCE, is one definite subgradient.  ``top_k = 1.0`` is ``top_k = None``;
    ``gamma = 0, top_k = None`` is ``MultiClassSegLoss``; with unit weights, nothing ignored and rho n an integer,
    ``gamma = 0, top_k = rho`` is ``torch.topk(F.cross_entropy(z, t, reduction="none").view(-1), k).values.mean()``.
    The Tversky term and every other argument are ``MultiClassSegLoss``'; ``per_sample`` concerns that term only.

    ``gamma`` is a host constant.  The fraction lives in a one-element device tensor the kernels read:
    ``set_top_k(rho)`` fills it in place, so a captured graph follows a schedule without a re-capture; ``top_k`` is
    the host copy (None: no selection, and that cannot be changed later).  ``schedule``: a callable epoch -> rho,
    applied by ``on_epoch(epoch)``, which csu.train.train_model calls at the start of every epoch.  ``last_terms``:
    the fp64 (4,) device tensor (HCE, Tversky term, tau, k) of the last call (no selection: tau = 0, k = n).

    On the GPU with K <= 32 everything comes from the fused csu_seg_hard kernels, the selection from
    csu_kth_largest, with no host synchronisation; CPU tensors and more classes take the same formula, tie rule
    included, in torch ops."""

    def __init__(self, num_classes: int, ce: float = 1.0, tversky: float = 1.0, alpha: float = 0.5, beta: float = 0.5,
                 smooth: float = 0.5, class_weight=None, ignore_index: int = -100, per_sample: bool = False,
                 include_background: bool = True, gamma: float = 0.0, top_k=None, schedule=None):
        super().__init__(num_classes, ce, tversky, alpha, beta, smooth, class_weight, ignore_index, per_sample,
                         include_background)
        if not float(gamma) >= 0.0 or float(gamma) == float("inf"):
            raise ValueError(f"HardExampleSegLoss: gamma must be a finite number >= 0 (got {gamma!r})")
        if top_k is not None:
            self._check_top_k(top_k)
        if schedule is not None and not callable(schedule):
            raise ValueError("HardExampleSegLoss: schedule is a callable epoch -> top_k fraction, or None")
        if schedule is not None and top_k is None:
            raise ValueError("HardExampleSegLoss: a schedule needs a top_k to start from")
        self.gamma, self.schedule = float(gamma), schedule
        self._rho, self._rhos = None if top_k is None else float(top_k), {}
        self.last_terms = None

    @staticmethod
    def _check_top_k(rho):
        if isinstance(rho, bool) or not 0.0 < float(rho) <= 1.0:
            raise ValueError(f"HardExampleSegLoss: top_k must be a fraction in (0, 1], or None (got {rho!r})")

    def __repr__(self):
        return (f"HardExampleSegLoss({super().__repr__()[len('MultiClassSegLoss('):-1]}, gamma={self.gamma}, "
                f"top_k={self._rho}, schedule={self.schedule!r})")

    @property
    def top_k(self):
        """The current top-k fraction (the host copy of the device scalar), or None."""
        return self._rho

    def set_top_k(self, rho: float) -> None:
        """Set the fraction; every device's scalar is filled in place (no re-capture, no synchronisation)."""
        if self._rho is None:
            raise ValueError("HardExampleSegLoss: this criterion was made without a selection (top_k=None)")
        self._check_top_k(rho)
        self._rho = float(rho)
        for t in self._rhos.values():
            t.fill_(self._rho)

    def on_epoch(self, epoch: int) -> None:
        """Apply the schedule, if there is one, for the epoch that starts (0-based)."""
        if self.schedule is not None:
            self.set_top_k(self.schedule(int(epoch)))

    def _scalar(self, device):
        if self._rho is None:
            return None
        t = self._rhos.get(device)
        if t is None:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("HardExampleSegLoss: call the criterion once on this device before capturing it in a "
                                   "graph (the fraction's device scalar is made at the first call)")
            t = self._rhos[device] = torch.full((1,), self._rho, dtype=torch.float32, device=device)
        return t

    def _hard_torch(self, z, t, rho):
        """(HCE, tau, k) in torch ops, in z's floating dtype: z (B, K, *), t (B, *) int64, rho a one-element fp32
        tensor or None."""
        B, K = z.shape[0], z.shape[1]
        z2, t2 = z.reshape(B, K, -1), t.reshape(B, -1)
        live = (t2 != self.ignore_index) & (t2 >= 0) & (t2 < K)
        tc = torch.where(live, t2, torch.zeros_like(t2))
        w = self._weight(z.device)
        w = torch.ones(K, dtype=z.dtype, device=z.device) if w is None else w.to(z.dtype)
        lv = live.to(z.dtype)
        lsm = torch.log_softmax(z2, 1)
        oh = F.one_hot(tc, K).permute(0, 2, 1).to(z.dtype)
        L = -lsm.gather(1, tc.unsqueeze(1)).squeeze(1)
        wt = w[tc] * lv
        if self.gamma == 0.0:
            ug = torch.ones_like(L)
        else:
            u = (lsm.exp() * (1.0 - oh)).sum(1)
            pos = u > 0            # u^gamma and its derivative are 0 at u = 0, whatever gamma > 0
            ug = torch.where(pos, torch.where(pos, u, torch.ones_like(u)).pow(self.gamma), torch.zeros_like(u))
        l = wt * ug * L
        n = live.sum()
        if rho is None:
            num, W, tau, k = l.sum(), wt.sum(), torch.zeros((), dtype=z.dtype, device=z.device), n.to(torch.float64)
        else:
            kk = torch.floor(rho[0].double() * n.double()).clamp(min=1.0).minimum(n.double())      # 0 when n = 0
            keys = torch.where(live, l.detach(), torch.full_like(l, -1.0)).reshape(-1)
            srt = torch.sort(keys, descending=True).values
            tau = srt[(kk.long() - 1).clamp(min=0)].clamp_min(0.0)
            gt, eq = live.reshape(-1) & (keys > tau), live.reshape(-1) & (keys == tau)
            n_gt, n_eq = gt.sum().double(), eq.sum().double()
            f = torch.where(n_eq > 0, (kk - n_gt) / n_eq.clamp(min=1.0), torch.zeros_like(kk))
            m = (gt.to(torch.float64) + f * eq.to(torch.float64)).to(z.dtype).reshape(l.shape)
            num, W, k = (m * l).sum(), (m * wt).sum(), kk
        hce = torch.where(W > 0, num / torch.where(W > 0, W, torch.ones_like(W)), num * 0.0)
        return hce, tau.detach(), k

    def _run(self, logits, target, with_stats):
        K = self.num_classes
        target = self._label_map(logits, target)
        with torch.autocast(logits.device.type, enabled=False):
            rho = self._scalar(logits.device)
            if logits.is_cuda and K <= 32:
                from . import ops
                z = logits if logits.dtype in (torch.float32, torch.bfloat16) else logits.float()
                rows = logits.shape[0] if self.per_sample else 1
                res = ops.seg_hard(z, target, self.params, self.gamma, rho, self._weight(logits.device), self.ignore_index,
                                   rows, self.include_background, with_stats)
                self.last_terms = res[1]
                return (res[0], res[2]) if with_stats else res[0]
            z, t = logits.float(), target.long()
            tv = self._terms_torch(z, t)[1]
            hce, tau, k = self._hard_torch(z, t, rho)
            self.last_terms = torch.stack([hce.detach().double(), tv.detach().double(), tau.double(), k.double()])
            loss = self.ce * hce + self.tversky * tv
            if not with_stats:
                return loss
            return loss, self.hard_stats(z.detach(), t)


def focal_loss(num_classes: int, gamma: float = 2.0, class_weight=None, ignore_index: int = -100) -> HardExampleSegLoss:
    """The multi-class focal loss: the weighted mean of (1 - p_t)^gamma (-log p_t)."""
    return HardExampleSegLoss(num_classes, ce=1.0, tversky=0.0, class_weight=class_weight, ignore_index=ignore_index,
                              gamma=gamma)


def dice_focal_loss(num_classes: int, gamma: float = 2.0, focal: float = 1.0, dice: float = 1.0, smooth: float = 1.0,
                    class_weight=None, ignore_index: int = -100, per_sample: bool = False,
                    include_background: bool = True) -> HardExampleSegLoss:
    """focal * focal loss + dice * mean over classes of (1 - Dice_c); smooth is Dice's, as in ce_dice_loss."""
    return HardExampleSegLoss(num_classes, ce=focal, tversky=dice, alpha=0.5, beta=0.5, smooth=smooth / 2,
                              class_weight=class_weight, ignore_index=ignore_index, per_sample=per_sample,
                              include_background=include_background, gamma=gamma)


def topk_ce_loss(num_classes: int, top_k: float = 0.1, class_weight=None, ignore_index: int = -100,
                 schedule=None) -> HardExampleSegLoss:
    """Cross-entropy averaged over the hardest top_k fraction of the batch's pixels (nnU-Net's TopKLoss, k = 10 %)."""
    return HardExampleSegLoss(num_classes, ce=1.0, tversky=0.0, class_weight=class_weight, ignore_index=ignore_index,
                              top_k=top_k, schedule=schedule)


def dice_topk_loss(num_classes: int, top_k: float = 0.1, ce: float = 1.0, dice: float = 1.0, smooth: float = 1.0,
                   class_weight=None, ignore_index: int = -100, per_sample: bool = False, include_background: bool = True,
                   schedule=None) -> HardExampleSegLoss:
    """ce * top-k CE + dice * mean over classes of (1 - Dice_c) (nnU-Net's DC_and_topk_loss); smooth is Dice's."""
    return HardExampleSegLoss(num_classes, ce=ce, tversky=dice, alpha=0.5, beta=0.5, smooth=smooth / 2,
                              class_weight=class_weight, ignore_index=ignore_index, per_sample=per_sample,
                              include_background=include_background, top_k=top_k, schedule=schedule)


def _lovasz_torch(z, t, classes, present_only: bool, per_image: bool, ignore_index: int):
    """The Lovasz-Softmax term LS in torch ops, in z's floating dtype: z (B, K, *), t (B, *) int64, classes a sorted
    list of class indices.  The order is ``torch.sort(descending=True, stable=True)`` of the clamped errors with the
    dead pixels behind the live ones; the increments g are formed in fp64 from the integer counts and are constants
    of the gradient, so autograd gives dLS/dp_c = -/+ g_rank scale."""
    B, K = z.shape[0], z.shape[1]
    z2, t2 = z.reshape(B, K, -1), t.reshape(B, -1)
    live = t2 != ignore_index
    p = torch.softmax(z2, 1)
    cls = torch.as_tensor(classes, dtype=torch.int64, device=z.device)
    fg = (t2.unsqueeze(0) == cls.view(-1, 1, 1)) & live.unsqueeze(0)                     # (|C|, B, HW)
    off = 1.0 - torch.eye(K, dtype=z.dtype, device=z.device)[:, cls]
    others = torch.einsum("bkn,kc->cbn", p, off)                                         # sum_{k != c} p_k, no 1 - p_c
    e = torch.where(fg, others, p[:, cls].permute(1, 0, 2))
    e = e + (torch.where(e < 1, e, torch.ones_like(e)) - e).detach()                     # fminf(e, 1); the gradient is e's
    rows = len(classes) * B if per_image else len(classes)
    e, fg, lv = e.reshape(rows, -1), fg.reshape(rows, -1), live.unsqueeze(0).expand_as(fg).reshape(rows, -1)
    key = torch.where(lv, e.detach(), torch.full_like(e, -1.0))
    order = torch.sort(key, dim=1, descending=True, stable=True).indices
    es, fs, ls = e.gather(1, order), fg.gather(1, order).long(), lv.gather(1, order)
    G = fs.sum(1, keepdim=True)
    I = G - (fs.cumsum(1) - fs)
    U = I + torch.arange(es.shape[1], device=z.device).view(1, -1)
    Id, Ud = I.double(), U.double()
    safe = torch.where(U > 0, Ud, torch.ones_like(Ud))
    g = torch.where(fs > 0, 1.0 / safe, torch.where(U > 0, Id / (safe * (safe + 1.0)), torch.ones_like(Ud)))
    g = torch.where(ls, g, torch.zeros_like(g))
    present = (G.view(len(classes), -1) > 0)                                            # (|C|, B or 1)
    counted = present if present_only else torch.ones_like(present)
    number = counted.sum(0, keepdim=True).clamp(min=1).double() * (B if per_image else 1)
    scale = (counted.double() / number).reshape(rows, 1)
    return (es * (g * scale).to(z.dtype)).sum()


def _lovasz_classes(classes, K: int, what: str):
    """(sorted class list, present_only) of the ``classes`` argument."""
    if isinstance(classes, str):
        if classes not in ("present", "all"):
            raise ValueError(f"{what}: classes is 'present', 'all' or a list of class indices (got {classes!r})")
        return list(range(K)), classes == "present"
    try:
        cls = [c for c in classes]
    except TypeError:
        raise ValueError(f"{what}: classes is 'present', 'all' or a list of class indices (got {classes!r})") from None
    if not cls or any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < K for c in cls) or len(set(cls)) != len(cls):
        raise ValueError(f"{what}: classes must be distinct class indices in [0, {K}) (got {classes!r})")
    return sorted(cls), False


def reference_lovasz_softmax(logits: torch.Tensor, target: torch.Tensor, classes="present", per_image: bool = False,
                             ignore_index: int = -100) -> torch.Tensor:
    """The Lovasz-Softmax term of ``LovaszSegLoss`` in fp64 torch ops on the tensors' device: the statement of its
    definition (differentiable in the logits).  logits (B, K, *spatial), target (B, *spatial) integer labels."""
    cls, present_only = _lovasz_classes(classes, logits.shape[1], "reference_lovasz_softmax")
    return _lovasz_torch(logits.double(), target.long(), cls, present_only, bool(per_image), int(ignore_index))


class LovaszSegLoss(MultiClassSegLoss):
    """``MultiClassSegLoss`` plus the Lovasz-Softmax loss of Berman, Triki and Blaschko ("The Lovasz-Softmax loss: a
    tractable surrogate for the optimization of the intersection-over-union measure in neural networks", CVPR 2018),
    the convex surrogate of the mean IoU that csu.train reports.  A segment is one class c of ``classes`` over the
    whole batch, or one (image, class) pair with ``per_image``.  For a segment with n live pixels (label not
    ``ignore_index``) in ascending flat index, p = softmax(z):

        fg_i = [t_i = c],   e_i = min(sum_{k != c} p_k if fg_i else p_c, 1),
        pi = the order of descending e, ties in ascending index,   G = sum fg,
        for j = 1 .. n:  F = #fg among pi(1 .. j-1),  I = G - F,  U = I + (j - 1),
        g_j = 1 / U if pi(j) is foreground, else I / (U (U + 1))            (g_1 = 1 when U = 0: G = 0),
        LS_seg = sum_j e_pi(j) g_j,

    the g_j being the increments of the Jaccard loss along the order (Berman's ``lovasz_grad``) in closed form.
    ``classes="present"`` (the default) averages LS_seg over the classes with a foreground pixel (0 when there is
    none), ``"all"`` or a list of class indices over all of them; with ``per_image`` that average is taken within
    every image and LS is the mean over the B images.

        loss = ce * CE + tversky * mean_r mean_{c in C} (1 - TI_rc) + lovasz_weight * LS.

    ``ce = tversky = 0`` is legal here (the term alone).  The weight lives in a one-element device tensor the kernels
    read: ``set_lovasz_weight(w)`` fills it in place, so a captured graph follows a schedule without a re-capture;
    ``lovasz_weight`` is the host copy.  ``schedule``: a callable epoch -> weight, applied by ``on_epoch(epoch)``,
    which csu.train.train_model calls at the start of every epoch.  ``last_terms``: the (2,) device tensor (loss
    without the term, LS) of the last call.

    On the GPU with K <= 32 the loss and its gradient come from the fused csu_seg_lovasz kernels and the stable
    radix sort csu_sort_pairs, with no host synchronisation; CPU tensors and more classes take the same formula in
    torch ops with ``torch.sort(stable=True)``."""

    _other_terms = True

    def __init__(self, num_classes: int, ce: float = 1.0, tversky: float = 1.0, alpha: float = 0.5, beta: float = 0.5,
                 smooth: float = 0.5, class_weight=None, ignore_index: int = -100, per_sample: bool = False,
                 include_background: bool = True, lovasz: float = 1.0, classes="present", per_image: bool = False,
                 schedule=None):
        super().__init__(num_classes, ce, tversky, alpha, beta, smooth, class_weight, ignore_index, per_sample,
                         include_background)
        self._check_weight(lovasz)
        self._classes, self.present_only = _lovasz_classes(classes, num_classes, "LovaszSegLoss")
        if schedule is not None and not callable(schedule):
            raise ValueError("LovaszSegLoss: schedule is a callable epoch -> weight, or None")
        self.classes = classes if isinstance(classes, str) else list(self._classes)
        self.per_image, self.schedule = bool(per_image), schedule
        self._w, self._wlv = float(lovasz), {}
        self.last_terms = None

    @staticmethod
    def _check_weight(w):
        if isinstance(w, bool) or not float(w) >= 0.0 or float(w) == float("inf"):
            raise ValueError(f"LovaszSegLoss: the Lovasz weight must be a finite number >= 0 (got {w!r})")

    def __repr__(self):
        return (f"LovaszSegLoss({super().__repr__()[len('MultiClassSegLoss('):-1]}, lovasz={self._w}, "
                f"classes={self.classes!r}, per_image={self.per_image}, schedule={self.schedule!r})")

    @property
    def lovasz_weight(self) -> float:
        """The current weight of the Lovasz-Softmax term (the host copy of the device scalar)."""
        return self._w

    def set_lovasz_weight(self, w: float) -> None:
        """Set the weight; every device's scalar is filled in place (no re-capture, no synchronisation)."""
        self._check_weight(w)
        self._w = float(w)
        for t in self._wlv.values():
            t.fill_(self._w)

    def on_epoch(self, epoch: int) -> None:
        """Apply the schedule, if there is one, for the epoch that starts (0-based)."""
        if self.schedule is not None:
            self.set_lovasz_weight(self.schedule(int(epoch)))

    def _scalar(self, device):
        t = self._wlv.get(device)
        if t is None:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("LovaszSegLoss: call the criterion once on this device before capturing it in a "
                                   "graph (the weight's device scalar is made at the first call)")
            t = self._wlv[device] = torch.full((1,), self._w, dtype=torch.float32, device=device)
        return t

    def _run(self, logits, target, with_stats):
        K = self.num_classes
        target = self._label_map(logits, target)
        with torch.autocast(logits.device.type, enabled=False):
            w = self._scalar(logits.device)
            if logits.is_cuda and K <= 32:
                from . import ops
                z = logits if logits.dtype in (torch.float32, torch.bfloat16) else logits.float()
                rows = logits.shape[0] if self.per_sample else 1
                res = ops.seg_lovasz(z, target, w, self.params, self._classes, self.present_only, self.per_image,
                                     self._weight(logits.device), self.ignore_index, rows, self.include_background,
                                     with_stats)
                self.last_terms = res[1]
                return (res[0], res[2]) if with_stats else res[0]
            z, t = logits.float(), target.long()
            base = self._torch(z, t)
            ls = _lovasz_torch(z, t, self._classes, self.present_only, self.per_image, self.ignore_index)
            self.last_terms = torch.stack([base.detach(), ls.detach()])
            loss = base + w[0] * ls
            if not with_stats:
                return loss
            return loss, self.hard_stats(z.detach(), t)


def lovasz_softmax_loss(num_classes: int, classes="present", per_image: bool = False, ignore_index: int = -100,
                        schedule=None) -> LovaszSegLoss:
    """The Lovasz-Softmax term alone (weight 1), with the per-class metrics of MultiClassSegLoss."""
    return LovaszSegLoss(num_classes, ce=0.0, tversky=0.0, ignore_index=ignore_index, lovasz=1.0, classes=classes,
                         per_image=per_image, schedule=schedule)


def ce_lovasz_loss(num_classes: int, ce: float = 1.0, lovasz: float = 1.0, classes="present", per_image: bool = False,
                   class_weight=None, ignore_index: int = -100, schedule=None) -> LovaszSegLoss:
    """ce * CE + lovasz * Lovasz-Softmax (Berman's recommended pairing for fine-tuning on the IoU)."""
    return LovaszSegLoss(num_classes, ce=ce, tversky=0.0, class_weight=class_weight, ignore_index=ignore_index,
                         lovasz=lovasz, classes=classes, per_image=per_image, schedule=schedule)
