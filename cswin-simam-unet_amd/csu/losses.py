"""Training criteria for binary segmentation beyond nn.BCELoss: soft Dice, BCE + Dice, Tversky.

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
