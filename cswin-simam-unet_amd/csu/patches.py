"""Patch training from full-size images (csrc/patch.hip, csu_patch_warp in csrc/augment_warp.hip; ABI and the
exact definitions in include/csu.h, "Patch pool"): the cases stay on the device at their own size, and every
step cuts a batch of patches from them there -- draw the image, force a share of the slots onto a random
foreground pixel of a random class present in it (nnU-Net's oversampling, without which small classes are almost
never seen), crop, augment, normalise -- with no host synchronisation, so the whole data path can be captured in
a HIP graph with ``rng.advance`` inside.  The reference has no counterpart: it trains on resized images only.

``PatchPool`` packs the cases and builds the row index once, ``PatchSampler.sample()`` is one step's batch,
``PatchLoader`` is the ``train_loader`` of ``train_model``.  ``reference_patch_draw`` / ``reference_patch_sample``
state the definitions in numpy / fp64 torch; a pool on the CPU runs them (its words come from a
``torch.Generator``: the CPU and GPU streams differ, the definitions do not)."""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import numpy as np
import torch

from .augment import (SpatialAugment, T_SIGMA, identity_table, reference_sample_at, reference_source_coords)

RECORD = 16
(R_N, R_CLS, R_CY, R_CX, R_OY, R_OX, R_FG, R_COUNT, R_W0) = range(9)
MAX_EXTENT = (1 << 24) - 2          # clamp bounds and origins stay exact fp32 integers

__all__ = ["PatchPool", "PatchSampler", "PatchLoader", "reference_patch_draw", "reference_patch_sample",
           "reference_row_index", "reference_locate", "class_map", "RECORD"]


def num_index_classes(K: int) -> int:
    """Classes the row index counts: 2 for the binary case (K = 1), else K."""
    return 2 if int(K) == 1 else int(K)


def class_map(label: np.ndarray, K: int) -> np.ndarray:
    """The class of every label value: K = 1: label > 0; else the label itself (a value >= K is no class)."""
    return (label > 0).astype(np.int64) if int(K) == 1 else label.astype(np.int64)


def reference_row_index(label: np.ndarray, K: int) -> np.ndarray:
    """int32 (Kc, H + 1): rows[c][y] = pixels of class c in rows [0, y) of the (H, W) label map."""
    Kc, cls = num_index_classes(K), class_map(label, K)
    rows = np.zeros((Kc, label.shape[0] + 1), dtype=np.int64)
    for c in range(Kc):
        rows[c, 1:] = np.cumsum((cls == c).sum(axis=1))
    return rows.astype(np.int32)


def reference_locate(label: np.ndarray, K: int, c: int, r: int, rows: Optional[np.ndarray] = None):
    """(y, x) of the r-th pixel of class c in raster order through the row index, as the kernel finds it: the row
    with rows[y] <= r < rows[y + 1], then the (r - rows[y])-th pixel of the class in that row; (-1, -1) when the
    rank is not below the class's count."""
    rows = reference_row_index(label, K) if rows is None else rows
    if not 0 <= c < rows.shape[0] or r < 0 or r >= int(rows[c, -1]):
        return -1, -1
    y = int(np.searchsorted(rows[c], r, side="right")) - 1
    xs = np.flatnonzero(class_map(label[y], K) == c)
    return y, int(xs[r - int(rows[c, y])])


def _pick(w: int, n: int) -> int:
    return (int(w) * int(n)) >> 32


def reference_origin(L: int, P: int, fg: bool, c: int, w: int) -> int:
    """The patch origin along one axis: image extent L, patch extent P, centre c of a foreground slot, word w."""
    if L < P:
        return -((P - L) // 2)
    return min(max(c - P // 2, 0), L - P) if fg else _pick(w, L - P + 1)


def default_class_mask(K: int) -> int:
    return (1 << max(int(K), 2)) - 2          # every class but 0


def reference_patch_draw(words, pool: "PatchPool", Ph: int, Pw: int, fg_slots: int = 0, p_fg: float = 0.0,
                         class_mask: Optional[int] = None, indices=None) -> np.ndarray:
    """csu_patch_draw from given Philox words: int32 (B, 16) records {n, cls, cy, cx, oy, ox, fg, count, w0..w7} of
    uint32 ``words`` (B, 8) (int32 bit patterns are taken as such) for a pool on the CPU."""
    w = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    B, K = w.shape[0], pool.num_classes
    Kc = num_index_classes(K)
    mask = default_class_mask(K) if class_mask is None else int(class_mask)
    p = float(np.float32(p_fg))
    rec = np.zeros((B, RECORD), dtype=np.int64)
    for b in range(B):
        n = min(max(int(indices[b]), 0), pool.N - 1) if indices is not None else _pick(w[b, 0], pool.N)
        label, rows = pool.label(n).numpy(), pool.row_table(n)
        H, W = label.shape
        fg = b < fg_slots or (int(w[b, 1]) >> 8) / 16777216.0 < p
        cls, cy, cx, count = -1, -1, -1, 0
        if fg:
            present = [c for c in range(Kc) if (mask >> c) & 1 and int(rows[c, -1]) > 0]
            if present:
                cls = present[_pick(w[b, 2], len(present))]
                count = int(rows[cls, -1])
                cy, cx = reference_locate(label, K, cls, _pick(w[b, 3], count), rows)
            else:
                fg = False
        oy, ox = reference_origin(H, Ph, fg, cy, w[b, 4]), reference_origin(W, Pw, fg, cx, w[b, 5])
        rec[b, :8] = (n, cls, cy, cx, oy, ox, int(fg), count)
    rec[:, 8:] = w
    return _to_i32(rec)


def _to_i32(a: np.ndarray) -> np.ndarray:
    """int64 values in [-2^31, 2^32) -> their int32 bit patterns."""
    return (a & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def reference_patch_sample(pool: "PatchPool", record, Ph: int, Pw: int, table: torch.Tensor,
                           ctrl: Optional[torch.Tensor] = None, *, spacing: int = 0, border: str = "constant",
                           image_fill: float = 0.0, pad_label: int = 0, mask_mode: str = "bilinear", out: str = "binary",
                           noise: Optional[torch.Tensor] = None):
    """The definitions of csu_patch_warp in fp64 for a pool on the CPU: slot b is image record[b, 0] sampled at
    (ox, oy) + A(p + d(p)), p over the Ph x Pw patch (``reference_source_coords`` in the patch frame, then
    ``reference_sample_at`` against that image with its own borders and mean) -> fp32 (B, 3, Ph, Pw) and the mask
    as ``reference_augment`` returns it."""
    rec = np.asarray(record)
    sx, sy = reference_source_coords(table, ctrl, spacing, Ph, Pw)
    imgs, masks = [], []
    for b in range(rec.shape[0]):
        n = min(max(int(rec[b, R_N]), 0), pool.N - 1)
        oy, ox = (min(max(int(v), -(1 << 24)), 1 << 24) for v in (rec[b, R_OY], rec[b, R_OX]))
        oi, om = reference_sample_at(pool.image(n)[None], pool.label(n)[None], table[b:b + 1], sx[b:b + 1] + ox,
                                     sy[b:b + 1] + oy, border=border, image_fill=image_fill, pad_label=pad_label,
                                     mask_mode=mask_mode, out=out, noise=None if noise is None else noise[b:b + 1],
                                     mean=pool.mean64(n))
        imgs.append(oi)
        masks.append(om)
    return torch.cat(imgs), torch.cat(masks)


class PatchPool:
    """The cases of a training set on ``device`` at their own sizes: ``images`` a sequence of uint8 (H_i, W_i, 3),
    ``labels`` of uint8 (H_i, W_i) (numpy arrays or tensors).  ``num_classes = 1``: binary masks, a value > 0 is
    class 1; otherwise 2 <= K <= 32 and a label >= K (``ignore_index``) is never a centre and passes through the
    warp unchanged.  Packed into ``pixels`` (uint8, HWC, back to back), ``labels`` (uint8), ``meta`` int64 (N, 4) =
    {pixel offset, H, W, row-table offset}, ``mean`` fp32 (N,) (csu_augment_mean, what the contrast step of a patch
    of that image uses) and ``rows``, the int32 row index of csu_patch_index.  N <= 2^20, H_i W_i < 2^31."""

    def __init__(self, images: Sequence, labels: Sequence, num_classes: int, device, ignore_index: Optional[int] = None):
        K = int(num_classes)
        if not (K == 1 or 2 <= K <= 32):
            raise ValueError("PatchPool: num_classes 1 (binary) or 2..32")
        if ignore_index is not None and not (K >= 2 and K <= int(ignore_index) <= 255):
            raise ValueError("PatchPool: ignore_index in num_classes..255 (multi-class only)")
        if len(images) != len(labels) or not 1 <= len(images) <= 1 << 20:
            raise ValueError("PatchPool: as many label maps as images, 1 .. 2^20 of them")
        self.num_classes, self.ignore_index, self.device = K, ignore_index, torch.device(device)
        self.N = len(images)
        Kc = num_index_classes(K)
        meta, off, roff = [], 0, 0
        for i, (im, lb) in enumerate(zip(images, labels)):
            H, W = int(im.shape[0]), int(im.shape[1])
            if im.dtype not in (np.uint8, torch.uint8) or lb.dtype not in (np.uint8, torch.uint8) or tuple(im.shape) != (H, W, 3) \
                    or tuple(lb.shape) != (H, W):
                raise ValueError(f"PatchPool: case {i}: a uint8 (H, W, 3) image and a uint8 (H, W) label map")
            if H < 1 or W < 1 or H * W >= 1 << 31 or max(H, W) > MAX_EXTENT:
                raise ValueError(f"PatchPool: case {i}: H W < 2^31 and H, W <= {MAX_EXTENT}")
            meta.append((off, H, W, roff))
            off, roff = off + H * W, roff + Kc * (H + 1)
        if roff >= 1 << 31:
            raise ValueError("PatchPool: the row index needs 2^31 entries or more")
        self._meta = meta
        self.pixels = torch.empty(3 * off, dtype=torch.uint8, device=self.device)
        self.labels = torch.empty(off, dtype=torch.uint8, device=self.device)
        for (o, H, W, _), im, lb in zip(meta, images, labels):        # case by case: no second host copy of the set
            self.pixels[3 * o:3 * (o + H * W)].copy_(torch.as_tensor(im).reshape(-1))
            self.labels[o:o + H * W].copy_(torch.as_tensor(lb).reshape(-1))
        self.meta = torch.tensor(meta, dtype=torch.int64).to(self.device)
        self._mean64 = {}
        if self.device.type == "cpu":
            self.mean = torch.tensor([self.mean64(i) for i in range(self.N)], dtype=torch.float64).float()
            self.rows = torch.from_numpy(np.concatenate([reference_row_index(self.label(i).numpy(), K).reshape(-1)
                                                         for i in range(self.N)]))
        else:
            from . import ops
            self.mean = torch.cat([ops.augment_mean(self.pixels[3 * o:3 * (o + H * W)][None]) for o, H, W, _ in meta])
            self.rows = ops.patch_index(self.labels, self.meta, K, max(m[1] for m in meta), roff)

    @classmethod
    def from_dataset(cls, ds, num_classes: int, device, ignore_index: Optional[int] = None) -> "PatchPool":
        """The pool of a dataset whose items are (uint8 (H, W, 3) image, uint8 (H, W) mask / label map), read case by
        case: ``SegmentationDataset(..., image_size=None, raw=True)``."""
        items = [ds[i] for i in range(len(ds))]
        return cls([it[0] for it in items], [it[1] for it in items], num_classes, device, ignore_index)

    def __len__(self):
        return self.N

    def size(self, i: int):
        return self._meta[i][1], self._meta[i][2]

    def image(self, i: int) -> torch.Tensor:
        """uint8 (H_i, W_i, 3) view of case i."""
        o, H, W, _ = self._meta[i]
        return self.pixels[3 * o:3 * (o + H * W)].view(H, W, 3)

    def label(self, i: int) -> torch.Tensor:
        """uint8 (H_i, W_i) view of case i's label map."""
        o, H, W, _ = self._meta[i]
        return self.labels[o:o + H * W].view(H, W)

    def row_table(self, i: int) -> np.ndarray:
        """int32 (Kc, H_i + 1) of case i, on the host."""
        _, H, _, r = self._meta[i]
        Kc = num_index_classes(self.num_classes)
        return self.rows[r:r + Kc * (H + 1)].view(Kc, H + 1).cpu().numpy()

    def mean64(self, i: int) -> torch.Tensor:
        """fp64 (1,): the exact byte mean / 255 of case i."""
        if i not in self._mean64:
            a = self.image(i).cpu().numpy()
            self._mean64[i] = torch.tensor([int(a.sum(dtype=np.uint64)) / (255.0 * a.size)], dtype=torch.float64)
        return self._mean64[i]

    def pairs(self) -> Iterable:
        """(image uint8 (H, W, 3), label map uint8 (H, W)) copies on the pool's device, for ``evaluate_full_res``."""
        for i in range(self.N):
            yield self.image(i).clone(), self.label(i).clone()

    def locate(self, image, cls, rank) -> torch.Tensor:
        """int32 (M, 2) {y, x} of the rank-th pixel (raster order) of class ``cls`` in case ``image`` (ints, sequences
        or int tensors, broadcast to a common length); {-1, -1} for a rank not below the class's count."""
        n, c, r = torch.broadcast_tensors(*(torch.as_tensor(v, dtype=torch.int32).reshape(-1) for v in (image, cls, rank)))
        if self.device.type == "cpu":
            out = [(-1, -1) if not 0 <= int(a) < self.N else
                   reference_locate(self.label(int(a)).numpy(), self.num_classes, int(b), int(q), self.row_table(int(a)))
                   for a, b, q in zip(n, c, r)]
            return torch.tensor(out, dtype=torch.int32)
        from . import ops
        return ops.patch_locate(self, *(t.contiguous().to(self.device) for t in (n, c, r)))


class PatchSampler:
    """Batches of ``batch_size`` patches of ``patch_size`` (int or (Ph, Pw)) from a ``PatchPool``.

    ``foreground``: the share of slots centred on a random pixel of a random eligible class present in the slot's
    image; ``foreground_mode`` "slots" forces the first round(foreground * B) slots (nnU-Net's rule), "probability"
    makes every slot foreground with that probability (a slot then stays a pure function of (seed, counter, site,
    slot)).  ``classes``: the eligible classes (default: all but 0).  A patch never leaves an image at least its
    size before augmentation; a smaller image is centred and padded (``augment``'s image_fill / pad_label, else 0
    and the pool's ignore_index).  ``augment``: a ``SpatialAugment`` drawn for the patch size (None: the identity).

    ``sample()`` -> (images fp32 (B, 3, Ph, Pw), labels int64 (B, Ph, Pw)), or for a binary pool masks fp32
    (B, 1, Ph, Pw) in the augment's ``mask_mode``; ``last_record`` holds the int32 (B, 16) record of the draw."""

    def __init__(self, pool: PatchPool, patch_size, batch_size: int, foreground: float = 0.33, foreground_mode: str = "slots",
                 classes: Optional[Sequence[int]] = None, augment: Optional[SpatialAugment] = None):
        self.pool, self.B = pool, int(batch_size)
        self.Ph, self.Pw = (int(patch_size),) * 2 if np.isscalar(patch_size) else (int(patch_size[0]), int(patch_size[1]))
        if self.B < 1 or self.Ph < 1 or self.Pw < 1:
            raise ValueError("PatchSampler: batch_size and patch_size >= 1")
        if not 0.0 <= float(foreground) <= 1.0 or foreground_mode not in ("slots", "probability"):
            raise ValueError("PatchSampler: foreground in [0, 1], foreground_mode 'slots' or 'probability'")
        slots = foreground_mode == "slots"
        self.fg_slots, self.p_fg = (int(round(float(foreground) * self.B)), 0.0) if slots else (0, float(foreground))
        Kc = num_index_classes(pool.num_classes)
        if classes is None:
            self.class_mask = default_class_mask(pool.num_classes)
        else:
            if not classes or any(not 0 <= int(c) < Kc for c in classes):
                raise ValueError(f"PatchSampler: classes within 0..{Kc - 1}")
            self.class_mask = sum(1 << c for c in set(int(c) for c in classes))
        self.augment = augment
        binary = pool.num_classes == 1
        self.mask_mode = (augment.mask_mode if augment is not None else "bilinear") if binary else "nearest"
        self.out = "binary" if binary else "labels"
        self.border = augment.border if augment is not None else "constant"
        self.image_fill = augment.image_fill if augment is not None else 0.0
        self.pad_label = augment.pad_label if augment is not None else (0 if pool.ignore_index is None else pool.ignore_index)
        self._identity = identity_table(self.B, pool.device)          # built here: sample() uploads nothing
        self.last_record = None

    def sample(self, snapshot: Optional[torch.Tensor] = None, indices: Optional[torch.Tensor] = None, generator=None):
        """One batch.  GPU pool: csu_patch_draw, csu_augment_draw and csu_patch_warp under one snapshot (default
        ``rng.snapshot``), no host synchronisation.  ``indices``: int32 (B,) cases instead of drawn ones.  CPU
        pool: the references, with words, draws and normals from ``generator``."""
        pool, aug, B, Ph, Pw = self.pool, self.augment, self.B, self.Ph, self.Pw
        kw = dict(border=self.border, image_fill=self.image_fill, pad_label=self.pad_label, mask_mode=self.mask_mode, out=self.out)
        if pool.device.type == "cpu":
            words = torch.randint(0, 1 << 32, (B, 8), dtype=torch.int64, generator=generator).numpy()
            rec = reference_patch_draw(words, pool, Ph, Pw, self.fg_slots, self.p_fg, self.class_mask,
                                       None if indices is None else indices.tolist())
            table, ctrl = (self._identity, None) if aug is None else aug.draw(B, Ph, Pw, "cpu", generator=generator)
            noise = None
            if bool((table[:, T_SIGMA] > 0).any()):
                noise = torch.randn(B, 3, Ph, Pw, dtype=torch.float64, generator=generator)
            self.last_record = torch.from_numpy(rec)
            return reference_patch_sample(pool, rec, Ph, Pw, table, ctrl, spacing=aug.spacing if aug else 0, noise=noise, **kw)
        from . import ops, rng
        snap = rng.snapshot(pool.device) if snapshot is None else snapshot
        rec = ops.patch_draw(pool, Ph, Pw, B, snap, self.fg_slots, self.p_fg, self.class_mask, indices)
        table, ctrl = (self._identity, None) if aug is None else aug.draw(B, Ph, Pw, pool.device, snapshot=snap)
        self.last_record = rec
        noisy = aug is not None and aug.noise is not None
        return ops.patch_warp(pool, rec, Ph, Pw, table, ctrl, spacing=aug.spacing if aug else 0, snap=snap if noisy else None, **kw)


class PatchLoader:
    """``steps_per_epoch`` batches of a ``PatchSampler`` per epoch, already on the pool's device: the
    ``train_loader`` of ``train_model`` (whose ``.to(device)`` of a device tensor is a no-op)."""

    def __init__(self, sampler: PatchSampler, steps_per_epoch: int):
        self.sampler, self.steps = sampler, int(steps_per_epoch)
        if self.steps < 1:
            raise ValueError("PatchLoader: steps_per_epoch >= 1")

    def __len__(self):
        return self.steps

    def __iter__(self):
        for _ in range(self.steps):
            yield self.sampler.sample()
