"""Signed distance maps of label maps: the ``phi`` of the boundary loss (Kervadec et al., "Boundary loss for
highly unbalanced segmentation", 2019; ``csu.losses.BoundarySegLoss``).  The reference trains with BCE only.

For an image and a class c, M is the set of pixels whose label is c.  A pixel that holds ``ignore_index`` or
any other value belongs to no class: it is outside every M.  Beyond the image there is nothing, so the image
edge is no border (``csu.metrics``' surface metrics count it as one).  With pixel size ``spacing = (sy, sx)``
and d(x, y) = sqrt(sy^2 dy^2 + sx^2 dx^2):

    M empty or the whole image:   phi = 0 everywhere,
    x outside M:                  phi(x) =   min over y in M of d(x, y),
    x in M:                       phi(x) = -(min over y outside M of d(x, y) - min(sy, sx)),

negative inside the class, 0 on its inner border pixels (those with a neighbour outside along the finer
axis), positive outside.  With unit spacing this is the authors' ``one_hot2dist``:
``edt(neg) * neg - (edt(pos) - 1) * pos``.  ``clip`` clamps phi to [-clip, clip].

On the GPU the maps come from csu_signed_distance (csrc/surface.hip) without a host-device synchronisation, so
they can be made from freshly augmented labels inside a captured training step;
``reference_signed_distance_map`` states the definition in fp64 torch ops for any device.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from .metrics import WORKSPACE_BUDGET, _as_labels, _check, reference_distance_transform_edt

MAX_CLASSES = 32                 # csu_signed_distance: classes per call
MAX_DIM = 16383                  # the rows of two uint16 fields fill 64 KiB of LDS


def _arguments(labels, num_classes, spacing, clip, classes):
    t = _as_labels(labels, "labels")
    squeeze = getattr(labels, "ndim", 3) == 2      # tensors and numpy arrays alike
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes < 1:
        raise ValueError(f"signed_distance_map: num_classes must be an integer >= 1 (got {num_classes!r})")
    sy, sx, _, _ = _check(spacing, 0.0, 0.0)
    if clip is not None and not 0.0 < float(clip) < math.inf:
        raise ValueError(f"signed_distance_map: clip must be positive and finite, or None (got {clip!r})")
    if classes is None:
        c0, c1 = 0, num_classes
    else:
        c0, c1 = (int(v) for v in classes)
        if not 0 <= c0 < c1 <= num_classes:
            raise ValueError(f"signed_distance_map: classes = (first, end) within [0, {num_classes}] (got {classes!r})")
    return t, squeeze, sy, sx, None if clip is None else float(clip), c0, c1


def reference_signed_distance_map(labels, num_classes: int, spacing: Sequence[float] = (1.0, 1.0),
                                  clip: Optional[float] = None, classes=None) -> torch.Tensor:
    """fp64 (B, K, H, W) (or (K, H, W) for an (H, W) map): the definition above in plain torch ops, on
    ``reference_distance_transform_edt`` (brute force), on the labels' device.  ``classes`` = (first, end):
    only those classes' planes (K = end - first)."""
    t, squeeze, sy, sx, clip, c0, c1 = _arguments(labels, num_classes, spacing, clip, classes)
    B, H, W = t.shape
    out = torch.zeros(B, c1 - c0, H, W, dtype=torch.float64, device=t.device)
    step = min(sy, sx)
    for b in range(B):
        for c in range(c0, c1):
            pos = t[b] == c
            n = int(pos.sum())
            if n == 0 or n == H * W:
                continue
            outside = reference_distance_transform_edt(~pos, (sy, sx))     # at the pixels off the class: to the class
            inside = reference_distance_transform_edt(pos, (sy, sx))       # at the pixels on it: to its complement
            out[b, c - c0] = torch.where(pos, step - inside, outside)
    if clip is not None:
        out = out.clamp(-clip, clip)
    return out[0] if squeeze else out


def signed_distance_map(labels, num_classes: int, spacing: Sequence[float] = (1.0, 1.0), clip: Optional[float] = None,
                        classes=None) -> torch.Tensor:
    """fp32 (B, K, H, W) signed distance maps of the classes 0 .. K-1 of a label map (B, H, W) -- (K, H, W)
    for an (H, W) map --, on the labels' device; see the module's text for the definition.

    ``labels``: uint8 / int64 / bool / other integers (those are converted to int64).  ``spacing`` = (sy, sx).
    ``clip``: clamp to [-clip, clip] (the kernel's search then stops at that radius), None: no clamp.
    ``classes`` = (first, end): only those classes' planes.  GPU tensors go through csu_signed_distance in
    chunks of classes / images under ``csu.metrics.WORKSPACE_BUDGET`` with no host-device synchronisation
    (H, W <= 16383); the result does not depend on the chunking.  CPU tensors take the reference."""
    t, squeeze, sy, sx, clip, c0, c1 = _arguments(labels, num_classes, spacing, clip, classes)
    if not t.is_cuda:
        out = reference_signed_distance_map(t, num_classes, (sy, sx), clip, (c0, c1)).float()
        return out[0] if squeeze else out
    from . import ops
    t = t.contiguous()
    B, H, W = t.shape
    C = c1 - c0
    if H > MAX_DIM or W > MAX_DIM:
        raise ValueError(f"signed_distance_map: H, W <= {MAX_DIM} on the GPU (got {H} x {W})")
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=t.device)
    # (image, class) pairs per call from the workspace budget (4 H W bytes a pair): all classes of a chunk of
    # images, or one image's classes in chunks
    pairs = max(1, min(WORKSPACE_BUDGET // (4 * H * W), 65535 // 2))
    cc = min(C, pairs, MAX_CLASSES)
    bb = max(1, pairs // cc) if cc == C else 1
    ws = None
    for b0 in range(0, B, bb):
        for k0 in range(0, C, cc):
            ws = ops.signed_distance(t[b0:b0 + bb], c0 + k0, min(cc, C - k0), out[b0:b0 + bb], k0, (sy, sx), clip, ws)
    return out[0] if squeeze else out
