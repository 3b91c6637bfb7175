"""Connected components of label maps and the component rules of segmentation post-processing: keep
the largest component of a class, drop components below a size, fill enclosed holes.  This is the step
between a hard prediction (csu.infer) and its surface distances (csu.metrics): HD and HD95 are decided
by a single stray island that Dice never notices.  The reference has no counterpart.

Definitions.  Value 0 is background.  Two neighbouring pixels belong to one component iff they hold
the same value and are adjacent: ``connectivity`` 4 (edges) or 8 (edges and corners) for the non-zero
values, always 4-adjacency for value 0 (scipy.ndimage.binary_fill_holes' convention), so the
background components come out of the same labelling.  Components are numbered 1 .. N within an image
in raster order of their first pixels (for a binary map: scipy.ndimage.label).  ``postprocess_labels``
is three steps, each on the map the step before produced:

1. fill holes: a hole is a background component that does not touch the image border (of at most
   ``max_hole_size`` pixels, if given); it takes the value of the pixel left of its first pixel in
   raster order -- which exists and is not 0 -- unless that value is >= num_classes;
2. remove small: every component of class c with fewer than ``min_size[c]`` pixels becomes 0;
3. keep largest: of every flagged class only the component with the most pixels stays, ties going to
   the lowest component number.

Classes are the values 1 .. num_classes - 1 (num_classes = 1: the map is binarised as > 0 and the only
class is 1).  Larger values (an ignore value) form components like any other, are never holes and no
rule touches them.

On the GPU the work runs in csrc/components.hip (csu_ccl / csu_cc_filter): union-find by tiles in
LDS, seams in global memory, integer atomics only, with no host-device synchronisation.  The
``reference_*`` functions state the same definitions in numpy (a two-pass union-find over row runs)
for any device; they are the CPU path and the yardstick of the kernels' tests.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .metrics import MAX_DIM, WORKSPACE_BUDGET, _as_labels, _dtype_code

MAX_CLASSES = 32
MAX_IMAGES = 65535               # csu_ccl / csu_cc_filter: images per call
MAX_TILES = 1 << 23              # ... and B ceil(H / 64) ceil(W / 64)
TILE = 64


# ---------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------
def _connectivity(c) -> int:
    if c not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8 (got {c!r})")
    return int(c)


class _Rules:
    """The validated arguments of postprocess_labels: ``min`` maps a class to its smallest kept size,
    ``keep`` is the set of classes of which only the largest component stays."""

    def __init__(self, num_classes, keep_largest, min_size, fill_holes, max_hole_size, connectivity):
        K = int(num_classes)
        if not 1 <= K <= MAX_CLASSES:
            raise ValueError(f"num_classes must be in 1..{MAX_CLASSES} (got {num_classes!r})")
        self.K = K
        self.classes = [1] if K == 1 else list(range(1, K))
        if isinstance(keep_largest, (bool, np.bool_)):
            self.keep = set(self.classes) if keep_largest else set()
        else:
            self.keep = {int(c) for c in keep_largest}
            bad = sorted(self.keep - set(self.classes))
            if bad:
                raise ValueError(f"keep_largest: classes {bad} are not in {self.classes[0]}..{self.classes[-1]}")
        if isinstance(min_size, (int, np.integer)):
            sizes = {c: int(min_size) for c in self.classes}
        else:
            seq = [int(v) for v in min_size]
            if len(seq) != K:
                raise ValueError(f"min_size: an int or one entry per class ({K}), got {len(seq)}")
            if any(v < 0 for v in seq):
                raise ValueError(f"min_size must be >= 0 (got {seq})")
            sizes = {1: seq[0]} if K == 1 else {c: seq[c] for c in self.classes}
        if any(v < 0 for v in sizes.values()):
            raise ValueError(f"min_size must be >= 0 (got {min_size!r})")
        if any(v > 2 ** 31 - 1 for v in sizes.values()):
            raise ValueError("min_size must fit int32")
        self.min = sizes
        self.fill = bool(fill_holes)
        if max_hole_size is not None and not 0 <= int(max_hole_size) <= 2 ** 31 - 1:
            raise ValueError(f"max_hole_size must be None or in 0..2^31 - 1 (got {max_hole_size!r})")
        self.max_hole = None if max_hole_size is None else int(max_hole_size)
        self.conn = _connectivity(connectivity)

    def tables(self):
        """(min_size int32[K], keep bit mask) as csu_cc_filter takes them."""
        arr = (ctypes.c_int * self.K)()
        mask = 0
        if self.K == 1:
            arr[0] = self.min[1]
            mask = 1 if 1 in self.keep else 0
        else:
            for c in self.classes:
                arr[c] = self.min[c]
                if c in self.keep:
                    mask |= 1 << c
        return arr, mask


# ---------------------------------------------------------------------------------------------
# the definitions in numpy
# ---------------------------------------------------------------------------------------------
def _roots(a: np.ndarray, conn: int) -> np.ndarray:
    """int64 (H, W): for every pixel the raster index y W + x of its component's first pixel.  Two-pass
    union-find over the row runs (maximal row segments of one value); the smaller run index wins a union
    and runs are indexed in raster order, so a component's root run holds its first pixel."""
    H, W = a.shape
    change = np.ones((H, W), dtype=bool)
    change[:, 1:] = a[:, 1:] != a[:, :-1]
    rid = (np.cumsum(change.ravel()) - 1).reshape(H, W)
    first = np.flatnonzero(change.ravel())
    pa, pb = [], []
    if H > 1:
        lo, up = a[1:], a[:-1]
        m = lo == up
        pa.append(rid[1:][m]); pb.append(rid[:-1][m])
        if conn == 8 and W > 1:
            m = (lo[:, 1:] == up[:, :-1]) & (lo[:, 1:] != 0)          # up-left
            pa.append(rid[1:, 1:][m]); pb.append(rid[:-1, :-1][m])
            m = (lo[:, :-1] == up[:, 1:]) & (lo[:, :-1] != 0)         # up-right
            pa.append(rid[1:, :-1][m]); pb.append(rid[:-1, 1:][m])
    parent = list(range(first.size))
    if pa:
        edges = np.unique(np.stack([np.concatenate(pa), np.concatenate(pb)], 1), axis=0)
        for x, y in edges.tolist():
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            while parent[y] != y:
                parent[y] = parent[parent[y]]
                y = parent[y]
            if x < y:
                parent[y] = x
            elif y < x:
                parent[x] = y
        for i in range(len(parent)):        # ascending: parent[i] <= i is a root by now
            parent[i] = parent[parent[i]]
    return first[np.asarray(parent, dtype=np.int64)][rid]


def _label_image(a: np.ndarray, conn: int):
    """(comp int32, area int32, count, root int64, touches bool), each (H, W) but the count."""
    H, W = a.shape
    root = _roots(a, conn)
    flat = root.ravel()
    area = np.bincount(flat, minlength=H * W)[flat].reshape(H, W)
    edge = np.zeros((H, W), dtype=bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    touches = (np.bincount(flat[edge.ravel()], minlength=H * W)[flat] > 0).reshape(H, W)
    fg = a.ravel() != 0
    num = np.cumsum((flat == np.arange(H * W)) & fg)
    comp = np.where(fg, num[flat], 0).reshape(H, W)
    return comp.astype(np.int32), area.astype(np.int32), int(num[-1]), root, touches


def _to_numpy(x: torch.Tensor) -> np.ndarray:
    return x.detach().cpu().numpy().astype(np.int64)


def reference_connected_components(labels, connectivity: int = 8, return_areas: bool = False):
    """``connected_components`` in numpy (a two-pass union-find over row runs), for any device; the result
    is on the input's device."""
    conn = _connectivity(connectivity)
    squeeze = _ndim(labels) == 2
    x = _as_labels(labels, "labels")
    a = _to_numpy(x)
    comp, area, count = np.empty(a.shape, np.int32), np.empty(a.shape, np.int32), np.empty(a.shape[0], np.int32)
    for b in range(a.shape[0]):
        comp[b], area[b], count[b], _, _ = _label_image(a[b], conn)
    res = [torch.from_numpy(v).to(x.device) for v in ((comp, count, area) if return_areas else (comp, count))]
    if squeeze:
        res = [v[0] for v in res]
    return tuple(res)


def _postprocess_image(a: np.ndarray, ru: _Rules) -> np.ndarray:
    a = a.copy()
    if ru.fill:
        _, area, _, root, touches = _label_image(a, ru.conn)
        hole = (a == 0) & ~touches
        if ru.max_hole is not None:
            hole &= area <= ru.max_hole
        left = a.ravel()[np.maximum(root - 1, 0)]       # the value left of the component's first pixel
        hole &= left <= ru.classes[-1]
        a[hole] = left[hole]
    if any(v > 0 for v in ru.min.values()):
        _, area, _, _, _ = _label_image(a, ru.conn)
        for c in ru.classes:
            a[(a == c) & (area < ru.min[c])] = 0
    if ru.keep:
        comp, area, _, _, _ = _label_image(a, ru.conn)
        for c in sorted(ru.keep):
            m = a == c
            if not m.any():
                continue
            big = area[m].max()
            winner = comp[m & (area == big)].min()       # ties: the lowest component number
            a[m & (comp != winner)] = 0
    return a


def reference_postprocess_labels(labels, num_classes: int = 1, keep_largest=False, min_size=0, fill_holes: bool = False,
                                 max_hole_size: Optional[int] = None, connectivity: int = 8):
    """``postprocess_labels`` in numpy, each step on a fresh labelling of the map before it, for any
    device; the result is on the input's device, in its dtype and shape."""
    ru = _Rules(num_classes, keep_largest, min_size, fill_holes, max_hole_size, connectivity)
    return _postprocess(labels, ru, reference=True)


# ---------------------------------------------------------------------------------------------
# the kernels (csrc/components.hip)
# ---------------------------------------------------------------------------------------------
def _ndim(labels) -> int:
    return labels.ndim if isinstance(labels, np.ndarray) else labels.dim() if isinstance(labels, torch.Tensor) else -1


def _images_per_call(B: int, H: int, W: int, bytes_per_pixel: int) -> int:
    tiles = -(-H // TILE) * -(-W // TILE)
    return max(1, min(B, WORKSPACE_BUDGET // (bytes_per_pixel * H * W), MAX_IMAGES, MAX_TILES // tiles))


def _check_size(x: torch.Tensor, what: str):
    if x.shape[1] > MAX_DIM or x.shape[2] > MAX_DIM:
        raise ValueError(f"{what}: H, W <= {MAX_DIM} (got {x.shape[1]} x {x.shape[2]})")


def _device_ccl(x: torch.Tensor, conn: int, comp: bool = True, area: bool = False, count: bool = True):
    """(comp, count, area) of a (B, H, W) uint8 / int64 device tensor through csu_ccl; None for the
    outputs not asked for."""
    from ._lib import lib, ptr, require_device, stream_ptr
    from .ledger import launch
    require_device(x)
    _check_size(x, "connected_components")
    x = x.contiguous()
    B, H, W = x.shape
    oc = torch.empty(B, H, W, dtype=torch.int32, device=x.device) if comp else None
    oa = torch.empty(B, H, W, dtype=torch.int32, device=x.device) if area else None
    on = torch.empty(B, dtype=torch.int32, device=x.device) if count else None
    L = lib()
    bb = _images_per_call(B, H, W, 12)
    ws = torch.empty(L.csu_ccl_workspace(bb, H, W), dtype=torch.uint8, device=x.device)
    for b0 in range(0, B, bb):
        xb = x[b0:b0 + bb]
        cb, ab, nb = (None if o is None else o[b0:b0 + bb] for o in (oc, oa, on))
        launch("ccl", lambda: L.csu_ccl(xb.shape[0], H, W, _dtype_code(xb), ptr(xb), conn, ptr(ws), ws.numel(), ptr(cb),
                                        ptr(ab), ptr(nb), stream_ptr(x.device)),
               0, xb.numel() * (xb.element_size() + 4 * (int(comp) + int(area))), prec="f32")
    return oc, on, oa


def _device_postprocess(x: torch.Tensor, ru: _Rules, out: torch.Tensor = None) -> torch.Tensor:
    """csu_cc_filter on a (B, H, W) uint8 / int64 device tensor; ``out`` may be ``x`` itself."""
    from ._lib import lib, ptr, require_device, stream_ptr
    from .ledger import launch
    require_device(x, out)
    _check_size(x, "postprocess_labels")
    x = x.contiguous()
    B, H, W = x.shape
    if out is None:
        out = torch.empty(B, H, W, dtype=x.dtype, device=x.device)
    elif out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError("postprocess_labels: out must be contiguous, of the labels' shape and dtype")
    L = lib()
    sizes, mask = ru.tables()
    bb = _images_per_call(B, H, W, 8)
    ws = torch.empty(L.csu_cc_filter_workspace(bb, H, W), dtype=torch.uint8, device=x.device)
    hole = -1 if ru.max_hole is None else ru.max_hole
    for b0 in range(0, B, bb):
        xb, ob = x[b0:b0 + bb], out[b0:b0 + bb]
        launch("cc_filter", lambda: L.csu_cc_filter(xb.shape[0], H, W, _dtype_code(xb), ptr(xb), ru.conn, ru.K, sizes, mask,
                                                    int(ru.fill), hole, ptr(ws), ws.numel(), ptr(ob), stream_ptr(x.device)),
               0, 2 * xb.numel() * xb.element_size(), prec="f32")
    return out


def connected_components(labels, connectivity: int = 8, return_areas: bool = False):
    """(comp, count) -- or (comp, count, area) with ``return_areas`` -- of a label map, on its device.

    ``labels``: (H, W) or (B, H, W), uint8 / int64 / bool (other integer types are read as int64), a
    tensor or a numpy array.  ``comp`` int32, of the map's shape: 0 at the zero pixels, elsewhere the
    component's number 1 .. N within its image, in raster order of the components' first pixels (a binary
    map: ``scipy.ndimage.label``).  ``count`` int32 (B,) (a scalar tensor for an (H, W) map): N per image.
    ``area`` int32, of the map's shape: every pixel, the zero ones included, holds the pixel count of its
    component.  GPU tensors go through csu_ccl without a host-device synchronisation; anything else
    through ``reference_connected_components``."""
    conn = _connectivity(connectivity)
    squeeze = _ndim(labels) == 2
    x = _as_labels(labels, "labels")
    if not x.is_cuda:
        return reference_connected_components(x[0] if squeeze else x, conn, return_areas)
    comp, count, area = _device_ccl(x, conn, True, bool(return_areas), True)
    res = (comp, count, area) if return_areas else (comp, count)
    return tuple(v[0] for v in res) if squeeze else res


def _postprocess(labels, ru: _Rules, reference: bool):
    if isinstance(labels, np.ndarray):
        labels = torch.from_numpy(np.ascontiguousarray(labels))
    squeeze = _ndim(labels) == 2
    x = _as_labels(labels, "labels")
    dtype = labels.dtype
    if ru.K == 1:
        x = (x > 0).to(x.dtype)
    if reference or not x.is_cuda:
        a = _to_numpy(x)
        for b in range(a.shape[0]):
            a[b] = _postprocess_image(a[b], ru)
        out = torch.from_numpy(a).to(x.device)
    else:
        out = _device_postprocess(x, ru)
    if out.dtype != dtype:
        out = out.to(dtype)
    return out[0] if squeeze else out


def postprocess_labels(labels, num_classes: int = 1, keep_largest: Union[bool, Iterable[int]] = False,
                       min_size: Union[int, Sequence[int]] = 0, fill_holes: bool = False,
                       max_hole_size: Optional[int] = None, connectivity: int = 8) -> torch.Tensor:
    """The label map cleaned by its connected components, in the input's dtype and shape, on its device.

    ``labels``: (H, W) or (B, H, W), uint8 / int64 / bool / another integer type; a tensor or a numpy
    array.  ``num_classes`` = K: the classes are the values 1 .. K - 1 (at most 32); K = 1: the map is
    binarised as > 0 first.  The steps, in this order (see the module docstring): ``fill_holes`` (holes of
    at most ``max_hole_size`` pixels, if given), ``min_size`` (an int for every class, or K entries
    indexed by class, entry 0 unused; K = 1: one entry), ``keep_largest`` (True: every class; or an
    iterable of classes).  With every rule off the map comes back unchanged (binarised for K = 1).  GPU
    tensors go through csu_cc_filter without a host-device synchronisation; anything else through
    ``reference_postprocess_labels``."""
    ru = _Rules(num_classes, keep_largest, min_size, fill_holes, max_hole_size, connectivity)
    return _postprocess(labels, ru, reference=False)


class PostProcess:
    """The arguments of ``postprocess_labels`` as an object: ``PostProcess(num_classes=5, keep_largest=True)(labels)``.
    ``SlidingWindowPredictor(..., postprocess=...)`` and ``evaluate_full_res(..., postprocess=...)`` take one."""

    def __init__(self, num_classes: int = 1, keep_largest: Union[bool, Iterable[int]] = False,
                 min_size: Union[int, Sequence[int]] = 0, fill_holes: bool = False, max_hole_size: Optional[int] = None,
                 connectivity: int = 8):
        self.rules = _Rules(num_classes, keep_largest, min_size, fill_holes, max_hole_size, connectivity)

    def __call__(self, labels) -> torch.Tensor:
        return _postprocess(labels, self.rules, reference=False)

    def __repr__(self):
        r = self.rules
        return (f"PostProcess(num_classes={r.K}, keep_largest={sorted(r.keep)}, min_size={r.min}, fill_holes={r.fill}, "
                f"max_hole_size={r.max_hole}, connectivity={r.conn})")
