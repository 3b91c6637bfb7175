"""Surface-distance metrics of label maps -- Hausdorff distance (HD), its 95th percentile (HD95),
average symmetric surface distance (ASSD) and surface Dice (NSD) -- and an exact Euclidean distance
transform.  The definitions are medpy's (``metric.binary.hd95`` is what the CSWin-UNet / TransUNet /
Swin-UNet tables report); the reference scores with Dice and IoU only (cswin:692-708).

For an image and a class, P and T are the predicted and the true mask, dP and dT their borders: the
mask pixels with at least one of the four edge neighbours outside the mask, everything beyond the
image counting as outside (``M ^ binary_erosion(M)``).  With pixel size ``spacing = (sy, sx)`` the
distance between pixels is sqrt(sy^2 dy^2 + sx^2 dx^2); d1 = for every pixel of dP the distance to the
nearest pixel of dT, d2 the same from dT to dP.  hd = max(max d1, max d2); hd95 = the q-th percentile
of the pooled d1 and d2 with numpy's linear interpolation; assd = (mean d1 + mean d2) / 2;
nsd = (#{d1 <= tau} + #{d2 <= tau}) / (|dP| + |dT|).  Where P or T is empty all four are NaN.

On the GPU the work runs in csrc/surface.hip (csu_surface_metrics / csu_edt): a column pass and a row
pass of an exact separable distance transform over the borders, fixed-order reductions and a radix
select for the percentile, with no host-device synchronisation.  ``reference_surface_metrics``
states the same definitions in plain torch ops (fp64, brute force) for any device.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np
import torch

MAX_CLASSES = 32                 # csu_surface_metrics: classes per call
MAX_DIM = 32767
WORKSPACE_BUDGET = 256 << 20     # bytes of workspace per kernel call: classes / images go in chunks
_PAIR_ELEMS = 1 << 22            # reference: coordinate differences per chunk
_COLS = ("hd", "hd95", "assd", "nsd")


# ---------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------
def _as_labels(t, name: str) -> torch.Tensor:
    """A label map as a (B, H, W) uint8 or int64 tensor (bool -> uint8, other integers -> int64)."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: a tensor or a numpy array")
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or min(t.shape) < 1:
        raise ValueError(f"{name}: a label map (H, W) or (B, H, W), got {tuple(t.shape)}")
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    elif t.dtype != torch.uint8:
        if t.is_floating_point() or t.is_complex():
            raise ValueError(f"{name}: an integer or bool label map, got {t.dtype}")
        t = t.to(torch.int64)
    return t


def _class_values(num_classes: int, include_background: bool) -> Tuple[bool, List[int]]:
    """(binary, label values): num_classes = 1 is the binary form (a pixel is in the mask where its
    value is > 0); otherwise classes 1 .. K - 1, or 0 .. K - 1 with the background."""
    K = int(num_classes)
    if K < 1:
        raise ValueError(f"num_classes must be >= 1 (got {num_classes!r})")
    if K == 1:
        return True, [1]
    return False, list(range(0 if include_background else 1, K))


def _check(spacing, tolerance, percentile):
    sy, sx = (float(v) for v in spacing)
    if not (0.0 < sy < math.inf and 0.0 < sx < math.inf):
        raise ValueError(f"spacing must be positive and finite (got {spacing!r})")
    tau, q = float(tolerance), float(percentile)
    if not tau >= 0.0:
        raise ValueError(f"tolerance must be >= 0 (got {tolerance!r})")
    if not 0.0 <= q <= 100.0:
        raise ValueError(f"percentile must be in [0, 100] (got {percentile!r})")
    return sy, sx, tau, q


def _pair(pred, target):
    p, t = _as_labels(pred, "pred"), _as_labels(target, "target")
    if p.shape != t.shape:
        raise ValueError(f"pred {tuple(p.shape)} and target {tuple(t.shape)} differ in shape")
    return p, t.to(p.device)


# ---------------------------------------------------------------------------------------------
# the definitions in plain torch ops (fp64)
# ---------------------------------------------------------------------------------------------
def _border(m: torch.Tensor) -> torch.Tensor:
    """The border of a bool (H, W) mask: its pixels with an edge neighbour outside it."""
    p = torch.nn.functional.pad(m, (1, 1, 1, 1))
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return m & ~inner


def _nearest(a: torch.Tensor, b: torch.Tensor, sy: float, sx: float) -> torch.Tensor:
    """For every pixel of ``a`` (n, 2 coordinates, fp64) the distance to the nearest of ``b`` (m >= 1):
    brute-force minima over explicit coordinate differences, in chunks."""
    n, m = a.shape[0], b.shape[0]
    out = torch.full((n,), math.inf, dtype=torch.float64, device=a.device)
    cb = max(1, min(m, 4096))
    ca = max(1, _PAIR_ELEMS // cb)
    sy2, sx2 = sy * sy, sx * sx
    for i in range(0, n, ca):
        ay, ax = a[i:i + ca, 0:1], a[i:i + ca, 1:2]
        best = out[i:i + ca]
        for j in range(0, m, cb):
            dy, dx = ay - b[j:j + cb, 0].unsqueeze(0), ax - b[j:j + cb, 1].unsqueeze(0)
            best = torch.minimum(best, (sy2 * (dy * dy) + sx2 * (dx * dx)).amin(1))
        out[i:i + ca] = best
    return out.sqrt()


def _percentile(v: torch.Tensor, q: float) -> torch.Tensor:
    """numpy.percentile(v, q) with linear interpolation (v fp64, at least one element)."""
    v = v.sort().values
    n = v.numel()
    h = (n - 1) * q / 100
    lo = int(math.floor(h))
    hi = min(lo + 1, n - 1)
    return v[lo] + (h - lo) * (v[hi] - v[lo])


def _masks(p: torch.Tensor, t: torch.Tensor, binary: bool, value: int):
    return (p > 0, t > 0) if binary else (p == value, t == value)


def reference_surface_metrics(pred, target, num_classes: int = 1, spacing: Sequence[float] = (1.0, 1.0),
                              tolerance: float = 1.0, percentile: float = 95.0,
                              include_background: bool = False) -> torch.Tensor:
    """fp64 (B, C, 6) = [hd, hd95, assd, nsd, |dP|, |dT|] per image and class in plain torch ops on the
    inputs' device (the CPU path of ``surface_metrics`` and the yardstick of the kernels' tests)."""
    p, t = _pair(pred, target)
    sy, sx, tau, q = _check(spacing, tolerance, percentile)
    binary, values = _class_values(num_classes, include_background)
    B = p.shape[0]
    out = torch.full((B, len(values), 6), math.nan, dtype=torch.float64, device=p.device)
    for b in range(B):
        for c, value in enumerate(values):
            mp, mt = _masks(p[b], t[b], binary, value)
            bp, bt = _border(mp).nonzero().double(), _border(mt).nonzero().double()
            out[b, c, 4], out[b, c, 5] = bp.shape[0], bt.shape[0]
            if bp.shape[0] == 0 or bt.shape[0] == 0:
                continue
            d1, d2 = _nearest(bp, bt, sy, sx), _nearest(bt, bp, sy, sx)
            out[b, c, 0] = torch.maximum(d1.max(), d2.max())
            out[b, c, 1] = _percentile(torch.cat([d1, d2]), q)
            out[b, c, 2] = (d1.mean() + d2.mean()) / 2
            out[b, c, 3] = ((d1 <= tau).sum() + (d2 <= tau).sum()).double() / (d1.numel() + d2.numel())
    return out


def reference_distance_transform_edt(mask, spacing: Sequence[float] = (1.0, 1.0)) -> torch.Tensor:
    """fp64 (B, H, W) (or (H, W)): for every non-zero pixel the distance to the nearest zero pixel, zero
    elsewhere, inf everywhere without a zero pixel -- brute force in plain torch ops."""
    m = torch.from_numpy(np.ascontiguousarray(mask)) if isinstance(mask, np.ndarray) else mask
    squeeze = m.dim() == 2
    m = (m.unsqueeze(0) if squeeze else m) != 0
    if m.dim() != 3 or min(m.shape) < 1:
        raise ValueError(f"mask: (H, W) or (B, H, W), got {tuple(mask.shape)}")
    sy, sx, _, _ = _check(spacing, 0.0, 0.0)
    out = torch.zeros(m.shape, dtype=torch.float64, device=m.device)
    for b in range(m.shape[0]):
        zeros = (~m[b]).nonzero().double()
        if zeros.shape[0] == 0:
            out[b] = math.inf
        elif zeros.shape[0] < m[b].numel():
            out[b][m[b]] = _nearest(m[b].nonzero().double(), zeros, sy, sx)
    return out[0] if squeeze else out


# ---------------------------------------------------------------------------------------------
# the kernels (csrc/surface.hip)
# ---------------------------------------------------------------------------------------------
def _dtype_code(t: torch.Tensor) -> int:
    return 0 if t.dtype == torch.uint8 else 1      # CSU_SURFACE_U8 / CSU_SURFACE_I64


def _device_metrics(p, t, binary, values, sy, sx, tau, q) -> torch.Tensor:
    from ._lib import lib, ptr, require_device, stream_ptr
    from .ledger import launch
    require_device(p, t)
    p, t = p.contiguous(), t.contiguous()
    B, H, W = p.shape
    C = len(values)
    if H > MAX_DIM or W > MAX_DIM:
        raise ValueError(f"surface_metrics: H, W <= {MAX_DIM} (got {H} x {W})")
    out = torch.empty(B, C, 6, dtype=torch.float64, device=p.device)
    L = lib()
    # (image, class) pairs per call from the workspace budget (12 H W bytes a pair): all classes of a
    # chunk of images, or one image's classes in chunks
    pairs = max(1, min(WORKSPACE_BUDGET // (12 * H * W), 65535 // 2))
    cc = min(C, pairs)
    bb = max(1, pairs // cc) if cc == C else 1
    ws = None
    for b0 in range(0, B, bb):
        nb = min(bb, B - b0)
        for c0 in range(0, C, cc):
            nc = min(cc, C - c0)
            need = L.csu_surface_workspace(nb, nc, H, W)
            if ws is None or ws.numel() < need:
                ws = torch.empty(need, dtype=torch.uint8, device=p.device)
            pb, tb, ob = p[b0:b0 + nb], t[b0:b0 + nb], out[b0:b0 + nb]
            launch("surface_metrics",
                   lambda: L.csu_surface_metrics(nb, nc, H, W, int(binary), values[c0], _dtype_code(pb), ptr(pb),
                                                 _dtype_code(tb), ptr(tb), sy, sx, tau, q, ptr(ws), ws.numel(), ptr(ob),
                                                 C, c0, stream_ptr(p.device)),
                   0, nb * nc * H * W * (3 * (pb.element_size() + tb.element_size()) + 16), prec="f32")
    return out


def surface_metrics(pred, target, num_classes: int = 1, spacing: Sequence[float] = (1.0, 1.0), tolerance: float = 1.0,
                    percentile: float = 95.0, include_background: bool = False) -> torch.Tensor:
    """fp64 (B, C, 6) = [hd, hd95, assd, nsd, |dP|, |dT|] per image and class, on the inputs' device.

    ``pred`` / ``target``: label maps (H, W) or (B, H, W), uint8 / int64 / bool (they may differ).
    ``num_classes`` = 1: the binary form, C = 1, a pixel is in the mask where its value is > 0.
    ``num_classes`` = K > 1: C = K - 1 (classes 1 .. K - 1), or K with ``include_background``; at most
    32 classes.  ``spacing`` = (sy, sx): the pixel size; ``tolerance``: tau of the surface Dice, in the
    units of ``spacing``; ``percentile``: q of hd95.  Where a mask is empty the four metrics are NaN and
    the border counts are still reported.  GPU tensors go through the kernels without a host-device
    synchronisation; anything else through ``reference_surface_metrics``."""
    p, t = _pair(pred, target)
    sy, sx, tau, q = _check(spacing, tolerance, percentile)
    binary, values = _class_values(num_classes, include_background)
    if len(values) > MAX_CLASSES:
        raise ValueError(f"surface_metrics: at most {MAX_CLASSES} classes per call (got {len(values)})")
    if not p.is_cuda:
        return reference_surface_metrics(p, t, num_classes, (sy, sx), tau, q, include_background)
    return _device_metrics(p, t, binary, values, sy, sx, tau, q)


def distance_transform_edt(mask, spacing: Sequence[float] = (1.0, 1.0)) -> torch.Tensor:
    """scipy.ndimage.distance_transform_edt(mask, sampling=spacing) as fp32, on the mask's device: for
    every non-zero pixel of ``mask`` ((H, W) or (B, H, W), any dtype) the distance to the nearest zero
    pixel, zero elsewhere; inf everywhere in an image without a zero pixel.  On the GPU: csu_edt."""
    m = torch.from_numpy(np.ascontiguousarray(mask)) if isinstance(mask, np.ndarray) else mask
    if not isinstance(m, torch.Tensor):
        raise TypeError("mask: a tensor or a numpy array")
    if not m.is_cuda:
        return reference_distance_transform_edt(m, spacing).float()
    from ._lib import lib, ptr, stream_ptr
    from .ledger import launch
    sy, sx, _, _ = _check(spacing, 0.0, 0.0)
    squeeze = m.dim() == 2
    m = m.unsqueeze(0) if squeeze else m
    if m.dim() != 3 or min(m.shape) < 1:
        raise ValueError(f"mask: (H, W) or (B, H, W), got {tuple(mask.shape)}")
    if m.dtype not in (torch.uint8, torch.int64):
        m = (m != 0).to(torch.uint8)
    m = m.contiguous()
    B, H, W = m.shape
    if H > MAX_DIM or W > MAX_DIM:
        raise ValueError(f"distance_transform_edt: H, W <= {MAX_DIM} (got {H} x {W})")
    out = torch.empty(B, H, W, dtype=torch.float32, device=m.device)
    L = lib()
    bb = max(1, min(WORKSPACE_BUDGET // (2 * H * W), 65535))
    ws = torch.empty(L.csu_edt_workspace(min(bb, B), H, W), dtype=torch.uint8, device=m.device)
    for b0 in range(0, B, bb):
        mb, ob = m[b0:b0 + bb], out[b0:b0 + bb]
        launch("edt", lambda: L.csu_edt(mb.shape[0], H, W, _dtype_code(mb), ptr(mb), sy, sx, ptr(ws), ws.numel(), ptr(ob),
                                        stream_ptr(m.device)),
               0, mb.numel() * (mb.element_size() + 12), prec="f32")
    return out[0] if squeeze else out


class SurfaceMetrics:
    """Accumulates ``surface_metrics`` over a data set.  ``update(pred, target)`` appends the (B, C, 6)
    rows on the device without a synchronisation; ``compute()`` returns a dict: "hd", "hd95", "assd",
    "nsd" -- the macro mean over the classes of the per-class mean over the images where both masks are
    non-empty (NaN when no such pair exists) --, "valid", the number of such (image, class) pairs, and
    "class_hd", "class_hd95", "class_assd", "class_nsd", the per-class means as lists (NaN for a class
    without a valid pair)."""

    def __init__(self, num_classes: int = 1, spacing: Sequence[float] = (1.0, 1.0), tolerance: float = 1.0,
                 percentile: float = 95.0, include_background: bool = False):
        self.num_classes, self.include_background = int(num_classes), bool(include_background)
        sy, sx, self.tolerance, self.percentile = _check(spacing, tolerance, percentile)
        self.spacing = (sy, sx)
        self.classes = _class_values(self.num_classes, self.include_background)[1]
        self.rows: List[torch.Tensor] = []

    def update(self, pred, target) -> torch.Tensor:
        r = surface_metrics(pred, target, self.num_classes, self.spacing, self.tolerance, self.percentile,
                            self.include_background)
        self.rows.append(r)
        return r

    def compute(self) -> dict:
        C = len(self.classes)
        nan = float("nan")
        if not self.rows:
            res = {k: nan for k in _COLS}
            res.update({f"class_{k}": [nan] * C for k in _COLS})
            res["valid"] = 0
            return res
        r = torch.cat([x.to(self.rows[0].device) for x in self.rows]).cpu()      # (N, C, 6): the one synchronisation
        ok = ~torch.isnan(r[:, :, 0])
        n = ok.sum(0)                                                            # valid images per class
        res = {"valid": int(n.sum())}
        for j, k in enumerate(_COLS):
            per = torch.where(ok, r[:, :, j], torch.zeros_like(r[:, :, j])).sum(0) / n      # 0 / 0 = NaN: no valid pair
            res[f"class_{k}"] = [float(v) for v in per]
            have = n > 0
            res[k] = float(per[have].mean()) if bool(have.any()) else nan
        return res
