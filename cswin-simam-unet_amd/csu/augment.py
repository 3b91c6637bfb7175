"""Affine, elastic and intensity augmentation on the device for images, binary masks and label maps
(csrc/augment_warp.hip, ABI in include/csu.h): rotation by any angle, zoom, shift, flips, quarter turns and
a cubic B-spline deformation in one fused warp, then contrast / brightness / gamma / Gaussian noise on the
image.  Labels are sampled nearest-neighbour, so a label map stays a label map.  The reference has no
counterpart: its augmentation (flips, quarter turns, crop) stays ``csu.data.DeviceAugment``, bit for bit.

Parameters are drawn ON THE GPU from the Philox snapshot stream of ``csu.rng`` (new site ids
``rng.SITE_AUGMENT_*``): nothing syncs with the host, no host random state is involved, and draw + warp
can be captured in a HIP graph with ``rng.advance`` inside, every replay then drawing fresh parameters.

The parameter table is fp32 (B, TABLE_P); see include/csu.h for the layout (``T_*`` below) and the exact
definitions.  ``reference_augment`` states those definitions in plain torch indexing in fp64.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _lib

TABLE_P = 20
(T_HFLIP, T_VFLIP, T_ROT90, T_ANGLE, T_SCALE, T_TX, T_TY, T_CONTRAST, T_BRIGHTNESS, T_GAMMA, T_SIGMA,
 T_ELASTIC, T_A) = range(13)

__all__ = ["SpatialAugment", "reference_augment", "reference_source_coords", "reference_sample_at", "compose_affine", "identity_table",
           "make_table", "control_grid", "TABLE_P"]


def control_grid(H: int, W: int, spacing: int) -> Tuple[int, int]:
    """(Gy, Gx) = (ceil(H / spacing) + 3, ceil(W / spacing) + 3): the control points of an H x W image."""
    return -(-int(H) // int(spacing)) + 3, -(-int(W) // int(spacing)) + 3


def compose_affine(raw: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """fp64 (B, 6) inverse affine {a00, a01, a02, a10, a11, a12} of the raw draws ``raw[:, :7]`` (hflip, vflip,
    k, angle, scale, tx, ty): the content transform is T(t) C R(angle) S(scale) Q(k) F(h, v) C^-1 about
    c = ((W - 1) / 2, (H - 1) / 2), so A = C F Q(k)^T R(angle)^T / scale C^-1 T(-t)."""
    r = raw.double()
    ang, inv = r[:, T_ANGLE], 1.0 / r[:, T_SCALE]
    c, s = torch.cos(ang), torch.sin(ang)
    l00, l01, l10, l11 = c * inv, s * inv, -s * inv, c * inv
    k = r[:, T_ROT90].long()
    for i in range(1, 4):       # Q^T = [[0, 1], [-1, 0]] from the left, k times
        m = k >= i
        l00, l01, l10, l11 = (torch.where(m, l10, l00), torch.where(m, l11, l01), torch.where(m, -l00, l10),
                              torch.where(m, -l01, l11))
    fh = 1.0 - 2.0 * (r[:, T_HFLIP] != 0).double()
    fv = 1.0 - 2.0 * (r[:, T_VFLIP] != 0).double()
    l00, l01, l10, l11 = l00 * fh, l01 * fh, l10 * fv, l11 * fv
    cx, cy = 0.5 * (W - 1), 0.5 * (H - 1)
    px, py = cx + r[:, T_TX], cy + r[:, T_TY]
    return torch.stack([l00, l01, cx - (l00 * px + l01 * py), l10, l11, cy - (l10 * px + l11 * py)], 1)


def identity_table(B: int, device="cpu") -> torch.Tensor:
    """The table that changes nothing: output = image / 255, mask unchanged."""
    t = torch.zeros(B, TABLE_P, dtype=torch.float32, device=device)
    t[:, [T_SCALE, T_CONTRAST, T_BRIGHTNESS, T_GAMMA, T_A, T_A + 4]] = 1.0
    return t


def make_table(H: int, W: int, rows, device="cpu") -> torch.Tensor:
    """A table from explicit raw draws: ``rows`` is a list of dicts with any of hflip, vflip, k, angle (rad),
    scale, tx, ty, contrast, brightness, gamma, sigma, elastic; A is composed in fp64 and rounded to fp32."""
    names = {"hflip": T_HFLIP, "vflip": T_VFLIP, "k": T_ROT90, "angle": T_ANGLE, "scale": T_SCALE, "tx": T_TX, "ty": T_TY,
             "contrast": T_CONTRAST, "brightness": T_BRIGHTNESS, "gamma": T_GAMMA, "sigma": T_SIGMA, "elastic": T_ELASTIC}
    t = identity_table(len(rows))
    for b, row in enumerate(rows):
        for key, v in row.items():
            t[b, names[key]] = float(v)
    t[:, T_A:T_A + 6] = compose_affine(t, H, W).float()
    return t.to(device)


def _bspline(f: torch.Tensor) -> torch.Tensor:
    """(n, 4) uniform cubic B-spline basis at f in [0, 1)."""
    g = 1.0 - f
    return torch.stack([g * g * g / 6.0, (3.0 * f ** 3 - 6.0 * f ** 2 + 4.0) / 6.0,
                        (-3.0 * f ** 3 + 3.0 * f ** 2 + 3.0 * f + 1.0) / 6.0, f ** 3 / 6.0], 1)


def reference_source_coords(table: torch.Tensor, ctrl: Optional[torch.Tensor], spacing: int, H: int, W: int):
    """fp64 (B, H, W) source positions (sx, sy) of every output pixel, before the border rule: the pixel is
    displaced by the cubic B-spline of ``ctrl`` (rows of elastic magnitude 0, or ctrl None: not at all), then
    mapped through the row's fp32 A taken as given."""
    B, dev = table.shape[0], table.device
    t = table.double()
    px = torch.arange(W, dtype=torch.float64, device=dev).expand(B, H, W).clone()
    py = torch.arange(H, dtype=torch.float64, device=dev)[:, None].expand(B, H, W).clone()
    if ctrl is not None:
        spacing = int(spacing)
        ax, ay = torch.arange(W, device=dev), torch.arange(H, device=dev)
        ix, iy = ax // spacing, ay // spacing
        wx = _bspline((ax - ix * spacing).double() / spacing)
        wy = _bspline((ay - iy * spacing).double() / spacing)
        four = torch.arange(4, device=dev)
        cc = ctrl.double()[:, :, (iy[:, None] + four)][:, :, :, :, (ix[:, None] + four)]      # (B, 2, H, 4, W, 4)
        base = cc[:, :, :, 0, :, 0]                                   # relative to the first point: a constant field is exact
        d = base + torch.einsum("ha,wc,bnhawc->bnhw", wy, wx, cc - base[:, :, :, None, :, None])
        d = d * (t[:, T_ELASTIC] != 0).double()[:, None, None, None]
        px, py = px + d[:, 0], py + d[:, 1]
    a = t[:, T_A:T_A + 6, None, None]
    return a[:, 0] * px + a[:, 1] * py + a[:, 2], a[:, 3] * px + a[:, 4] * py + a[:, 5]


def _check_modes(who, border, mask_mode, out):
    if border not in ("constant", "replicate") or (mask_mode, out) not in (("bilinear", "binary"), ("nearest", "binary"),
                                                                          ("nearest", "labels")):
        raise ValueError(f"{who}: border constant / replicate; mask_mode bilinear / nearest; out binary, or "
                         "labels with nearest")


def reference_augment(images: torch.Tensor, masks: torch.Tensor, table: torch.Tensor, ctrl: Optional[torch.Tensor] = None,
                      *, spacing: int = 0, border: str = "constant", image_fill: float = 0.0, pad_label: int = 0,
                      mask_mode: str = "bilinear", out: str = "binary", noise: Optional[torch.Tensor] = None):
    """The definitions of csu_augment_warp in plain torch indexing, in fp64, on any device: uint8 images
    (B, H, W, 3) and masks (B, H, W) -> fp32 (B, 3, H, W) and fp32 (B, 1, H, W) or int64 (B, H, W) labels.
    ``noise``: standard normals (B, 3, H, W) scaled by the rows' sigma, or None for no noise (the kernel's
    own normals come from its Philox stream)."""
    _check_modes("reference_augment", border, mask_mode, out)
    B, H, W = images.shape[:3]
    sx, sy = reference_source_coords(table, ctrl, spacing, H, W)
    return reference_sample_at(images, masks, table, sx, sy, border=border, image_fill=image_fill, pad_label=pad_label,
                               mask_mode=mask_mode, out=out, noise=noise)


def reference_sample_at(images: torch.Tensor, masks: torch.Tensor, table: torch.Tensor, sx: torch.Tensor, sy: torch.Tensor,
                        *, border: str = "constant", image_fill: float = 0.0, pad_label: int = 0,
                        mask_mode: str = "bilinear", out: str = "binary", noise: Optional[torch.Tensor] = None,
                        mean: Optional[torch.Tensor] = None):
    """reference_augment from given source positions on: fp64 (B, h, w) ``sx``, ``sy`` in the pixel coordinates of
    the uint8 images (B, H, W, 3) / masks (B, H, W) -> the border rule, the bilinear / nearest samples and the
    table's intensity chain, as fp32 (B, 3, h, w) and the mask.  The output h x w need not be H x W (a patch of a
    larger image: csu.patches).  ``mean``: fp64 (B,) in [0, 1] for the contrast step (default: each image's own)."""
    _check_modes("reference_sample_at", border, mask_mode, out)
    B, H, W = images.shape[:3]
    h, w_ = sx.shape[1:]
    dev = images.device
    t = table.double()
    rep = border == "replicate"
    sx = sx.clamp(0, W - 1) if rep else sx.clamp(-2, W + 1)      # constant: a band where every tap is still outside
    sy = sy.clamp(0, H - 1) if rep else sy.clamp(-2, H + 1)
    x0, y0 = torch.floor(sx), torch.floor(sy)
    fx, fy = sx - x0, sy - y0
    x0, y0 = x0.long(), y0.long()
    bi = torch.arange(B, device=dev)[:, None, None].expand(B, h, w_)
    fill = float(torch.tensor(image_fill, dtype=torch.float32)) * 255.0
    acc, macc = torch.zeros(B, h, w_, 3, dtype=torch.float64, device=dev), torch.zeros(B, h, w_, dtype=torch.float64, device=dev)
    for i, wy in ((0, 1.0 - fy), (1, fy)):
        for j, wx in ((0, 1.0 - fx), (1, fx)):
            yy, xx = y0 + i, x0 + j
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W) if not rep else torch.ones_like(yy, dtype=torch.bool)
            yc, xc = yy.clamp(0, H - 1), xx.clamp(0, W - 1)
            w = wy * wx
            acc += w[..., None] * torch.where(inside[..., None], images[bi, yc, xc].double(), torch.full_like(acc, fill))
            macc += w * torch.where(inside, masks[bi, yc, xc].double(), torch.zeros_like(macc))
    v = acc.permute(0, 3, 1, 2) / 255.0

    def col(i):
        return t[:, i, None, None, None]
    mean = (images.double().mean(dim=(1, 2, 3)) / 255.0 if mean is None else mean.double())[:, None, None, None]
    contrast, bright, gamma, sigma = col(T_CONTRAST), col(T_BRIGHTNESS), col(T_GAMMA), col(T_SIGMA)
    v = torch.where(contrast != 1, (v - mean) * contrast + mean, v)     # a step at its identity value is skipped
    v = torch.where(bright != 1, v * bright, v)
    v = v.clamp(0, 1)
    v = torch.where(gamma != 1, v ** gamma, v)
    if noise is not None:
        v = torch.where(sigma > 0, (v + sigma * noise.double()).clamp(0, 1), v)
    oimg = v.float()
    if mask_mode == "bilinear":
        return oimg, (macc / 255.0).float()[:, None]
    nx, ny = torch.floor(sx + 0.5).long(), torch.floor(sy + 0.5).long()
    inside = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W) if not rep else torch.ones_like(nx, dtype=torch.bool)
    lab = torch.where(inside, masks[bi, ny.clamp(0, H - 1), nx.clamp(0, W - 1)].long(), torch.full_like(nx, int(pad_label)))
    if out == "labels":
        return oimg, lab
    return oimg, (lab.double() / 255.0).float()[:, None]


def _pair(v, name, positive=False):
    if v is None:
        return None
    lo, hi = (float(v[0]), float(v[1]))
    if hi < lo or (positive and lo <= 0):
        raise ValueError(f"SpatialAugment: {name}=(lo, hi) needs lo <= hi" + (" and lo > 0" if positive else ""))
    return lo, hi


class SpatialAugment:
    """Batch augmentation of uint8 images (B, H, W, 3) with uint8 masks or label maps (B, H, W).

    rotate=(lo, hi) degrees (positive turns the content clockwise on screen), scale=(lo, hi) (log-uniform
    zoom), translate=frac (shift uniform in +-frac of the width / height), flip_prob (each flip), rot90_prob
    (a quarter turn of 1, 2 or 3 steps), elastic=(spacing, magnitude_lo, magnitude_hi) in pixels,
    brightness / contrast / gamma=(lo, hi), noise=(sigma_lo, sigma_hi).  Each has its own probability
    ``p_*`` (default 0.5, translate 1.0); None / 0 turns a transform off.

    border "constant" (image taps outside read ``image_fill`` in [0, 1], labels ``pad_label``, e.g. an ignore
    index) or "replicate"; mask_mode "bilinear" (soft binary masks, the reference's convention) or
    "nearest"; out "binary" (fp32 (B, 1, H, W) = value / 255) or "labels" (int64 (B, H, W), what
    MultiClassSegLoss takes; needs mask_mode="nearest").

    ``draw`` returns (table, ctrl), ``apply`` warps with them, ``__call__`` does both.  On the GPU the draws
    come from the Philox snapshot (default: ``rng.snapshot(device)``), on CPU tensors from a
    ``torch.Generator`` and ``apply`` runs ``reference_augment``: the CPU and GPU streams differ, the
    distributions and the meaning of the table do not."""

    def __init__(self, rotate=None, p_rotate=0.5, scale=None, p_scale=0.5, translate=0.0, p_translate=1.0,
                 flip_prob=0.0, rot90_prob=0.0, elastic=None, p_elastic=0.5, brightness=None, p_brightness=0.5,
                 contrast=None, p_contrast=0.5, gamma=None, p_gamma=0.5, noise=None, p_noise=0.5,
                 border="constant", image_fill=0.0, pad_label=0, mask_mode="bilinear", out="binary"):
        self.rotate, self.scale = _pair(rotate, "rotate"), _pair(scale, "scale", positive=True)
        self.translate = float(translate)
        self.flip_prob, self.rot90_prob = float(flip_prob), float(rot90_prob)
        self.spacing, self.elastic = 0, None
        if elastic is not None:
            self.spacing, self.elastic = int(elastic[0]), _pair(elastic[1:], "elastic magnitude")
            if self.spacing < 4 or self.elastic[0] < 0:
                raise ValueError("SpatialAugment: elastic=(spacing >= 4, magnitude_lo >= 0, magnitude_hi)")
        self.brightness, self.contrast = _pair(brightness, "brightness"), _pair(contrast, "contrast")
        self.gamma, self.noise = _pair(gamma, "gamma", positive=True), _pair(noise, "noise")
        if self.noise is not None and self.noise[0] < 0:
            raise ValueError("SpatialAugment: noise sigma must be >= 0")
        self.p = {"rotate": p_rotate, "scale": p_scale, "translate": p_translate, "elastic": p_elastic,
                  "brightness": p_brightness, "contrast": p_contrast, "gamma": p_gamma, "noise": p_noise}
        for k, v in list(self.p.items()) + [("flip", self.flip_prob), ("rot90", self.rot90_prob)]:
            if not 0.0 <= float(v) <= 1.0:
                raise ValueError(f"SpatialAugment: probability of {k} outside [0, 1]")
        if border not in ("constant", "replicate") or mask_mode not in ("bilinear", "nearest") or out not in ("binary", "labels"):
            raise ValueError("SpatialAugment: border constant / replicate, mask_mode bilinear / nearest, out binary / labels")
        if out == "labels" and mask_mode != "nearest":
            raise ValueError("SpatialAugment: out='labels' needs mask_mode='nearest' (class indices cannot be interpolated)")
        if not 0.0 <= float(image_fill) <= 1.0:
            raise ValueError("SpatialAugment: image_fill in [0, 1]")
        self.border, self.image_fill, self.pad_label = border, float(image_fill), int(pad_label)
        self.mask_mode, self.out = mask_mode, out

    def config(self, H: int, W: int) -> "_lib.AugmentConfig":
        """The csu_augment_config of an H x W image (rotation in radians, shifts in pixels)."""
        c = _lib.AugmentConfig()
        c.p_hflip = c.p_vflip = self.flip_prob
        c.p_rot90 = self.rot90_prob

        def put(name, rng, identity, conv=float):
            on = rng is not None
            setattr(c, "p_" + name, float(self.p[name]) if on else 0.0)
            setattr(c, name + "_lo", conv(rng[0]) if on else identity)
            setattr(c, name + "_hi", conv(rng[1]) if on else identity)
        put("rotate", self.rotate, 0.0, math.radians)
        put("scale", self.scale, 1.0)
        put("contrast", self.contrast, 1.0)
        put("brightness", self.brightness, 1.0)
        put("gamma", self.gamma, 1.0)
        put("noise", self.noise, 0.0)
        put("elastic", self.elastic, 0.0)
        c.p_translate = float(self.p["translate"]) if self.translate > 0 else 0.0
        c.translate_x, c.translate_y = self.translate * W, self.translate * H
        c.spacing = self.spacing
        return c

    # -- draw ---------------------------------------------------------------------------------------
    def draw(self, B: int, H: int, W: int, device, snapshot: Optional[torch.Tensor] = None, generator=None):
        """(table fp32 (B, TABLE_P), ctrl fp32 (B, 2, Gy, Gx) or None when elastic is off)."""
        device = torch.device(device)
        if device.type == "cpu":
            return self._draw_cpu(B, H, W, generator)
        from . import ops, rng
        snap = rng.snapshot(device) if snapshot is None else snapshot
        return ops.augment_draw(self.config(H, W), B, H, W, snap, elastic=self.elastic is not None)

    def _draw_cpu(self, B, H, W, generator):
        c = self.config(H, W)
        u = torch.rand(B, 24, dtype=torch.float64, generator=generator)
        t = identity_table(B).double()

        def uni(j, lo, hi):
            return lo + u[:, j] * (hi - lo)
        t[:, T_HFLIP] = (u[:, 0] < c.p_hflip).double()
        t[:, T_VFLIP] = (u[:, 1] < c.p_vflip).double()
        t[:, T_ROT90] = torch.where(u[:, 2] < c.p_rot90, 1.0 + torch.floor(u[:, 3] * 3.0).clamp(max=2.0), t[:, T_ROT90])
        t[:, T_ANGLE] = torch.where(u[:, 4] < c.p_rotate, uni(5, c.rotate_lo, c.rotate_hi), t[:, T_ANGLE])
        if c.p_scale > 0:
            l0, l1 = math.log(c.scale_lo), math.log(c.scale_hi)
            t[:, T_SCALE] = torch.where(u[:, 6] < c.p_scale, torch.exp(uni(7, l0, l1)).clamp(c.scale_lo, c.scale_hi), t[:, T_SCALE])
        tr = u[:, 8] < c.p_translate
        t[:, T_TX] = torch.where(tr, uni(9, -c.translate_x, c.translate_x), t[:, T_TX])
        t[:, T_TY] = torch.where(tr, uni(10, -c.translate_y, c.translate_y), t[:, T_TY])
        for col, j, name in ((T_CONTRAST, 11, "contrast"), (T_BRIGHTNESS, 13, "brightness"), (T_GAMMA, 15, "gamma"),
                             (T_SIGMA, 17, "noise"), (T_ELASTIC, 19, "elastic")):
            lo, hi = getattr(c, name + "_lo"), getattr(c, name + "_hi")
            t[:, col] = torch.where(u[:, j] < getattr(c, "p_" + name), uni(j + 1, lo, hi), t[:, col])
        t = t.float()
        t[:, T_A:T_A + 6] = compose_affine(t, H, W).float()
        ctrl = None
        if self.elastic is not None:
            g = torch.rand((B, 2) + control_grid(H, W, self.spacing), dtype=torch.float64, generator=generator)
            ctrl = ((2.0 * g - 1.0) * t[:, T_ELASTIC].double()[:, None, None, None]).float()
        return t, ctrl

    # -- apply --------------------------------------------------------------------------------------
    def apply(self, images: torch.Tensor, masks: torch.Tensor, table: torch.Tensor, ctrl: Optional[torch.Tensor] = None,
              mask_mode: Optional[str] = None, out: Optional[str] = None, snapshot: Optional[torch.Tensor] = None,
              generator=None):
        """(images fp32 (B, 3, H, W), masks) of the table and control field; ``mask_mode`` / ``out`` override the
        constructor's.  GPU: one csu_augment_warp launch (noise from ``snapshot``, default ``rng.snapshot``);
        CPU: ``reference_augment`` with normals from ``generator``."""
        mask_mode = self.mask_mode if mask_mode is None else mask_mode
        out = self.out if out is None else out
        kw = dict(spacing=self.spacing, border=self.border, image_fill=self.image_fill, pad_label=self.pad_label,
                  mask_mode=mask_mode, out=out)
        if not images.is_cuda:
            noise = None
            if bool((table[:, T_SIGMA] > 0).any()):
                B, H, W = images.shape[:3]
                noise = torch.randn(B, 3, H, W, dtype=torch.float64, generator=generator)
            return reference_augment(images, masks, table, ctrl, noise=noise, **kw)
        from . import ops, rng
        snap = snapshot
        if snap is None and self.noise is not None:
            snap = rng.snapshot(images.device)
        return ops.augment_warp(images, masks, table, ctrl, snap=snap, **kw)

    def __call__(self, images: torch.Tensor, masks: torch.Tensor, mask_mode: Optional[str] = None,
                 out: Optional[str] = None, generator=None):
        B, H, W = images.shape[:3]
        snap = None
        if images.is_cuda:
            from . import rng
            snap = rng.snapshot(images.device)        # one snapshot for the table, the field and the noise
        table, ctrl = self.draw(B, H, W, images.device, snapshot=snap, generator=generator)
        return self.apply(images, masks, table, ctrl, mask_mode=mask_mode, out=out, snapshot=snap, generator=generator)
