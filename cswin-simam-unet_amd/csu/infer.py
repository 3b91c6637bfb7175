"""Whole-image inference: sliding-window prediction of images of any size with a network of fixed
S x S input, with test-time augmentation (the reference has no prediction path beyond
evaluate_model, cswin:712-747).

The image is covered by S x S tiles (plan_axis: a regular stride, the last tile pulled back to the
edge); every tile is shown to the network in each TTA variant, the outputs are turned into
probabilities, mapped back, weighted by a separable window and accumulated; the sum is divided by
the (separable) sum of the weights.  On the GPU the tile traffic runs in three csu kernels
(csrc/tile.hip: csu_tile_gather / csu_tile_blend / csu_tile_finish) around a captured batch forward;
``reference_predict`` states the same arithmetic in plain torch ops (fp64) for any device.
"""
from __future__ import annotations

from typing import Iterable, List, Tuple

import numpy as np
import torch

# name -> (hflip, vflip, clockwise quarter turns after the flips): the eight symmetries of the square,
# in the parameters of csu.data.AugmentationTransform / csu_augment_batch
TTA_VARIANTS = {
    "identity": (0, 0, 0), "hflip": (1, 0, 0), "vflip": (0, 1, 0), "rot90": (0, 0, 1), "rot180": (0, 0, 2),
    "rot270": (0, 0, 3), "transpose": (1, 0, 3), "antitranspose": (1, 0, 1),
}
D4 = tuple(TTA_VARIANTS)
MAX_SLOTS = 128         # csu_tile_blend: slots per launch
MAX_CLASSES = 32
_OWN = object()         # predict(postprocess=...): the predictor's own setting


def parse_tta(tta) -> List[Tuple[int, int, int]]:
    """``tta`` as a list of (hflip, vflip, rot) triples: "d4" (all eight), a name, or a sequence of
    names and / or explicit triples."""
    if isinstance(tta, str):
        tta = D4 if tta == "d4" else (tta,)
    out = []
    for v in tta:
        if isinstance(v, str):
            if v not in TTA_VARIANTS:
                raise ValueError(f"tta: unknown variant {v!r} (one of {', '.join(D4)}, or 'd4')")
            out.append(TTA_VARIANTS[v])
        else:
            h, f, r = (int(c) for c in v)
            if h not in (0, 1) or f not in (0, 1) or not 0 <= r <= 3:
                raise ValueError(f"tta: (hflip, vflip, rot) with flips 0/1 and rot 0..3 (got {tuple(v)!r})")
            out.append((h, f, r))
    if not out:
        raise ValueError("tta: at least one variant")
    return out


def plan_axis(L: int, S: int, overlap: float) -> List[int]:
    """Tile positions along an axis of length L for tiles of S: [0] when L <= S; otherwise a stride of
    max(1, S - round(S * overlap)), ceil((L - S) / stride) + 1 tiles at min(i * stride, L - S) -- the
    last tile is pulled back to the edge, so nothing is padded."""
    L, S = int(L), int(S)
    if L < 1 or S < 1:
        raise ValueError("plan_axis: L and S must be >= 1")
    if not 0.0 <= overlap < 1.0:
        raise ValueError("plan_axis: 0 <= overlap < 1")
    if L <= S:
        return [0]
    stride = max(1, S - int(round(S * overlap)))
    n = -(-(L - S) // stride) + 1
    return [min(i * stride, L - S) for i in range(n)]


def plan_tiles(H: int, W: int, S: int, overlap: float = 0.5, tta=("identity",)) -> np.ndarray:
    """The ordered tile table, int32 (N, 6): y0, x0, hflip, vflip, rot, active (= 1).  Row-major over
    the tiles, the TTA variants innermost."""
    var = parse_tta(tta)
    rows = [(y, x, h, v, r, 1) for y in plan_axis(H, S, overlap) for x in plan_axis(W, S, overlap) for (h, v, r) in var]
    return np.asarray(rows, dtype=np.int32).reshape(-1, 6)


def window_1d(S: int, kind: str = "gaussian") -> np.ndarray:
    """The 1-D blending window (fp64, length S); a tile pixel weighs w[ty] * w[tx].  "uniform": ones;
    "gaussian": exp(-0.5 ((i - (S - 1) / 2) / (0.125 S))^2), strictly positive."""
    if kind == "uniform":
        return np.ones(S, dtype=np.float64)
    if kind == "gaussian":
        i = np.arange(S, dtype=np.float64)
        return np.exp(-0.5 * ((i - (S - 1) / 2.0) / (0.125 * S)) ** 2)
    raise ValueError(f"window {kind!r} ('uniform' or 'gaussian')")


def axis_weight(L: int, S: int, overlap: float, w1: np.ndarray) -> np.ndarray:
    """Sum of the window over an axis' tiles (fp64, length L).  The 2-D weight sum of a plan is
    outer(axis_weight(H), axis_weight(W)) * n_tta: the window is a product and the plan a grid."""
    r = np.zeros(L, dtype=np.float64)
    for p in plan_axis(L, S, overlap):
        n = min(S, L - p)
        r[p:p + n] += np.asarray(w1, dtype=np.float64)[:n]
    return r


def _as_image(image, device=None):
    """(tensor, kind): uint8 (H, W, 3) -> kind 0, fp32 (3, H, W) -> kind 1; contiguous, on ``device``."""
    t = torch.from_numpy(np.ascontiguousarray(image)) if isinstance(image, np.ndarray) else image
    if not isinstance(t, torch.Tensor):
        raise TypeError("image: a numpy array or a tensor")
    if t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3:
        kind = 0
    elif t.dtype == torch.float32 and t.dim() == 3 and t.shape[0] == 3:
        kind = 1
    else:
        raise ValueError(f"image: uint8 (H, W, 3) or float32 (3, H, W), got {t.dtype} {tuple(t.shape)}")
    if device is not None:
        t = t.to(device, non_blocking=True)
    return t.contiguous(), kind


def _output_kind(model, output):
    """'prob' or 'logits': what the module's forward returns."""
    if output is not None:
        if output not in ("prob", "logits"):
            raise ValueError(f"output {output!r} ('prob' or 'logits')")
        return output
    if hasattr(model, "set_head"):          # CSWinTransformer, UNet
        return "logits" if getattr(model, "_head", "sigmoid") == "logits" else "prob"
    return "logits"


# ---------------------------------------------------------------------------------------------
# the same arithmetic in plain torch ops
# ---------------------------------------------------------------------------------------------
def _forward_view(t, h, v, r):
    """rot(vflip(hflip(t))) on the last two dims, rot = clockwise quarter turns."""
    if h:
        t = torch.flip(t, (-1,))
    if v:
        t = torch.flip(t, (-2,))
    return torch.rot90(t, -r, (-2, -1)) if r else t


def _backward_view(t, h, v, r):
    """The inverse of _forward_view."""
    if r:
        t = torch.rot90(t, r, (-2, -1))
    if v:
        t = torch.flip(t, (-2,))
    if h:
        t = torch.flip(t, (-1,))
    return t


def _to_prob(out, kind, dtype):
    out = out.to(dtype)
    if out.dim() != 4:
        raise ValueError(f"model output must be (B, K, S, S), got {tuple(out.shape)}")
    if kind == "prob":
        return out
    return torch.sigmoid(out) if out.shape[1] == 1 else torch.softmax(out, 1)


def reference_predict(fn, image, tile: int, overlap: float = 0.5, window: str = "gaussian", tta=("identity",),
                      batch_size: int = 16, output: str = "logits", return_prob: bool = False, dtype=torch.float64):
    """Sliding-window prediction in plain torch ops on the image's device (the CPU path, and the
    yardstick of the kernels' tests).  ``fn`` maps an fp32 (B, 3, S, S) batch to (B, K, S, S) outputs,
    ``output`` says what they are: 'prob' (K = 1 probabilities) or 'logits' (sigmoid for K = 1, softmax
    otherwise).  Accumulation in ``dtype`` (fp64).  Returns uint8 labels (H, W) and, with
    ``return_prob``, probabilities (K, H, W) in ``dtype``."""
    img, kind = _as_image(image)
    S = int(tile)
    if kind == 0:      # value / 255 as an IEEE division on any device (a device's scalar division may multiply by 1 / 255)
        lut = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(img.device)
        chw = lut[img.long()].permute(2, 0, 1)
    else:
        chw = img
    H, W = chw.shape[1], chw.shape[2]
    dev = chw.device
    var = parse_tta(tta)
    w1 = window_1d(S, window)
    w2 = torch.from_numpy(np.outer(w1, w1)).to(dev, dtype)
    table = plan_tiles(H, W, S, overlap, var)
    ar = torch.arange(S, device=dev)
    canvas = None
    for i in range(0, len(table), int(batch_size)):
        recs = table[i:i + int(batch_size)]
        xs = []
        for y0, x0, h, v, r, _ in recs.tolist():
            crop = chw[:, (y0 + ar).clamp(max=H - 1)][:, :, (x0 + ar).clamp(max=W - 1)]   # replicate past the edge
            xs.append(_forward_view(crop, h, v, r))
        with torch.no_grad():
            p = _to_prob(fn(torch.stack(xs).contiguous()), output, dtype)
        if canvas is None:
            canvas = torch.zeros(p.shape[1], H, W, dtype=dtype, device=dev)
        for j, (y0, x0, h, v, r, _) in enumerate(recs.tolist()):
            hh, ww = min(S, H - y0), min(S, W - x0)
            canvas[:, y0:y0 + hh, x0:x0 + ww] += (_backward_view(p[j], h, v, r) * w2)[:, :hh, :ww]
    ry, rx = axis_weight(H, S, overlap, w1), axis_weight(W, S, overlap, w1)
    den = torch.from_numpy(np.outer(ry, rx) * len(var)).to(dev, dtype)
    prob = canvas / den
    labels = (prob[0] > 0.5).to(torch.uint8) if prob.shape[0] == 1 else prob.argmax(0).to(torch.uint8)
    return (labels, prob) if return_prob else labels


# ---------------------------------------------------------------------------------------------
# the kernels (csrc/tile.hip)
# ---------------------------------------------------------------------------------------------
def tile_gather(image: torch.Tensor, table: torch.Tensor, S: int, out: torch.Tensor = None) -> torch.Tensor:
    """csu_tile_gather: the fp32 (B, 3, S, S) network input of the B slots of ``table`` (int32 (B, 6) on
    the device) from a device image, uint8 (H, W, 3) or fp32 (3, H, W)."""
    from ._lib import lib, ptr, require_device, stream_ptr
    from .ledger import launch
    require_device(image, table, out)
    image, kind = _as_image(image)
    H, W = (image.shape[0], image.shape[1]) if kind == 0 else (image.shape[1], image.shape[2])
    B = _check_table(table)
    if out is None:
        out = torch.empty(B, 3, S, S, dtype=torch.float32, device=image.device)
    elif tuple(out.shape) != (B, 3, S, S) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("tile_gather: out must be contiguous fp32 (B, 3, S, S)")
    launch("tile_gather", lambda: lib().csu_tile_gather(B, S, H, W, kind, ptr(image), ptr(table), ptr(out),
                                                        stream_ptr(image.device)),
           0, B * S * S * 3 * (4 + image.element_size()), prec="f32")
    return out


def _check_table(table: torch.Tensor) -> int:
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 6 or not table.is_contiguous() or table.shape[0] < 1:
        raise ValueError("tile table: contiguous int32 (B, 6) with B >= 1")
    return table.shape[0]


def tile_region(recs: np.ndarray, S: int, H: int, W: int):
    """(y0, x0, y1, x1): the bounding box, inside the canvas, of the active records' tiles (host table)."""
    on = recs[recs[:, 5] != 0]
    if len(on) == 0:
        raise ValueError("tile_region: no active record")
    return (max(int(on[:, 0].min()), 0), max(int(on[:, 1].min()), 0),
            min(int(on[:, 0].max()) + S, H), min(int(on[:, 1].max()) + S, W))


def tile_blend(out: torch.Tensor, table: torch.Tensor, w1: torch.Tensor, canvas: torch.Tensor, form: str = "logits",
               region=None):
    """csu_tile_blend: accumulate the (B, K, S, S) outputs of the B slots of ``table`` into the fp32
    (K, H, W) ``canvas`` in table order (in place).  ``form``: 'prob' (fp32, K = 1) or 'logits' (fp32 or
    bf16, read in place in the layouts csu.ops.seg_ce reads).  ``region`` (y0, x0, y1, x1): the part of the
    canvas to launch over, which must hold every active slot's tile (tile_region; None: all of it)."""
    from . import ops
    from ._lib import dtype_code, lib, ptr, require_device, stream_ptr
    from .ledger import launch
    require_device(out, table, w1, canvas)
    B = _check_table(table)
    if out.dim() != 4 or out.shape[0] != B or out.shape[2] != out.shape[3]:
        raise ValueError(f"tile_blend: outputs (B, K, S, S) for the table's {B} slots, got {tuple(out.shape)}")
    K, S = out.shape[1], out.shape[2]
    if canvas.dtype != torch.float32 or canvas.dim() != 3 or canvas.shape[0] != K or not canvas.is_contiguous():
        raise ValueError("tile_blend: canvas must be contiguous fp32 (K, H, W)")
    if w1.dtype != torch.float32 or tuple(w1.shape) != (S,) or not w1.is_contiguous():
        raise ValueError("tile_blend: w1 must be fp32 (S,)")
    if form not in ("prob", "logits"):
        raise ValueError(f"form {form!r}")
    if form == "prob":
        out = out.float()
    z, sb, sk, sp, _, pad_ok = ops._seg_ce_layout(out)
    if K == 1:       # one class: no bucket beyond the element itself is read
        pad_ok = False
    H, W = canvas.shape[1], canvas.shape[2]
    ry0, rx0, ry1, rx1 = (0, 0, H, W) if region is None else (int(v) for v in region)
    nbytes = B * K * S * S * (z.element_size() + 8)
    launch("tile_blend", lambda: lib().csu_tile_blend(B, S, H, W, K, 0 if form == "prob" else 1, dtype_code(z), ptr(z), sb,
                                                      sk, sp, int(pad_ok), ptr(table), ptr(w1), ptr(canvas), ry0, rx0, ry1,
                                                      rx1, stream_ptr(canvas.device)),
           0, nbytes, idem=False, prec="f32")
    return canvas


def tile_finish(canvas: torch.Tensor, ry: torch.Tensor, rx: torch.Tensor, n_tta: int, return_prob: bool = False,
                return_labels: bool = True):
    """csu_tile_finish: (labels uint8 (H, W) or None, prob fp32 (K, H, W) or None) = canvas / (ry[y] rx[x]
    n_tta) and its hard decision."""
    from ._lib import lib, ptr, require_device, stream_ptr
    from .ledger import launch
    require_device(canvas, ry, rx)
    K, H, W = canvas.shape
    if canvas.dtype != torch.float32 or not canvas.is_contiguous():
        raise ValueError("tile_finish: canvas must be contiguous fp32 (K, H, W)")
    for v, n in ((ry, H), (rx, W)):
        if v.dtype != torch.float32 or tuple(v.shape) != (n,) or not v.is_contiguous():
            raise ValueError("tile_finish: ry (H,) and rx (W,) fp32")
    prob = torch.empty(K, H, W, dtype=torch.float32, device=canvas.device) if return_prob else None
    labels = torch.empty(H, W, dtype=torch.uint8, device=canvas.device) if return_labels else None
    launch("tile_finish", lambda: lib().csu_tile_finish(K, H, W, ptr(canvas), ptr(ry), ptr(rx), float(n_tta), ptr(prob),
                                                        ptr(labels), stream_ptr(canvas.device)),
           0, H * W * (4 * K * (2 if return_prob else 1) + 1), prec="f32")
    return labels, prob


class _GraphedForward:
    """The eval-mode batch forward captured once for a static (B, 3, S, S) input and replayed (as
    csu.train._GraphedEval captures evaluate_model's body).  The gather writes ``x`` in place and the
    blend reads ``out`` in place, all on one stream."""

    def __init__(self, model, B, S, amp_dtype, device):
        from .train import _capture_mode, _gc_paused
        self.model, self.dtype = model, amp_dtype
        self.x = torch.zeros(B, 3, S, S, dtype=torch.float32, device=device)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            self._body()                 # warm-up: lazily built caches / kernels outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        mode = _capture_mode()
        self.graph = torch.cuda.CUDAGraph()
        with _gc_paused(), torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode=mode):
            self.out = self._body()

    def _body(self):
        with torch.autocast("cuda", dtype=self.dtype or torch.float32, enabled=self.dtype is not None):
            return self.model(self.x)

    def __call__(self):
        from .train import sync_shadows
        sync_shadows(self.model)     # the captured forward reads the optimizer-written weight shadows
        self.graph.replay()
        return self.out


class SlidingWindowPredictor:
    """Predict images of any size with a network of fixed ``tile`` x ``tile`` input.

    ``model``: CSWinTransformer (sigmoid head: fp32 probabilities; ``set_head("logits")``: any
    num_classes up to 32), UNet, or any module returning (B, K, tile, tile) -- logits unless
    ``output="prob"`` says K = 1 probabilities.  ``tile`` defaults to ``model.img_size``; ``overlap`` is
    the fraction of a tile shared with its neighbour; ``window`` "gaussian" or "uniform"; ``tta`` a
    sequence of variant names / (hflip, vflip, rot) triples, or "d4"; ``batch_size`` tiles per forward
    (at most 128); ``amp_dtype``: run the forward under autocast; ``graph`` (None = automatic for the csu
    models on a GPU): capture the batch forward once per (batch, dtype) and replay it.  ``postprocess``
    (None: off): a csu.components.PostProcess, or any callable on a label map; ``predict`` then returns
    the cleaned labels (the probabilities of ``return_prob`` are untouched).

    ``predict`` uploads the image and the whole tile table once, then launches gather -> forward ->
    blend per batch and one finish, with no host-device synchronisation in between.  The result is
    deterministic: the canvas does not depend on ``batch_size`` (csu_tile_blend keeps table order)."""

    def __init__(self, model, tile: int = None, overlap: float = 0.5, window: str = "gaussian", tta=("identity",),
                 batch_size: int = 16, amp_dtype=None, graph=None, output: str = None, postprocess=None):
        self.model = model
        self.postprocess = postprocess
        S = tile if tile is not None else getattr(model, "img_size", None)
        if S is None:
            raise ValueError("SlidingWindowPredictor: tile is required (the model has no img_size)")
        self.tile = int(S)
        plan_axis(self.tile + 1, self.tile, overlap)     # validates tile and overlap
        self.overlap, self.window = float(overlap), window
        self.variants = parse_tta(tta)
        if not 1 <= int(batch_size) <= MAX_SLOTS:
            raise ValueError(f"SlidingWindowPredictor: 1 <= batch_size <= {MAX_SLOTS}")
        self.batch_size, self.amp_dtype, self.graph, self.output = int(batch_size), amp_dtype, graph, output
        self.w1 = window_1d(self.tile, window)
        self._w1_dev = None

    def _device(self):
        p = next(self.model.parameters(), None)
        return p.device if p is not None else torch.device("cpu")

    def _use_graph(self, dev) -> bool:
        if self.graph is False or dev.type != "cuda" or torch.cuda.is_current_stream_capturing():
            return False
        if isinstance(self.model, torch.nn.parallel.DistributedDataParallel):
            return False
        return True if self.graph else hasattr(self.model, "set_head")

    def _forward(self, x):
        with torch.autocast(x.device.type, dtype=self.amp_dtype or torch.float32, enabled=self.amp_dtype is not None):
            return self.model(x)

    def predict(self, image, return_prob: bool = False, postprocess=_OWN):
        """uint8 labels (H, W) -- and fp32 probabilities (K, H, W) with ``return_prob`` -- on the model's
        device, for a uint8 (H, W, 3) (numpy or tensor) or fp32 (3, H, W) image.  ``postprocess``: applied to
        the labels instead of the predictor's own setting for this call (None: nothing is)."""
        post = self.postprocess if postprocess is _OWN else postprocess
        res = self._predict(image, return_prob)
        if post is None:
            return res
        return (post(res[0]), res[1]) if return_prob else post(res)

    def _predict(self, image, return_prob: bool):
        self.model.eval()
        dev = self._device()
        kind = _output_kind(self.model, self.output)
        if dev.type != "cuda":       # the kernels have no CPU path: the same arithmetic in torch ops
            img, _ = _as_image(image, dev)
            res = reference_predict(self._forward, img, self.tile, self.overlap, self.window, self.variants, self.batch_size,
                                    kind, True)
            return (res[0], res[1].float()) if return_prob else res[0]
        from .train import _graph_cache
        img, src = _as_image(image, dev)
        H, W = (img.shape[0], img.shape[1]) if src == 0 else (img.shape[1], img.shape[2])
        S = self.tile
        table = plan_tiles(H, W, S, self.overlap, self.variants)
        B = min(self.batch_size, len(table))
        nb = -(-len(table) // B)
        pad = np.zeros((nb * B, 6), dtype=np.int32)       # active = 0: the ragged last batch's padding
        pad[:len(table)] = table
        tab = torch.from_numpy(pad).to(dev, non_blocking=True)
        regions = [tile_region(pad[i * B:(i + 1) * B], S, H, W) for i in range(nb)]
        ry = torch.from_numpy(axis_weight(H, S, self.overlap, self.w1).astype(np.float32)).to(dev, non_blocking=True)
        rx = torch.from_numpy(axis_weight(W, S, self.overlap, self.w1).astype(np.float32)).to(dev, non_blocking=True)
        if self._w1_dev is None or self._w1_dev.device != dev:
            self._w1_dev = torch.from_numpy(self.w1.astype(np.float32)).to(dev)
        g = None
        if self._use_graph(dev):
            cache = _graph_cache(self.model)
            key = ("infer", B, S, self.amp_dtype, kind)
            g = cache.get(key)
            if g is None:
                g = cache[key] = _GraphedForward(self.model, B, S, self.amp_dtype, dev)
        x = g.x if g is not None else torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
        canvas = None
        with torch.no_grad():
            for i in range(nb):
                t = tab[i * B:(i + 1) * B]
                tile_gather(img, t, S, out=x)
                out = g() if g is not None else self._forward(x)
                if canvas is None:
                    if out.dim() != 4 or tuple(out.shape[2:]) != (S, S) or out.shape[0] != B:
                        raise ValueError(f"model output must be ({B}, K, {S}, {S}), got {tuple(out.shape)}")
                    if not 1 <= out.shape[1] <= MAX_CLASSES or (kind == "prob" and out.shape[1] != 1):
                        raise ValueError(f"SlidingWindowPredictor: {out.shape[1]} output channels as {kind!r} "
                                         f"(probabilities need K = 1, logits 1 <= K <= {MAX_CLASSES})")
                    canvas = torch.zeros(out.shape[1], H, W, dtype=torch.float32, device=dev)
                tile_blend(out, t, self._w1_dev, canvas, kind, regions[i])
            labels, prob = tile_finish(canvas, ry, rx, len(self.variants), return_prob=return_prob)
        return (labels, prob) if return_prob else labels


def evaluate_full_res(predictor, pairs: Iterable, num_classes: int = 1, surface=None, postprocess=None):
    """(Dice, IoU) of full-resolution hard predictions over ``pairs`` = (image, label map) items.
    Binary (num_classes = 1; a pixel is foreground where the map is > 0.5): the reference's
    batch-flattened formulas (cswin:692-708) per image, averaged over the images.  Multi-class: the
    per-class sums of all images, Dice and IoU as the macro means over the classes that occur
    (csu.train._epoch_means).  ``surface``: a csu.metrics.SurfaceMetrics accumulator; every
    (prediction, label map) pair is also fed to it (on the prediction's device, without a
    synchronisation) and the result is (Dice, IoU, surface.compute()).  ``postprocess``: a
    csu.components.PostProcess (or any callable on a label map) applied to every prediction before it is
    scored, instead of the predictor's own setting; None leaves the predictor as it is."""
    from .train import _epoch_means
    K = int(num_classes)
    rows = []
    for image, target in pairs:
        if postprocess is None:
            pred = predictor.predict(image)
        else:       # the raw labels of a predictor that has a setting of its own, then this call's rules
            own = getattr(predictor, "postprocess", None)
            pred = postprocess(predictor.predict(image) if own is None else predictor.predict(image, postprocess=None))
        t = torch.as_tensor(np.asarray(target) if not isinstance(target, torch.Tensor) else target).to(pred.device)
        t = t.reshape(pred.shape)
        if surface is not None:
            surface.update(pred, t > 0.5 if K == 1 else t.long())
        if K == 1:
            p, tt = pred.to(torch.float64), (t > 0.5).to(torch.float64)
            rows.append(torch.stack([p.new_zeros(()), (p * tt).sum(), p.sum(), tt.sum()]))
        else:
            cls = torch.arange(K, device=pred.device).view(K, 1)
            pm, tm = pred.reshape(1, -1).long() == cls, t.reshape(1, -1).long() == cls
            sums = torch.cat([(pm & tm).sum(1), pm.sum(1), tm.sum(1)]).double()
            rows.append(torch.cat([sums.new_zeros(1), sums]))
    _, dice, iou = _epoch_means(rows)
    return (dice, iou) if surface is None else (dice, iou, surface.compute())
