"""Times the device augmentation paths at the benchmark shape (B = 16, 512 x 512) on one MI355X:
csu_augment_batch (the reference-parity path, the yardstick), csu_augment_warp with the identity table and with
the full pipeline (rotation + scale + shift + elastic + contrast / brightness / gamma / noise), csu_augment_draw
and csu_augment_mean alone, and AugmentationTransform on the host for the same 16 images.

Device events around RUNS back-to-back launches after warm-up, the forms alternated over ROUNDS rounds in one
process; the median and the range over the rounds are printed.  Bytes: the uint8 image and mask read once, the
fp32 image and mask written once = 20 B per pixel."""
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "cswin-simam-unet_amd")]

from csu import augment as A, ops  # noqa: E402
from csu.augment import SpatialAugment, identity_table  # noqa: E402
from csu.data import AugmentationTransform  # noqa: E402

B, S, RUNS, ROUNDS = 16, 512, 200, 7


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(RUNS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / RUNS * 1e3      # us per launch


def main():
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=g).to(d)
    msk = ((torch.rand(B, S, S, generator=g) > 0.5).to(torch.uint8) * 255).to(d)
    np.random.seed(0)
    tr = AugmentationTransform()
    drawn = [tr.draw(S, S) for _ in range(B)]
    plain = [(0, 0, 0, 0, 0, S, S)] * B
    lib, ptr, st = ops.lib(), ops.ptr, ops.stream_ptr(d)
    oi = torch.empty(B, 3, S, S, device=d)
    om = torch.empty(B, 1, S, S, device=d)
    ol = torch.empty(B, S, S, dtype=torch.int64, device=d)

    def batch(params):
        pd = torch.tensor(params, dtype=torch.int32, device=d)
        return lambda: lib.csu_augment_batch(B, S, ptr(img), ptr(msk), ptr(pd), ptr(oi), ptr(om), st)
    full = SpatialAugment(rotate=(-30, 30), p_rotate=1.0, scale=(0.7, 1.4), p_scale=1.0, translate=0.1, flip_prob=0.5,
                          rot90_prob=0.25, elastic=(32, 4.0, 8.0), p_elastic=1.0, brightness=(0.8, 1.2), p_brightness=1.0,
                          contrast=(0.75, 1.25), p_contrast=1.0, gamma=(0.7, 1.5), p_gamma=1.0, noise=(0.01, 0.05), p_noise=1.0)
    cfg = full.config(S, S)
    snap = torch.tensor([1, 2], dtype=torch.int64, device=d)
    table, ctrl = ops.augment_draw(cfg, B, S, S, snap, elastic=True)
    ident = identity_table(B, d)
    mean = ops.augment_mean(img)
    sums = torch.empty(B, dtype=torch.int64, device=d)

    def warp(tab, c, sp, rng, mode, out):
        return lambda: lib.csu_augment_warp(B, S, S, ptr(img), ptr(msk), ptr(tab), ptr(c), sp, ptr(mean), ptr(rng),
                                            4082, 0, 0.0, 0, mode, ptr(oi), ptr(out), st)
    forms = [("csu_augment_batch, no-op parameters (parent yardstick)", batch(plain)),
             ("csu_augment_batch, drawn flips / turns / crops", batch(drawn)),
             ("csu_augment_warp, identity table, bilinear mask", warp(ident, None, 0, None, 0, om)),
             ("csu_augment_warp, identity table, int64 labels", warp(ident, None, 0, None, 2, ol)),
             ("csu_augment_warp, full pipeline, bilinear mask", warp(table, ctrl, 32, snap, 0, om)),
             ("csu_augment_warp, full pipeline, int64 labels", warp(table, ctrl, 32, snap, 2, ol)),
             ("csu_augment_draw (table + control field)",
              lambda: lib.csu_augment_draw(cfg, B, S, S, ptr(snap), 4080, 4081, ptr(table), ptr(ctrl), st)),
             ("csu_augment_mean (memset + sum + finish)", lambda: lib.csu_augment_mean(B, S * S * 3, ptr(img), ptr(sums), ptr(mean), st))]
    for _, fn in forms:
        for _ in range(20):
            assert fn() == 0
    torch.cuda.synchronize()
    times = {name: [] for name, _ in forms}
    for _ in range(ROUNDS):
        for name, fn in forms:
            times[name].append(timed(fn))
    nbytes = B * S * S * 20
    print(f"B = {B}, {S} x {S}; {RUNS} back-to-back launches between two device events, {ROUNDS} rounds alternating the forms; "
          f"us per launch: median (min .. max)")
    for name, ts in times.items():
        med = statistics.median(ts)
        rate = f" = {nbytes / med / 1e3:7.1f} GB/s of {nbytes / 1e6:.1f} MB" if "warp" in name or "batch" in name else ""
        print(f"{name:58s}: {med:8.2f} ({min(ts):.2f} .. {max(ts):.2f}){rate}")
    # end to end through the Python surface: draw + mean + warp, three launches and their allocations
    for _ in range(10):
        full(img, msk)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(100):
        full(img, msk)
    torch.cuda.synchronize()
    print(f"{'SpatialAugment.__call__ (snapshot, draw, mean, warp), host clock':58s}: {(time.perf_counter() - t0) / 100 * 1e6:8.1f} us per batch")
    # the host path the data loader workers run: 16 images, one process
    himg, hmsk = img.cpu().numpy(), msk.cpu().numpy()
    t0 = time.perf_counter()
    for b in range(B):
        tr(himg[b], hmsk[b])
    print(f"{'AugmentationTransform on the host, 16 images, one process':58s}: {(time.perf_counter() - t0) * 1e3:8.1f} ms")


if __name__ == "__main__":
    main()
