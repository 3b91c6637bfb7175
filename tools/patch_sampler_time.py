"""Times the patch sampler at the training shape (B = 16, 512 x 512 patches from a pool of 2048 x 2048 five-class
images) on one MI355X: csu_patch_index, csu_patch_draw, csu_patch_warp with the identity table and with everything
on, the whole PatchSampler.sample() step, and in the same process, alternating, csu_augment_warp at 512 x 512 from
this build and (``--ab-lib``) from another build of the library, e.g. the parent commit's.  For context the host
path the sampler replaces: a numpy crop of 16 patches, their upload and SpatialAugment.

Every device form is captured in a HIP graph of RUNS back-to-back launches; a replay is timed between two device
events, the forms alternate over ROUNDS rounds; the median and the range over the rounds are printed, in us per
launch.  Bytes of a warp: the fp32 image and int64 labels written once, the uint8 sources read once = 24 B per
output pixel."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "cswin-simam-unet_amd")]

from csu import _lib, ops, rng  # noqa: E402
from csu.augment import SpatialAugment, identity_table  # noqa: E402
from csu.patches import PatchPool, PatchSampler  # noqa: E402

B, S, N, L, K, RUNS, ROUNDS = 16, 512, 16, 2048, 5, 20, 9


def captured(fn, runs=RUNS):
    """A graph of `runs` launches of fn on the capture stream; returns a function timing one replay in us per launch."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(runs):
            fn()
    graph.replay()
    torch.cuda.synchronize()

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / runs * 1e3
    return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab-lib", default=None, help="another build of libcsu_hip.so whose csu_augment_warp is timed beside this one's")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "patch_sampler_timing.txt"))
    args = ap.parse_args()
    d = torch.device("cuda:0")
    torch.manual_seed(0)
    images = [torch.randint(0, 256, (L, L, 3), dtype=torch.uint8, device=d) for _ in range(N)]
    labels = [torch.randint(0, K, (L, L), dtype=torch.uint8, device=d) for _ in range(N)]
    pool = PatchPool(images, labels, K, d)
    full = SpatialAugment(rotate=(-30, 30), p_rotate=1.0, scale=(0.7, 1.4), p_scale=1.0, translate=0.1, flip_prob=0.5,
                          rot90_prob=0.25, elastic=(32, 4.0, 8.0), p_elastic=1.0, brightness=(0.8, 1.2), p_brightness=1.0,
                          contrast=(0.75, 1.25), p_contrast=1.0, gamma=(0.7, 1.5), p_gamma=1.0, noise=(0.01, 0.05), p_noise=1.0,
                          pad_label=255, mask_mode="nearest", out="labels")
    snap = torch.tensor([1, 2], dtype=torch.int64, device=d)
    table, ctrl = ops.augment_draw(full.config(S, S), B, S, S, snap, elastic=True)
    ident = identity_table(B, d)
    lib, ptr = ops.lib(), ops.ptr
    st = lambda: ops.stream_ptr(d)      # the capture stream while capturing
    rows = torch.empty_like(pool.rows)
    record = ops.patch_draw(pool, S, S, B, snap, fg_slots=5)
    oi = torch.empty(B, 3, S, S, device=d)
    ol = torch.empty(B, S, S, dtype=torch.int64, device=d)
    bimg = torch.stack([im[:S, :S] for im in images[:B]]).contiguous()
    blab = torch.stack([lb[:S, :S] for lb in labels[:B]]).contiguous()
    bmean = ops.augment_mean(bimg)

    def pwarp(tab, c, sp, r):
        return lambda: lib.csu_patch_warp(B, S, S, pool.N, ptr(pool.pixels), ptr(pool.labels), ptr(pool.meta), ptr(pool.mean),
                                          ptr(record), ptr(tab), ptr(c), sp, ptr(r), 4082, 0, 0.0, 255, 2, ptr(oi), ptr(ol), st())

    def awarp(L_, tab, c, sp, r):
        return lambda: L_.csu_augment_warp(B, S, S, ptr(bimg), ptr(blab), ptr(tab), ptr(c), sp, ptr(bmean), ptr(r), 4082, 0, 0.0,
                                           255, 2, ptr(oi), ptr(ol), st())
    sampler = PatchSampler(pool, S, B, foreground=0.33, augment=full)
    forms = [("csu_patch_index, 16 cases of 2048 x 2048 (count + scan)",
              lambda: lib.csu_patch_index(pool.N, K, L, ptr(pool.labels), ptr(pool.meta), ptr(rows), st()), 4),
             ("csu_patch_draw, 16 slots, 5 forced foreground",
              lambda: lib.csu_patch_draw(ptr(pool.labels), ptr(pool.meta), ptr(pool.rows), pool.N, K, 30, S, S, B, 5, 0.0, None,
                                         ptr(snap), 4083, ptr(record), st()), RUNS),
             ("csu_patch_warp, identity table, int64 labels", pwarp(ident, None, 0, None), RUNS),
             ("csu_patch_warp, full pipeline, int64 labels", pwarp(table, ctrl, 32, snap), RUNS),
             ("csu_augment_warp, identity table, int64 labels", awarp(lib, ident, None, 0, None), RUNS),
             ("csu_augment_warp, full pipeline, int64 labels", awarp(lib, table, ctrl, 32, snap), RUNS),
             ("PatchSampler.sample(): advance, draw, augment draw, warp", lambda: sampler.sample(snapshot=rng.advance(d)), RUNS)]
    if args.ab_lib:
        other = ctypes.CDLL(os.path.abspath(args.ab_lib))
        other.csu_augment_warp.restype, other.csu_augment_warp.argtypes = _lib._SIGS["csu_augment_warp"]
        forms += [("csu_augment_warp, identity table, int64 labels  [--ab-lib]", awarp(other, ident, None, 0, None), RUNS),
                  ("csu_augment_warp, full pipeline, int64 labels  [--ab-lib]", awarp(other, table, ctrl, 32, snap), RUNS)]
    timers = [(name, captured(fn, runs)) for name, fn, runs in forms]
    times = {name: [] for name, _ in timers}
    for _ in range(ROUNDS):
        for name, t in timers:
            times[name].append(t())
    nbytes = B * S * S * 24
    lines = [f"B = {B}, {S} x {S} patches, pool of {N} cases of {L} x {L}, {K} classes; HIP graphs of {RUNS} back-to-back launches "
             f"(the index: 4), one replay between two device events, {ROUNDS} rounds alternating the forms; us per launch: "
             f"median (min .. max)"]
    for name, ts in times.items():
        med = statistics.median(ts)
        rate = f" = {nbytes / med / 1e3:7.1f} GB/s of {nbytes / 1e6:.1f} MB" if name.startswith("csu_") and "warp" in name else ""
        lines.append(f"{name:62s}: {med:8.2f} ({min(ts):.2f} .. {max(ts):.2f}){rate}")
    # the host path: crop 16 patches with numpy, upload them, SpatialAugment on the device
    himg = [im.cpu().numpy() for im in images]
    hlab = [lb.cpu().numpy() for lb in labels]
    g = np.random.default_rng(0)
    host = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = g.integers(0, N, B)
        oy, ox = g.integers(0, L - S + 1, B), g.integers(0, L - S + 1, B)
        ci = np.stack([himg[n[b]][oy[b]:oy[b] + S, ox[b]:ox[b] + S] for b in range(B)])
        cl = np.stack([hlab[n[b]][oy[b]:oy[b] + S, ox[b]:ox[b] + S] for b in range(B)])
        full(torch.from_numpy(ci).to(d), torch.from_numpy(cl).to(d))
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
    lines.append(f"{'host path: numpy crop of 16 patches + upload + SpatialAugment':62s}: {statistics.median(host):8.1f} "
                 f"({min(host):.1f} .. {max(host):.1f}) us per batch, host clock, uniform origins only")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
