"""Timing of the fused multi-class loss (csrc/seg_ce.hip) beside torch's composition of the same
formula, one MI355X, one process, device events:
    python tools/seg_ce_timing.py [--runs 30] [--no-step] > profiles/seg_ce_timing.txt

== loss: B 16, K 8, 512 x 512, bf16 class-last logits (the (B, HW, 8) output of the head GEMM viewed
as (B, K, H, W)), uint8 labels, ce_dice_loss(8).  Every sample is one call between its own two
events after a warm-up; the variants alternate inside every run; medians of --runs runs.
  fused   loss_stats forward (csu_seg_ce_fwd: partial + finish), backward (csu_seg_ce_bwd), and both
  torch   log_softmax + nll_loss + softmax + one-hot + per-class sums + argmax metrics on the
          device, forward, backward, and both
  kernels the two C entry points alone on preallocated buffers, --reps back-to-back launches between
          two events per sample (no Python, allocator or launch gap inside the figure): the achieved
          bytes per second of each fused kernel against its algorithmic bytes
The 67 MB of logits fit the 256 MB Infinity Cache, so back-to-back launches read them cache-warm.
== step: the captured 64 x 64 3-class train step of tests/test_gpu_seg_ce.py with and without
metrics=True (the per-class sums inside the graph), alternating, 200 replays per sample."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cswin-simam-unet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8e12


def mmm(v):
    return statistics.median(v), min(v), max(v)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, out      # us


def torch_composition(z, t, K, smooth):
    """ce_dice_loss(K) and the (3, K) argmax sums in torch ops (fp32, as the criterion computes)."""
    zf = z.float()
    tl = t.long()
    lsm = F.log_softmax(zf, 1)
    ce = F.nll_loss(lsm, tl)
    p = lsm.exp()
    oh = F.one_hot(tl, K).permute(0, 3, 1, 2).float()
    tp, ps, ts = (p * oh).sum((0, 2, 3)), p.sum((0, 2, 3)), oh.sum((0, 2, 3))
    loss = ce + (1.0 - (tp + smooth) / (0.5 * ps + 0.5 * ts + smooth)).mean()
    pred = F.one_hot(zf.argmax(1), K).permute(0, 3, 1, 2)
    ohb = oh.bool()
    stats = torch.stack([(pred.bool() & ohb).sum((0, 2, 3)), pred.sum((0, 2, 3)), ohb.sum((0, 2, 3))]).double()
    return loss, stats


def loss_part(args, d):
    from csu.losses import ce_dice_loss
    B, K, S = 16, 8, 512
    g = torch.Generator().manual_seed(0)
    buf = (torch.randn(B, S * S, K, generator=g) * 3).to(torch.bfloat16).to(d)
    t = torch.randint(0, K, (B, S, S), generator=g).to(torch.uint8).to(d)
    crit = ce_dice_loss(K)

    def logits():
        return buf.transpose(1, 2).reshape(B, K, S, S).detach().requires_grad_(True)

    nz, nt = buf.numel() * 2, t.numel()
    by_f, by_b = nz + nt, 2 * nz + nt
    variants = {}
    for name, fwd in (("fused", lambda z: crit.loss_stats(z, t)), ("torch", lambda z: torch_composition(z, t, K, crit.smooth))):
        variants[name] = fwd
    lf, sf = variants["fused"](logits())
    lt, st = variants["torch"](logits())
    torch.cuda.synchronize()
    print(f"== loss: B {B} K {K} {S}x{S}, bf16 class-last logits ({nz / 1e6:.1f} MB), uint8 labels ({nt / 1e6:.1f} MB), "
          f"ce_dice_loss({K})")
    print(f"fused loss {float(lf):.6f}, torch loss {float(lt):.6f}; hard sums equal: {bool(torch.equal(sf, st))}")
    print(f"algorithmic bytes: forward {by_f / 1e6:.1f} MB (logits + labels read), backward {by_b / 1e6:.1f} MB "
          f"(the same + the gradient written); HBM peak {HBM_PEAK / 1e12:.0f} TB/s")
    res = {(n, k): [] for n in variants for k in ("fwd", "bwd", "fwd+bwd")}
    for r in range(args.runs + 3):
        for n, fwd in variants.items():
            z = logits()
            tf_, (loss, _) = timed(lambda: fwd(z))
            tb, _ = timed(lambda: loss.backward())
            z = logits()
            tfb, _ = timed(lambda: fwd(z)[0].backward())
            if r >= 3:          # three warm-up runs
                res[(n, "fwd")].append(tf_)
                res[(n, "bwd")].append(tb)
                res[(n, "fwd+bwd")].append(tfb)
    print(f"-- one call per event pair, 3 warm-up + {args.runs} runs, variants alternating")
    print(f"{'variant':<18}{'median us':>11}{'min us':>10}{'max us':>10}{'  algorithmic bytes/s':>22}{'  of HBM peak':>14}")
    med = {}
    for (n, k), v in res.items():
        m, lo, hi = mmm(v)
        med[(n, k)] = m
        rate = ""
        if n == "fused":
            by = {"fwd": by_f, "bwd": by_b, "fwd+bwd": by_f + by_b}[k]
            rate = f"{by / m * 1e6 / 1e12:>17.2f} TB/s{by / m * 1e6 / HBM_PEAK:>14.3f}"
        print(f"{n + ' ' + k:<18}{m:>11.1f}{lo:>10.1f}{hi:>10.1f}{rate}")
    print(f"ratio torch / fused (medians): fwd {med[('torch', 'fwd')] / med[('fused', 'fwd')]:.1f}x, "
          f"bwd {med[('torch', 'bwd')] / med[('fused', 'bwd')]:.1f}x, fwd+bwd "
          f"{med[('torch', 'fwd+bwd')] / med[('fused', 'fwd+bwd')]:.1f}x")


def kernel_part(args, d):
    from csu._lib import check, lib, ptr, stream_ptr
    B, K, S = 16, 8, 512
    HW = S * S
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(B, HW, K, generator=g) * 3).to(torch.bfloat16).to(d)
    t = torch.randint(0, K, (B, HW), generator=g).to(torch.uint8).to(d)
    dz = torch.empty_like(z)
    L, st = lib(), stream_ptr(d)
    nws = L.csu_seg_ce_workspace(B, K, HW)
    ws = torch.empty(nws // 4, dtype=torch.float32, device=d)
    loss, dl = torch.empty((), device=d), torch.ones((), device=d)
    stats = torch.empty(3, K, dtype=torch.float64, device=d)
    coef = torch.empty(2 * K + 1, device=d)
    geom = (B, K, HW, 1, 1, ptr(z), HW * K, 1, K, 0, 0, ptr(t), -100, None)

    def fwd():
        check(L.csu_seg_ce_fwd(*geom, 1.0, 1.0, 0.5, 0.5, 0.5, 1, ptr(loss), ptr(stats), ptr(coef), ptr(ws), nws, st), "fwd")

    def bwd():
        check(L.csu_seg_ce_bwd(*geom, ptr(dl), ptr(coef), 1.0, 1.0, 1, ptr(dz), st), "bwd")

    nz, nt = z.numel() * 2, t.numel()
    by = {"csu_seg_ce_fwd": nz + nt, "csu_seg_ce_bwd": 2 * nz + nt}
    res = {k: [] for k in by}
    for r in range(args.runs + 3):
        for k, fn in (("csu_seg_ce_fwd", fwd), ("csu_seg_ce_bwd", bwd)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            e1.synchronize()
            if r >= 3:
                res[k].append(e0.elapsed_time(e1) * 1e3 / args.reps)
    print(f"\n-- kernels: C-ABI calls on preallocated buffers, {args.reps} back-to-back launches per sample, 3 warm-up + "
          f"{args.runs} samples, alternating (cache-warm: 67 MB of logits in a 256 MB Infinity Cache)")
    print(f"{'entry point':<18}{'median us':>11}{'min us':>10}{'max us':>10}{'  algorithmic bytes/s':>22}{'  of HBM peak':>14}")
    for k, v in res.items():
        m, lo, hi = mmm(v)
        print(f"{k:<18}{m:>11.2f}{lo:>10.2f}{hi:>10.2f}{by[k] / m * 1e6 / 1e12:>17.2f} TB/s{by[k] / m * 1e6 / HBM_PEAK:>14.3f}")


def step_part(args, d):
    from csu.data import SyntheticSegmentation
    from csu.losses import ce_dice_loss
    from csu.model import CSWinTransformer
    from csu.train import GraphedTrainStep, make_optimizer
    ds = SyntheticSegmentation(8, 64, seed=5, num_classes=3)
    batches = [tuple(torch.stack(v).to(d) for v in zip(*[ds[4 * b + i] for i in range(4)])) for b in range(2)]
    steps = {}
    for name, metrics in (("metrics=False", False), ("metrics=True", True)):
        torch.manual_seed(0)
        m = CSWinTransformer(img_size=64, split_size=[1, 2, 2, 2], num_classes=3).set_head("logits").to(d)
        opt = make_optimizer(m, capturable=True)
        steps[name] = GraphedTrainStep(m, opt, ce_dice_loss(3), batches[0][0], batches[0][1], torch.bfloat16, warmup=3,
                                       metrics=metrics)
    print("\n== step: graph-captured train step, CSWinTransformer 64x64 split [1,2,2,2] num_classes 3 logits head, batch 4, "
          f"bf16 autocast, ce_dice_loss(3); 200 replays per sample, {args.step_rounds} alternating rounds")
    res = {k: [] for k in steps}
    for r in range(args.step_rounds + 1):
        for k, gs in steps.items():
            for i in range(5):
                gs(*batches[i % 2])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(200):
                gs(*batches[i % 2])
            e1.record()
            e1.synchronize()
            if r:
                res[k].append(e0.elapsed_time(e1) * 1e3 / 200)
    for k in steps:
        m, lo, hi = mmm(res[k])
        print(f"{k:<16}{m:>9.1f} us/step   (min {lo:.1f}, max {hi:.1f})")
    a, b = (statistics.median(res[k]) for k in steps)
    print(f"metrics=True - metrics=False (medians): {b - a:+.1f} us/step; per-class sums after the last replay: "
          f"{steps['metrics=True'].stats.tolist()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs must be at least 20")
    d = torch.device("cuda:0")
    print("fused softmax-CE + per-class Dice (csrc/seg_ce.hip) beside torch's composition, one MI355X, one process")
    loss_part(args, d)
    kernel_part(args, d)
    if not args.no_step:
        torch.cuda.empty_cache()
        step_part(args, d)


if __name__ == "__main__":
    main()
