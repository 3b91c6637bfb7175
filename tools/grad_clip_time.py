"""Timing of the fused gradient clipping (csrc/grad_norm.hip, adamw_kernel's CLIP variant) beside the
plain AdamW step, one MI355X, one process:
    python tools/grad_clip_time.py [--kernels-only] [--rounds 7] [--reps 50] > profiles/grad_clip_timing.txt

== kernels: the headline model's own parameter table (512 x 512, depth [1,2,9,1], split [1,2,8,8],
SimAM; gradients of one real backward, bf16 shadows registered), C-ABI calls on that table, device
events.  Two ways of timing, because the 94 MB of gradients fit the 256 MB Infinity Cache:
  back-to-back   `reps` launches of ONE variant between two events (the norm pass then re-reads
                 gradients it has just read: cache-warm, the best case);
  in sequence    norm -> adamw -> norm -> adamw_ex ..., every launch between its own two events, as
                 they follow each other in a training step (the 660 MB the step moves have passed
                 through the cache before the next norm pass).
Variants alternate inside every round; median / min / max over the rounds.
== whole step: the captured 512 x 512 batch-16 bf16 train step with and without max_grad_norm,
alternating, 20 replays each."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cswin-simam-unet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def mmm(v):
    return statistics.median(v), min(v), max(v)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us per launch


def kernels(args, d):
    from csu._lib import check, lib, stream_ptr
    from csu.data import ellipse_batch
    from csu.model import CSWinTransformer
    from csu.train import bce_loss, make_optimizer
    torch.manual_seed(0)
    m = CSWinTransformer(img_size=512, depth=[1, 2, 9, 1], split_size=[1, 2, 8, 8], simam=True).to(d)
    x, t = (v.to(d) for v in ellipse_batch(np.random.default_rng(7), 2, 512))
    opt = make_optimizer(m, capturable=True, max_grad_norm=1.0)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
    bce_loss(y, t).backward()
    opt.step()                       # builds the optimizer state and the device table
    torch.cuda.synchronize()
    _, _, table, n, chunks = opt._tables[0]
    gs, g = opt._gstate[0], opt.param_groups[0]
    numel = sum(p.numel() for p in m.parameters() if p.grad is not None)
    L, st = lib(), stream_ptr(d)
    part, ctl = opt._partial, opt._ctl
    b1, b2 = g["betas"]
    common = (table.data_ptr(), n, chunks, gs["lr"].data_ptr(), float(g["lr"]), float(b1), float(b2), float(g["eps"]),
              float(g["weight_decay"]), gs["step"].data_ptr(), 0.0)

    def norm():
        check(L.csu_grad_sumsq(table.data_ptr(), n, chunks, part.data_ptr(), st), "sumsq")
        check(L.csu_grad_norm_finish(part.data_ptr(), chunks, 1.0, ctl.data_ptr(), st), "finish")

    def sumsq():
        check(L.csu_grad_sumsq(table.data_ptr(), n, chunks, part.data_ptr(), st), "sumsq")

    def adamw():
        check(L.csu_adamw_step(*common, st), "adamw")

    def adamw_ex():
        check(L.csu_adamw_step_ex(*common, ctl.data_ptr(), 0, 0, st), "adamw_ex")

    variants = [("norm (sumsq+finish)", norm), ("sumsq alone", sumsq), ("adamw", adamw), ("adamw_ex (ctl)", adamw_ex),
                ("adamw again", adamw)]
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    print(f"== kernels: {n} tensors, {numel} parameters ({numel / 1e6:.1f} M), {chunks} chunks; pre-clip norm "
          f"{float(ctl[0]):.4g}, coefficient {float(ctl[1]):.4g}")
    print(f"algorithmic bytes: norm 4 B/param = {4 * numel / 1e6:.1f} MB, step 28 B/param = {28 * numel / 1e6:.1f} MB "
          "(+ bf16 shadows); HBM peak 8 TB/s")
    print(f"-- back-to-back: {args.reps} launches per sample, {args.rounds} alternating rounds")
    res = {k: [] for k, _ in variants}
    for _ in range(args.rounds):
        for k, fn in variants:
            res[k].append(timed(fn, args.reps))
    print(f"{'variant':<22}{'median us':>10}{'min us':>10}{'max us':>10}")
    for k, _ in variants:
        print(f"{k:<22}" + "".join(f"{v:>10.2f}" for v in mmm(res[k])))
    ta = statistics.median(res["adamw"])
    spread = abs(ta - statistics.median(res["adamw again"]))
    print(f"run-to-run spread of adamw (|median adamw - median adamw again|): {spread:.2f} us; "
          f"adamw_ex - adamw (medians): {statistics.median(res['adamw_ex (ctl)']) - ta:+.2f} us")
    print(f"pro-rata yardstick of the norm pass: t_adamw x 4/28 = {ta * 4 / 28:.2f} us, with the 2x margin "
          f"{ta * 8 / 28:.2f} us; measured {statistics.median(res['norm (sumsq+finish)']):.2f} us")
    # in sequence: each launch between its own events
    seq = [("norm", norm), ("adamw", adamw), ("norm", norm), ("adamw_ex", adamw_ex)]
    ev = []
    for _ in range(args.rounds * 8):
        for k, fn in seq:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev.append((k, e0, e1))
    torch.cuda.synchronize()
    per = {}
    for k, e0, e1 in ev[len(seq):]:
        per.setdefault(k, []).append(e0.elapsed_time(e1) * 1e3)
    print(f"-- in sequence (norm, adamw, norm, adamw_ex, ...; one launch per event pair, {len(ev) // len(seq) - 1} "
          "rounds; an event pair itself costs a few us)")
    print(f"{'variant':<22}{'median us':>10}{'min us':>10}{'max us':>10}")
    for k in ("norm", "adamw", "adamw_ex"):
        print(f"{k:<22}" + "".join(f"{v:>10.2f}" for v in mmm(per[k])))
    ts = statistics.median(per["adamw"])
    print(f"pro-rata yardstick in sequence: t_adamw x 4/28 = {ts * 4 / 28:.2f} us, with the 2x margin {ts * 8 / 28:.2f} us; "
          f"measured {statistics.median(per['norm']):.2f} us; adamw_ex - adamw {statistics.median(per['adamw_ex']) - ts:+.2f} us")
    return statistics.median(per["norm"]) + statistics.median(per["adamw_ex"]) - ts


def whole_step(args, d, kernel_sum):
    from csu.data import ellipse_batch
    from csu.model import CSWinTransformer
    from csu.train import GraphedTrainStep, bce_loss, make_optimizer
    rng = np.random.default_rng(1234)
    batches = [tuple(v.to(d) for v in ellipse_batch(rng, 16, 512)) for _ in range(2)]
    steps = {}
    for name, c in (("no clipping", None), ("max_grad_norm=1.0", 1.0)):
        torch.manual_seed(0)
        m = CSWinTransformer(img_size=512, depth=[1, 2, 9, 1], split_size=[1, 2, 8, 8], simam=True).to(d)
        opt = make_optimizer(m, capturable=True, max_grad_norm=c)
        steps[name] = (GraphedTrainStep(m, opt, bce_loss, batches[0][0], batches[0][1], torch.bfloat16, warmup=3,
                                        metrics=True), opt)
    print("\n== whole step")
    print("graph-captured train step, CSWinTransformer 512x512 depth [1,2,9,1] split [1,2,8,8] SimAM, batch 16, bf16 "
          f"autocast, 20 replays per sample after 3, {args.step_rounds} alternating rounds (device events)")
    res = {k: [] for k in steps}
    for r in range(args.step_rounds + 1):
        for k, (gs, opt) in steps.items():
            for i in range(3):
                gs(*batches[i % 2])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(20):
                loss = gs(*batches[i % 2])[0]
            e1.record()
            e1.synchronize()
            if r:                      # round 0 warms both graphs up
                res[k].append(e0.elapsed_time(e1) / 20)
    for k, (gs, opt) in steps.items():
        md, lo, hi = mmm(res[k])
        extra = f"   last pre-clip norm {float(opt.grad_norm):.4g}, coefficient {float(opt._ctl[1]):.4g}" if opt.max_grad_norm else ""
        print(f"{k:<22}{md:>9.3f} ms/step   (min {lo:.3f}, max {hi:.3f}){extra}")
    a, b = (statistics.median(res[k]) for k in steps)
    print(f"difference of the medians: {(b - a) * 1e3:+.1f} us/step; kernel-level sum (norm + adamw_ex - adamw, in sequence): "
          f"{kernel_sum:+.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    d = torch.device("cuda:0")
    print("fused gradient clipping (csrc/grad_norm.hip, csu_adamw_step_ex) beside the AdamW step (csrc/adamw.hip), one "
          "MI355X, one process")
    ks = kernels(args, d)
    if not args.kernels_only:
        torch.cuda.empty_cache()
        whole_step(args, d, ks)


if __name__ == "__main__":
    main()
