"""Timing of the Lovasz-Softmax loss (csu_seg_lovasz_*, csu_sort_pairs) beside ce_dice_loss and torch's composition
of the same loss, one MI355X, device events around replays of captured graphs:
    python tools/lovasz_loss_time.py [--ab PARENT_LIB] [--step] > profiles/lovasz_loss_timing.txt

B 16, K 5, 512 x 512, bf16 class-last logits (the (B, HW, 8) output of the head GEMM viewed as (B, 5, H, W)), uint8
labels: the inputs, the capture and the sampling of tools/hard_example_loss_timing.py.  Each case is one captured
graph; a sample is --reps replays between two events; the cases alternate inside every run; medians of --runs runs
after 3 warm-up runs.
  1  ce_dice_loss(5) forward + backward        csu_seg_ce_fwd + csu_seg_ce_bwd
  2  ce_loss(5) forward + backward             the same without the Dice weight: what ce_lovasz_loss adds the term to
  3  ce_lovasz_loss(5) forward + backward      csu_seg_lovasz_fwd + csu_seg_lovasz_bwd
  3f ce_lovasz_loss(5) forward alone           key pass, sort, scan and coefficient passes, finish
  2f ce_loss(5) forward alone                  the forward without the keys
  3s csu_sort_pairs alone                      5 segments of 4.2 M pairs, 31 key bits, on case 3's unsorted keys; with
                                               the two copies that put the unsorted pairs back before every replay
  3c the two copies alone
  4  torch: F.cross_entropy + the term from torch.sort(stable=True), cumsum and gather
so that  sort = 3s - 3c,  key pass = what 3f's first launch adds to 2f,  scan + coefficients = 3f - 2f - sort - key
writes, backward = 3 - 3f.  The key pass and the scan / coefficient passes are separated per kernel by
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/lovasz_loss_time.py --kernels
which runs case 3 eagerly --reps times and nothing else.
--ab PARENT_LIB: case 1 again in fresh processes that alternate between this tree's library and PARENT_LIB (a build
of the parent commit), --ab-rounds times.  --step: the headline-shaped 5-class training step (CSWinTransformer 512,
depth [1,2,9,1], split [1,2,8,8], SimAM, logits head, batch 16, bf16 autocast, captured) with ce_loss and with
ce_lovasz_loss."""
import argparse
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hard_example_loss_timing import B, HBM_PEAK, K, S, capture, fwd_bwd, inputs, measure, trim_sigs  # noqa: E402


def torch_ce_lovasz(z, t):
    """ce_lovasz_loss(5) in torch ops on the device: classes 'present', segments over the batch."""
    zf, tl = z.float(), t.long()
    ce = F.cross_entropy(zf, tl)
    p = torch.softmax(zf, 1).permute(1, 0, 2, 3).reshape(K, -1)
    fg = (tl.reshape(1, -1) == torch.arange(K, device=z.device).view(K, 1))
    e = torch.where(fg, 1.0 - p, p)
    es, order = torch.sort(e, dim=1, descending=True, stable=True)
    fs = fg.gather(1, order).float()
    G = fs.sum(1, keepdim=True)
    inter = G - fs.cumsum(1)
    union = G + (1.0 - fs).cumsum(1)
    jac = 1.0 - inter / union
    jac = torch.cat([jac[:, :1], jac[:, 1:] - jac[:, :-1]], 1)
    present = (G[:, 0] > 0).float()
    return ce + ((es * jac.detach()).sum(1) * present).sum() / present.sum().clamp(min=1.0)


def unsorted_pairs(z, t):
    """The keys and values csu_seg_lovasz_fwd hands to the sort, made in torch ops: (5, B HW) int32 each."""
    p = torch.softmax(z.detach().float(), 1).permute(1, 0, 2, 3).reshape(K, -1)
    fg = (t.long().reshape(1, -1) == torch.arange(K, device=z.device).view(K, 1))
    e = torch.where(fg, 1.0 - p, p).clamp(0.0, 1.0).contiguous()
    keys = 0x3F800000 - e.view(torch.int32)
    vals = torch.arange(p.shape[1], device=z.device, dtype=torch.int32).repeat(K, 1) | (fg.to(torch.int32) << 31)
    return keys.contiguous(), vals.contiguous()


def fwd_only(crit, z, t):
    def fn():
        with torch.no_grad():
            return crit(z, t)
    return fn


def child(args, d):
    trim_sigs()
    from csu.losses import ce_dice_loss
    z, t = inputs(d)
    g, _ = capture(fwd_bwd(ce_dice_loss(K), z, t))
    v = measure({"ce_dice": g}, args.runs, args.reps)["ce_dice"]
    print(f"{statistics.median(v):.2f} {min(v):.2f} {max(v):.2f}")


def kernels(args, d):
    from csu.losses import ce_lovasz_loss
    z, t = inputs(d)
    fn = fwd_bwd(ce_lovasz_loss(K), z, t)
    for _ in range(args.reps):
        fn()
    torch.cuda.synchronize()


def step_part(args, d):
    from csu.losses import ce_loss, ce_lovasz_loss
    from csu.model import CSWinTransformer
    from csu.train import GraphedTrainStep, make_optimizer
    g = torch.Generator().manual_seed(1)
    batches = [(torch.rand(B, 3, S, S, generator=g).to(d), torch.randint(0, K, (B, S, S), generator=g).to(d)) for _ in range(2)]
    steps = {}
    for name, crit in (("ce_loss(5)", ce_loss(K)), ("ce_lovasz_loss(5)", ce_lovasz_loss(K))):
        torch.manual_seed(0)
        m = CSWinTransformer(img_size=S, depth=[1, 2, 9, 1], split_size=[1, 2, 8, 8], simam=True, num_classes=K).set_head("logits").to(d)
        opt = make_optimizer(m, capturable=True)
        steps[name] = GraphedTrainStep(m, opt, crit, batches[0][0], batches[0][1], torch.bfloat16, warmup=3, metrics=True)
    print(f"\n-- the headline-shaped 5-class step: CSWinTransformer {S}x{S} depth [1,2,9,1] split [1,2,8,8] SimAM, logits head, "
          f"batch {B}, bf16 autocast, captured, metrics on; 20 replays per sample after 3, {args.step_rounds} alternating rounds")
    res = {k: [] for k in steps}
    for r in range(args.step_rounds + 1):
        for k, gs in steps.items():
            for i in range(3):
                gs(*batches[i % 2])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(20):
                gs(*batches[i % 2])
            e1.record()
            e1.synchronize()
            if r:
                res[k].append(e0.elapsed_time(e1) / 20)
    for k, v in res.items():
        print(f"{k:<20}{statistics.median(v):>9.3f} ms/step   (min {min(v):.3f}, max {max(v):.3f})")
    a, b = (statistics.median(v) for v in res.values())
    print(f"the term: {b - a:+.3f} ms/step, {100.0 * (b - a) / a:+.1f} % of the step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ab", default=None)
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    d = torch.device("cuda:0")
    if args.child:
        return child(args, d)
    if args.kernels:
        return kernels(args, d)
    from csu import ops
    from csu.losses import ce_dice_loss, ce_loss, ce_lovasz_loss
    z, t = inputs(d)
    npx = B * S * S
    lv = ce_lovasz_loss(K)
    cases, losses = {}, {}
    for name, fn in (("1  ce_dice_loss fwd+bwd", fwd_bwd(ce_dice_loss(K), z, t)), ("2  ce_loss fwd+bwd", fwd_bwd(ce_loss(K), z, t)),
                     ("3  ce_lovasz_loss fwd+bwd", fwd_bwd(lv, z, t)), ("3f ce_lovasz_loss fwd", fwd_only(lv, z, t)),
                     ("2f ce_loss fwd", fwd_only(ce_loss(K), z, t))):
        cases[name], losses[name] = capture(fn)
    keys, vals = unsorted_pairs(z, t)
    cases["3s csu_sort_pairs + copies"], srt = capture(lambda: ops.sort_pairs(keys, vals, K, 31))
    kc, vc = torch.empty_like(keys), torch.empty_like(vals)
    cases["3c the two copies"], _ = capture(lambda: (kc.copy_(keys), vc.copy_(vals)))
    cases["4  torch CE + Lovasz"], losses["4  torch CE + Lovasz"] = capture(fwd_bwd(torch_ce_lovasz, z, t))
    res = measure(cases, args.runs, args.reps)
    torch.cuda.synchronize()
    assert bool((srt[0][:, 1:] >= srt[0][:, :-1]).all())
    nz, nt, npair = npx * 8 * 2, npx, K * npx
    print(f"Lovasz-Softmax loss, one MI355X, one process; B {B} K {K} {S}x{S}, bf16 class-last logits of pitch 8 ({nz / 1e6:.1f} MB),"
          f" uint8 labels ({nt / 1e6:.1f} MB); captured graphs; {npair / 1e6:.1f} M (key, value) pairs in {K} segments")
    print(f"{args.reps} replays per sample, 3 warm-up + {args.runs} runs, cases alternating; losses: "
          + ", ".join(f"{k.split()[0]}: {float(v):.6f}" for k, v in losses.items()))
    print(f"case 3 last_terms (CE, LS): {lv.last_terms.tolist()}")
    print(f"{'case':<30}{'median us':>11}{'min us':>10}{'max us':>10}")
    med = {}
    for k, v in res.items():
        med[k.split()[0]] = statistics.median(v)
        print(f"{k:<30}{statistics.median(v):>11.2f}{min(v):>10.2f}{max(v):>10.2f}")
    sort = med["3s"] - med["3c"]
    sort_bytes = 20 * npair * 4
    print(f"sort = 3s - 3c: {sort:.2f} us for 4 passes x 20 B/pair (4 B read by the histogram, 8 B read and 8 B written by the "
          f"scatter) = {sort_bytes / 1e6:.0f} MB: {sort_bytes / sort * 1e6 / 1e12:.2f} TB/s = "
          f"{sort_bytes / sort * 1e6 / HBM_PEAK:.3f} of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    print(f"forward: 3f {med['3f']:.2f} us = 2f {med['2f']:.2f} us + sort {sort:.2f} us + key writes, scan, coefficients and finish "
          f"{med['3f'] - med['2f'] - sort:.2f} us (8 B/pair written, then 4 + 8 B/pair read and 4 B/pair of psi scattered)")
    print(f"backward: 3 - 3f = {med['3'] - med['3f']:.2f} us (case 2's: {med['2'] - med['2f']:.2f} us; 4 B/pair of psi read on top)")
    print(f"case 3 - case 2: {med['3'] - med['2']:+.2f} us; case 4 / case 3: {med['4'] / med['3']:.1f}x")
    if args.ab:
        print(f"\n-- case 1 in fresh processes, this tree's library (head) and {os.path.basename(args.ab)} (parent) alternating, "
              f"{args.ab_rounds} rounds: median min max us")
        meds = {"head": [], "parent": []}
        for r in range(args.ab_rounds):
            for name in ("head", "parent"):
                env = dict(os.environ)
                env.pop("CSU_LIB_PATH", None)
                if name == "parent":
                    env["CSU_LIB_PATH"] = os.path.abspath(args.ab)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(args.runs), "--reps",
                                      str(args.reps)], env=env, capture_output=True, text=True, timeout=300, check=True).stdout
                line = out.strip().splitlines()[-1]
                meds[name].append(float(line.split()[0]))
                print(f"round {r} {name:<7}{line}")
        sp = max(max(v) - min(v) for v in meds.values())
        dh = statistics.median(meds["head"]) - statistics.median(meds["parent"])
        print(f"run-to-run spread of the medians (largest max - min of one library): {sp:.2f} us; head - parent (medians of "
              f"medians): {dh:+.2f} us")
    if args.step:
        del cases
        torch.cuda.empty_cache()
        step_part(args, d)


if __name__ == "__main__":
    main()
