"""Timing of the hard-example losses (csu_seg_hard_*, csu_kth_largest) beside ce_dice_loss and torch's composition
of the top-k loss, one MI355X, device events around replays of captured graphs:
    python tools/hard_example_loss_timing.py [--ab PARENT_LIB] > profiles/hard_example_loss_timing.txt

B 16, K 5, 512 x 512, bf16 class-last logits (the (B, HW, 8) output of the head GEMM viewed as (B, 5, H, W)), uint8
labels.  Each case is one captured graph of criterion(z, t).backward(); a sample is --reps replays between two
events; the cases alternate inside every run; medians of --runs runs after 3 warm-up runs.
  1 ce_dice_loss(5)                       csu_seg_ce_fwd + csu_seg_ce_bwd
  2 dice_focal_loss(5, gamma=2)           csu_seg_hard_fwd + csu_seg_hard_bwd, no selection
  3 dice_topk_loss(5, 0.1)                the same with the keys written, csu_kth_largest, the selected sums
    3s csu_kth_largest alone              on case 3's keys (clear + 4 histogram passes + finish)
  4 torch: F.cross_entropy(reduction="none") + torch.topk + a torch Dice
--ab PARENT_LIB: case 1 again in fresh processes that alternate between this tree's library and PARENT_LIB (a build
of the parent commit), --ab-rounds times: the medians' spread between rounds of one library is the run-to-run
spread, the difference between the libraries the cost of the change to ce_dice_loss."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cswin-simam-unet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

B, K, S = 16, 5, 512
HBM_PEAK = 8e12


def inputs(d):
    g = torch.Generator().manual_seed(0)
    buf = torch.zeros(B, S * S, 8, dtype=torch.bfloat16)
    buf[..., :K] = (torch.randn(B, S * S, K, generator=g) * 3).to(torch.bfloat16)
    t = torch.randint(0, K, (B, S, S), generator=g).to(torch.uint8)
    buf = buf.to(d)
    z = buf[..., :K].transpose(1, 2).reshape(B, K, S, S).detach().requires_grad_(True)
    assert z.data_ptr() == buf.data_ptr()
    return z, t.to(d)


def torch_dice_topk(z, t, rho=0.1, smooth=1.0):
    zf, tl = z.float(), t.long()
    ce = F.cross_entropy(zf, tl, reduction="none").view(-1)
    topk = torch.topk(ce, int(rho * ce.numel())).values.mean()
    p = torch.softmax(zf, 1)
    oh = F.one_hot(tl, K).permute(0, 3, 1, 2).float()
    tp, ps, ts = (p * oh).sum((0, 2, 3)), p.sum((0, 2, 3)), oh.sum((0, 2, 3))
    return topk + (1.0 - (2 * tp + smooth) / (ps + ts + smooth)).mean()


def capture(fn):
    """A graph of fn() after a warm-up on a side stream."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def sample(g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps      # us


def measure(cases, runs, reps):
    res = {k: [] for k in cases}
    for r in range(runs + 3):
        for k, g in cases.items():
            v = sample(g, reps)
            if r >= 3:
                res[k].append(v)
    return res


def fwd_bwd(crit, z, t):
    def fn():
        z.grad = None
        loss = crit(z, t)
        loss.backward()
        return loss.detach()
    return fn


def trim_sigs():
    """A library of the parent commit has none of the new entry points: bind what it has."""
    from csu import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in [n for n in _lib._SIGS if not hasattr(L, n)]:
        del _lib._SIGS[n]


def child(args, d):
    trim_sigs()
    from csu.losses import ce_dice_loss
    z, t = inputs(d)
    g, _ = capture(fwd_bwd(ce_dice_loss(K), z, t))
    v = measure({"ce_dice": g}, args.runs, args.reps)["ce_dice"]
    print(f"{statistics.median(v):.2f} {min(v):.2f} {max(v):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ab", default=None)
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    d = torch.device("cuda:0")
    if args.child:
        return child(args, d)
    from csu import ops
    from csu.losses import ce_dice_loss, dice_focal_loss, dice_topk_loss
    z, t = inputs(d)
    npx = B * S * S
    crits = {"1 ce_dice_loss": ce_dice_loss(K), "2 dice_focal_loss(gamma=2)": dice_focal_loss(K, gamma=2.0),
             "3 dice_topk_loss(0.1)": dice_topk_loss(K, top_k=0.1)}
    cases, losses = {}, {}
    for name, crit in crits.items():
        cases[name], losses[name] = capture(fwd_bwd(crit, z, t))
    cases["4 torch CE + topk + Dice"], losses["4 torch CE + topk + Dice"] = capture(fwd_bwd(lambda a, b: torch_dice_topk(a, b), z, t))
    # the selection alone, on keys like case 3's: the per-pixel CE of the same logits
    keys = F.cross_entropy(z.detach().float(), t.long(), reduction="none").reshape(-1).contiguous()
    rho = torch.full((1,), 0.1, device=d)
    cases["3s csu_kth_largest alone"], sel = capture(lambda: ops.kth_largest(keys, rho))
    res = measure(cases, args.runs, args.reps)
    torch.cuda.synchronize()
    nz, nt = npx * 8 * 2, npx
    print(f"hard-example losses, one MI355X, one process; B {B} K {K} {S}x{S}, bf16 class-last logits of pitch 8 ({nz / 1e6:.1f} MB),"
          f" uint8 labels ({nt / 1e6:.1f} MB); forward + backward in one captured graph")
    print(f"{args.reps} replays per sample, 3 warm-up + {args.runs} runs, cases alternating; losses: "
          + ", ".join(f"{k.split()[0]}: {float(v):.6f}" for k, v in losses.items()))
    print(f"selection of case 3s: tau {float(sel[0]):.6f} n_gt {int(sel[1])} n_eq {int(sel[2])} k {int(sel[3])} n {int(sel[4])}; "
          f"case 3 last_terms {crits['3 dice_topk_loss(0.1)'].last_terms.tolist()}")
    print(f"{'case':<30}{'median us':>11}{'min us':>10}{'max us':>10}")
    med = {}
    for k, v in res.items():
        med[k] = statistics.median(v)
        print(f"{k:<30}{med[k]:>11.2f}{min(v):>10.2f}{max(v):>10.2f}")
    m1, m2, m3, m4, ms = (med[k] for k in cases)
    print(f"case 2 - case 1: {m2 - m1:+.2f} us; case 3 - case 1: {m3 - m1:+.2f} us; case 4 / case 3: {m4 / m3:.1f}x")
    sel_bytes = 4 * 4 * npx
    print(f"selection passes: 4 x 4 B/pixel = {sel_bytes / 1e6:.1f} MB in {ms:.2f} us (six launches) = {sel_bytes / ms * 1e6 / 1e12:.2f} TB/s "
          f"= {sel_bytes / ms * 1e6 / HBM_PEAK:.3f} of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak (the 16.8 MB of keys stay in the "
          f"256 MB Infinity Cache between passes)")
    extra = (4 + 4 + 4) * npx      # keys written, read by the selected sums, read by the backward
    print(f"case 3 beyond the selection: {extra / 1e6:.1f} MB more than case 1's {(2 * nz + 2 * nt + nz) / 1e6:.1f} MB "
          f"(keys written, read for the selected sums, read in the backward); measured {m3 - m1 - ms:+.2f} us for them")
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


if __name__ == "__main__":
    main()
