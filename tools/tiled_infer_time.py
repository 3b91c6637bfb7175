"""Tiled inference timing record (profiles/tiled_infer_timing.txt): 2048x2048 uint8 image, tile 512, overlap
0.5 (49 tiles), bf16, batch 16; K = 1 (sigmoid head) and K = 5 (logits head), one and eight TTA variants.
    python tools/tiled_infer_time.py [--out FILE]
Per configuration: the whole predict (host clock around calls that end in a device synchronise), and in runs
of their own the device-event time of the captured forwards and of each tile kernel, with the kernel's
share of the HBM peak from its compulsory bytes; alongside, reference_predict in fp32 torch ops on the GPU
with the eager forward -- the loop a user would otherwise write."""
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "cswin-simam-unet_amd")]
import numpy as np
import torch

from csu import infer
from csu.model import CSWinTransformer

PEAK = 8.0e12          # HBM3E spec; ~6.3e12 achievable by a float4 copy
d = torch.device("cuda:0")
H = W = 2048
S, OV, B = 512, 0.5, 16
out_lines = []


def say(*a):
    s = " ".join(str(v) for v in a)
    print(s, flush=True)
    out_lines.append(s)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


class Stage:
    """wraps a callable, recording a device event pair per call"""

    def __init__(self, fn):
        self.fn, self.ev = fn, []

    def __call__(self, *a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = self.fn(*a, **k)
        e1.record()
        self.ev.append((e0, e1))
        return r

    def total(self):
        t = sum(a.elapsed_time(b) for a, b in self.ev)
        n = len(self.ev)
        self.ev = []
        return t, n


def union_pixels(recs):
    m = np.zeros((H, W), dtype=bool)
    for y0, x0, *_rest, on in recs.tolist():
        if on:
            m[y0:y0 + S, x0:x0 + S] = True
    return int(m.sum())


img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(d)
say(f"device {torch.cuda.get_device_name(0)}; image {H}x{W} uint8, tile {S}, overlap {OV}, batch {B}, bf16 autocast")
say("times in ms: median [min .. max] over the repeats; each predict ends in a device synchronise")
for K in (1, 5):
    torch.manual_seed(0)
    m = CSWinTransformer(img_size=S, depth=[1, 2, 9, 1], split_size=[1, 2, 8, 8], num_classes=K)
    if K > 1:
        m.set_head("logits")
    m = m.to(d).eval()
    for tta in (("identity",), "d4"):
        nv = len(infer.parse_tta(tta))
        p = infer.SlidingWindowPredictor(m, overlap=OV, tta=tta, batch_size=B, amp_dtype=torch.bfloat16)
        table = infer.plan_tiles(H, W, S, OV, tta)
        nrec = len(table)
        nb = -(-nrec // B)
        for _ in range(2):          # warm-up: capture, code objects, allocator
            p.predict(img, return_prob=True)
        reps = 7 if nv == 1 else 4
        tot = timed(lambda: p.predict(img, return_prob=True), reps)
        # stage times: device events around each launch, in runs of their own
        g, b, f = Stage(infer.tile_gather), Stage(infer.tile_blend), Stage(infer.tile_finish)
        fw = Stage(infer._GraphedForward.__call__)
        saved = (infer.tile_gather, infer.tile_blend, infer.tile_finish, infer._GraphedForward.__call__)
        infer.tile_gather, infer.tile_blend, infer.tile_finish = g, b, f
        infer._GraphedForward.__call__ = lambda self: fw(self)
        st = {"gather": [], "blend": [], "finish": [], "forward": []}
        for _ in range(3):
            p.predict(img, return_prob=True)
            torch.cuda.synchronize()
            for k, s in (("gather", g), ("blend", b), ("finish", f), ("forward", fw)):
                st[k].append(s.total())
        infer.tile_gather, infer.tile_blend, infer.tile_finish, infer._GraphedForward.__call__ = saved
        med = {k: statistics.median(t for t, _ in v) for k, v in st.items()}
        cnt = {k: v[0][1] for k, v in st.items()}
        # compulsory bytes
        es = 4 if K == 1 else 2                       # PROB fp32; logits bf16
        pad = np.zeros((nb * B, 6), dtype=np.int32)
        pad[:nrec] = table
        gather_bytes = nb * B * S * S * (3 + 12)
        blend_bytes = nrec * S * S * K * es + sum(union_pixels(pad[i * B:(i + 1) * B]) for i in range(nb)) * K * 8
        finish_bytes = H * W * (4 * K + 4 * K + 1)
        say(f"\nK = {K} ({'sigmoid head, fp32 probabilities' if K == 1 else 'logits head, bf16 class-last pitch 8'}), "
            f"{nv} TTA variant(s): {nrec} records, {nb} batches")
        say(f"  predict total      {statistics.median(tot):9.2f}  [{min(tot):.2f} .. {max(tot):.2f}]  ({reps} repeats)")
        say(f"  captured forwards  {med['forward']:9.2f}  ({cnt['forward']} replays, {med['forward'] / cnt['forward']:.2f} each)")
        for k, nbytes in (("gather", gather_bytes), ("blend", blend_bytes), ("finish", finish_bytes)):
            bw = nbytes / (med[k] * 1e-3)
            say(f"  {k:<7} {med[k]:9.3f}  ({cnt[k]} launches, {med[k] / cnt[k] * 1e3:.1f} us each); compulsory {nbytes / 1e6:.1f} MB "
                f"-> {bw / 1e12:.3f} TB/s = {100 * bw / PEAK:.1f} % of the 8 TB/s HBM peak")
        say(f"  tile kernels together {med['gather'] + med['blend'] + med['finish']:.2f} = "
            f"{100 * (med['gather'] + med['blend'] + med['finish']) / statistics.median(tot):.1f} % of predict")
        # the loop a user would otherwise write: reference_predict in fp32 torch ops on the GPU, same model
        def fwd(x):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return m(x)
        kind = "prob" if K == 1 else "logits"
        run = lambda: infer.reference_predict(fwd, img, S, OV, "gaussian", tta, B, kind, True, torch.float32)  # noqa: E731
        run()
        rt = timed(run, 3)
        say(f"  reference_predict (fp32 torch ops, eager forward) {statistics.median(rt):9.2f}  [{min(rt):.2f} .. {max(rt):.2f}]")
        del p
    del m
    torch.cuda.empty_cache()
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
        fh.write("\n".join(out_lines) + "\n")
