"""ms/step of the graph-captured headline step (512x512, batch 16, bf16, +SimAM) with and without a
weight EMA (profiles/ema_timing.txt):
    python tools/ema_time.py <none|fused|standalone> [--pkg DIR] [--swap]
  none       : no EMA
  fused      : make_optimizer(ema_decay=0.999): the EMA inside the step launch (csu_adamw_step_ema)
  standalone : plain step + a captured stand-alone ema.update() (csu_ema_update)
--pkg DIR: import csu from DIR instead of this tree (a checkout of another commit with its library
built: `none --pkg <parent>/cswin-simam-unet_amd` is the parent's step).
--swap: after the timing, 10 ``with ema.applied(): pass`` blocks (20 csu_ema_swap launches, for a
rocprofv3 --kernel-trace --stats run of this script).
One fresh process per sample; alternate the configurations in one session to compare them.  Prints
one ``TIMING {json}`` line: 5 windows of 40 replays each, host clock around work ending in a device
synchronise, after 3 warm-up steps and 10 replays."""
import json
import os
import sys
import time

mode = sys.argv[1]
if mode not in ("none", "fused", "standalone"):
    sys.exit(__doc__)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = sys.argv[sys.argv.index("--pkg") + 1] if "--pkg" in sys.argv else os.path.join(ROOT, "cswin-simam-unet_amd")
sys.path.insert(0, pkg)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import csu  # noqa: E402
from csu.model import CSWinTransformer  # noqa: E402
from csu.train import GraphedTrainStep, bce_loss, make_optimizer  # noqa: E402

d = torch.device("cuda:0")
torch.manual_seed(0)
model = CSWinTransformer(img_size=512, depth=[1, 2, 9, 1], split_size=[1, 2, 8, 8], simam=True).to(d)
g = torch.Generator().manual_seed(1234)
batches = [(torch.rand(16, 3, 512, 512, generator=g).to(d), (torch.rand(16, 1, 512, 512, generator=g) > 0.5).float().to(d))
           for _ in range(2)]
ema = None
if mode == "fused":
    opt = make_optimizer(model, capturable=True, ema_decay=0.999)
    ema = opt.ema
else:
    opt = make_optimizer(model, capturable=True)
if mode == "standalone":
    from csu.ema import WeightEMA
    ema = WeightEMA(model, decay=0.999)
    ema.prepare_capture()
    plain = opt.step

    def step_then_update(*a, **k):
        r = plain(*a, **k)
        ema.update()
        return r
    opt.step = step_then_update
gs = GraphedTrainStep(model, opt, bce_loss, batches[0][0], batches[0][1], torch.bfloat16, warmup=3, metrics=True)
for i in range(10):
    gs(*batches[i % 2])
torch.cuda.synchronize()
wins = []
for w in range(5):
    t0 = time.perf_counter()
    for i in range(40):
        gs(*batches[i % 2])
    torch.cuda.synchronize()
    wins.append((time.perf_counter() - t0) / 40 * 1e3)
out = {"mode": mode, "csu": os.path.dirname(csu.__file__), "ms_per_step_windows": [round(x, 4) for x in wins],
       "ms_per_step_median": round(float(np.median(wins)), 4), "loss": float(gs.loss),
       "ema_updates": None if ema is None else float(ema.num_updates)}
if "--swap" in sys.argv and ema is not None:
    for _ in range(10):
        with ema.applied():
            pass
    torch.cuda.synchronize()
print("TIMING " + json.dumps(out), flush=True)
