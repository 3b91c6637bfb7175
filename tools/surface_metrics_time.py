"""Timing of csu.surface_metrics on one 2048 x 2048 image with K = 5 (four foreground classes): the kernels
(csrc/surface.hip), reference_surface_metrics in plain torch ops on the GPU, and medpy's formulas with
scipy.ndimage on the host (download of the label maps included) when scipy is installed.
    python tools/surface_metrics_time.py [out.txt]    host clock around calls that end in a device synchronise
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/surface_metrics_time.py prof
                                                      13 calls per spacing and one transform, for the per-kernel split"""
import os
import sys
import time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "cswin-simam-unet_amd")]   # noqa: E402
import numpy as np
import torch
import csu
from csu import metrics

S, K = 2048, 5
PROF = len(sys.argv) > 1 and sys.argv[1] == "prof"


def ellipse_map(rng, jitter):
    """An ellipse_batch-style label map with all four foreground classes: two ellipses per class."""
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32) + 0.5
    lab = np.zeros((S, S), dtype=np.int64)
    prm = np.random.default_rng(99)
    for i in range(8):
        cy, cx = prm.uniform(0.15, 0.85, size=2) * S + jitter.normal(0, 6.0, size=2)
        ay, ax = prm.uniform(0.05, 0.2, size=2) * S * (1 + jitter.normal(0, 0.03, size=2))
        th = prm.uniform(0.0, np.pi)
        c, s = np.cos(th), np.sin(th)
        u, v = c * (xx - cx) + s * (yy - cy), -s * (xx - cx) + c * (yy - cy)
        lab[(u / ax) ** 2 + (v / ay) ** 2 <= 1.0] = 1 + i % 4
    return lab


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, r


d = torch.device("cuda:0")
target = torch.from_numpy(ellipse_map(None, np.random.default_rng(1)))
pred = torch.from_numpy(ellipse_map(None, np.random.default_rng(2))).to(torch.uint8)     # what the predictor yields
pg, tg = pred.to(d), target.to(d)
fn = lambda: csu.surface_metrics(pg, tg, K, (1.0, 1.0), 2.0)
fn_aniso = lambda: csu.surface_metrics(pg, tg, K, (0.7, 1.3), 2.0)
for _ in range(3):
    fn(); fn_aniso()
if PROF:
    for _ in range(10):
        fn(); fn_aniso()
    csu.distance_transform_edt(pg)
    torch.cuda.synchronize()
    sys.exit(0)
lines = []
out = lambda s: (print(s, flush=True), lines.append(s))
out(f"surface_metrics timing, one {S} x {S} image, K = {K} (4 foreground classes), uint8 prediction, int64 target")
ms, r = timed(fn, 50)
out(f"csu.surface_metrics, spacing (1, 1) [int32 path]      : {ms:8.3f} ms per call (mean of 50 after warm-up)")
ms2, r2 = timed(fn_aniso, 50)
out(f"csu.surface_metrics, spacing (0.7, 1.3) [fp32 path]   : {ms2:8.3f} ms per call (mean of 50 after warm-up)")
out("result (1, 1): " + str(r.cpu().numpy().round(4).tolist()))
L = csu._lib.lib()
out(f"workspace: {L.csu_surface_workspace(1, 4, S, S) / 2**20:.1f} MiB for the 4 classes in one call")
ref_fn = lambda: metrics.reference_surface_metrics(pg, tg, K, (1.0, 1.0), 2.0)
ref_fn()
msr, rr = timed(ref_fn, 2)
out(f"reference_surface_metrics on the GPU (plain torch)    : {msr:8.1f} ms per call (mean of 2)")
out(f"kernels vs GPU reference, max rel diff                : {float(((r - rr).abs() / rr.abs().clamp_min(1e-300)).max()):.3e}")
e_ms, e = timed(lambda: csu.distance_transform_edt(pg), 20)
out(f"csu.distance_transform_edt of the prediction != 0     : {e_ms:8.3f} ms per call (mean of 20)")
try:
    import scipy.ndimage as ndi
except ImportError:
    out("scipy is not installed on the GPU machine: host formulas not measured")
else:
    def host():
        p, t = pg.cpu().numpy(), tg.cpu().numpy()          # the download of the label maps
        st = ndi.generate_binary_structure(2, 1)
        res = []
        for c in range(1, K):
            P, T = p == c, t == c
            bp, bt = P ^ ndi.binary_erosion(P, st), T ^ ndi.binary_erosion(T, st)
            d1, d2 = ndi.distance_transform_edt(~bt)[bp], ndi.distance_transform_edt(~bp)[bt]
            pool = np.concatenate([d1, d2])
            res.append([max(d1.max(), d2.max()), np.percentile(pool, 95), (d1.mean() + d2.mean()) / 2,
                        ((d1 <= 2.0).sum() + (d2 <= 2.0).sum()) / pool.size, bp.sum(), bt.sum()])
        return np.asarray(res, dtype=np.float64)
    host()
    t0 = time.perf_counter()
    for _ in range(3):
        h = host()
    out(f"scipy.ndimage formulas on the host, with the download : {(time.perf_counter() - t0) / 3 * 1e3:8.1f} ms per call (mean of 3)")
    out(f"kernels vs scipy, max abs diff                        : {float(np.abs(r.cpu().numpy()[0] - h).max()):.3e}")
    es = ndi.distance_transform_edt(pred.numpy() != 0)
    out(f"csu.distance_transform_edt vs scipy (fp32 of fp64)     : equal = {bool((e.cpu().numpy() == es.astype(np.float32)).all())}")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
