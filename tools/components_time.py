"""Timing of csu.connected_components and csu.postprocess_labels on one 2048 x 2048 five-class ellipse map
(the workload of tools/surface_metrics_time.py) and on the same map with 2 % salt noise (many small
components): the kernels (csrc/components.hip), the same work with scipy.ndimage on the host (download
and upload included) when scipy is installed, and the numpy reference called on the GPU tensor.
    python tools/components_time.py [out.txt]    host clock around calls that end in a device synchronise
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/components_time.py prof
                                                 13 calls of each on the salted map, for the per-kernel split"""
import os
import sys
import time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "cswin-simam-unet_amd")]   # noqa: E402
import numpy as np
import torch
import csu
from csu.ledger import HBM_GBS

S, K = 2048, 5
RULES = dict(keep_largest=True, min_size=64, fill_holes=True)
PROF = len(sys.argv) > 1 and sys.argv[1] == "prof"


def ellipse_map(jitter):
    """tools/surface_metrics_time.py's map: two ellipses per foreground class."""
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32) + 0.5
    lab = np.zeros((S, S), dtype=np.uint8)
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


def host_label(x):
    """What a user does today for the components: download, scipy per class, upload."""
    import scipy.ndimage as ndi
    p = x.cpu().numpy()
    comp, n = np.zeros(p.shape, np.int32), 0
    for c in range(1, K):
        lab, k = ndi.label(p == c, structure=np.ones((3, 3)))
        comp[lab > 0] = lab[lab > 0] + n
        n += k
    return torch.from_numpy(comp).to(x.device), n


def host_postprocess(x):
    """... and for the rules: fill, drop below 64 pixels, keep the largest, class by class."""
    import scipy.ndimage as ndi
    p = x.cpu().numpy()
    out = np.zeros_like(p)
    for c in range(1, K):
        m = ndi.binary_fill_holes(p == c)
        lab, k = ndi.label(m, structure=np.ones((3, 3)))
        if k == 0:
            continue
        sizes = np.bincount(lab.ravel(), minlength=k + 1)
        sizes[0] = 0
        best = int(np.argmax(sizes))
        if sizes[best] >= RULES["min_size"]:
            out[lab == best] = c
    return torch.from_numpy(out).to(x.device)


d = torch.device("cuda:0")
clean = ellipse_map(np.random.default_rng(2))
rng = np.random.default_rng(3)
salted = clean.copy()
hit = rng.random(clean.shape) < 0.02
salted[hit] = rng.integers(0, K, size=int(hit.sum()))
maps = {"ellipses": torch.from_numpy(clean).to(d), "ellipses + 2 % salt": torch.from_numpy(salted).to(d)}
ccl = lambda x: csu.connected_components(x, 8)
ccl_area = lambda x: csu.connected_components(x, 8, return_areas=True)
post = lambda x: csu.postprocess_labels(x, K, **RULES)
for x in maps.values():
    for _ in range(3):
        ccl(x); ccl_area(x); post(x)
if PROF:
    x = maps["ellipses + 2 % salt"]
    for _ in range(10):
        ccl_area(x); post(x)
    torch.cuda.synchronize()
    sys.exit(0)
lines = []
out = lambda s: (print(s, flush=True), lines.append(s))
px = S * S
out(f"connected components and post-processing, one {S} x {S} uint8 label map, K = {K}, connectivity 8; rules: keep the largest "
    f"component of every class, min_size {RULES['min_size']}, fill holes")
out(f"least bytes: components read 1 B and write comp 4 B per pixel = {5 * px / 1e6:.1f} MB (+ area: {9 * px / 1e6:.1f} MB); "
    f"post-processing reads and writes 1 B per pixel = {2 * px / 1e6:.1f} MB; HBM peak {HBM_GBS / 1e3:.0f} TB/s")
L = csu._lib.lib()
out(f"workspace: csu_ccl {L.csu_ccl_workspace(1, S, S) / 2**20:.1f} MiB, csu_cc_filter {L.csu_cc_filter_workspace(1, S, S) / 2**20:.1f} MiB")
for name, x in maps.items():
    comp, count = ccl(x)
    out(f"--- {name}: {int(count)} foreground components")
    for what, fn, nbytes in (("csu.connected_components (comp, count)", ccl, 5 * px), ("csu.connected_components (+ area)", ccl_area, 9 * px),
                             ("csu.postprocess_labels", post, 2 * px)):
        ms, _ = timed(lambda: fn(x), 50)
        out(f"{what:<48}: {ms:8.3f} ms per call (mean of 50 after warm-up) = {nbytes / ms / 1e6:7.1f} GB/s of least bytes, "
            f"{nbytes / ms / 1e6 / HBM_GBS * 100:5.2f} % of the HBM rate")
    cleaned = post(x)
    t0 = time.perf_counter()
    rc = csu.reference_connected_components(x, 8, return_areas=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    rp = csu.reference_postprocess_labels(x, K, **RULES)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out(f"{'numpy reference on the GPU tensor, components':<48}: {(t1 - t0) * 1e3:8.1f} ms (once)")
    out(f"{'numpy reference on the GPU tensor, rules':<48}: {(t2 - t1) * 1e3:8.1f} ms (once)")
    got = ccl_area(x)
    out(f"kernels equal the reference: components {all(torch.equal(a, b) for a, b in zip(got, rc))}, rules {torch.equal(cleaned, rp)}")
    try:
        import scipy.ndimage  # noqa: F401
    except ImportError:
        out("scipy is not installed on the GPU machine: the host path was not measured")
        continue
    host_label(x); host_postprocess(x)
    hl, (hc, hn) = timed(lambda: host_label(x), 3)
    hp, hout = timed(lambda: host_postprocess(x), 3)
    out(f"{'scipy.ndimage.label per class on the host':<48}: {hl:8.1f} ms per call (mean of 3, download and upload included)")
    out(f"{'scipy fill / size / largest per class on the host':<48}: {hp:8.1f} ms per call (mean of 3, download and upload included)")
    out(f"host count {hn} (kernels {int(count)}); host rules equal the kernels': {torch.equal(hout, cleaned)} "
        "(the per-class host form fills a hole inside one class only: it differs where a hole borders two classes)")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
