"""Per-workgroup timeline of the grouped weight-gradient launches (wgrad_group) of one train step:
where the launch time goes between busy CUs and the idle tail behind each CU's last workgroup.
Needs the debug build (make -C cswin-simam-unet_amd/csrc dbg: WG_TIMING start / staged / loop end /
end stamps at 100 MHz plus the XCD and CU each workgroup ran on).

    CSU_LIB_PATH=.../libcsu_hip_dbg.so python tools/wgrad_group_timeline.py [--img 512] [--batch 16]
        [--plan legacy|balanced|both] [--per-cu] [--json OUT]

The list of deferred Linears (M, N, K, in flush order) is recorded from one eager bf16 step of the
bench model; every launch of the chosen plan is then replayed alone on operands of its own (the
stamps are indexed by workgroup id, so one launch at a time), warmed up twice and stamped once.
Per launch: workgroups, span (first start to last end), per XCD the time its last workgroup ended,
the mean busy time of its CUs and the earliest CU to run dry; over all CUs the idle tail
(span - the CU's last end, as a share of CUs x span) and the busy share."""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "cswin-simam-unet_amd")]
os.environ.setdefault("CSU_LIB_PATH", os.path.join(REPO, "cswin-simam-unet_amd", "csu", "_lib", "libcsu_hip_dbg.so"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from csu import _lib, ops  # noqa: E402
from csu._lib import lib  # noqa: E402

PASSES = [(256, 128), (128, 128), (128, 64), (64, 128), (64, 64)]   # csu_linear_wgrad_group's launch order
WGG_MAX = 48


def headline_list(img, batch):
    """(M, N, K) of every Linear the end-of-backward flush groups, in flush order."""
    from csu.model import CSWinTransformer
    from csu.train import bce_loss
    d = torch.device("cuda")
    torch.manual_seed(0)
    model = CSWinTransformer(img_size=img, depth=[1, 2, 9, 1], split_size=[1, 2, 8, 8], simam=True).to(d)
    ops.SIDE_WGRAD = False   # like the captured step
    seen = []
    flush = ops._wgrad_flush

    def spy():
        seen.extend((dy2.shape[0], dy2.shape[1], x2.shape[1]) for dy2, x2, _ in ops._WG_DEFER)
        flush()
    ops._wgrad_flush = spy
    try:
        x = torch.rand(batch, 3, img, img, device=d)
        t = (torch.rand(batch, 1, img, img, device=d) > 0.5).float()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = model(x)
        bce_loss(y, t).backward()
        torch.cuda.synchronize()
    finally:
        ops._wgrad_flush = flush
    del model, x, t, y
    torch.cuda.empty_cache()
    return seen


def legacy_launches(shapes):
    """[(label, [item index], [(tn, tk, chunks, slab bytes)])]: per tile shape, 48 items per launch."""
    L = lib()
    plans = []
    for M, N, K in shapes:
        tn, tk, ch = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        nb = L.csu_linear_wgrad_group_plan(M, N, K, ctypes.byref(tn), ctypes.byref(tk), ctypes.byref(ch))
        plans.append((tn.value, tk.value, ch.value, nb))
    out = []
    for tn, tk in PASSES:
        idx = [i for i, p in enumerate(plans) if p[:2] == (tn, tk)]
        for j in range(0, len(idx), WGG_MAX):
            out.append((f"{tn}x{tk}#{j // WGG_MAX}", idx[j:j + WGG_MAX], plans))
    return out


def balanced_launches(shapes, cus):
    L = lib()
    n = len(shapes)
    items = (_lib.WgradGroupItem * n)(*[_lib.WgradGroupItem(None, None, None, None, M, N, K) for M, N, K in shapes])
    pl = (_lib.WgradGroupPlan * n)()
    assert L.csu_linear_wgrad_group_plan_all(items, n, cus, pl) == 0
    plans = [(p.tn, p.tk, p.chunks, p.slab_bytes) for p in pl]
    out = []
    for la in sorted({p.launch for p in pl}):
        idx = sorted((i for i in range(n) if pl[i].launch == la), key=lambda i: pl[i].pos)
        out.append((f"{pl[idx[0]].tn}x{pl[idx[0]].tk}#{la}", idx, plans))
    return out, pl


def union_busy(iv):
    iv = sorted(iv)
    tot, (a, b) = 0, iv[0]
    for s, e in iv[1:]:
        if s > b:
            tot += b - a
            a, b = s, e
        else:
            b = max(b, e)
    return tot + b - a


def timeline(grid, ncu, per_cu):
    L = lib()
    ts = np.zeros((4, 16384), dtype=np.uint64)
    hw = np.zeros(16384, dtype=np.uint32)
    for name, buf in (("csu_debug_wgrad_ts", ts), ("csu_debug_wgrad_hw", hw)):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p]
        assert fn(buf.ctypes.data) == 0
    n = min(grid, 16384)
    t = ts[:, :n].astype(np.int64)
    t0 = t[0].min()
    start, end = (t[0] - t0) / 100.0, (t[3] - t0) / 100.0
    span = float(end.max())
    xcd, cu = hw[:n] >> 16, (hw[:n] >> 8) & 0xff
    cus = {}
    for i in range(n):
        cus.setdefault((int(xcd[i]), int(cu[i])), []).append((start[i], end[i]))
    last = {k: max(e for _, e in v) for k, v in cus.items()}
    busy = {k: union_busy(v) for k, v in cus.items()}
    idle_tail = (sum(span - v for v in last.values()) + (ncu - len(cus)) * span) / (ncu * span)
    rec = {"workgroups": grid, "span_us": round(span, 1), "cus_used": len(cus),
           "wg_us_p50": round(float(np.median(end - start)), 1), "wg_us_max": round(float((end - start).max()), 1),
           "idle_tail": round(idle_tail, 4), "busy": round(sum(busy.values()) / (ncu * span), 4), "xcd": {}}
    for x in sorted({k[0] for k in cus}):
        ks = [k for k in cus if k[0] == x]
        rec["xcd"][x] = {"cus": len(ks), "workgroups": sum(len(cus[k]) for k in ks),
                         "last_end_us": round(max(last[k] for k in ks), 1), "first_dry_us": round(min(last[k] for k in ks), 1),
                         "mean_busy_us": round(float(np.mean([busy[k] for k in ks])), 1)}
    if per_cu:
        rec["cu"] = {f"{k[0]}.{k[1]}": [len(cus[k]), round(busy[k], 1), round(last[k], 1)] for k in sorted(cus)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--plan", default="legacy", choices=["legacy", "balanced", "both"])
    ap.add_argument("--per-cu", action="store_true", help="also one line per CU: workgroups, busy us, last end us")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    d = torch.device("cuda")
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    shapes = headline_list(a.img, a.batch)
    runs = []
    for s in dict.fromkeys(shapes):
        print(f"  {shapes.count(s):3d} x (M {s[0]}, N {s[1]}, K {s[2]})")
    print(f"{len(shapes)} grouped Linears, {ncu} CUs", flush=True)
    L = lib()
    dys = [torch.randn(M, N, device=d).to(torch.bfloat16) for M, N, K in shapes]
    xs = [torch.randn(M, K, device=d).to(torch.bfloat16) for M, N, K in shapes]
    outs = [torch.empty(N * K + N, device=d) for M, N, K in shapes]
    out = {"img": a.img, "batch": a.batch, "cus": ncu, "shapes": shapes, "plans": {}}
    for mode in (("legacy", "balanced") if a.plan == "both" else (a.plan,)):
        if mode == "legacy":
            launches, pl = legacy_launches(shapes), None
        else:
            launches, pl = balanced_launches(shapes, 0)
        recs = []
        for label, idx, plans in launches:
            slabs = [torch.empty(max(plans[i][3] // 4, 4), device=d) for i in idx]
            its = (_lib.WgradGroupItem * len(idx))(*[
                _lib.WgradGroupItem(dys[i].data_ptr(), xs[i].data_ptr(), outs[i].data_ptr(),
                                    sl.data_ptr() if plans[i][3] else None, *shapes[i]) for i, sl in zip(idx, slabs)])
            if pl is None:
                call = lambda: L.csu_linear_wgrad_group(its, len(idx), torch.cuda.current_stream().cuda_stream)
            else:
                sub = (_lib.WgradGroupPlan * len(idx))(*[pl[i] for i in idx])
                call = lambda: L.csu_linear_wgrad_group_planned(its, sub, len(idx), torch.cuda.current_stream().cuda_stream)
            grid = 0
            for i in idx:
                M, N, K = shapes[i]
                tn, tk, ch, _ = plans[i]
                grid += -(-N // tn) * -(-K // tk) * ch
            for _ in range(3):
                assert call() == 0
            torch.cuda.synchronize()
            rec = timeline(grid, ncu, a.per_cu)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(5):
                call()
            ev[1].record()
            torch.cuda.synchronize()
            rec.update(launch=label, items=len(idx), event_us=round(ev[0].elapsed_time(ev[1]) * 200.0, 1),
                       slab_bytes=int(sum(plans[i][3] for i in idx)))
            recs.append(rec)
            print(f"{mode} {label}: {len(idx)} items, {grid} workgroups ({grid / ncu:.2f} per CU), span {rec['span_us']} us "
                  f"(events {rec['event_us']} us), workgroup p50 {rec['wg_us_p50']} max {rec['wg_us_max']} us, "
                  f"{rec['cus_used']} CUs used, busy {rec['busy']:.1%}, idle tail {rec['idle_tail']:.1%}, "
                  f"slabs {rec['slab_bytes'] / 2**20:.1f} MiB")
            for x, r in rec["xcd"].items():
                print(f"    XCD {x}: {r['cus']} CUs, {r['workgroups']} workgroups, last end {r['last_end_us']} us, "
                      f"first CU dry at {r['first_dry_us']} us, mean busy {r['mean_busy_us']} us")
            if a.per_cu:
                for k, (nw, b, le) in rec["cu"].items():
                    print(f"      CU {k}: {nw} workgroups, busy {b} us, last end {le} us")
            sys.stdout.flush()
            del slabs
        tot = sum(r["span_us"] for r in recs)
        tail = sum(r["span_us"] * r["idle_tail"] for r in recs) / tot
        print(f"{mode}: {len(recs)} launches, {tot:.1f} us of spans, idle tail {tail:.1%} of CU time", flush=True)
        out["plans"][mode] = recs
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
