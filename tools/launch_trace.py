"""Launch-and-bits trace of three eager train steps, to compare two builds of csu.ops kernel for
kernel (profiles/README.md, "ops_dedup_trace"):
    python tools/launch_trace.py <a|b|c|d|e|f> DIR     one configuration, one process -> DIR/<cfg>.json
    python tools/launch_trace.py summary DIR OUT.json  the committed digest of DIR's traces
    python tools/launch_trace.py compare PARENT1 PARENT2 NEW
Configurations (CSWinTransformer(img_size=128, split_size=[1, 2, 4, 4]), torch.manual_seed(0), one
ellipse_batch(default_rng(1), 4, 128)):
  a  bf16 autocast, ops.SIDE_WGRAD = False      d  fp32, no autocast
  b  bf16, side-stream weight gradients         e  bf16, dropout / attention dropout / DropPath 0.1
  c  bf16 after set_weight_format('fp8_e4m3')   f  a with the LayerNorm / Mlp fusions switched off
Steps 0 and 1 start from zero_grad(set_to_none=True) (deferred / late gradients), step 2 keeps the
gradients in place (every op's inline branch).  Per step: the ordered launches of
KernelLedger(repeat=1) as (kernel, tag, flops, bytes), the loss bits and a SHA-256 per parameter
gradient.  ``compare`` takes three trace directories: the launch lists of NEW must equal PARENT1's
entry for entry; loss and gradient bits too wherever PARENT1 and PARENT2 (two runs of one build)
agree bitwise.  Exit status 1 on a mismatch, after printing the first differing launch."""
import hashlib
import json
import os
import sys

CONFIGS = "abcdef"
UNFUSED = ("CSU_FUSE_LN_QKV", "CSU_FUSE_LN_MLP", "CSU_FUSE_PROJ_LN", "CSU_MLP64_FUSED_WGRAD")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sha(obj) -> str:
    return hashlib.sha256(json.dumps(obj, separators=(",", ":")).encode()).hexdigest()


def run(cfg: str, out_dir: str) -> int:
    if cfg == "f":   # read when csu.ops is imported
        os.environ.update({k: "0" for k in UNFUSED})
    sys.path.insert(0, os.path.join(ROOT, "cswin-simam-unet_amd"))
    import numpy as np
    import torch

    from csu import ops
    from csu.data import ellipse_batch
    from csu.ledger import KernelLedger
    from csu.model import CSWinTransformer
    from csu.train import bce_loss, make_optimizer

    d = torch.device("cuda:0")
    torch.manual_seed(0)
    drop = 0.1 if cfg == "e" else 0.0
    model = CSWinTransformer(img_size=128, split_size=[1, 2, 4, 4], drop_rate=drop, attn_drop_rate=drop,
                             drop_path_rate=drop).to(d)
    if cfg == "c":
        model.set_weight_format("fp8_e4m3")
    if cfg != "b":
        ops.SIDE_WGRAD = False
    opt = make_optimizer(model)
    x, t = (v.to(d) for v in ellipse_batch(np.random.default_rng(1), 4, 128))
    steps = []
    for i in range(3):
        if i < 2:
            opt.zero_grad(set_to_none=True)
        led = KernelLedger(repeat=1)
        with led:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=cfg != "d"):
                y = model(x)
            loss = bce_loss(y, t)
            loss.backward()
            grads = {n: hashlib.sha256(p.grad.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
                     for n, p in model.named_parameters() if p.grad is not None}
            opt.step()
        launches = [(r["kernel"], r["tag"], r["flops"], r["bytes"]) for r in led.launches()]
        steps.append({"launches": launches, "loss_bits": "%08x" % (loss.detach().float().view(torch.int32).item() & 0xffffffff),
                      "grads": grads})
    if cfg == "a":   # the trace must reach the fused LayerNorm-backward paths to mean anything
        seen = steps[0]["launches"]
        need = {"a launch tagged :lnbwd:ws": any(":lnbwd:ws" in r[1] for r in seen),
                "an mlp_bwd tagged lnbwd": any(r[0] == "mlp_bwd" and "lnbwd" in r[1] for r in seen),
                "a gemm tagged rbln:ws": any(r[0] == "gemm" and "rbln:ws" in r[1] for r in seen)}
        if not all(need.values()):
            print("config a does not reach:", [k for k, v in need.items() if not v], flush=True)
            return 1
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, cfg + ".json"), "w") as f:
        json.dump({"config": cfg, "steps": steps}, f)
    print(cfg, [(len(s["launches"]), s["loss_bits"]) for s in steps], flush=True)
    return 0


def _load(d: str) -> dict:
    out = {}
    for cfg in CONFIGS:
        p = os.path.join(d, cfg + ".json")
        if os.path.exists(p):
            with open(p) as f:
                out[cfg] = json.load(f)["steps"]
    return out


def summary(d: str, out: str) -> int:
    dig = {cfg: [{"launches": len(s["launches"]), "launch_sha256": _sha(s["launches"]), "loss_bits": s["loss_bits"],
                  "grad_sha256": _sha(sorted(s["grads"].items()))} for s in steps] for cfg, steps in _load(d).items()}
    with open(out, "w") as f:
        json.dump(dig, f, indent=1)
        f.write("\n")
    return 0


def _bits(step: dict):
    return step["loss_bits"], step["grads"]


def compare(p1: str, p2: str, new: str) -> int:
    a, b, c = _load(p1), _load(p2), _load(new)
    bad = 0
    for cfg in CONFIGS:
        if cfg not in a or cfg not in b or cfg not in c:
            print(f"{cfg}: missing from {[n for n, t in ((p1, a), (p2, b), (new, c)) if cfg not in t]}")
            bad += 1
            continue
        for i, (sa, sb, sc) in enumerate(zip(a[cfg], b[cfg], c[cfg])):
            repro = _bits(sa) == _bits(sb)
            la, lc = [tuple(r) for r in sa["launches"]], [tuple(r) for r in sc["launches"]]
            same_l = la == lc
            if not same_l:
                k = next((k for k, (u, v) in enumerate(zip(la, lc)) if u != v), min(len(la), len(lc)))
                print(f"{cfg} step {i}: launch {k} differs: parent {la[k] if k < len(la) else None} "
                      f"new {lc[k] if k < len(lc) else None} ({len(la)} vs {len(lc)} launches)")
            same_b = _bits(sa) == _bits(sc)
            if repro and not same_b:
                diff = [n for n in sa["grads"] if sa["grads"][n] != sc["grads"].get(n)]
                print(f"{cfg} step {i}: loss {sa['loss_bits']} vs {sc['loss_bits']}, {len(diff)} gradients differ {diff[:4]}")
            bad += (not same_l) + (repro and not same_b)
            print(f"{cfg} step {i}: {len(la)} launches {'same' if same_l else 'DIFFER'}; parent "
                  f"{'reproduces bitwise' if repro else 'does NOT reproduce bitwise (launch list only)'}; "
                  f"bits {'same' if same_b else 'differ'}")
    print("MISMATCH" if bad else "OK")
    return 1 if bad else 0


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) == 2 and a[0] in CONFIGS:
        sys.exit(run(a[0], a[1]))
    if len(a) == 3 and a[0] == "summary":
        sys.exit(summary(a[1], a[2]))
    if len(a) == 4 and a[0] == "compare":
        sys.exit(compare(*a[1:]))
    sys.exit(__doc__)
