"""Cases of the convolution launch-plan tests (tests/test_gpu_conv_plans.py runs them on the GPU,
tests/test_conv_plans.py checks their plans, and the models' plans, through csu_conv2d_plan; nothing
here needs a GPU).

The persistent LDS-DMA convolutions (igemm_dma in 12 tile configurations, conv3_halo64, conv3_c16,
conv3_c16d) launch a fixed grid of 1 or 2 workgroups per CU and walk their tiles as one stream through
a ring.  At test sizes that grid gives a workgroup one tile at most, so the logic that only matters
from the second tile on never runs.  csu_conv2d_ex2's `wgs` shrinks the grid to 8 or 16 workgroups,
which walk a few dozen tiles of a shape of a few thousand rows.

STEADY_CASES     every igemm_dma configuration x {3x3 (nk 9), 1x1 (nk 1), 1x1 over 320 channels (nk 5)}
                 x {forward, input gradient}, forced, at grids 8 / 16 / default
STRIDE2_CASES    stride-2 input gradients on odd sizes (four phases of 1, 2, 2, 4 taps)
SPLIT_CASES      the two-source form under the configurations the split entries can select
ITEM_CASES       conv3_halo64 (cfg 20) and conv3_c16 / conv3_c16d (cfg 21)
EQUAL_CASES      grids under which every workgroup owns the same number (>= 2) of tiles
AUTO_CASES       plans selected by shape alone, run through ops.conv2d / conv2d_cat / conv_transpose2d
"""
import functools
import math

import torch
import torch.nn.functional as F

BF16, F32 = torch.bfloat16, torch.float32
WGS = (8, 16, 0)            # persistent grids every forced case runs under (0: the product grid)
HALO64_CFG, C16_CFG = 20, 21

# csrc/conv.hip kIDCfgs: cfg (1 + k) -> (BM, BN, ring stages S)
IGEMM_DMA = {1: (128, 128, 3), 2: (256, 128, 2), 3: (256, 128, 3), 4: (128, 64, 4), 5: (256, 64, 3), 6: (128, 64, 3),
             7: (256, 256, 2), 8: (256, 256, 2), 9: (512, 64, 2), 10: (64, 64, 4), 11: (128, 64, 3), 12: (64, 128, 3)}
# output columns and image side of each configuration's steady-state shape (B = 1): M = 1369 rows for
# the 64- and 128-row tiles, 2209 for the 256- and 512-row ones -- 18 to 44 tiles, never a multiple of 8,
# a partial last M tile, 2 to 4 N tiles per M tile
STEADY_N = {1: 256, 2: 256, 3: 256, 4: 128, 5: 128, 6: 128, 7: 512, 8: 512, 9: 256, 10: 128, 11: 128, 12: 256}
STEADY_H = {1: 37, 2: 47, 3: 47, 4: 37, 5: 47, 6: 37, 7: 47, 8: 47, 9: 47, 10: 37, 11: 37, 12: 37}
STEADY_KINDS = {"k3": (3, 64), "k1": (1, 64), "k1c320": (1, 320)}   # kernel size, gathered channels: nk 9, 1, 5
STEADY_NMAX = 512
STEADY_CASES = [(kind, op, cfg) for kind in STEADY_KINDS for op in (0, 1) for cfg in IGEMM_DMA]

# (B, H, W, C, N, k, pad): dx (B, H, W, C) of a stride-2 conv, gathered channels N = 64.  3x3 / pad 1 on odd
# sizes: four phases of 1, 2, 2, 4 taps and different row counts ("thin": 64 to 102 rows each).  2x2 / pad 0
# (ConvTranspose2d(2, 2), the UNet Up): four equal phases of 16 tiles ("up_equal", every workgroup of 8 owns
# two) or 18 ("up_ragged"), under the two configurations the UNet sizes select
STRIDE2_GEOMS = {"square": (2, 37, 37, 256, 64, 3, 1), "thin": (2, 33, 5, 128, 64, 3, 1),
                 "up_equal": (2, 64, 64, 512, 64, 2, 0), "up_ragged": (2, 66, 66, 512, 64, 2, 0)}
STRIDE2_CASES = [(name, cfg) for name, g in STRIDE2_GEOMS.items() for cfg, (_, bn, _) in IGEMM_DMA.items()
                 if g[3] % bn == 0 and (g[5] == 3 or cfg in (3, 8))]

# two sources (forward) / two destinations (input gradient): 3x3 / stride 1 / pad 1, 64 + 192 channels.
# The split entries launch with cfg -1 and one problem: id_pick(single) can return 7, 2 or 11 (cfg 8, 3,
# 12), else the v2 kernel (cfg 0)
SPLIT_GEOM = (1, 37, 64, 256, 256)
SPLIT_AT = 64
SPLIT_CASES = [(op, cfg) for op in (0, 1) for cfg in (8, 3, 12, 0, -1)]
# the same with 16 (cfg 8) or 32 (cfg 3) tiles: every workgroup of 8 owns the same number.  64 + 64 gathered
# channels (forward), 64 + 192 output channels (input gradient)
SPLIT_EQUAL_GEOM = {0: (1, 64, 64, 128, 256), 1: (1, 64, 64, 256, 128)}
SPLIT_EQUAL_CASES = [(op, cfg) for op in (0, 1) for cfg in (8, 3)]

# conv3_halo64: items of two rows x 64 pixels, 7 row pairs x 2 segments per image, 42 items: XCD ranges of
# 5 or 6 items cross the image boundaries at 14 and 28.  conv3_c16 / c16d: one row x 64 pixels, same count
ITEM_GEOMS = {HALO64_CFG: (3, 14, 128, 64, 64), C16_CFG: (3, 7, 128, 16, 144)}
ITEM_CASES = [(cfg, op) for cfg in ITEM_GEOMS for op in (0, 1)]

# every workgroup the same count >= 2: (op, (B, H, W, C, N, k), cfg, wgs)
EQUAL_CASES = [
    (0, (1, 64, 32, 64, 512, 1), 8, 8),       # 16 tiles of 256 x 256 on 8 workgroups
    (0, (1, 64, 32, 64, 256, 1), 3, 8),       # 16 tiles of 256 x 128
    (0, (1, 32, 32, 64, 128, 1), 12, 8),      # 16 tiles of 64 x 128
    (1, (1, 64, 32, 512, 64, 1), 8, 8),
    (1, (1, 64, 32, 256, 64, 1), 3, 8),
    (0, (2, 16, 64, 64, 64, 3), HALO64_CFG, 8),    # 16 items
    (1, (2, 16, 64, 64, 64, 3), HALO64_CFG, 8),
    (0, (2, 8, 64, 16, 144, 3), C16_CFG, 8),       # 16 items
    (1, (2, 8, 64, 16, 144, 3), C16_CFG, 8),
]

# plans chosen by shape alone (cfg -1, default grid), through csu.ops under autocast:
# name -> (entry, dtype, (B, H, W, C, N, k, stride, pad) of the conv [conv_transpose2d: of the matching conv], note)
AUTO_CASES = {
    "pick7": ("conv2d", BF16, (1, 127, 127, 64, 1024, 1, 1, 0)),      # 64 x 4 tiles of 256 x 256 >= 256 CUs
    "pick2": ("conv2d", BF16, (1, 115, 115, 64, 640, 1, 1, 0)),       # 52 x 5 tiles of 256 x 128
    "pick11": ("conv2d", BF16, (1, 58, 58, 64, 640, 1, 1, 0)),        # 53 x 5 tiles of 64 x 128, one problem
    "v2_phase": ("conv2d", BF16, (1, 229, 229, 640, 64, 1, 2, 0)),    # dgrad: phase (0, 0) picks 2, the tapless phases none
    "ksplit0": ("conv2d", BF16, (1, 16, 16, 128, 36, 3, 1, 1)),       # exact_inputs.CONV_KSPLIT_CASES
    "ksplit1": ("conv2d", BF16, (1, 32, 32, 64, 36, 3, 1, 1)),
    "ksplit_dgrad": ("conv2d", BF16, (1, 37, 37, 64, 256, 3, 1, 1)),  # forward 3 parts, input gradient 8
    "wd_halo128": ("conv2d", BF16, (1, 37, 64, 64, 128, 3, 1, 1)),    # 37 segments: chunks of 13, 13, 11
    "wd_halo64": ("conv2d", BF16, (1, 37, 64, 64, 64, 3, 1, 1)),
    "wd_3": ("conv2d", BF16, (1, 37, 37, 64, 256, 1, 1, 0)),          # 1369 rows: chunks of 704 + 665
    "wd_3_one": ("conv2d", BF16, (1, 20, 20, 64, 256, 1, 1, 0)),      # one chunk
    "wd_2": ("conv2d", BF16, (1, 37, 37, 64, 128, 3, 1, 1)),
    "wd_v2": ("conv2d", BF16, (1, 37, 37, 64, 64, 3, 1, 1)),          # 6 chunks of 256 rows, the last 89
    "halo64": ("conv2d", BF16, (2, 6, 128, 64, 64, 3, 1, 1)),
    "c16": ("conv2d", BF16, (1, 8, 128, 16, 144, 3, 1, 1)),
    "narrow": ("conv2d", BF16, (2, 20, 20, 64, 1, 1, 1, 0)),          # the UNet head: 256 x 32 tiles, scalar input gradient
    "embed": ("conv2d", BF16, (2, 32, 32, 3, 64, 7, 4, 2)),           # patch embed: channels padded to 8
    "embed_f32": ("conv2d", F32, (2, 32, 32, 3, 64, 7, 4, 2)),
    "merge": ("conv2d", BF16, (2, 17, 17, 64, 128, 3, 2, 1)),
    "merge_f32": ("conv2d", F32, (1, 9, 9, 64, 128, 3, 2, 1)),
    "carafe_enc": ("conv2d", BF16, (1, 16, 16, 128, 36, 3, 1, 1)),
    "enc32": ("conv2d", BF16, (1, 16, 16, 32, 36, 3, 1, 1)),          # input gradient: 256 x 32 tiles, 4-wide gathers, K split
    "enc32_k1": ("conv2d", BF16, (1, 20, 20, 32, 36, 1, 1, 0)),       # the same without a K split (one K slice)
    "enc64_k1": ("conv2d", BF16, (1, 20, 20, 64, 36, 1, 1, 0)),       # 128 x 64 tiles, 4-wide gathers, no K split
    "v2_k1": ("conv2d", BF16, (1, 20, 20, 64, 128, 1, 1, 0)),         # input gradient: 128 x 64 tiles, 8-wide, no K split
    "f32_3x3": ("conv2d", F32, (1, 20, 20, 16, 144, 3, 1, 1)),        # weight gradient in two chunks
    "f32_head": ("conv2d", F32, (1, 12, 12, 64, 1, 1, 1, 0)),
    "cat": ("conv2d_cat", BF16, (1, 37, 64, 256, 256, 3, 1, 1)),      # 64 + 192 channels, never concatenated
    "cat64": ("conv2d_cat", BF16, (1, 37, 64, 128, 64, 3, 1, 1)),     # 64 + 64 channels, 64-column halo weight gradient
    "cat_f32": ("conv2d_cat", F32, (1, 10, 10, 128, 64, 3, 1, 1)),    # materialised concatenation
    "convT": ("conv_transpose2d", BF16, (1, 38, 38, 64, 128, 2, 2, 0)),   # 128 -> 64 channels, 19 x 19 -> 38 x 38
    "convT_f32": ("conv_transpose2d", F32, (1, 12, 12, 16, 32, 2, 2, 0)),
}
AUTO_SPLIT = {"cat": 64, "cat64": 64, "cat_f32": 64}


def geom(B, H, W, C, N, k, stride=1, pad=None):
    from csu import ops
    return ops._conv_geom(B, H, W, C, N, k, k, stride, k // 2 if pad is None else pad)


def plan(op, g, dtype=BF16, cfg=-1, wgs=0, c_split=0, ws_bytes=None):
    from csu import ops
    return ops.conv_plan(op, g, dtype, cfg, wgs, c_split, ws_bytes)


def phases(p):
    return range(min(p.n_problems, 16))


def describe(p):
    if p.family == 6:
        return f"wgrad pick {p.wgrad_pick} v2 kernel {p.wgrad_v2} chunks {p.wgrad_chunks} x {p.wgrad_rpc} (last {p.wgrad_last})"
    ph = "; ".join(f"cfg {p.phase_cfg[i]} rows {p.phase_rows[i]} tiles {p.phase_tiles[i]} nk {p.phase_nk[i]} grid "
                   f"{p.phase_grid[i]} per-wg {p.phase_tiles_min[i]}..{p.phase_tiles_max[i]} idle {p.phase_idle[i]}"
                   for i in phases(p))
    return f"family {p.family} ksplit {p.ksplit} [{ph}]"


def bucket(p):
    """Tiles per workgroup: 0 = at most one, 1 = at least two and all equal, 2 = at least two, unequal."""
    return 0 if p.wg_tiles_max <= 1 else (1 if p.wg_tiles_max == p.wg_tiles_min else 2)


def plan_class(op, p, dtype):
    """What a GPU case has to share with a model's launch to stand for it."""
    dt = "bf16" if dtype == BF16 else "f32"
    if op == 2:
        return ("wgrad", dt, p.wgrad_pick, p.wgrad_v2, bool(p.two_source), p.wgrad_chunks > 1)
    return (("fwd", "dgrad")[op], dt, p.family, tuple(p.phase_cfg[i] for i in phases(p)), p.n_problems,
            bool(p.two_source), p.ksplit > 1, p.v2_bn, p.v2_vw, p.gemm_vec, bucket(p))


# ---------------------------------------------------------------------------------------------
# geometries of the forced cases
# ---------------------------------------------------------------------------------------------
def steady_geom(kind, op, cfg):
    k, gath = STEADY_KINDS[kind]
    h, n = STEADY_H[cfg], STEADY_N[cfg]
    return geom(1, h, h, gath, n, k) if op == 0 else geom(1, h, h, n, gath, k)


def stride2_geom(name):
    B, H, W, C, N, k, pad = STRIDE2_GEOMS[name]
    return geom(B, H, W, C, N, k, 2, pad)


def split_equal_geom(op):
    B, H, W, C, N = SPLIT_EQUAL_GEOM[op]
    return geom(B, H, W, C, N, 3)


def split_geom():
    B, H, W, C, N = SPLIT_GEOM
    return geom(B, H, W, C, N, 3)


def item_geom(cfg):
    B, H, W, C, N = ITEM_GEOMS[cfg]
    return geom(B, H, W, C, N, 3)


def equal_geom(case):
    B, H, W, C, N, k = case[1]
    return geom(B, H, W, C, N, k)


def check_steady(kind, op, cfg):
    """The conditions the steady-state shapes exist for, from the plans.  Returns {wgs: plan}."""
    g = steady_geom(kind, op, cfg)
    bm, bn, S = IGEMM_DMA[cfg]
    ps = {w: plan(op, g, BF16, cfg, w) for w in WGS}
    for w, p in ps.items():
        assert p.family == 2 and p.n_problems == 1 and p.phase_cfg[0] == cfg, (cfg, w, describe(p))
        assert (p.phase_bm[0], p.phase_bn[0], p.phase_ring[0]) == (bm, bn, S)
        assert p.phase_grid[0] == (w if w else p.cus * (2 if cfg >= 10 else 1))
    p8, p16, p0 = ps[8], ps[16], ps[0]
    T, M = p8.phase_tiles[0], p8.phase_rows[0]
    ncols = g.N if op == 0 else g.C
    assert T == -(-M // bm) * (ncols // bn)
    assert p8.wg_tiles_max >= 3, describe(p8)                                  # a stream of >= 3 tiles
    assert p8.wg_tiles_max != p8.wg_tiles_min and p16.wg_tiles_max != p16.wg_tiles_min   # unequal counts
    assert p0.wgs_idle > 0 and p0.wg_tiles_min == 0                            # some workgroup owns none
    assert T % 8 != 0 and p8.phase_xcd_rem[0] == T % 8                         # XCD remainder
    assert M % bm != 0 and M > bm                                              # partial last M tile, several M tiles
    assert ncols // bn >= 2                                                    # N tiles of one M tile
    nk = p8.phase_nk[0]
    assert nk == {"k3": 9, "k1": 1, "k1c320": 5}[kind]
    if kind == "k1c320":
        assert nk > S and nk % S != 0
    return ps


def check_stride2(name, cfg):
    g = stride2_geom(name)
    ps = {w: plan(1, g, BF16, cfg, w) for w in WGS}
    for p in ps.values():
        assert p.family == 2 and p.n_problems == 4 and [p.phase_cfg[i] for i in range(4)] == [cfg] * 4
        if STRIDE2_GEOMS[name][5] == 3:
            assert sorted(p.phase_nk[i] for i in range(4)) == [1, 2, 2, 4]     # 1, 2, 2 and 4 taps of 64 channels
            assert len({p.phase_rows[i] for i in range(4)}) >= 3
    if name == "thin":
        assert min(ps[8].phase_rows[i] for i in range(4)) == 64                # one tile or less
    if name == "up_equal":
        assert bucket(ps[8]) == 1 and ps[8].wgs_idle == 0
    if name == "up_ragged":
        assert bucket(ps[8]) == 2 and ps[8].wg_tiles_max >= 3 and ps[8].phase_xcd_rem[0]
    return ps


def check_split_equal(op, cfg):
    p = plan(op, split_equal_geom(op), BF16, cfg, 8, SPLIT_AT)
    assert p.two_source == SPLIT_AT and p.phase_cfg[0] == cfg and bucket(p) == 1 and p.wgs_idle == 0, describe(p)
    return p


def check_split(op, cfg):
    g = split_geom()
    ps = {w: plan(op, g, BF16, cfg, w, SPLIT_AT) for w in WGS}
    for p in ps.values():
        assert p.two_source == SPLIT_AT and p.n_problems == 1
        assert p.phase_cfg[0] == (0 if cfg < 0 else cfg), describe(p)          # this shape's own choice is v2
    if cfg > 0:
        assert ps[8].wg_tiles_max >= 2 and ps[8].wg_tiles_max != ps[8].wg_tiles_min and ps[8].phase_xcd_rem[0]
    return ps


def check_item(cfg, op):
    g = item_geom(cfg)
    ps = {w: plan(op, g, BF16, cfg, w) for w in WGS}
    fam = 3 if cfg == HALO64_CFG else (4 if op == 0 else 5)
    for p in ps.values():
        assert p.family == fam and p.phase_cfg[0] == cfg and p.phase_tiles[0] == 42, describe(p)
    assert (ps[8].wg_tiles_max, ps[8].wg_tiles_min) == (6, 5) and (ps[16].wg_tiles_max, ps[16].wg_tiles_min) == (3, 2)
    assert ps[0].wgs_idle > 0 and ps[8].phase_xcd_rem[0] == 2
    # an image boundary inside one workgroup's item range (grid 8: a workgroup owns its XCD's whole range)
    per_image = ps[8].phase_tiles[0] // g.B
    assert ps[8].phase_tiles[0] == g.B * per_image
    assert any(lo < b < lo + cnt for lo, cnt in xcd_ranges(ps[8].phase_tiles[0]) for b in range(per_image, g.B * per_image, per_image))
    for w in (8, 16):      # the plan's per-workgroup counts are those of the kernels' ranges
        c = workgroup_counts(ps[w].phase_tiles[0], ps[w].phase_grid[0])
        assert (max(c), min(c), c.count(0)) == (ps[w].phase_tiles_max[0], ps[w].phase_tiles_min[0], ps[w].phase_idle[0])
    return ps


def xcd_ranges(tiles):
    """(first tile, count) of each of the 8 XCDs' contiguous ranges, as the persistent kernels divide them."""
    q, rem = divmod(tiles, 8)
    return [(x * (q + 1) if x < rem else rem * (q + 1) + (x - rem) * q, q + (x < rem)) for x in range(8)]


def workgroup_counts(tiles, grid):
    """Tiles of every workgroup: workgroup kk of an XCD takes every nloc-th tile of the XCD's range."""
    nloc = grid // 8
    return [len(range(kk, cnt, nloc)) for _, cnt in xcd_ranges(tiles) for kk in range(nloc)]


def operand_bytes(g, dtype):
    """Largest activation operand of a convolution, in bytes."""
    return max(g.B * g.H * g.W * g.C, g.B * g.OH * g.OW * g.N) * (2 if dtype == BF16 else 4)


def check_equal(case):
    op, _, cfg, wgs = case
    p = plan(op, equal_geom(case), BF16, cfg, wgs)
    assert p.phase_cfg[0] == cfg and p.wg_tiles_max == p.wg_tiles_min == 2 and p.wgs_idle == 0, describe(p)
    return p


# ---------------------------------------------------------------------------------------------
# inputs and fp64 references (computed once per process, never modified)
# ---------------------------------------------------------------------------------------------
def _seed(*key):
    s = 17
    for ch in "/".join(str(k) for k in key):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def conv_reference(op, B, H, W, C, N, k, stride, pad, key):
    """bf16 operands and the fp64 result of one forward (op 0) or input gradient (op 1) of the conv
    (B, H, W, C) -> N channels.  Returns dict(src, w [torch (N, C, k, k)], bias, ref [NHWC fp64])."""
    g = _seed(key, op, B, H, W, C, N, k, stride, pad)
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    w = (torch.randn(N, C, k, k, generator=g) / math.sqrt((C if op == 0 else N) * k * k)).bfloat16()
    if op == 0:
        src = torch.randn(B, H, W, C, generator=g).bfloat16()
        bias = torch.randn(N, generator=g)
        ref = F.conv2d(src.double().permute(0, 3, 1, 2), w.double(), bias.double(), stride, pad).permute(0, 2, 3, 1)
    else:
        src = torch.randn(B, OH, OW, N, generator=g).bfloat16()
        bias = torch.randn(C, generator=g)
        op_h, op_w = H - ((OH - 1) * stride - 2 * pad + k), W - ((OW - 1) * stride - 2 * pad + k)
        ref = F.conv_transpose2d(src.double().permute(0, 3, 1, 2), w.double(), bias.double(), stride, pad,
                                 output_padding=(op_h, op_w)).permute(0, 2, 3, 1)
    return dict(src=src, w=w, bias=bias, ref=ref.contiguous())


@functools.lru_cache(maxsize=None)
def steady_reference(kind, op, h):
    """One reference per (kind, op, image side) at STEADY_NMAX output columns: a configuration with fewer
    columns uses the leading ones (a conv's output channels are independent of one another)."""
    k, gath = STEADY_KINDS[kind]
    if op == 0:
        return conv_reference(0, 1, h, h, gath, STEADY_NMAX, k, 1, k // 2, "steady")
    return conv_reference(1, 1, h, h, STEADY_NMAX, gath, k, 1, k // 2, "steady")


def steady_inputs(kind, op, cfg):
    r = steady_reference(kind, op, STEADY_H[cfg])
    n = STEADY_N[cfg]
    w = r["w"][:n] if op == 0 else r["w"][:, :n]
    return dict(src=r["src"], w=w.contiguous(), bias=r["bias"][:n].contiguous(), ref=r["ref"][..., :n].contiguous())


@functools.lru_cache(maxsize=None)
def stride2_reference(name):
    B, H, W, C, N, k, pad = STRIDE2_GEOMS[name]
    return conv_reference(1, B, H, W, C, N, k, 2, pad, "stride2")


@functools.lru_cache(maxsize=None)
def split_equal_reference(op):
    B, H, W, C, N = SPLIT_EQUAL_GEOM[op]
    return conv_reference(op, B, H, W, C, N, 3, 1, 1, "split_equal")


@functools.lru_cache(maxsize=None)
def split_reference(op):
    B, H, W, C, N = SPLIT_GEOM
    return conv_reference(op, B, H, W, C, N, 3, 1, 1, "split")


@functools.lru_cache(maxsize=None)
def item_reference(cfg, op):
    B, H, W, C, N = ITEM_GEOMS[cfg]
    r = conv_reference(op, B, H, W, C, N, 3, 1, 1, "item")
    if cfg == C16_CFG and op == 1:      # conv3_c16d takes no bias
        r = dict(r, ref=(r["ref"] - r["bias"].double()).contiguous(), bias=None)
    return r


@functools.lru_cache(maxsize=None)
def equal_reference(case):
    op, (B, H, W, C, N, k), cfg, _ = case
    r = conv_reference(op, B, H, W, C, N, k, 1, k // 2, "equal")
    if cfg == C16_CFG and op == 1:
        r = dict(r, ref=(r["ref"] - r["bias"].double()).contiguous(), bias=None)
    return r


def weight_layout(op, w):
    """The kernel's weight layout of a torch (N, C, k, k) weight: OHWI (forward) or IHWO (input gradient)."""
    return (w.permute(0, 2, 3, 1) if op == 0 else w.permute(1, 2, 3, 0)).contiguous()


def block_usage(out, ref, bm, bound=4e-3):
    """Largest used fraction of `bound` by the rel-L2 error of any block of bm consecutive GEMM rows (pixels in
    NHWC order), all columns: one wrong tile is not averaged away by the rest of the output.  NaN -> inf."""
    ncols = ref.shape[-1]
    a, r = out.detach().double().cpu().reshape(-1, ncols), ref.double().reshape(-1, ncols)
    assert a.shape == r.shape, (a.shape, r.shape)
    worst = 0.0
    for m0 in range(0, r.shape[0], bm):
        e = float((a[m0:m0 + bm] - r[m0:m0 + bm]).norm() / r[m0:m0 + bm].norm().clamp_min(1e-30))
        worst = max(worst, e / bound) if e == e else float("inf")
    return worst


def forced_launches():
    """(name, op, geometry, dtype, cfg, wgs, c_split) of every launch of the forced GPU cases."""
    for kind, op, cfg in STEADY_CASES:
        for w in WGS:
            yield f"steady/{kind}/{op}/{cfg}/{w}", op, steady_geom(kind, op, cfg), BF16, cfg, w, 0
    for name, cfg in STRIDE2_CASES:
        for w in WGS:
            yield f"stride2/{name}/{cfg}/{w}", 1, stride2_geom(name), BF16, cfg, w, 0
    for op, cfg in SPLIT_CASES:
        for w in WGS:
            yield f"split/{op}/{cfg}/{w}", op, split_geom(), BF16, cfg, w, SPLIT_AT
    for op, cfg in SPLIT_EQUAL_CASES:
        yield f"split_equal/{op}/{cfg}", op, split_equal_geom(op), BF16, cfg, 8, SPLIT_AT
    for cfg, op in ITEM_CASES:
        for w in WGS:
            yield f"item/{cfg}/{op}/{w}", op, item_geom(cfg), BF16, cfg, w, 0
    for case in EQUAL_CASES:
        yield f"equal/{case}", case[0], equal_geom(case), BF16, case[2], case[3], 0


# ---------------------------------------------------------------------------------------------
# the launches of csu.ops for one convolution, as csu/ops.py makes them
# ---------------------------------------------------------------------------------------------
def ops_launches(entry, dtype, B, H, W, C, N, k, stride, pad, c_split=0, input_grad=True):
    """(form, op, geometry, c_split, ws_bytes) of the launches behind ops.conv2d / conv2d_cat / conv_transpose2d
    (forward and backward) for one convolution; ws_bytes None = csu_conv2d_workspace's, as _Conv2dFn passes."""
    from csu import _lib, ops
    import ctypes
    if entry == "conv2d_cat":
        g = geom(B, H, W, C, N, k, 1, pad)
        if dtype == BF16 and _lib.lib().csu_conv2d_split_ok(ctypes.byref(g), c_split):
            return [("fwd", 0, g, c_split, 0), ("dgrad", 1, g, c_split, 0), ("wgrad", 2, g, c_split, 0)]
        entry = "conv2d"
    if entry == "conv2d":
        g = geom(B, H, W, ops._pad_channels(C), N, k, stride, pad)
        out = [("fwd", 0, g, 0, None), ("wgrad", 2, g, 0, 0)]
        return out + ([("dgrad", 1, g, 0, None)] if input_grad else [])
    assert entry == "conv_transpose2d"      # (B, H, W, C) is the transposed conv's OUTPUT: the matching conv's input
    g = geom(B, H, W, C, N, k, stride, 0)
    # forward = the input-gradient operator, its input gradient = the forward conv, both without a workspace;
    # the weight gradient swaps the operands' roles but not the geometry
    return [("fwd", 1, g, 0, 0), ("dgrad", 0, g, 0, 0), ("wgrad", 2, g, 0, 0)]


def auto_launches(name):
    entry, dtype, (B, H, W, C, N, k, s, p) = AUTO_CASES[name]
    return dtype, ops_launches(entry, dtype, B, H, W, C, N, k, s, p, AUTO_SPLIT.get(name, 0), input_grad=True)


def tested_classes():
    """{plan class: a launch of the GPU file that has it}"""
    out = {}
    for name, op, g, dt, cfg, w, cs in forced_launches():
        out.setdefault(plan_class(op, plan(op, g, dt, cfg, w, cs, 0), dt), name)
    for name in AUTO_CASES:
        dt, ls = auto_launches(name)
        for form, op, g, cs, ws in ls:
            out.setdefault(plan_class(op, plan(op, g, dt, -1, 0, cs, ws), dt), f"auto/{name}/{form}")
    return out


# ---------------------------------------------------------------------------------------------
# every convolution of the two models, read from the modules csu/unet.py and csu/model.py build
# ---------------------------------------------------------------------------------------------
def _conv_args(conv):
    return conv.in_channels, conv.out_channels, conv.kernel_size[0], conv.stride[0], conv.padding[0]


@functools.lru_cache(maxsize=None)
def _unet_modules():
    from csu.unet import UNet
    with torch.device("meta"):
        return UNet()


@functools.lru_cache(maxsize=None)
def _cswin_modules(img):
    from csu.model import CSWinTransformer
    # depth and split sizes shape the attention blocks only; no convolution depends on them
    return CSWinTransformer(img_size=img, depth=[1, 1, 1, 1], split_size=[1, 2, 8, 8])


def unet_convs(img, B):
    """(name, entry, (B, H, W, C, N, k, stride, pad), c_split, input_grad) of UNet.forward's convolutions."""
    m = _unet_modules()
    out = []

    def double(name, dc, h, cat=0):
        c1, c2 = dc.double_conv[0], dc.double_conv[3]
        C, N, k, s, p = _conv_args(c1)
        out.append((name + ".c1", "conv2d_cat" if cat else "conv2d", (B, h, h, C, N, k, s, p), cat, name != "inc"))
        C, N, k, s, p = _conv_args(c2)
        out.append((name + ".c2", "conv2d", (B, h, h, C, N, k, s, p), 0, True))

    double("inc", m.inc, img)
    h = img
    for name in ("down1", "down2", "down3", "down4"):
        h //= 2                                         # MaxPool2d(2)
        double(name, getattr(m, name).maxpool_conv[1], h)
    for name in ("up1", "up2", "up3", "up4"):
        up = getattr(m, name)
        k, s = up.up.kernel_size[0], up.up.stride[0]
        h = (h - 1) * s + k
        # ConvTranspose2d(in, in / 2): the input gradient of a conv from in / 2 to in channels on the upsampled size
        out.append((name + ".up", "conv_transpose2d", (B, h, h, up.up.out_channels, up.up.in_channels, k, s, 0), 0, True))
        cin = up.conv.double_conv[0].in_channels
        double(name, up.conv, h, cat=cin - up.up.out_channels)   # cat([skip, upsampled]): the skip comes first
    C, N, k, s, p = _conv_args(m.outc)
    out.append(("outc", "conv2d", (B, h, h, C, N, k, s, p), 0, True))
    return out


def cswin_convs(img, B):
    from csu.model import CARAFE, Merge_Block
    m = _cswin_modules(img)
    conv = m.stage1_conv_embed[0]
    C, N, k, s, p = _conv_args(conv)
    out = [("embed", "conv2d", (B, img, img, C, N, k, s, p), 0, False)]
    h = (img + 2 * p - k) // s + 1
    for name in ("merge1", "merge2", "merge3"):
        mb = getattr(m, name)
        assert isinstance(mb, Merge_Block)
        C, N, k, s, p = _conv_args(mb.conv)
        out.append((name, "conv2d", (B, h, h, C, N, k, s, p), 0, True))
        h = (h + 2 * p - k) // s + 1
    for name in ("upsample4", "upsample3", "upsample2", "upsample1"):
        up = getattr(m, name)
        assert isinstance(up, CARAFE)
        C, N, k, s, p = _conv_args(up.encoder)
        out.append((name + ".encoder", "conv2d", (B, h, h, C, N, k, s, p), 0, True))
        h *= up.up_factor
    assert h == img
    return out


def model_launches(model, img, B, dtype):
    """(name, form, op, geometry, c_split, ws_bytes) of every conv launch of one training step."""
    for name, entry, (b, H, W, C, N, k, s, p), cat, ig in (unet_convs if model == "unet" else cswin_convs)(img, B):
        for form, op, g, cs, ws in ops_launches(entry, dtype, b, H, W, C, N, k, s, p, cat, ig):
            yield f"{model}{img}/B{B}/{name}", form, op, g, cs, ws
