"""csu_sort_pairs on the MI355X: the stable segmented radix sort against numpy's stable argsort, bit for bit.

The values are the pairs' places in the input, so equal keys that kept their order are the only permutation that
passes.  Lengths sit around a wave (63, 64, 65) and around the tile T = csu_sort_pairs_tile() one workgroup ranks
per pass (T - 1, T, T + 1, 3 T + 5: a ragged last tile after full ones); 1, 3 and 7 segments; key_bits 1, 8, 9, 31
and 32 (one to four passes, an odd number of which ends in the copy back, and a top digit cut by key_bits)."""
import numpy as np
import pytest
import torch

from test_gpu_seg_ce import dev

pytestmark = pytest.mark.gpu

KEY_BITS = [1, 8, 9, 31, 32]
SEGMENTS = [1, 3, 7]


def tile():
    from csu import ops
    return ops.sort_pairs_tile()


def key_patterns(n, g):
    """name -> n uint32 keys."""
    r = lambda hi: torch.randint(0, hi, (n,), generator=g, dtype=torch.int64).numpy().astype(np.uint32)
    ar = np.arange(n, dtype=np.uint32)
    return {"equal": np.full(n, 0xDEADBEEF, np.uint32),
            "sorted": ar * np.uint32(2654435761 // max(n, 1)),
            "reversed": (np.uint32(n) - ar) * np.uint32(40503),
            "two_values": np.where(r(2) > 0, np.uint32(0x80000001), np.uint32(0x00FF00FF)),
            "one_per_bucket": (ar % 256) * np.uint32(0x01010101),
            "top_byte": (r(256) << np.uint32(24)) | np.uint32(0x00123456)}


def reference(keys, vals, segments, key_bits):
    mask = np.uint32(0xFFFFFFFF if key_bits == 32 else (1 << key_bits) - 1)
    k2, v2 = keys.reshape(segments, -1), vals.reshape(segments, -1)
    order = np.argsort(k2 & mask, axis=1, kind="stable")
    return np.take_along_axis(k2, order, 1).reshape(-1), np.take_along_axis(v2, order, 1).reshape(-1)


def run(keys, vals, segments, key_bits, d):
    from csu import ops
    kd = torch.from_numpy(keys.view(np.int32)).to(d)
    vd = torch.from_numpy(vals.view(np.int32)).to(d)
    ko, vo = ops.sort_pairs(kd, vd, segments, key_bits)
    assert torch.equal(kd.cpu(), torch.from_numpy(keys.view(np.int32)))          # the inputs are left alone
    return ko.cpu().numpy().view(np.uint32), vo.cpu().numpy().view(np.uint32)


LENGTHS = {"1": lambda T: 1, "2": lambda T: 2, "63": lambda T: 63, "64": lambda T: 64, "65": lambda T: 65,
           "T-1": lambda T: T - 1, "T": lambda T: T, "T+1": lambda T: T + 1, "3T+5": lambda T: 3 * T + 5}


@pytest.mark.parametrize("length", list(LENGTHS))
def test_sort_vs_numpy_stable_argsort(length):
    d = dev()
    n1 = LENGTHS[length](tile())
    g = torch.Generator().manual_seed(n1)
    for segments in SEGMENTS:
        n = n1 * segments
        vals = np.arange(n, dtype=np.uint32)
        for name, keys in key_patterns(n, g).items():
            for bits in KEY_BITS:
                gk, gv = run(keys, vals, segments, bits, d)
                wk, wv = reference(keys, vals, segments, bits)
                assert np.array_equal(gk, wk) and np.array_equal(gv, wv), (name, segments, bits)


def test_large_segments_and_uint32_tensors():
    """2 x 199 800 pairs (98 tiles a segment, the last one ragged), random 32-bit keys with many duplicates; the
    uint32 dtype is taken as it is."""
    from csu import ops
    d = dev()
    n1, segments = 199800, 2
    g = torch.Generator().manual_seed(5)
    keys = (torch.randint(0, 1 << 16, (n1 * segments,), generator=g).numpy().astype(np.uint32) * np.uint32(65537)) >> np.uint32(3)
    vals = np.arange(n1 * segments, dtype=np.uint32)
    for bits in (31, 32):
        gk, gv = run(keys, vals, segments, bits, d)
        wk, wv = reference(keys, vals, segments, bits)
        assert np.array_equal(gk, wk) and np.array_equal(gv, wv), bits
    ku = torch.from_numpy(keys.view(np.int32)).to(d).view(torch.uint32)
    ko, vo = ops.sort_pairs(ku, torch.from_numpy(vals.view(np.int32)).to(d), segments)
    assert ko.dtype == torch.uint32 and np.array_equal(ko.view(torch.int32).cpu().numpy().view(np.uint32), wk)


def test_bits_above_key_bits_are_ignored_and_carried():
    d = dev()
    T = tile()
    n, g = T + 77, torch.Generator().manual_seed(9)
    low = torch.randint(0, 1 << 9, (n,), generator=g).numpy().astype(np.uint32)
    high = torch.randint(0, 1 << 23, (n,), generator=g).numpy().astype(np.uint32) << np.uint32(9)
    vals = np.arange(n, dtype=np.uint32)
    gk, gv = run(low | high, vals, 1, 9, d)
    hk, hv = run(low, vals, 1, 9, d)
    assert np.array_equal(gv, hv) and np.array_equal(gk & np.uint32(0x1FF), hk)          # the order of the low bits alone
    assert np.array_equal(gk, (low | high)[gv])                                           # the whole key travels


def test_bitwise_repeatable():
    d = dev()
    n, g = 3 * tile() + 5, torch.Generator().manual_seed(3)
    keys = torch.randint(0, 1 << 12, (3 * n,), generator=g).numpy().astype(np.uint32)
    vals = np.arange(3 * n, dtype=np.uint32)
    a, b = run(keys, vals, 3, 32, d), run(keys, vals, 3, 32, d)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_capturable_in_a_graph():
    from csu import ops
    d = dev()
    n, g = 2 * tile() + 9, torch.Generator().manual_seed(4)
    keys = torch.randint(0, 1 << 20, (n,), generator=g).numpy().astype(np.uint32)
    vals = np.arange(n, dtype=np.uint32)
    kd = torch.from_numpy(keys.view(np.int32)).to(d)
    vd = torch.from_numpy(vals.view(np.int32)).to(d)
    ops.sort_pairs(kd, vd, 1, 20)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ko, vo = ops.sort_pairs(kd, vd, 1, 20)
    for seed in (0, 1):          # new keys in the captured input between replays
        k2 = np.roll(keys, 17 * seed + 1)
        kd.copy_(torch.from_numpy(k2.view(np.int32)))
        graph.replay()
        wk, wv = reference(k2, vals, 1, 20)
        assert np.array_equal(ko.cpu().numpy().view(np.uint32), wk) and np.array_equal(vo.cpu().numpy().view(np.uint32), wv)


def test_ops_argument_checks():
    from csu import ops
    from csu._lib import CsuError
    d = dev()
    k = torch.zeros(12, dtype=torch.int32, device=d)
    with pytest.raises(CsuError):
        ops.sort_pairs(k.cpu(), k.cpu(), 1)
    for a, b, s, bits in ((k.float(), k, 1, 32), (k, k[:6], 1, 32), (k[:0], k[:0], 1, 32), (k, k, 5, 32), (k, k, 0, 32),
                          (k, k, 1, 0), (k, k, 1, 33)):
        with pytest.raises(ValueError):
            ops.sort_pairs(a, b, s, bits)
