"""Guard-band cases of csu.components (README "Testing"): csu_ccl and csu_cc_filter stay inside their
outputs and workspaces, write all of their outputs, initialise every workspace field they read (the
workspace payload is poisoned), and let no byte outside the label map reach a result (the guards of
the map hold 1, a legal label: a read past the edge would join or grow a component)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from guard_alloc import GuardedAlloc
from test_gpu_guard_bands import dev, gin, guarded, mod, verify

T = 64                      # the tile edge of csrc/components.hip
H, W = T + 1, T - 1


def label_map(seed, dtype):
    """Four values over blobs and salt, ones along every edge so that a read past an edge would matter."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 5, (2, H, W)) * (rng.random((2, H, W)) < 0.6)
    m[:, 20:40, 10:50][rng.random((2, 20, 40)) < 0.8] = 2
    m[:, 0, ::2] = 1
    m[:, -1, 1::2] = 1
    m[:, ::2, 0] = 1
    m[:, 1::2, -1] = 1
    return torch.from_numpy(m).to(dtype)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("conn", [4, 8])
def test_connected_components(conn, dtype, monkeypatch):
    cc, L = mod("components"), mod("_lib").lib()
    d = dev()
    m = label_map(conn, dtype)
    want = cc.reference_connected_components(m, conn, return_areas=True)
    ga = GuardedAlloc()
    md = gin(ga, m, d, fill=1)
    with guarded(monkeypatch, "components", registry=ga):
        got = cc.connected_components(md, conn, return_areas=True)
    verify(ga, got, ws=L.csu_ccl_workspace(2, H, W))
    for g, w in zip(got, want):
        assert g.dtype == torch.int32 and torch.equal(g.cpu(), w)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("conn", [4, 8])
def test_postprocess_labels(conn, dtype, monkeypatch):
    cc, L = mod("components"), mod("_lib").lib()
    d = dev()
    m = label_map(10 + conn, dtype)
    kw = dict(keep_largest=True, min_size=[0, 3, 3, 2, 4], fill_holes=True, max_hole_size=6, connectivity=conn)
    want = cc.reference_postprocess_labels(m, 5, **kw)
    assert not torch.equal(want, m)
    ga = GuardedAlloc()
    md = gin(ga, m, d, fill=1)
    with guarded(monkeypatch, "components", registry=ga):
        got = cc.postprocess_labels(md, 5, **kw)
    verify(ga, [got], ws=L.csu_cc_filter_workspace(2, H, W))
    assert got.dtype == dtype and torch.equal(got.cpu(), want)
