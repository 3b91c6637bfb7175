"""The exact-integer parity tests' instrument (exact_inputs.py), checked on the CPU.

  * preconditions() holds for every reference test_gpu_exact_integer.py compares against (both files take
    their cases from exact_inputs.py), so a mismatch there is the kernel's and not the input's;
  * the instrument is sharper than the whole-tensor criteria: a reference with one element off by 1, or
    its last three rows off by 1, passes test_gpu_kernels.assert_close and is rejected -- and located --
    by first_mismatch;
  * the ReLU-regime claim: on the lattice 16 j + 8 (|h| <= 2048) torch's fp32 GELU and line-for-line fp32
    transcriptions of gelu_pair_as / gelu_pair_fast (csrc/common.hpp) give gelu = h and gelu' = 1 exactly
    for h > 0, and magnitudes < 1e-12 / < 1e-11 for h < 0."""
import pytest
import torch

import exact_inputs as E


@pytest.mark.parametrize("family", E.FAMILIES)
def test_preconditions_hold(family):
    n = 0
    for label, ref, terms, dt, q, active, operands in E.family_checks(family):
        try:
            f = E.preconditions(ref, terms, dt, operands, q, active)
        except AssertionError as e:
            raise AssertionError(f"{family} {label}: {e}") from e
        n += 1
        print(f"{family} {label}: sum|terms| {f['terms']:.0f}, |ref| {f['ref']:.0f}, non-zero {f['nonzero']:.3f}")
    assert n > 0
    count, tmax, rmax = E.family_figures(family)
    assert count == n and tmax <= E.TERMS_MAX
    print(f"{family}: {count} references, max sum|terms| / quantum {tmax:.0f}, max |ref| / quantum {rmax:.0f}")


def test_preconditions_reject():
    """Each condition fails when it should."""
    g = E.gen(1)
    ref = E.ints((64, 64), 1, 9, g)
    E.preconditions(ref, ref, torch.bfloat16)
    with pytest.raises(AssertionError):
        E.preconditions(ref * 40, ref * 40, torch.bfloat16)                 # 360 is not a bf16 integer range
    E.preconditions(ref * 40, ref * 40, torch.float32)
    E.preconditions(ref * 64, ref * 64, torch.bfloat16, quantum=16)
    with pytest.raises(AssertionError):
        E.preconditions(ref, ref * 2 ** 13, torch.float32)                  # sum |terms| over 2^15
    with pytest.raises(AssertionError):
        E.preconditions(ref * (ref > 3), ref, torch.float32)                # a third of it zero
    with pytest.raises(AssertionError):
        E.preconditions(ref + 0.5, ref + 1, torch.float32)                  # off the lattice
    dead = ref.clone()
    dead[:, 5] = 0
    with pytest.raises(AssertionError):
        E.preconditions(ref, ref, torch.float32, operands=(("dead column", dead),))
    on = ref > 3
    E.preconditions(ref * on, ref, torch.float32, active=on)
    with pytest.raises(AssertionError):
        E.preconditions(ref, ref, torch.float32, active=on)                 # "inactive" elements must be zero


def test_case_lists_follow_the_kernel_tests():
    """The lists copied from test_gpu_kernels.py stay its lists (the conv cases but for the two B = 16)."""
    import test_gpu_kernels as T
    assert E._CONV_CASES_SOURCE == T.CONV_CASES
    assert E.DMA_CONV_CASES == T.DMA_CONV_CASES and E.IGEMM_DMA_BN == T.IGEMM_DMA_BN
    assert [c for c in E.CONV_CASES if c not in E.CONV_KSPLIT_CASES] == [c for c in T.CONV_CASES if c[0] != 16]
    assert [c[1:] for c in E.CONV_KSPLIT_CASES] == [c[1:] for c in T.CONV_CASES if c[0] == 16]
    assert set(E.GEMM_WS_SHAPES) <= set(T.GEMM_WS_SHAPES) | {(1024, 256, 768)}
    assert set(E.MLP_CASES) == {(64, 4096), (64, 37), (128, 1000), (256, 4160), (256, 100)}


def _sensitivity_cases():
    c = E.gemm_case(4099, 192, 64, "plain")
    yield "gemm (4099, 192, 64)", c["ref"], None
    v = E.conv_case_sq(E.DMA_CONV_CASES[0])
    B, H, W, C, N, k, s, p, OH, OW = v["geom"]
    yield f"conv {E.DMA_CONV_CASES[0]}", v["refs"][0], (B, OH, OW)


@pytest.mark.parametrize("which", [0, 1])
def test_sharper_than_the_whole_tensor_criterion(which):
    from test_gpu_kernels import assert_close
    name, ref, image = list(_sensitivity_cases())[which]
    ref2 = ref.reshape(-1, ref.shape[-1])
    rows, cols = ref2.shape
    good = ref.bfloat16()
    assert E.first_mismatch(good, ref, image=image) is None
    E.assert_exact(good, ref, name)

    one = good.clone().reshape(rows, cols)
    r, c = rows // 2 + 3, cols // 2 + 1
    one[r, c] += 1
    assert_close(one, ref2, torch.bfloat16)                    # the old criterion accepts it
    rep = E.first_mismatch(one.view_as(good), ref, image=image)
    assert rep["count"] == 1 and rep["first"] == (r, c) and rep["tile"] == (r // 64, c // 64)
    assert rep["got"] == float(ref2[r, c]) + 1 and rep["expected"] == float(ref2[r, c])
    assert rep["coords"] == [(r, c)]
    assert not rep["all_in_last_row_tile"] and not rep["all_in_last_col_tile"]
    with pytest.raises(AssertionError):
        E.assert_exact(one.view_as(good), ref, name)

    tail = good.clone().reshape(rows, cols)
    tail[-3:] += 1
    assert_close(tail, ref2, torch.bfloat16)                   # ... and this
    rep = E.first_mismatch(tail.view_as(good), ref, image=image)
    assert rep["count"] == 3 * cols and rep["first"] == (rows - 3, 0) and rep["tile"] == ((rows - 3) // 64, 0)
    assert rep["all_in_last_row_tile"] and not rep["all_in_last_col_tile"]
    assert rep["coords"] == [(rows - 3, j) for j in range(16)]
    if image is not None:
        assert rep["all_in_last_batch"] and rep["all_on_image_border"]
    with pytest.raises(AssertionError):
        E.assert_exact(tail.view_as(good), ref, name)


def test_first_mismatch_values():
    ref = torch.arange(12.0).view(1, 3, 4) - 5                 # holds a 0
    assert E.first_mismatch(-ref.float() * -1.0, ref) is None
    assert E.first_mismatch(ref * -0.0 + ref, ref) is None
    neg0 = ref.clone()
    neg0[0, 1, 1] = -0.0                                       # ref there is 0: equal in value
    assert float(ref[0, 1, 1]) == 0 and E.first_mismatch(neg0, ref) is None
    nan = ref.clone()
    nan[0, 2, 3] = float("nan")                                # an element the kernel never wrote
    rep = E.first_mismatch(nan, ref, tile=(2, 2))
    assert rep["count"] == 1 and rep["first"] == (2, 3) and rep["tile"] == (1, 1)
    assert rep["all_in_last_row_tile"] and rep["all_in_last_col_tile"]
    img = torch.zeros(2, 3, 3, 2)
    bad = img.clone()
    bad[0, 1, 1, 0] = 1                                        # the centre pixel of the first image
    rep = E.first_mismatch(bad, img, image=(2, 3, 3))
    assert not rep["all_in_last_batch"] and not rep["all_on_image_border"]


def test_relu_regime_criterion():
    ref = torch.tensor([[0.0, 8.0, 0.0, 24.0]])
    tail = torch.tensor([[True, False, False, False]])
    E.assert_relu_regime(torch.tensor([[-3e-13, 8.0, -0.0, 24.0]]), ref, tail)
    with pytest.raises(AssertionError):
        E.assert_relu_regime(torch.tensor([[0.0, 8.0, -3e-13, 24.0]]), ref, tail)    # no tail reaches it: exact
    with pytest.raises(AssertionError):
        E.assert_relu_regime(torch.tensor([[1e-5, 8.0, 0.0, 24.0]]), ref, tail)
    with pytest.raises(AssertionError):
        E.assert_relu_regime(torch.tensor([[0.0, 9.0, 0.0, 24.0]]), ref, tail)


# ---------------------------------------------------------------------------------------------
# the ReLU regime of the GELUs
# ---------------------------------------------------------------------------------------------
def _lattice():
    j = torch.arange(-128, 128, dtype=torch.float32)
    h = 16 * j + 8
    assert float(h.abs().max()) <= 2048 and h.numel() == 256
    return h


def _f(v):
    return torch.tensor(v, dtype=torch.float32)


def _erf_poly_as(t):
    return t * (_f(0.254829592) + t * (_f(-0.284496736) + t * (_f(1.421413741) + t * (_f(-1.453152027) + t * _f(1.061405429)))))


def gelu_pair_as(x, rcp_ulp=0):
    """csrc/common.hpp gelu_pair_as in torch.float32 (rcp_ulp: the reciprocal moved by that many ulps)."""
    z = x.abs() * _f(0.70710678118654752)
    ex = torch.exp(-z * z)
    t = _ulps(torch.reciprocal(_f(1.0) + _f(0.3275911) * z), rcp_ulp)
    e = _f(1.0) - _erf_poly_as(t) * ex
    phi2 = _f(0.5) * (_f(1.0) + torch.where(x >= 0, e, -e))
    return x * phi2, phi2 + x * _f(0.3989422804014327) * ex


def gelu_pair_fast(x, rcp_ulp=0):
    """csrc/common.hpp half_erfc_as + gelu_pair_fast in torch.float32."""
    t = _ulps(torch.reciprocal(torch.addcmul(_f(1.0), _f(0.33267904), x.abs())), rcp_ulp)
    ex = torch.exp2(_f(-0.72134752) * (x * x))
    q = t * (_f(0.1740121) + t * (_f(-0.0479399) + t * _f(0.3739278))) * ex
    phi = torch.where(x >= 0, _f(1.0) - q, q)
    return x * phi, torch.addcmul(phi, x * _f(0.3989422804014327), ex)


def _ulps(t, n):
    for _ in range(abs(n)):
        t = torch.nextafter(t, torch.full_like(t, float("inf") if n > 0 else 0.0))
    return t


def _assert_relu_regime(h, g, dg, name):
    assert g.dtype == torch.float32 and dg.dtype == torch.float32
    pos = h > 0
    assert int(pos.sum()) == 128 and not bool((h == 0).any())
    assert torch.equal(g[pos], h[pos]), name
    assert torch.equal(dg[pos], torch.ones_like(h[pos])), name
    assert float(g[~pos].abs().max()) < 1e-12, (name, float(g[~pos].abs().max()))
    assert float(dg[~pos].abs().max()) < 1e-11, (name, float(dg[~pos].abs().max()))


def test_torch_gelu_on_the_lattice():
    h = _lattice().requires_grad_(True)
    g = torch.nn.functional.gelu(h)
    # the analytic derivative Phi(h) + h phi(h), in fp32
    hd = h.detach()
    dg = 0.5 * (1 + torch.erf(hd * _f(0.70710678118654752))) + hd * _f(0.3989422804014327) * torch.exp(-0.5 * hd * hd)
    _assert_relu_regime(hd, g.detach(), dg, "torch")
    g.sum().backward()
    _assert_relu_regime(hd, g.detach(), h.grad, "torch autograd")


@pytest.mark.parametrize("rcp_ulp", [0, 1, -1])
@pytest.mark.parametrize("pair", [gelu_pair_as, gelu_pair_fast])
def test_kernel_gelus_on_the_lattice(pair, rcp_ulp):
    h = _lattice()
    g, dg = pair(h, rcp_ulp)
    _assert_relu_regime(h, g, dg, pair.__name__)
    # the operands the GEMM prologue / epilogues see: {+-8, +-16}
    # 32 j + 8, the fused Mlp's lattice: the negative points start at -24, where the tail is exactly 0
    neg = h[(h < 0) & (torch.remainder(h, 32) == 8)]
    assert float(neg.max()) == -24 and neg.numel() == 64
    g, dg = pair(neg, rcp_ulp)
    assert not bool(g.any()) and not bool(dg.any())
    s = torch.tensor([-16.0, -8.0, 8.0, 16.0])
    g, dg = pair(s, rcp_ulp)
    assert torch.equal(g[2:], s[2:]) and torch.equal(dg[2:], torch.ones(2))
    assert float(g[:2].abs().max()) < 1e-12 and float(dg[:2].abs().max()) < 1e-11
