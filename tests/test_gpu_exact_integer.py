"""Exact-integer parity on the MI355X for the accumulate-type kernels: gemm, gemm_ws, gemm_f32, colsum,
linear_wgrad, the Linear ops, the implicit-GEMM convolutions and their weight gradients, the fused Mlp.

Inputs are small integers (exact_inputs.py), so every product and every partial sum in any order is exact
and every result is representable in the output type: the kernel must equal the float64 reference element
for element, whatever its tile shape, split or summation order.  The criterion is equality in value
(exact_inputs.assert_exact; -0 counts as 0) with no tolerance.  The GELU-bearing kernels run in the ReLU
regime (h on the lattice 16 Z + 8, where gelu(h) = h or ~0 and gelu'(h) = 1 or ~0): exact wherever no negative
tail contributes, |got - ref| <= 1e-6 elsewhere (exact_inputs.assert_relu_regime).  A failure prints
first_mismatch's report: how many elements differ, the first one's coordinates, tile and values, and whether
all of them sit in the last row / column tile, the last batch item or on the image border.

The conditions that make this exact are asserted on the CPU for the same case lists (test_exact_inputs.py)."""
import ctypes

import pytest
import torch

import exact_inputs as E

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def put(t, dtype, d):
    """An exact_inputs tensor (integer-valued float64) on the device in `dtype` (exact), or None."""
    return None if t is None else t.to(dtype).to(d).contiguous()


def check(got, ref, tail=None, name="", image=None):
    if tail is None:
        E.assert_exact(got, ref, name, image=image)
    else:
        E.assert_relu_regime(got, ref, tail, name)


# ---------------------------------------------------------------------------------------------
# ops.gemm
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", E.GEMM_SHAPES)
@pytest.mark.parametrize("b_trans", [False, True])
@pytest.mark.parametrize("mode", E.GEMM_LINEAR_MODES + E.GEMM_RELU_MODES)
def test_gemm(M, N, K, b_trans, mode):
    from csu import ops
    d = dev()
    c = E.gemm_case(M, N, K, mode)
    a, w = put(c["a"], BF, d), put(c["w"], BF, d)
    b = w.t().contiguous() if b_trans else w
    out = ops.gemm(a, b, b_trans, c["odt"], bias=put(c["bias"], F32, d), a_gelu=mode == "a_gelu",
                   gelu_aux=put(c["aux"], BF, d), resid=put(c["res"], F32, d))
    assert out.dtype == c["odt"]
    check(out, c["ref"], c["tail"], f"gemm {(M, N, K)} b_trans={b_trans} {mode}")


@pytest.mark.parametrize("cfg", E.GEMM_CFGS)
@pytest.mark.parametrize("M,N,K", E.GEMM_CFG_SHAPES)
def test_gemm_tile_configs_and_gelu_out(M, N, K, cfg):
    """Every tile configuration of the b[n][k] kernel with the dual (h, gelu(h)) epilogue: h exact, gelu(h)
    = relu(h) in the ReLU regime."""
    from csu import ops
    d = dev()
    c = E.gemm_gelu_out_case(M, N, K)
    h, gh = ops.gemm(put(c["a"], BF, d), put(c["w"], BF, d), False, BF, bias=put(c["bias"], F32, d), cfg=cfg, gelu_out=True)
    check(h, c["h"], None, f"gemm cfg {cfg} {(M, N, K)} h")
    check(gh, c["gh"], c["tail"], f"gemm cfg {cfg} {(M, N, K)} gelu(h)")


# ---------------------------------------------------------------------------------------------
# ops.gemm_ws, csu_gemm_ws_ln
# ---------------------------------------------------------------------------------------------
def _ws_operands(c, d):
    """The strided token operand (row pitch K + 64, the padding filled with other integers) and the
    fragment-ordered weight."""
    from test_gpu_kernels import _frag_ref
    M, K = c["x"].shape
    xfull = E.ints((M, K + 64), -2, 2, E.gen(M, K, 1), nonzero=True)
    xfull[:, :K] = c["x"]
    return put(xfull, BF, d)[:, :K], _frag_ref(put(c["w"], BF, d)).contiguous()


@pytest.mark.parametrize("M,N,K", E.GEMM_WS_SHAPES)
@pytest.mark.parametrize("mode", E.GEMM_WS_MODES)
def test_gemm_ws(M, N, K, mode):
    from csu import ops
    d = dev()
    c = E.linear_fwd_case(M, N, K, mode)
    x, wf = _ws_operands(c, d)
    assert x.stride(0) == K + 64
    out = ops.gemm_ws(x, wf, N, c["odt"], bias=put(c["bias"], F32, d), resid=put(c["res"], F32, d))
    torch.cuda.synchronize()
    check(out, c["ref"], None, f"gemm_ws {(M, N, K)} {mode}")


@pytest.mark.parametrize("M,C", E.GEMM_WS_LN_SHAPES)
def test_gemm_ws_ln_y(M, C):
    """csu_gemm_ws_ln's fp32 output y = res + x W^T + bias (its LayerNorm outputs are not linear: not judged here)."""
    from csu._lib import lib, ptr, stream_ptr
    d = dev()
    c = E.linear_fwd_case(M, C, C, "resid")
    x, wf = _ws_operands(c, d)
    x = x.contiguous()
    bias, res = put(c["bias"], F32, d), put(c["res"], F32, d)
    gam, bet = torch.ones(C, device=d), torch.zeros(C, device=d)
    assert lib().csu_gemm_ws_ln_supported(M, C, C)
    y = torch.full((M, C), float("nan"), device=d)
    h = torch.empty(M, C, device=d, dtype=BF)
    mean, rstd = torch.empty(M, device=d), torch.empty(M, device=d)
    rc = lib().csu_gemm_ws_ln(M, C, ptr(x), C, ptr(wf), ptr(bias), ptr(res), ptr(y), ptr(gam), ptr(bet), 1e-5, ptr(h),
                              ptr(mean), ptr(rstd), stream_ptr(d))
    torch.cuda.synchronize()
    assert rc == 0, lib().csu_last_error_string()
    check(y, c["ref"], None, f"gemm_ws_ln {(M, C)} y")


# ---------------------------------------------------------------------------------------------
# ops.gemm_f32, ops.colsum
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,M,N,K", E.GEMM_F32_CASES)
def test_gemm_f32(layout, M, N, K):
    from csu import ops
    d = dev()
    c = E.gemm_f32_case(layout, M, N, K)
    a, b = put(c["a"], F32, d), put(c["b"], F32, d)
    if layout == 0:
        out = ops.gemm_f32(0, a, b, M, N, K, bias=put(c["bias"], F32, d), resid=put(c["res"], F32, d))
    elif layout == 1:
        out = ops.gemm_f32(1, a, b, M, N, K)
    else:
        out, asum = ops.gemm_f32(2, a, b, M, N, K, with_asum=True)
        check(asum, c["asum"], None, f"gemm_f32 {(layout, M, N, K)} asum")
    check(out, c["ref"], None, f"gemm_f32 {(layout, M, N, K)}")


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("rows,cols", E.COLSUM_SHAPES)
def test_colsum(rows, cols, dtype):
    from csu import ops
    d = dev()
    c = E.colsum_case(rows, cols)
    check(ops.colsum(put(c["x"], dtype, d)).view(1, cols), c["ref"].view(1, cols), None, f"colsum {(rows, cols)}")


# ---------------------------------------------------------------------------------------------
# ops.linear_wgrad: the default plan, every forced plan, the 8-wave tile, the deferred and grouped paths
# ---------------------------------------------------------------------------------------------
def _check_wgrad(dw, db, c, name):
    check(dw, c["dw"], None, f"{name} dW")
    check(db.view(1, -1), c["db"].view(1, -1), None, f"{name} db")


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("M,N,K", E.WGRAD_SHAPES)
def test_linear_wgrad(M, N, K, dtype):
    from csu import ops
    d = dev()
    c = E.wgrad_case(M, N, K)
    dw, db = ops.linear_wgrad(put(c["dy"], dtype, d), put(c["x"], dtype, d))
    assert dw.dtype == F32 and db.dtype == F32
    _check_wgrad(dw, db, c, f"linear_wgrad {(M, N, K)} {dtype}")


def _wgrad_tuned(M, N, K, tn, tk, chunks, c, d):
    """csu_linear_wgrad_tuned on a poisoned workspace and output: (dW, db)."""
    from csu._lib import check as ok, lib, ptr, stream_ptr
    L = lib()
    dy, x = put(c["dy"], BF, d), put(c["x"], BF, d)
    n = L.csu_linear_wgrad_tuned_workspace(M, N, K, tn, tk, chunks)
    ws = torch.full((max(n, 16) // 4,), float("nan"), device=d)
    out = torch.full((N * K + N,), float("nan"), device=d)
    ok(L.csu_linear_wgrad_tuned(M, N, K, 1, ptr(dy), ptr(x), ptr(out), ptr(ws), n, tn, tk, chunks, stream_ptr(d)),
       "linear_wgrad_tuned")
    torch.cuda.synchronize()
    return out[:N * K].view(N, K), out[N * K:], (dy, x, out, ws, n)


@pytest.mark.parametrize("M,N,K", E.WGRAD_PLAN_SHAPES)
@pytest.mark.parametrize("tn,tk,chunks", E.WGRAD_PLANS)
def test_linear_wgrad_plans(M, N, K, tn, tk, chunks):
    d = dev()
    c = E.wgrad_case(M, N, K)
    dw, db, _ = _wgrad_tuned(M, N, K, tn, tk, chunks, c, d)
    _check_wgrad(dw, db, c, f"linear_wgrad_tuned {(M, N, K)} plan {(tn, tk, chunks)}")


@pytest.mark.parametrize("M,N,K,chunks", E.WGRAD_8WAVE)
def test_linear_wgrad_8wave_tile(M, N, K, chunks):
    from csu._lib import lib, ptr, stream_ptr
    d = dev()
    c = E.wgrad_case(M, N, K)
    dw, db, (dy, x, out, ws, n) = _wgrad_tuned(M, N, K, 256, 128, chunks, c, d)
    _check_wgrad(dw, db, c, f"linear_wgrad_tuned 256x128 {(M, N, K)} chunks {chunks}")
    assert lib().csu_linear_wgrad_tuned(M, 192, K, 1, ptr(dy), ptr(x), ptr(out), ptr(ws), n, 256, 128, chunks,
                                        stream_ptr(d)) != 0   # N % 256 != 0: refused


@pytest.mark.parametrize("grouped", [False, True])
def test_linear_wgrad_deferred_and_grouped(grouped, monkeypatch):
    """defer=True: with GROUP_WGRAD off the tile kernels run now and one batched slab reduction at the flush;
    with it on the whole weight gradients of Linears of mixed shapes join the grouped end-of-backward launch."""
    from csu import ops
    monkeypatch.setattr(ops, "GROUP_WGRAD", grouped)
    d = dev()
    cases = [E.wgrad_case(*s) for s in E.WGRAD_GROUPED]
    ins = [(put(c["dy"], BF, d), put(c["x"], BF, d)) for c in cases]
    res = [ops.linear_wgrad(dy, x, defer=True) for dy, x in ins]
    assert len(ops._WG_DEFER) == (len(cases) if grouped else 0)
    ops._wgrad_flush()
    torch.cuda.synchronize()
    assert not ops._WG_DEFER and not ops._WG_PENDING
    for s, c, (dw, db) in zip(E.WGRAD_GROUPED, cases, res):
        _check_wgrad(dw, db, c, f"linear_wgrad {'grouped' if grouped else 'deferred'} {s}")


# ---------------------------------------------------------------------------------------------
# ops.linear, ops.concat_linear through autograd
# ---------------------------------------------------------------------------------------------
def _leaf(t, dtype, d):
    return put(t, dtype, d).requires_grad_(True)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,L,C,N", E.LINEAR_CASES)
def test_linear_autograd(B, L, C, N, dtype):
    from csu import ops
    d = dev()
    c = E.linear_case(B, L, C, N, False)
    x, w, b = _leaf(c["x"], dtype, d), _leaf(c["w"], F32, d), _leaf(c["b"], F32, d)
    with torch.autocast("cuda", dtype=BF, enabled=dtype == BF):
        y = ops.linear(x, w, b)
    assert y.dtype == dtype
    y.backward(put(c["gy"], y.dtype, d))
    torch.cuda.synchronize()
    for name, got, ref in zip(c["names"], (y, x.grad, w.grad, b.grad), c["refs"]):
        check(got, ref, None, f"linear {(B, L, C, N)} {dtype} {name}")


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,L,C,N", E.LINEAR_CASES)
def test_concat_linear_autograd(B, L, C, N, dtype):
    from csu import ops
    d = dev()
    c = E.linear_case(B, L, C, N, True)
    skip, up = _leaf(c["skip"], dtype, d), _leaf(c["up"], dtype, d)
    w, b = _leaf(c["w"], F32, d), _leaf(c["b"], F32, d)
    with torch.autocast("cuda", dtype=BF, enabled=dtype == BF):
        y = ops.concat_linear(skip, up, w, b)
    assert y.dtype == F32
    y.backward(put(c["gy"], y.dtype, d))
    torch.cuda.synchronize()
    for name, got, ref in zip(c["names"], (y, skip.grad, up.grad, w.grad, b.grad), c["refs"]):
        check(got, ref, None, f"concat_linear {(B, L, C, N)} {dtype} {name}")


# ---------------------------------------------------------------------------------------------
# ops.conv2d, conv2d_cat, conv_transpose2d through autograd
# ---------------------------------------------------------------------------------------------
def _check_conv_grads(c, y, x, w, b, name):
    B, H, W, C, N, k, s, p, OH, OW = c["geom"]
    refs = dict(zip(c["names"], c["refs"]))
    check(y, refs["y"], None, f"{name} y", image=(B, OH, OW))
    check(x.grad, refs["dx"], None, f"{name} dx", image=(B, H, W))
    check(w.grad.reshape(N, -1), refs["dW"].reshape(N, -1), None, f"{name} dW (N, C k k)")
    check(b.grad.view(1, -1), refs["db"].view(1, -1), None, f"{name} db")


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("case", E.CONV_CASES)
def test_conv2d_autograd(case, dtype):
    from csu import ops
    from csu._lib import lib, CSU_BF16
    d = dev()
    B, H, C, N, k, s, p = case
    c = E.conv_case_sq(case)
    if case in E.CONV_KSPLIT_CASES and dtype == BF:
        gm = ops._conv_geom(B, H, H, C, N, k, k, s, p)
        for op in (0, 1):      # the forward and the input gradient both take the K split
            assert lib().csu_conv2d_workspace(op, ctypes.byref(gm), CSU_BF16) > 0, op
    x, w, b = _leaf(c["x"], dtype, d), _leaf(c["w"], F32, d), _leaf(c["b"], F32, d)
    with torch.autocast("cuda", dtype=BF, enabled=dtype == BF):
        y = ops.conv2d(x, w, b, s, p)
    assert y.dtype == dtype
    y.backward(put(c["gy"], y.dtype, d))
    torch.cuda.synchronize()
    _check_conv_grads(c, y, x, w, b, f"conv2d {case} {dtype}")


@pytest.mark.parametrize("B,H,Ca,Cb,N", E.CONV_CAT_CASES)
def test_conv2d_cat(B, H, Ca, Cb, N):
    from csu import ops
    from csu._lib import lib
    d = dev()
    c = E.conv_case(B, H, H, Ca + Cb, N, 3, 1, 1)
    gm = ops._conv_geom(B, H, H, Ca + Cb, N, 3, 3, 1, 1)
    assert bool(lib().csu_conv2d_split_ok(ctypes.byref(gm), Ca)) == (H % 64 == 0)
    xa, xb = _leaf(c["x"][..., :Ca], BF, d), _leaf(c["x"][..., Ca:], BF, d)
    w, b = _leaf(c["w"], F32, d), _leaf(c["b"], F32, d)
    with torch.autocast("cuda", dtype=BF):
        y = ops.conv2d_cat(xa, xb, w, b, 1)
    y.backward(put(c["gy"], y.dtype, d))
    torch.cuda.synchronize()
    name = f"conv2d_cat {(B, H, Ca, Cb, N)}"
    refs = dict(zip(c["names"], c["refs"]))
    check(y, refs["y"], None, f"{name} y", image=(B, H, H))
    check(xa.grad, refs["dx"][..., :Ca], None, f"{name} dxa", image=(B, H, H))
    check(xb.grad, refs["dx"][..., Ca:], None, f"{name} dxb", image=(B, H, H))
    check(w.grad.reshape(N, -1), refs["dW"].reshape(N, -1), None, f"{name} dW (N, C k k)")
    check(b.grad.view(1, -1), refs["db"].view(1, -1), None, f"{name} db")


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,H,Cin,Cout", E.CONVT_CASES)
def test_conv_transpose2d_autograd(B, H, Cin, Cout, dtype):
    from csu import ops
    d = dev()
    c = E.convt_case(B, H, Cin, Cout)
    x, w, b = _leaf(c["x"], dtype, d), _leaf(c["w"], F32, d), _leaf(c["b"], F32, d)
    with torch.autocast("cuda", dtype=BF, enabled=dtype == BF):
        y = ops.conv_transpose2d(x, w, b, 2)
    y.backward(put(c["gy"], y.dtype, d))
    torch.cuda.synchronize()
    name = f"conv_transpose2d {(B, H, Cin, Cout)} {dtype}"
    refs = dict(zip(c["names"], c["refs"]))
    check(y, refs["y"], None, f"{name} y", image=(B, 2 * H, 2 * H))
    check(x.grad, refs["dx"], None, f"{name} dx", image=(B, H, H))
    check(w.grad.reshape(Cin, -1), refs["dW"].reshape(Cin, -1), None, f"{name} dW (Cin, Cout k k)")
    check(b.grad.view(1, -1), refs["db"].view(1, -1), None, f"{name} db")


# ---------------------------------------------------------------------------------------------
# csu_conv2d_ex: forced configurations, forward (op 0) and input gradient (op 1), bf16
# ---------------------------------------------------------------------------------------------
def _conv_ex_operands(c, d):
    """[(op, source, weight, bias, reference, image)] of the forward and the input gradient."""
    B, H, W, C, N, k, s, p, OH, OW = c["geom"]
    refs = dict(zip(c["names"], c["refs"]))
    w = c["w"]
    return [(0, put(c["x"], BF, d), put(w.permute(0, 2, 3, 1), BF, d), put(c["b"], F32, d), refs["y"], (B, OH, OW)),
            (1, put(c["gy"], BF, d), put(w.permute(1, 2, 3, 0), BF, d), None, refs["dx"], (B, H, W))]


def _conv_ex(op, gm, src, wt, bias, ref, cfg, d):
    """(error code, output on a poisoned buffer) of one csu_conv2d_ex call."""
    from csu._lib import lib, CSU_BF16
    out = torch.full(tuple(ref.shape), float("nan"), dtype=BF, device=d)
    e = lib().csu_conv2d_ex(op, ctypes.byref(gm), CSU_BF16, src.data_ptr(), wt.data_ptr(),
                            bias.data_ptr() if bias is not None else None, out.data_ptr(), cfg,
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return e, out


@pytest.mark.parametrize("case", E.DMA_CONV_CASES)
def test_conv2d_ex_dma_cfgs(case):
    """Every LDS-DMA tile configuration; a configuration whose BN does not divide the output columns must
    refuse, and so must the halo kernel (cfg 20), which none of these geometries is eligible for."""
    from csu import ops
    from csu._lib import lib
    d = dev()
    B, H, C, N, k, s, p = case
    c = E.conv_case_sq(case)
    gm = ops._conv_geom(B, H, H, C, N, k, k, s, p)
    ran = 0
    for op, src, wt, bias, ref, image in _conv_ex_operands(c, d):
        ncols, cs = (N, C) if op == 0 else (C, N)
        for cfg, bn in E.IGEMM_DMA_BN.items():
            e, out = _conv_ex(op, gm, src, wt, bias, ref, cfg, d)
            if ncols % bn or cs % 64:
                assert e != 0, (op, cfg)
                continue
            assert e == 0, (op, cfg, lib().csu_last_error_string())
            check(out, ref, None, f"conv2d_ex {case} op {op} cfg {cfg}", image=image)
            ran += 1
        e, _ = _conv_ex(op, gm, src, wt, bias, ref, 20, d)
        assert e != 0, (op, 20)
    assert ran >= 8


@pytest.mark.parametrize("B,H,W", E.HALO64_SHAPES)
def test_conv2d_ex_halo64(B, H, W):
    from csu import ops
    from csu._lib import lib
    d = dev()
    c = E.conv_case(B, H, W, 64, 64, 3, 1, 1)
    gm = ops._conv_geom(B, H, W, 64, 64, 3, 3, 1, 1)
    for op, src, wt, bias, ref, image in _conv_ex_operands(c, d):
        e, out = _conv_ex(op, gm, src, wt, bias, ref, 20, d)
        if H % 2:
            assert e != 0      # H odd: not eligible
            continue
        assert e == 0, lib().csu_last_error_string()
        check(out, ref, None, f"conv2d_ex halo64 {(B, H, W)} op {op}", image=image)


@pytest.mark.parametrize("B,H,W", E.CONV_C16_SHAPES)
def test_conv2d_ex_c16(B, H, W):
    """The few-channel kernels of the CARAFE4 encoder (cfg 21 and the default dispatch), forward and input gradient;
    W % 64 != 0 is refused."""
    from csu import ops
    from csu._lib import lib
    d = dev()
    c = E.conv_case(B, H, W, 16, 144, 3, 1, 1)
    gm = ops._conv_geom(B, H, W, 16, 144, 3, 3, 1, 1)
    for op, src, wt, bias, ref, image in _conv_ex_operands(c, d):
        for cfg in (21, -1):
            e, out = _conv_ex(op, gm, src, wt, bias, ref, cfg, d)
            assert e == 0, lib().csu_last_error_string()
            check(out, ref, None, f"conv2d_ex c16 {(B, H, W)} op {op} cfg {cfg}", image=image)
    gm2 = ops._conv_geom(1, 8, 40, 16, 144, 3, 3, 1, 1)
    op, _, wt, bias, _, _ = _conv_ex_operands(c, d)[0]
    xs = torch.zeros(1, 8, 40, 16, dtype=BF, device=d)
    e, _ = _conv_ex(0, gm2, xs, wt, bias, torch.empty(1, 8, 40, 144), 21, d)
    assert e != 0


# ---------------------------------------------------------------------------------------------
# csu_conv2d_wgrad_ex: cfg 0..7, both output layouts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.CONV_WGRAD_CASES)
def test_conv2d_wgrad_ex(case):
    from csu import ops
    from csu._lib import lib, CSU_BF16
    d = dev()
    B, H, C, N, k, s, p = case
    c = E.conv_case_sq(case)
    refs = dict(zip(c["names"], c["refs"]))
    dw, db = refs["dW"], refs["db"]
    gm = ops._conv_geom(B, H, H, C, N, k, k, s, p)
    xd, dyd = put(c["x"], BF, d), put(c["gy"], BF, d)
    st = torch.cuda.current_stream().cuda_stream
    halo = k == 3 and s == 1 and p == 1 and H % 64 == 0 and C % 64 == 0
    ran = 0
    for cfg in range(0, 8):
        nws = lib().csu_conv2d_wgrad_workspace_ex(ctypes.byref(gm), cfg)
        if nws == 0:     # refused: the reasons test_conv_wgrad_cfgs states
            assert C % 8 or N % 8 or (cfg == 6 and not (halo and N % 64 == 0)) or (cfg == 7 and not (halo and N % 128 == 0))
            continue
        work = torch.empty(nws, dtype=torch.uint8, device=d)
        for creal, ref in ((0, torch.cat([dw.permute(0, 2, 3, 1).reshape(-1), db])), (C, torch.cat([dw.reshape(-1), db]))):
            out = torch.full((ref.numel(),), float("nan"), device=d)
            e = lib().csu_conv2d_wgrad_ex(ctypes.byref(gm), CSU_BF16, xd.data_ptr(), dyd.data_ptr(), creal,
                                          out.data_ptr(), work.data_ptr(), nws, cfg, st)
            assert e == 0, (cfg, lib().csu_last_error_string())
            torch.cuda.synchronize()
            nk = N * k * k * C
            layout = "OHWI" if creal == 0 else "OIHW"
            check(out[:nk].view(N, -1), ref[:nk].view(N, -1), None, f"conv2d_wgrad_ex {case} cfg {cfg} dW {layout} (N, rest)")
            check(out[nk:].view(1, -1), ref[nk:].view(1, -1), None, f"conv2d_wgrad_ex {case} cfg {cfg} db")
            ran += 1
    assert ran >= 2


# ---------------------------------------------------------------------------------------------
# the fused Mlp through the C ABI, ReLU regime
# ---------------------------------------------------------------------------------------------
def _mlp_operands(c, d):
    return {k: put(c[k], BF if k in ("x", "w1", "w2", "dy") else F32, d) for k in ("x", "w1", "b1", "w2", "b2", "res", "dy")}


def _no_drop(M):
    from csu.ops import MlpDrop
    md = MlpDrop(None, 0, 0, 0.0).c_struct()
    md.rows_per_sample = M
    return md


def _check_mlp(c, got, name):
    for k, t in got.items():
        ref = c["refs"][k]
        check(t.view(ref.shape) if ref.dim() == 2 else t.view(1, -1), ref if ref.dim() == 2 else ref.view(1, -1),
              c["tail"][k] if ref.dim() == 2 else c["tail"][k].view(1, -1), f"{name} {k}")


_MLP_FUSED = [(v, C, M) for v in ("default", "dp", "per_panel") for C, M in E.MLP_CASES if v != "per_panel" or C == 128]


@pytest.mark.parametrize("variant,C,M", _MLP_FUSED, ids=[f"{v}-{C}-{M}" for v, C, M in _MLP_FUSED])
def test_mlp_fused(C, M, variant):
    """csu_mlp_fwd / csu_mlp_bwd, csu_mlp_bwd_dp, and at C = 128 the per-panel backward csu_mlp_bwd_per_panel --
    at C = 64 also csu_mlp_bwd_wgrad, which forms dW1 / db1 / dW2 / db2 inside the kernel: y, g, dh, dx (and the
    four weight gradients) against the ReLU network.  The activations are even (exact_inputs.mlp_case), so no hidden
    value is -8 and every tail is exactly 0: with activations in {-2..2} the bf16 MFMA dot product, given the ~1e-14
    tails as addends, rounded a partial sum down by one ulp in 2 to 13 elements per tensor (dx 0 -> -1.9e-6 .. -7.6e-6,
    y -21 -> -21.0000076, dW2 168 -> 167.999985; the same through ops.gemm in every configuration), which is the matrix
    unit's arithmetic and not the kernels'."""
    from csu._lib import check as ok, lib, ptr, stream_ptr
    d = dev()
    L, st = lib(), stream_ptr(d)
    c = E.mlp_case(C, M)
    t = _mlp_operands(c, d)
    x, w1, b1, w2, b2, res, dy = (t[k] for k in ("x", "w1", "b1", "w2", "b2", "res", "dy"))
    y = torch.full((M, C), float("nan"), device=d)
    dh = torch.full((M, 4 * C), float("nan"), device=d, dtype=BF)
    g = torch.full((M, 4 * C), float("nan"), device=d, dtype=BF)
    dx = torch.full((M, C), float("nan"), device=d, dtype=BF)
    name = f"mlp {variant} {(C, M)}"
    if variant == "default":
        ok(L.csu_mlp_fwd(M, C, ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(res), ptr(y), st), "mlp_fwd")
        ok(L.csu_mlp_bwd(M, C, ptr(x), ptr(dy), ptr(w1), ptr(b1), ptr(w2), ptr(dh), ptr(g), ptr(dx), st), "mlp_bwd")
    elif variant == "per_panel":
        md = _no_drop(M)
        ok(L.csu_mlp_bwd_per_panel(M, C, ptr(x), ptr(dy), ptr(w1), ptr(b1), ptr(w2), ptr(dh), ptr(g), ptr(dx), ctypes.byref(md),
                                   st), "mlp_bwd_per_panel")
    else:
        ok(L.csu_mlp_bwd_dp(M, C, ptr(x), ptr(dy), ptr(w1), ptr(b1), ptr(w2), ptr(dh), ptr(g), ptr(dx), None, st), "mlp_bwd_dp")
    torch.cuda.synchronize()
    got = {"g": g, "dh": dh, "dx": dx}
    if variant == "default":
        got["y"] = y
    _check_mlp(c, got, name)
    if variant == "dp" and C == 64:
        from test_gpu_mlp_wgrad import _fused
        dx2, dw1, db1, dw2, db2 = _fused(M, x, dy, w1, b1, w2, None)
        _check_mlp(c, {"dx": dx2, "dW1": dw1, "db1": db1, "dW2": dw2, "db2": db2}, f"mlp bwd_wgrad {(C, M)}")
