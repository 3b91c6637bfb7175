"""Small-integer inputs, exact references and the failure report of the exact-integer parity tests
(test_gpu_exact_integer.py, test_exact_inputs.py).  Plain torch on the CPU; nothing here needs a GPU
or imports csu.

The idea: a linear kernel fed small integers has nothing to round.  Every product is exact in bf16
and fp32, every partial sum in any order is an integer far below 2^24, and every result is exactly
representable in the output type -- so the kernel must equal a float64 reference (exact as well: all
values are integers below 2^53) element for element, whatever its tiles, splits or summation order.

Linear recipe: activations in {-2..2}; weights in {-1, 0, 1} thinned to density min(1, 256 / Kred)
(Kred: the reduction length of the forward); biases and residuals in {-4..4}; upstream gradients in
{-1, 0, 1}.

ReLU regime for the GELU paths: on the lattice h = 16 j + 8 both GELUs of csrc/common.hpp give
gelu(h) = h and gelu'(h) = 1 exactly for h >= 8, and values of magnitude <= ~1e-12 for h <= -8
(test_exact_inputs.py shows it), so ReLU and the step function are the reference.  First-layer weights
are in {-16, 0, 16}, b1 = 8.  All values then lie on a lattice of `quantum` 8 or 16: bf16 holds
quantum * k exactly for |k| <= 256 and the fp32 sums are quantum times an integer sum, so the
conditions below are stated on value / quantum.  An element that ReLU zeroes ("inactive") is zero
by construction; the non-zero condition is asked of the active elements, and at least 40 % of all.
An output that a negative tail reaches (`tail`) may differ from the reference by <= 1e-6; every other
output is exact.

The fused Mlp takes its activations from {-2, 0, 2}, not {-2..2}: h then lies on 32 Z + 8, a subset of the
lattice whose negative points start at -24, where the kernels' GELU and GELU' are exactly 0 (exp2 underflows)
instead of ~-5e-15 / -4e-14 at h = -8.  Measured on the MI355X with activations in {-2..2}: the bf16 MFMA
dot product, given addends some 2^-40 below its partial sums, now and then returns a partial sum rounded down
by one ulp -- always towards -inf, always an exact power of two (-2^-19 .. -2^-16 on dx, y and dW2, 2 to 13
elements per tensor), i.e. up to 1.5e-5 where 1e-6 is allowed.  The Mlp kernels wrote the tails as predicted
(g = -5.2e-15, dh / dg = -4.0e-14); ops.gemm in every tile configuration, fed the dh they wrote, showed the same
errors, and none once the tails were zeroed.  That is the matrix unit's arithmetic, not a kernel's indexing or
accumulation, so the inputs avoid it -- no tolerance is added -- and the Mlp outputs are exact everywhere.
(The gemm prologue's own GELU, the erf form of csrc/gemm.hip, is exactly 0 at -8 and -16.)

preconditions() states, for every case, what makes the comparison exact; it is asserted on the CPU
for the very case lists the GPU tests run (test_exact_inputs.py)."""
import functools

import torch
import torch.nn.functional as F

TERMS_MAX = 2 ** 15      # sum |terms| / quantum per output element: nine bits under fp32's 2^24
BF16_INT_MAX = 256       # |ref| / quantum where the output is bf16 (8 significant bits)
NONZERO_MIN = 0.8
TAIL_ATOL = 1e-6         # > 1e3 x the largest tail sum (4C terms of 2048 * 1e-12), 1e-6 x the smallest real error


# ---------------------------------------------------------------------------------------------
# case lists (shared by the CPU and the GPU file)
# ---------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1000, 64, 64), (4099, 192, 64), (513, 256, 32), (300, 520, 1024), (1030, 520, 128)]   # (M, N, K)
GEMM_LINEAR_MODES = ["plain", "bias", "resid"]
GEMM_RELU_MODES = ["a_gelu", "gelu_aux"]
GEMM_CFGS = [0, 1, 2, 3, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19]    # test_gemm_tile_configs_and_gelu_out's list
GEMM_CFG_SHAPES = [(1000, 64, 64), (300, 520, 1024)]
GEMM_WS_SHAPES = [(192, 128, 128), (384, 192, 64), (1024, 384, 128), (1024, 256, 768)]
GEMM_WS_MODES = ["bf16_bias", "f32", "resid"]
GEMM_WS_LN_SHAPES = [(384, 64), (1024, 128), (192, 256)]            # (M, C): csu_gemm_ws_ln, y only
GEMM_F32_CASES = [(0, 4096, 192, 64), (0, 37, 64, 128), (0, 1000, 256, 1024), (1, 4096, 64, 192), (1, 300, 512, 128),
                  (2, 1024, 256, 4096), (2, 64, 16, 100)]           # (layout, M, N, K)
COLSUM_SHAPES = [(7, 40), (4099, 200), (1, 8)]
WGRAD_SHAPES = [(77, 64, 8), (700, 64, 64), (3001, 136, 200), (130, 1024, 256), (4099, 192, 64)]     # (M, N, K)
WGRAD_PLANS = [(64, 64, 1), (128, 128, 0), (128, 64, 5), (64, 128, 37), (0, 0, 0), (128, 128, 300)]  # (tn, tk, chunks)
WGRAD_PLAN_SHAPES = [(4099, 192, 64), (700, 32, 128)]
WGRAD_8WAVE = [(130, 256, 128, 1), (130, 256, 128, 2), (130, 256, 128, 0)]   # N % 256 == 0, K % 128 == 0: smallest
# deferred / grouped: square, rectangular 128x64 / 64x128 (N or K = 64), the 8-wave tile, ragged token counts
WGRAD_GROUPED = [(4099, 192, 64), (1000, 256, 64), (1001, 64, 256), (700, 256, 128), (100, 64, 64), (2050, 384, 128),
                 (513, 64, 128)]
LINEAR_CASES = [(1, 100, 64, 64), (3, 256, 256, 256)]               # (B, L, C, N)

_CONV_CASES_SOURCE = [  # (B, H, C, N, k, stride, pad): test_gpu_kernels.CONV_CASES
    (2, 32, 3, 64, 7, 4, 2), (2, 16, 64, 128, 3, 2, 1), (1, 8, 16, 144, 3, 1, 1), (2, 64, 16, 144, 3, 1, 1),
    (2, 9, 32, 36, 3, 1, 1), (16, 16, 128, 36, 3, 1, 1), (16, 32, 64, 36, 3, 1, 1), (1, 10, 32, 68, 3, 1, 1),
    (1, 12, 8, 24, 3, 1, 1), (2, 6, 40, 16, 1, 1, 0), (2, 11, 64, 128, 3, 2, 1), (1, 70, 64, 72, 3, 1, 1),
    (1, 13, 12, 20, 5, 3, 2),
]
# The two B = 16 entries exist for the K split of a few-tile launch (csrc/conv.hip ksplit_plan: 128 x 64
# tiles, split when the tiles are fewer than the CUs and K has >= 4 slices of 64).  B = 1 leaves 2 and 8
# tiles of 18 and 9 slices -- still split; the GPU test asserts it through csu_conv2d_workspace.
CONV_KSPLIT_CASES = [(1, 16, 128, 36, 3, 1, 1), (1, 32, 64, 36, 3, 1, 1)]
CONV_CASES = [c for c in _CONV_CASES_SOURCE if c[0] != 16] + CONV_KSPLIT_CASES
DMA_CONV_CASES = [(1, 20, 64, 256, 3, 1, 1), (2, 9, 128, 512, 3, 2, 1), (1, 12, 256, 256, 2, 2, 0), (2, 7, 64, 64, 1, 1, 0)]
IGEMM_DMA_BN = {1: 128, 2: 128, 3: 128, 4: 64, 5: 64, 6: 64, 7: 256, 8: 256, 9: 64, 10: 64, 11: 64, 12: 128}
HALO64_SHAPES = [(2, 64, 64), (1, 6, 128), (1, 5, 64)]              # (B, H, W); H odd: refused
CONV_WGRAD_CASES = DMA_CONV_CASES + [(2, 16, 64, 128, 3, 2, 1), (1, 70, 64, 72, 3, 1, 1), (2, 9, 32, 64, 3, 1, 1),
                                     (1, 64, 64, 128, 3, 1, 1)]
CONV_CAT_CASES = [(1, 64, 64, 64, 64), (1, 32, 64, 64, 64)]         # (B, H, Ca, Cb, N); H = 32: not eligible
CONV_C16_SHAPES = [(1, 5, 128), (2, 64, 64)]                        # (B, H, W)
CONVT_CASES = [(2, 8, 64, 32), (1, 5, 128, 64)]                     # (B, H, Cin, Cout)
MLP_CASES = [(64, 37), (64, 4096), (128, 1000), (256, 100), (256, 4160)]   # (C, M)


# ---------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------
def gen(*key):
    """A CPU generator seeded by the case."""
    seed = 20240
    for i, k in enumerate(key):
        seed = (seed * 1000003 + (i + 1) * int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ints(shape, lo, hi, g, density=1.0, nonzero=False):
    """Integer-valued float64 tensor with entries uniform in {lo..hi} from the CPU generator g;
    density < 1 zeroes each entry with probability 1 - density; nonzero turns a drawn 0 into 1."""
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g)
    if nonzero:
        t = torch.where(t == 0, torch.ones_like(t), t)
    if density < 1.0:
        t = t * (torch.rand(tuple(shape), generator=g) < density)
    return t.double()


def weight_density(kred, n=None):
    """min(1, 256 / Kred); for a conv with few output channels n at least 16 / n, so that every (c, ky, kx)
    index of the weight is used by some output channel (at 36 channels and density 0.22 some were not)."""
    d = 256.0 / kred
    if n is not None:
        d = max(d, 16.0 / n)
    return min(1.0, d)


def lattice(shape, g):
    """Entries in {+-8, +-16}: the operand of gemm(a_gelu=True) and the gelu_aux tensor."""
    return ints(shape, 1, 2, g) * 8 * (ints(shape, 0, 1, g) * 2 - 1)


# ---------------------------------------------------------------------------------------------
# conditions and the failure report
# ---------------------------------------------------------------------------------------------
def covered(t, name="operand"):
    """Every row and every column of the operand (seen as (-1, last dim)) holds a non-zero entry."""
    t2 = t.reshape(-1, t.shape[-1])
    assert bool((t2 != 0).any(1).all()), f"{name}: a row is all zero"
    assert bool((t2 != 0).any(0).all()), f"{name}: a column is all zero"


def preconditions(ref, terms_l1, out_dtype, operands=(), quantum=1, active=None):
    """The conditions under which `ref` must be reproduced exactly; asserts them and returns the
    figures (max sum|terms| / quantum, max |ref| / quantum, non-zero fraction).
      * sum |terms| <= 2^15 quantum for every output element;
      * ref is a multiple of quantum, and |ref| <= 256 quantum where the output is bf16;
      * >= 80 % of the reference is non-zero (of the `active` elements where ReLU zeroes the rest, which
        must then be zero, and >= 40 % of all);
      * every operand in `operands` (2-D views; (name, tensor) pairs) is `covered`."""
    ref, terms_l1 = ref.double(), terms_l1.double()
    assert ref.shape == terms_l1.shape
    assert bool((ref.abs() <= terms_l1).all())
    tmax = float(terms_l1.max()) / quantum
    rmax = float(ref.abs().max()) / quantum
    assert tmax <= TERMS_MAX, f"sum|terms| / quantum = {tmax}"
    assert bool((torch.remainder(ref, quantum) == 0).all()), "reference off the lattice"
    if out_dtype == torch.bfloat16:
        assert rmax <= BF16_INT_MAX, f"|ref| / quantum = {rmax}"
        assert torch.equal(ref.bfloat16().double(), ref)
    else:
        assert torch.equal(ref.float().double(), ref)
    if active is None:
        nz = float((ref != 0).double().mean())
    else:
        assert not bool(ref[~active].any())
        nz = float((ref[active] != 0).double().mean())
        assert float((ref != 0).double().mean()) >= NONZERO_MIN / 2
    assert nz >= NONZERO_MIN, f"non-zero fraction {nz}"
    for name, t in operands:
        covered(t, name)
    return {"terms": tmax, "ref": rmax, "nonzero": nz}


def first_mismatch(got, ref, tile=(64, 64), image=None):
    """None if got == ref in value; else a dict describing the difference on the (rows, cols) view
    (-1, last dim): `count`; `first` = (row, col) of the first differing element and `tile` = its tile
    coordinates; `got` / `expected` there; `coords` of the first 16; whether all of them fall in the
    last row tile / last column tile; and, with image = (B, H, W) describing the rows, whether all lie
    in the last batch item / on the image border."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    g2, r2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    bad = (g2 != r2).nonzero()               # NaN != anything: an unwritten (poisoned) element is reported
    if bad.numel() == 0:
        return None
    rows, cols = g2.shape
    r, c = int(bad[0, 0]), int(bad[0, 1])
    rep = {"count": int(bad.shape[0]), "shape": (rows, cols), "first": (r, c), "tile": (r // tile[0], c // tile[1]),
           "got": float(g2[r, c]), "expected": float(r2[r, c]), "coords": [tuple(x) for x in bad[:16].tolist()],
           "all_in_last_row_tile": bool((bad[:, 0] // tile[0] == (rows - 1) // tile[0]).all()),
           "all_in_last_col_tile": bool((bad[:, 1] // tile[1] == (cols - 1) // tile[1]).all())}
    if image is not None:
        B, H, W = image
        assert B * H * W == rows
        b, y, x = bad[:, 0] // (H * W), bad[:, 0] // W % H, bad[:, 0] % W
        rep["all_in_last_batch"] = bool((b == B - 1).all())
        rep["all_on_image_border"] = bool(((y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)).all())
    return rep


def assert_exact(got, ref, name="", tile=(64, 64), image=None):
    """torch.equal(got.double().cpu(), ref.double()) -- equality in value, -0 == 0 -- with
    first_mismatch's report on failure."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    if g.shape == r.shape and torch.equal(g, r):
        return
    raise AssertionError(f"{name}: {first_mismatch(g, r, tile, image)}")


def assert_relu_regime(got, ref, tail, name="", tile=(64, 64)):
    """Exact wherever no negative GELU tail contributes (`tail` False); |got - ref| <= 1e-6 elsewhere."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    assert g.shape == r.shape, (name, tuple(g.shape), tuple(r.shape))
    tail = tail.expand_as(r) if tail.shape != r.shape else tail
    ok = torch.where(tail, (g - r).abs() <= TAIL_ATOL, g == r)
    if bool(ok.all()):
        return
    rep = first_mismatch(torch.where(ok, r, g), r, tile)
    raise AssertionError(f"{name}: {rep}")


# ---------------------------------------------------------------------------------------------
# references.  Every op here is bilinear, so float64 autograd gives the exact gradients, and the same
# function on the absolute values gives sum |terms| of the output and of every gradient.
# ---------------------------------------------------------------------------------------------
def _bilinear(fn, ins, gy):
    """(y, grads...) of y = fn(*ins), y.backward(gy), in float64."""
    ins = [t.detach().double().clone().requires_grad_(True) for t in ins]
    y = fn(*ins)
    y.backward(gy.double())
    return [y.detach()] + [t.grad for t in ins]


def _with_terms(fn, ins, gy):
    return _bilinear(fn, ins, gy), _bilinear(fn, [t.abs() for t in ins], gy.abs())


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K, mode):
    """ops.gemm operands (a (M, K), w (N, K): pass w or w.t() for b_trans) and the reference.
    plain / bias / resid: the linear recipe.  a_gelu: a in {+-8, +-16}, gelu(a) -> relu(a); bias in 8 Z.
    gelu_aux: out = (a w^T) gelu'(aux) -> (a w^T) step(aux)."""
    g = gen(M, N, K, (GEMM_LINEAR_MODES + GEMM_RELU_MODES).index(mode))
    c = {"bias": None, "aux": None, "res": None, "tail": None, "active": None, "quantum": 1,
         "odt": torch.float32 if mode == "resid" else torch.bfloat16}
    if mode == "a_gelu":
        a = lattice((M, K), g)
        w = ints((N, K), -1, 1, g, min(1.0, 128.0 / K))
        c["bias"] = ints((N,), -4, 4, g) * 8
        ae = a.clamp_min(0)
        c["ref"] = ae @ w.t() + c["bias"]
        c["terms"] = ae @ w.abs().t() + c["bias"].abs()
        c["tail"] = ((a < 0).double() @ w.abs().t()) > 0
        c["quantum"] = 8
    else:
        a = ints((M, K), -2, 2, g)
        w = ints((N, K), -1, 1, g, weight_density(K))
        c["ref"] = a @ w.t()
        c["terms"] = a.abs() @ w.abs().t()
        if mode == "bias":
            c["bias"] = ints((N,), -4, 4, g)
            c["ref"], c["terms"] = c["ref"] + c["bias"], c["terms"] + c["bias"].abs()
        if mode == "resid":
            c["res"] = ints((M, N), -4, 4, g)
            c["ref"], c["terms"] = c["ref"] + c["res"], c["terms"] + c["res"].abs()
        if mode == "gelu_aux":
            c["aux"] = lattice((M, N), g)
            c["active"] = c["aux"] > 0
            c["tail"] = ~c["active"]
            c["ref"] = c["ref"] * c["active"]
    c["a"], c["w"] = a, w
    c["operands"] = (("a", a), ("w", w))
    return c


@functools.lru_cache(maxsize=None)
def gemm_gelu_out_case(M, N, K):
    """gemm(gelu_out=True): h = a w^T + 8 on the lattice 16 Z + 8, gelu(h) -> relu(h)."""
    g = gen(M, N, K, 77)
    a = ints((M, K), -2, 2, g)
    w = ints((N, K), -1, 1, g, min(1.0, 32.0 / K)) * 16
    bias = torch.full((N,), 8.0, dtype=torch.float64)
    h = a @ w.t() + bias
    assert bool((torch.remainder(h, 16) == 8).all())
    return {"a": a, "w": w, "bias": bias, "h": h, "terms": a.abs() @ w.abs().t() + 8, "gh": h.clamp_min(0),
            "active": h > 0, "tail": h < 0, "quantum": 8, "operands": (("a", a), ("w", w))}


@functools.lru_cache(maxsize=None)
def linear_fwd_case(M, N, K, mode):
    """x (M, K), w (N, K), optional bias / resid of a forward-only token GEMM (gemm_ws, gemm_f32 layout 0)."""
    g = gen(M, N, K, 5, len(mode))
    x = ints((M, K), -2, 2, g)
    w = ints((N, K), -1, 1, g, weight_density(K))
    bias = ints((N,), -4, 4, g) if mode in ("bf16_bias", "resid") else None
    res = ints((M, N), -4, 4, g) if mode == "resid" else None
    ref, terms = x @ w.t(), x.abs() @ w.abs().t()
    if bias is not None:
        ref, terms = ref + bias, terms + bias.abs()
    if res is not None:
        ref, terms = ref + res, terms + res.abs()
    return {"x": x, "w": w, "bias": bias, "res": res, "ref": ref, "terms": terms,
            "odt": torch.bfloat16 if mode == "bf16_bias" else torch.float32, "operands": (("x", x), ("w", w))}


@functools.lru_cache(maxsize=None)
def gemm_f32_case(layout, M, N, K):
    """csu_gemm_f32: 0 C = A B^T + bias + resid, 1 C = A B, 2 C = A^T B and asum = sum_k A[k][m]."""
    g = gen(layout, M, N, K, 9)
    if layout == 0:
        c = dict(linear_fwd_case(M, N, K, "resid"))
        c["a"], c["b"] = c["x"], c["w"]
        return c
    if layout == 1:
        a, b = ints((M, K), -2, 2, g), ints((K, N), -1, 1, g, weight_density(K))
        return {"a": a, "b": b, "ref": a @ b, "terms": a.abs() @ b.abs(), "operands": (("a", a), ("b", b))}
    a, b = ints((K, M), -1, 1, g), ints((K, N), -2, 2, g)       # the weight gradient: A = dy, B = x
    return {"a": a, "b": b, "ref": a.t() @ b, "terms": a.abs().t() @ b.abs(), "asum": a.sum(0), "asum_terms": a.abs().sum(0),
            "operands": (("a", a), ("b", b))}


@functools.lru_cache(maxsize=None)
def colsum_case(rows, cols):
    """x in {-2, -1, 1, 2}: with a 0 in the set a single-row sum would be zero a fifth of the time."""
    x = ints((rows, cols), -2, 2, gen(rows, cols, 3), nonzero=True)
    return {"x": x, "ref": x.sum(0), "terms": x.abs().sum(0)}


@functools.lru_cache(maxsize=None)
def wgrad_case(M, N, K):
    """dy (M, N) in {-1, 0, 1}, x (M, K) in {-2..2}; dW = dy^T x, db = colsum(dy)."""
    g = gen(M, N, K, 11)
    dy, x = ints((M, N), -1, 1, g), ints((M, K), -2, 2, g)
    return {"dy": dy, "x": x, "dw": dy.t() @ x, "dw_terms": dy.abs().t() @ x.abs(), "db": dy.sum(0), "db_terms": dy.abs().sum(0),
            "operands": (("dy", dy), ("x", x))}


@functools.lru_cache(maxsize=None)
def linear_case(B, L, C, N, concat):
    """nn.Linear on (B, L, C) tokens (concat: on cat([skip, up], -1), weight (N, 2C)) through autograd:
    refs / terms = [y, dx (or dskip, dup), dW, db]."""
    g = gen(B, L, C, N, int(concat))
    Kin = 2 * C if concat else C
    w, b = ints((N, Kin), -1, 1, g, weight_density(Kin)), ints((N,), -4, 4, g)
    gy = ints((B, L, N), -1, 1, g)
    if concat:
        skip, up = ints((B, L, C), -2, 2, g), ints((B, L, C), -2, 2, g)
        refs, terms = _with_terms(lambda s, u, w_, b_: F.linear(torch.cat([s, u], -1), w_, b_), [skip, up, w, b], gy)
        return {"skip": skip, "up": up, "w": w, "b": b, "gy": gy, "refs": refs, "terms": terms,
                "names": ["y", "dskip", "dup", "dW", "db"], "operands": (("skip", skip), ("up", up), ("w", w), ("gy", gy))}
    x = ints((B, L, C), -2, 2, g)
    refs, terms = _with_terms(F.linear, [x, w, b], gy)
    return {"x": x, "w": w, "b": b, "gy": gy, "refs": refs, "terms": terms, "names": ["y", "dx", "dW", "db"],
            "operands": (("x", x), ("w", w), ("gy", gy))}


@functools.lru_cache(maxsize=None)
def conv_case(B, H, W, C, N, k, s, p):
    """x (B, H, W, C) NHWC, w (N, C, k, k), b (N), gy (B, OH, OW, N); refs / terms = [y, dx, dW, db] with y and
    dx NHWC and dW in torch's (N, C, k, k)."""
    g = gen(B, H, W, C, N, k, s, p)
    x = ints((B, H, W, C), -2, 2, g)
    w = ints((N, C, k, k), -1, 1, g, weight_density(C * k * k, N))
    b = ints((N,), -4, 4, g)
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    gy = ints((B, OH, OW, N), -1, 1, g)

    def fn(x_, w_, b_):
        return F.conv2d(x_.permute(0, 3, 1, 2), w_, b_, stride=s, padding=p).permute(0, 2, 3, 1)
    refs, terms = _with_terms(fn, [x, w, b], gy)
    # an input pixel no output reads has a zero gradient by construction, not by chance
    reach = _bilinear(fn, [torch.ones_like(x), torch.ones_like(w), torch.zeros_like(b)], torch.ones_like(gy))[1] > 0
    return {"x": x, "w": w, "b": b, "gy": gy, "refs": refs, "terms": terms, "names": ["y", "dx", "dW", "db"], "reach": reach,
            "geom": (B, H, W, C, N, k, s, p, OH, OW),
            "operands": (("x", x.reshape(B * H, W * C)), ("w", w.permute(0, 2, 3, 1).reshape(N, -1)), ("gy", gy))}


def conv_case_sq(case):
    B, H, C, N, k, s, p = case
    return conv_case(B, H, H, C, N, k, s, p)


@functools.lru_cache(maxsize=None)
def convt_case(B, H, Cin, Cout):
    """ConvTranspose2d(Cin, Cout, 2, 2) on (B, H, H, Cin): refs / terms = [y, dx, dW (Cin, Cout, 2, 2), db]."""
    g = gen(B, H, Cin, Cout, 2)
    x = ints((B, H, H, Cin), -2, 2, g)
    w = ints((Cin, Cout, 2, 2), -1, 1, g, weight_density(Cin))
    b = ints((Cout,), -4, 4, g)
    gy = ints((B, 2 * H, 2 * H, Cout), -1, 1, g)

    def fn(x_, w_, b_):
        return F.conv_transpose2d(x_.permute(0, 3, 1, 2), w_, b_, stride=2).permute(0, 2, 3, 1)
    refs, terms = _with_terms(fn, [x, w, b], gy)
    return {"x": x, "w": w, "b": b, "gy": gy, "refs": refs, "terms": terms, "names": ["y", "dx", "dW", "db"],
            "operands": (("x", x), ("w", w.permute(0, 2, 3, 1).reshape(Cin, -1)), ("w^T", w.reshape(Cin, -1).t()), ("gy", gy))}


MLP_OUT = ("y", "g", "dh", "dx", "dW1", "db1", "dW2", "db2")
MLP_QUANTUM = {"y": 1, "g": 8, "dh": 1, "dx": 16, "dW1": 1, "db1": 1, "dW2": 8, "db2": 1}
MLP_DTYPE = {"y": torch.float32, "g": torch.bfloat16, "dh": torch.bfloat16, "dx": torch.bfloat16, "dW1": torch.float32,
             "db1": torch.float32, "dW2": torch.float32, "db2": torch.float32}


@functools.lru_cache(maxsize=None)
def mlp_case(C, M):
    """The fused Mlp y = res + fc2(gelu(fc1 x)) in the ReLU regime: x in {-2, 0, 2} (h on 32 Z + 8: no tail at
    h = -8, see the module docstring), W1 in {-16, 0, 16} at
    density min(1, 32 / C) (|h| stays below 2048 and dx = dh W1, on the lattice 16 Z, within 256 * 16), b1 = 8,
    W2 in {-1, 0, 1} at density min(1, 96 / C) (dense enough that dy W2 is rarely 0), b2 and res in {-4..4},
    dy in {-1, 0, 1}.  refs / terms / tail / active per MLP_OUT name."""
    g = gen(C, M, 13)
    x = ints((M, C), -1, 1, g) * 2
    w1 = ints((4 * C, C), -1, 1, g, min(1.0, 32.0 / C)) * 16
    b1 = torch.full((4 * C,), 8.0, dtype=torch.float64)
    w2 = ints((C, 4 * C), -1, 1, g, min(1.0, 96.0 / C))
    b2, res = ints((C,), -4, 4, g), ints((M, C), -4, 4, g)
    dy = ints((M, C), -1, 1, g)
    h = x @ w1.t() + b1
    assert bool((torch.remainder(h, 32) == 8).all()) and float(h.abs().max()) <= 2048
    on = h > 0
    gl = h * on
    dg, dg_l1 = dy @ w2, dy.abs() @ w2.abs()
    dh, dh_l1 = dg * on, dg_l1 * on
    da = dh.abs()      # dh is materialised (an exact small integer in bf16): the later sums' terms are |dh| |.|
    refs = {"y": res + gl @ w2.t() + b2, "g": gl, "dh": dh, "dx": dh @ w1, "dW1": dh.t() @ x, "db1": dh.sum(0),
            "dW2": dy.t() @ gl, "db2": dy.sum(0)}
    terms = {"y": res.abs() + gl @ w2.abs().t() + b2.abs(), "g": x.abs() @ w1.abs().t() + 8, "dh": dh_l1,
             "dx": da @ w1.abs(), "dW1": da.t() @ x.abs(), "db1": da.sum(0), "dW2": dy.abs().t() @ gl,
             "db2": dy.abs().sum(0)}
    off = (~on).double()
    # an output is reached by a tail when an inactive hidden unit feeds it through a non-zero weight
    tail = {"y": (off @ w2.abs().t()) > 0, "g": ~on, "dh": ~on & (dg_l1 > 0), "dx": ((off * dg_l1) @ w1.abs()) > 0,
            "dW1": ((off * dg_l1).t() @ x.abs()) > 0, "db1": (off * dg_l1).sum(0) > 0, "dW2": (dy.abs().t() @ off) > 0,
            "db2": torch.zeros(C, dtype=torch.bool)}
    active = {"g": on, "dh": on}
    return {"x": x, "w1": w1, "b1": b1, "w2": w2, "b2": b2, "res": res, "dy": dy, "h": h, "refs": refs, "terms": terms,
            "tail": tail, "active": active,
            "operands": (("x", x), ("w1", w1), ("w2", w2), ("dy", dy))}


# ---------------------------------------------------------------------------------------------
# every reference the GPU file compares against, per family: (label, ref, sum|terms|, output dtype, quantum,
# active mask or None, operands).  test_exact_inputs.py asserts preconditions() on all of them.
# ---------------------------------------------------------------------------------------------
FAMILIES = ("gemm", "gemm_ws", "gemm_f32", "colsum", "linear_wgrad", "linear", "conv2d", "conv2d_ex", "conv2d_wgrad_ex",
            "conv_other", "mlp")
_BF, _F32 = torch.bfloat16, torch.float32


def _grad_checks(label, c, dtypes):
    """y / dx / dW / db style cases: one check per output; dtypes = the narrowest type each is held in."""
    for name, ref, terms, dt in zip(c["names"], c["refs"], c["terms"], dtypes):
        active = None
        if name == "dx" and "reach" in c and not bool(c["reach"].all()):
            active = c["reach"]
        yield f"{label} {name}", ref, terms, dt, 1, active, c["operands"] if name == "y" else ()


def family_checks(family):
    if family == "gemm":
        for M, N, K in GEMM_SHAPES:
            for mode in GEMM_LINEAR_MODES + GEMM_RELU_MODES:
                c = gemm_case(M, N, K, mode)
                yield f"{(M, N, K)} {mode}", c["ref"], c["terms"], c["odt"], c["quantum"], c["active"], c["operands"]
        for M, N, K in GEMM_CFG_SHAPES:
            c = gemm_gelu_out_case(M, N, K)
            yield f"{(M, N, K)} h", c["h"], c["terms"], _BF, 8, None, c["operands"]
            yield f"{(M, N, K)} gelu(h)", c["gh"], c["terms"], _BF, 8, c["active"], ()
    elif family == "gemm_ws":
        for M, N, K in GEMM_WS_SHAPES:
            for mode in GEMM_WS_MODES:
                c = linear_fwd_case(M, N, K, mode)
                yield f"{(M, N, K)} {mode}", c["ref"], c["terms"], c["odt"], 1, None, c["operands"]
        for M, C in GEMM_WS_LN_SHAPES:
            c = linear_fwd_case(M, C, C, "resid")
            yield f"ln {(M, C)}", c["ref"], c["terms"], _F32, 1, None, c["operands"]
    elif family == "gemm_f32":
        for case in GEMM_F32_CASES:
            c = gemm_f32_case(*case)
            yield f"{case}", c["ref"], c["terms"], _F32, 1, None, c["operands"]
            if case[0] == 2:
                yield f"{case} asum", c["asum"], c["asum_terms"], _F32, 1, None, ()
    elif family == "colsum":
        for shape in COLSUM_SHAPES:
            c = colsum_case(*shape)
            yield f"{shape}", c["ref"], c["terms"], _F32, 1, None, ()
    elif family == "linear_wgrad":
        for shape in sorted(set(WGRAD_SHAPES + WGRAD_PLAN_SHAPES + [s[:3] for s in WGRAD_8WAVE] + WGRAD_GROUPED)):
            c = wgrad_case(*shape)
            yield f"{shape} dW", c["dw"], c["dw_terms"], _F32, 1, None, c["operands"]
            yield f"{shape} db", c["db"], c["db_terms"], _F32, 1, None, ()
    elif family == "linear":
        for case in LINEAR_CASES:
            yield from _grad_checks(f"linear {case}", linear_case(*case, False), (_BF, _BF, _F32, _F32))
            yield from _grad_checks(f"concat_linear {case}", linear_case(*case, True), (_F32, _BF, _BF, _F32, _F32))
    elif family == "conv2d":
        for case in CONV_CASES:
            yield from _grad_checks(f"{case}", conv_case_sq(case), (_BF, _BF, _F32, _F32))
    elif family == "conv2d_ex":
        for case in DMA_CONV_CASES:
            yield from _grad_checks(f"{case}", conv_case_sq(case), (_BF, _BF, _F32, _F32))
        for B, H, W in HALO64_SHAPES:
            if H % 2 == 0:
                yield from _grad_checks(f"halo64 {(B, H, W)}", conv_case(B, H, W, 64, 64, 3, 1, 1), (_BF, _BF, _F32, _F32))
    elif family == "conv2d_wgrad_ex":
        for case in CONV_WGRAD_CASES:
            yield from _grad_checks(f"{case}", conv_case_sq(case), (_BF, _BF, _F32, _F32))
    elif family == "conv_other":
        for B, H, Ca, Cb, N in CONV_CAT_CASES:
            yield from _grad_checks(f"cat {(B, H, Ca, Cb, N)}", conv_case(B, H, H, Ca + Cb, N, 3, 1, 1), (_BF, _BF, _F32, _F32))
        for B, H, W in CONV_C16_SHAPES:
            yield from _grad_checks(f"c16 {(B, H, W)}", conv_case(B, H, W, 16, 144, 3, 1, 1), (_BF, _BF, _F32, _F32))
        for case in CONVT_CASES:
            yield from _grad_checks(f"convT {case}", convt_case(*case), (_BF, _BF, _F32, _F32))
    elif family == "mlp":
        for C, M in MLP_CASES:
            c = mlp_case(C, M)
            for name in MLP_OUT:
                yield (f"{(C, M)} {name}", c["refs"][name], c["terms"][name], MLP_DTYPE[name], MLP_QUANTUM[name],
                       c["active"].get(name), c["operands"] if name == "y" else ())
    else:
        raise KeyError(family)


def family_figures(family):
    """(number of references, largest sum|terms| / quantum, largest |ref| / quantum) of a family."""
    figs = [preconditions(ref, terms, dt, ops_, q, act) for _, ref, terms, dt, q, act, ops_ in family_checks(family)]
    return len(figs), max(f["terms"] for f in figs), max(f["ref"] for f in figs)
