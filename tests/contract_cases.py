"""The table behind tests/test_gpu_autograd_contract.py and tests/test_contract_cases.py: one entry per
differentiable op of csu.ops, csu.unet and csu.simam.  Plain torch on the CPU; nothing here needs a GPU.

An entry (``Case``) gives
  * ``build(seed)``: seeded CPU inputs -- ``acts`` (the differentiable activations, in the dtype the op
    receives), ``params`` (the fp32 parameters, in the order of the op's signature) and ``aux`` (targets,
    running statistics, geometry: not differentiated);
  * ``call(m, a, p, x)``: the op on device tensors; ``m`` carries the csu modules (m.ops, m.simam, m.unet,
    m.rng), ``a`` / ``p`` the placed acts / params, ``x`` the aux (with what ``gpu_aux`` added).  Returns the
    differentiable outputs as a tuple;
  * ``ref(a, p, x)``: the same operation on fp64 tensors in plain torch, differentiable, from the references
    the suite already has (stress_inputs, oracle.cswin_ref / fp8_ref, the loss references of test_seg_loss,
    test_seg_ce and test_boundary, test_gpu_unet._ref_bn);
  * ``tol``: torch.float32 or torch.bfloat16 -- which criterion of test_gpu_kernels.assert_close applies;
  * ``gpu_aux(m, x)``: what must be read back from the device for the reference (dropout masks: a function
    of (snapshot, site), read back as the dropout tests do);
  * ``setup(m, p, x)``: a context manager around every forward (the cast cache of the ops that need one,
    set up as their own tests do);
  * ``switches``: csu.ops module switches held for the whole test (SIDE_WGRAD off for the in-kernel weight
    gradients of the C = 64 Mlp);
  * ``defers``: the op's parameter gradients are written by another KERNEL when they may not be deferred to
    the end of backward (an existing .grad, a hook, a shared weight, create_graph) or when the side stream is
    off: the grouped / batched end-of-backward launches sum in another order than the inline ones.  For such
    an op the bitwise comparison with the plain call covers outputs and activation gradients (``fused_dx``:
    not even those: the C = 64 Mlp's in-kernel weight gradients come from another backward kernel than the
    two-step path), the fp64 criterion covers everything;
  * ``stats_call``: the with_stats form of a loss (pattern E); ``nout``: the number of differentiable outputs.

Shapes are each op's smallest case in tests/test_gpu_guard_bands.py.  ``not_applicable(case, pattern)`` is the
written reason why a pattern of tests/test_gpu_autograd_contract.py does not apply to an op (None: it applies).

Pattern B's view constructors are here too (``LAYOUTS``): each takes a contiguous tensor and an allocator
``new(shape, dtype)`` and returns a view equal in value that is non-contiguous or at a storage offset."""
import contextlib
import types

import torch
import torch.nn.functional as F

import stress_inputs as S

F32, BF16 = torch.float32, torch.bfloat16
NS = types.SimpleNamespace
EPS = 1e-5


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape, scale=1.0, shift=0.0, dtype=F32):
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype)


class Case:
    def __init__(self, name, build, call, ref, tol, *, autocast=False, gpu_aux=None, setup=None, switches=None,
                 defers=False, fused_dx=False, stats_call=None, nout=1):
        self.name, self.build, self.call, self.ref, self.tol = name, build, call, ref, tol
        self.autocast, self.gpu_aux, self.setup, self.switches = autocast, gpu_aux, setup, dict(switches or {})
        self.defers, self.fused_dx, self.stats_call, self.nout = defers, fused_dx, stats_call, nout

    def __repr__(self):
        return f"Case({self.name})"


def inputs(acts, params=None, **aux):
    return NS(acts=dict(acts), params=dict(params or {}), aux=dict(aux))


# ---------------------------------------------------------------------------------------------
# pattern B: views equal in value to a contiguous tensor
# ---------------------------------------------------------------------------------------------
def batch_dim(t):
    """The dim the step-2 slice runs along: the batch, or for a batch of one the first dim of size > 1
    (a stride on a dim of size one is no layout at all)."""
    for d in range(t.dim()):
        if t.shape[d] > 1:
            return d
    raise ValueError("a tensor of one element has no layout")


def view_wider(t, new):
    """t as big[..., :C] of a buffer with 8 more elements in the last dim."""
    big = new(t.shape[:-1] + (t.shape[-1] + 8,), t.dtype)
    big.zero_()
    big[..., :t.shape[-1]] = t
    return big[..., :t.shape[-1]]


def view_step2(t, new):
    """t as big[::2] along batch_dim(t) of a buffer twice as long there."""
    d = batch_dim(t)
    shape = list(t.shape)
    shape[d] *= 2
    big = new(tuple(shape), t.dtype)
    big.zero_()
    idx = [slice(None)] * t.dim()
    idx[d] = slice(None, None, 2)
    big[tuple(idx)] = t
    return big[tuple(idx)]


def view_transposed(t, new):
    """t stored with its last two dims swapped, seen through the transpose back."""
    store = new(t.transpose(-1, -2).shape, t.dtype)
    store.copy_(t.transpose(-1, -2))
    return store.transpose(-1, -2)


def view_offset(t, new):
    """t contiguous, 8 elements (16 B in bf16, 32 B in fp32) into its storage."""
    buf = new((t.numel() + 8,), t.dtype)
    buf.zero_()
    v = buf[8:].view(t.shape)
    v.copy_(t)
    return v


LAYOUTS = {"wider": view_wider, "step2": view_step2, "transposed": view_transposed, "offset": view_offset}


# ---------------------------------------------------------------------------------------------
# references that are (loss, gradient) pairs in the suite: wrapped so that fp64 autograd can use them
# ---------------------------------------------------------------------------------------------
class _RefLoss(torch.autograd.Function):
    """fn(z) -> (loss, d loss / dz) of an existing loss reference as a differentiable fp64 scalar."""

    @staticmethod
    def forward(ctx, z, fn):
        with torch.enable_grad():       # the references differentiate their Tversky / boundary parts by autograd
            loss, grad = fn(z.detach())
        ctx.save_for_backward(grad.to(z.dtype))
        return loss.detach().to(z.dtype).reshape(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return g * grad, None


# ---------------------------------------------------------------------------------------------
# stripe attention
# ---------------------------------------------------------------------------------------------
def _attn_one(name, case, dtype, drop=False):
    reso, idx, sw, cb, heads, B = case
    hs, ws = S.stripe_geometry(reso, idx, sw)
    scale = (cb // heads) ** -0.5

    def build(seed=0):
        g = _g(1000 + 7 * reso + cb + seed)
        return inputs({"qkv": _rn(g, B, reso * reso, 3 * cb, dtype=dtype)},
                      {"lepe_w": _rn(g, cb, 1, 3, 3, scale=0.3), "lepe_b": _rn(g, cb, scale=0.1)})

    def call(m, a, p, x):
        geom = m.ops.StripeGeometry(reso, cb, heads, [(hs, ws, 0)], scale)
        return (m.ops.stripe_attention(a["qkv"], geom, [p["lepe_w"]], [p["lepe_b"]], x.get("drop")),)

    def ref(a, p, x):
        q = a["qkv"]
        return (S.lepe_attention_plain(q[..., :cb], q[..., cb:2 * cb], q[..., 2 * cb:], reso, hs, ws, heads, p["lepe_w"],
                                       p["lepe_b"], scale, attn_mask=x.get("attn_mask")),)

    def gpu_aux(m, x):
        from test_gpu_dropout import _attn_provider
        snap = torch.tensor([77, 1], dtype=torch.int64, device=m.dev)
        return {"drop": m.ops.AttnDrop(snap, 40, 0.3), "attn_mask": _attn_provider(snap, 40, 0.3, None)}

    return Case(name, build, call, ref, dtype, gpu_aux=gpu_aux if drop else None, defers=True)


def _attn_two(name, dtype):
    reso, C, heads, sw, B = 16, 64, 2, 2, 2
    scale = (C // heads) ** -0.5

    def build(seed=0):
        g = _g(1100 + seed)
        ps = {}
        for i in range(2):
            ps[f"lepe_w{i}"] = _rn(g, C // 2, 1, 3, 3, scale=0.3)
        for i in range(2):
            ps[f"lepe_b{i}"] = _rn(g, C // 2, scale=0.1)
        return inputs({"qkv": _rn(g, B, reso * reso, 3 * C, dtype=dtype)}, ps)

    def call(m, a, p, x):
        geom = m.ops.StripeGeometry(reso, C, heads // 2, [(reso, sw, 0), (sw, reso, C // 2)], scale)
        return (m.ops.stripe_attention(a["qkv"], geom, [p["lepe_w0"], p["lepe_w1"]], [p["lepe_b0"], p["lepe_b1"]]),)

    def ref(a, p, x):
        q = a["qkv"]
        outs = []
        for i, sl in enumerate((slice(0, C // 2), slice(C // 2, C))):
            hs, ws = S.stripe_geometry(reso, i, sw)
            outs.append(S.lepe_attention_plain(q[..., :C][..., sl], q[..., C:2 * C][..., sl], q[..., 2 * C:][..., sl], reso,
                                               hs, ws, heads // 2, p[f"lepe_w{i}"], p[f"lepe_b{i}"], scale))
        return (torch.cat(outs, -1),)

    return Case(name, build, call, ref, dtype, defers=True)


# ---------------------------------------------------------------------------------------------
# dropout, LayerNorm
# ---------------------------------------------------------------------------------------------
def _dropout():
    B, L, C, p_, site = 3, 37, 72, 0.3, 9

    def build(seed=0):
        g = _g(1200 + seed)
        return inputs({"x": _rn(g, B, L, C), "res": _rn(g, B, L, C)})

    def call(m, a, p, x):
        return (m.ops.dropout(a["x"], p_, site, x["snap"], row_scale=x["rs"], rows_per_sample=L, residual=a["res"]),)

    def ref(a, p, x):
        mask, rs = x.get("mask", 1.0), x.get("rs64", 1.0)
        return (a["res"] + rs * mask * a["x"],)

    def gpu_aux(m, x):
        snap = torch.tensor([11, 3], dtype=torch.int64, device=m.dev)
        rs = m.ops.droppath_scale(B, 0.5, 17, m.dev, snap)
        mask = m.rng.dropout_mask(snap, site, p_, B * L * C).view(B, L, C).double().cpu() / (1 - p_)
        return {"snap": snap, "rs": rs, "mask": mask, "rs64": rs.double().cpu().view(B, 1, 1)}

    return Case("dropout", build, call, ref, F32, gpu_aux=gpu_aux)


def _ln_build(C, seed_base):
    def build(seed=0):
        g = _g(seed_base + C + seed)
        return inputs({"x": _rn(g, 1, 37, C, scale=2.0, shift=0.5)}, {"gamma": _rn(g, C), "beta": _rn(g, C)})
    return build


def _layer_norm(C, odt):
    def call(m, a, p, x):
        return (m.ops.layer_norm(a["x"], p["gamma"], p["beta"], EPS, odt),)

    def ref(a, p, x):
        return (F.layer_norm(a["x"], (C,), p["gamma"], p["beta"], EPS),)

    return Case(f"layer_norm_{C}", _ln_build(C, 1300), call, ref, odt, defers=True)


def _layer_norm_fork(C):
    def call(m, a, p, x):
        return tuple(m.ops.layer_norm_fork(a["x"], p["gamma"], p["beta"], EPS, BF16))

    def ref(a, p, x):
        return (a["x"] * 1.0, F.layer_norm(a["x"], (C,), p["gamma"], p["beta"], EPS))

    return Case(f"layer_norm_fork_{C}", _ln_build(C, 1400), call, ref, BF16, defers=True, nout=2)


# ---------------------------------------------------------------------------------------------
# CARAFE and the heads
# ---------------------------------------------------------------------------------------------
def _carafe_acts(g, B, H, C, s, dtype):
    return {"x": _rn(g, B, H * H, C, dtype=dtype), "enc": _rn(g, B, H, H, 9 * s * s, scale=2.0, dtype=dtype)}


def _carafe_reassemble():
    B, H, C, s = 1, 5, 8, 2

    def build(seed=0):
        return inputs(_carafe_acts(_g(1500 + seed), B, H, C, s, F32))

    def call(m, a, p, x):
        return (m.ops.carafe_reassemble(a["x"], a["enc"], H, H, s),)

    def ref(a, p, x):
        return (S.carafe_reassemble_ref(a["x"], a["enc"], H, s),)

    return Case("carafe_reassemble", build, call, ref, F32)


def _sigmoid_head():
    def build(seed=0):
        g = _g(1600 + seed)
        return inputs({"x": _rn(g, 2, 37, 64)}, {"w": _rn(g, 1, 64, 1, 1, scale=0.2)})

    def call(m, a, p, x):
        return (m.ops.sigmoid_head(a["x"], p["w"]),)

    def ref(a, p, x):
        return (torch.sigmoid(a["x"] @ p["w"].view(64)),)

    return Case("sigmoid_head", build, call, ref, F32)


def _carafe_head():
    B, H, C, s = 2, 5, 64, 2

    def build(seed=0):
        g = _g(1700 + seed)
        acts = _carafe_acts(g, B, H, C, s, F32)
        return inputs(acts, {"u": _rn(g, C, scale=0.15), "cb": _rn(g, 1, scale=0.3).reshape(())})

    def call(m, a, p, x):
        return (m.ops.carafe_head(a["x"], a["enc"], p["u"], p["cb"], H, H, s),)

    def ref(a, p, x):
        y = S.carafe_reassemble_ref(a["x"], a["enc"], H, s)
        return (torch.sigmoid(y @ p["u"] + p["cb"]).view(B, 1, s * H, s * H),)

    return Case("carafe_head", build, call, ref, F32)


def _carafe_head_folded():
    B, H, C, s = 1, 5, 32, 4

    def build(seed=0):
        g = _g(1800 + seed)
        acts = _carafe_acts(g, B, H, C, s, BF16)
        return inputs(acts, {"w_out": _rn(g, C, C, 1, 1, scale=C ** -0.5), "b_out": _rn(g, C, scale=0.3),
                             "w_h": _rn(g, 1, C, 1, 1, scale=0.3)})

    def call(m, a, p, x):
        return (m.ops.carafe_head_folded(a["x"], a["enc"], p["w_out"], p["b_out"], p["w_h"], H, H, s),)

    def ref(a, p, x):
        u = p["w_out"].view(C, C).t() @ p["w_h"].view(C)
        cb = p["w_h"].view(C) @ p["b_out"]
        y = S.carafe_reassemble_ref(a["x"], a["enc"], H, s)
        return (torch.sigmoid(y @ u + cb).view(B, 1, s * H, s * H),)

    return Case("carafe_head_folded", build, call, ref, BF16)


# ---------------------------------------------------------------------------------------------
# token Linears
# ---------------------------------------------------------------------------------------------
def _linear(name, dtype, M, K, N):
    def build(seed=0):
        g = _g(1900 + K + seed)
        return inputs({"x": _rn(g, 1, M, K, dtype=dtype)}, {"w": _rn(g, N, K, scale=K ** -0.5), "b": _rn(g, N, scale=0.1)})

    def call(m, a, p, x):
        return (m.ops.linear(a["x"], p["w"], p["b"]),)

    def ref(a, p, x):
        return (F.linear(a["x"], p["w"], p["b"]),)

    return Case(name, build, call, ref, dtype, autocast=dtype == BF16, defers=dtype == BF16)


def _shared_cast():
    def build(seed=0):
        return inputs({"x": _rn(_g(2000 + seed), 1, 100, 64)})

    def call(m, a, p, x):
        return tuple(m.ops.shared_cast(a["x"], BF16))

    def ref(a, p, x):
        return (a["x"] * 1.0, a["x"] * 1.0)

    return Case("shared_cast", build, call, ref, BF16, nout=2)


def _concat_linear():
    L, C, N = 100, 64, 64

    def build(seed=0):
        g = _g(2100 + seed)
        return inputs({"a": _rn(g, 1, L, C, dtype=BF16), "b": _rn(g, 1, L, C, dtype=BF16)},
                      {"w": _rn(g, N, 2 * C, scale=0.05), "bias": _rn(g, N)})

    def call(m, a, p, x):
        return (m.ops.concat_linear(a["a"], a["b"], p["w"], p["bias"]),)

    def ref(a, p, x):
        return (F.linear(torch.cat([a["a"], a["b"]], -1), p["w"], p["bias"]),)

    return Case("concat_linear", build, call, ref, BF16, autocast=True, defers=True)


@contextlib.contextmanager
def _cast_cache(m, weights):
    """The cast cache with the fragment-ordered shadows of ``weights``, as the model's forward sets it up."""
    cache = m.ops.CastCache()
    cache.refresh(list(weights), BF16)
    cache.refresh_frag()
    m.ops.set_cast_cache(cache)
    try:
        yield cache
    finally:
        m.ops.set_cast_cache(None)


def _fork_after(m, y, p, outs_log):
    """layer_norm_fork on an output that carries its LayerNorm (``_csu_ln``): (residual, LN(y))."""
    assert getattr(y, "_csu_ln", None) is not None, "the producing launch did not attach the next LayerNorm"
    outs_log.append(y)
    return tuple(m.ops.layer_norm_fork(y, p["gamma"], p["beta"], EPS, BF16))


def _linear_residual(ln_next):
    M, C = (64, 128) if ln_next else (37, 64)

    def build(seed=0):
        g = _g(2200 + C + seed)
        ps = {"w": _rn(g, C, C, scale=C ** -0.5), "b": _rn(g, C, scale=0.1)}
        if ln_next:
            ps.update(gamma=torch.rand(C, generator=g) + 0.5, beta=torch.rand(C, generator=g) * 0.4 - 0.2)
        return inputs({"res": _rn(g, 1, M, C), "x": _rn(g, 1, M, C, dtype=BF16)}, ps)

    def call(m, a, p, x):
        if not ln_next:
            return (m.ops.linear_residual(a["res"], a["x"], p["w"], p["b"]),)
        y = m.ops.linear_residual(a["res"], a["x"], p["w"], p["b"], ln_next=(p["gamma"], p["beta"], EPS))
        return _fork_after(m, y, p, x["log"])

    def ref(a, p, x):
        y = a["res"] + F.linear(a["x"], p["w"], p["b"])
        return (y, F.layer_norm(y, (C,), p["gamma"], p["beta"], EPS)) if ln_next else (y,)

    def setup(m, p, x):
        return _cast_cache(m, [p["w"]])

    return Case("linear_residual_ln_next" if ln_next else "linear_residual", build, call, ref, BF16, autocast=True,
                setup=setup if ln_next else None, defers=True, nout=2 if ln_next else 1)


# ---------------------------------------------------------------------------------------------
# Mlp
# ---------------------------------------------------------------------------------------------
def _mlp_params(g, C, Hd):
    return {"w1": _rn(g, Hd, C, scale=C ** -0.5), "b1": _rn(g, Hd, scale=0.1), "w2": _rn(g, C, Hd, scale=Hd ** -0.5),
            "b2": _rn(g, C, scale=0.1)}


def _fc(p, C, Hd):
    return (NS(weight=p["w1"], bias=p["b1"], in_features=C, out_features=Hd),
            NS(weight=p["w2"], bias=p["b2"], in_features=Hd, out_features=C))


def _mlp_ref(x, p, mh=1.0):
    return F.linear(S.gelu_exact(F.linear(x, p["w1"], p["b1"])) * mh, p["w2"], p["b2"])


def _mlp_residual(name, C, M, Hd=None, drop=False, ln_next=False, switches=None, fused_dx=False):
    Hd = Hd or 4 * C
    p_ = 0.3

    def build(seed=0):
        g = _g(2300 + C + M + seed)
        ps = _mlp_params(g, C, Hd)
        if ln_next:
            ps.update(gamma=torch.rand(C, generator=g) + 0.5, beta=torch.rand(C, generator=g) * 0.4 - 0.2)
        return inputs({"res": _rn(g, 1, M, C), "x": _rn(g, 1, M, C, dtype=BF16)}, ps)

    def call(m, a, p, x):
        fc1, fc2 = _fc(p, C, Hd)
        y = m.ops.mlp_residual(a["res"], a["x"], fc1, fc2, x.get("drop"),
                               ln_next=(p["gamma"], p["beta"], EPS) if ln_next else None)
        return _fork_after(m, y, p, x["log"]) if ln_next else (y,)

    def ref(a, p, x):
        y = a["res"] + x.get("mo", 1.0) * _mlp_ref(a["x"], p, x.get("mh", 1.0))
        return (y, F.layer_norm(y, (C,), p["gamma"], p["beta"], EPS)) if ln_next else (y,)

    def gpu_aux(m, x):
        snap = torch.tensor([5, 2], dtype=torch.int64, device=m.dev)
        mh = m.rng.dropout_mask(snap, 21, p_, M * Hd).view(1, M, Hd).double().cpu() / (1 - p_)
        mo = m.rng.dropout_mask(snap, 22, p_, M * C).view(1, M, C).double().cpu() / (1 - p_)
        return {"drop": m.ops.MlpDrop(snap, 21, 22, p_, None, M), "mh": mh, "mo": mo}

    return Case(name, build, call, ref, BF16, autocast=True, gpu_aux=gpu_aux if drop else None, switches=switches,
                defers=True, fused_dx=fused_dx, nout=2 if ln_next else 1)


def _mlp_fp8():
    C, M = 64, 37
    Hd = 4 * C

    def build(seed=0):
        g = _g(2400 + seed)
        return inputs({"res": _rn(g, 1, M, C), "x": _rn(g, 1, M, C, dtype=BF16)}, _mlp_params(g, C, Hd))

    @contextlib.contextmanager
    def setup(m, p, x):
        ws = [p["w1"], p["w2"]]
        fp8 = m.ops.Fp8Weights(ws, mlp_pairs=[(p["w1"], p["w2"])])
        cache = m.ops.CastCache()
        cache.refresh(ws, BF16, (), sources=fp8.sources())
        fp8.quantize(cache)
        m.ops.set_cast_cache(cache, fp8)
        try:
            yield
        finally:
            m.ops.set_cast_cache(None)

    def call(m, a, p, x):
        fc1, fc2 = _fc(p, C, Hd)
        y = m.ops.mlp_fp8(a["res"], a["x"], fc1, fc2)
        assert y is not None, "mlp_fp8 declined"
        return (y,)

    def ref(a, p, x):
        from oracle import fp8_ref as Q
        w1d, _, s1 = Q.quant_rows(p["w1"].detach())
        w2d, _, s2 = Q.quant_rows(p["w2"].detach())
        w1 = p["w1"] + (w1d - p["w1"]).detach()       # straight-through: the gradients go to the masters
        w2 = p["w2"] + (w2d - p["w2"]).detach()
        return (a["res"] + Q.fp8_mlp(a["x"], w1, p["b1"], w2, p["b2"], s1, s2, None, False),)

    return Case("mlp_fp8", build, call, ref, BF16, autocast=True, setup=setup, defers=True)


def _ln_linear_ws():
    M, C = 64, 128

    def build(seed=0):
        g = _g(2500 + seed)
        return inputs({"x": _rn(g, 1, M, C)},
                      {"gamma": torch.rand(C, generator=g) + 0.5, "beta": torch.rand(C, generator=g) * 0.4 - 0.2,
                       "w": _rn(g, 3 * C, C, scale=C ** -0.5), "b": torch.rand(3 * C, generator=g) * 0.2 - 0.1})

    def call(m, a, p, x):
        got = m.ops.ln_linear_ws(a["x"], NS(weight=p["gamma"], bias=p["beta"], eps=EPS), NS(weight=p["w"], bias=p["b"]))
        assert got is not None, "ln_linear_ws declined"
        return tuple(got)

    def ref(a, p, x):
        return (a["x"] * 1.0, F.linear(F.layer_norm(a["x"], (C,), p["gamma"], p["beta"], EPS), p["w"], p["b"]))

    def setup(m, p, x):
        return _cast_cache(m, [p["w"]])

    return Case("ln_linear_ws", build, call, ref, BF16, autocast=True, setup=setup, defers=True, nout=2)


def _ln_mlp_residual():
    M, C = 64, 128
    Hd = 4 * C

    def build(seed=0):
        g = _g(2600 + seed)
        ps = {"gamma": torch.rand(C, generator=g) + 0.5, "beta": torch.rand(C, generator=g) * 0.4 - 0.2}
        ps.update(_mlp_params(g, C, Hd))
        return inputs({"x": _rn(g, 1, M, C) + 2.0 * _rn(g, 1, M, 1)}, ps)

    def call(m, a, p, x):
        fc1, fc2 = _fc(p, C, Hd)
        y = m.ops.ln_mlp_residual(a["x"], NS(weight=p["gamma"], bias=p["beta"], eps=EPS), fc1, fc2, None, None)
        assert y is not None, "ln_mlp_residual declined"
        return (y,)

    def ref(a, p, x):
        return (a["x"] + _mlp_ref(F.layer_norm(a["x"], (C,), p["gamma"], p["beta"], EPS), p),)

    return Case("ln_mlp_residual", build, call, ref, BF16, autocast=True, defers=True)


# ---------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------
def _bce_loss():
    shape = (25, 40)

    def build(seed=0):
        g = _g(2700 + seed)
        return inputs({"p": torch.rand(shape, generator=g) * 0.998 + 0.001}, t=(torch.rand(shape, generator=g) > 0.5).float())

    def call(m, a, p, x):
        return (m.ops.bce_loss(a["p"], x["t"]),)

    def stats_call(m, a, p, x):
        return m.ops.bce_loss_stats(a["p"], x["t"])

    def ref(a, p, x):
        return (F.binary_cross_entropy(a["p"], x["t"].to(a["p"].dtype)),)

    return Case("bce_loss", build, call, ref, F32, stats_call=stats_call)


def _seg_loss():
    import test_seg_loss as T
    shape, ps = (3, 1, 37, 41), T.PARAM_SETS[2]
    bce, tv, alpha, beta, pw = ps

    def build(seed=0):
        g = _g(2800 + seed)
        return inputs({"p": torch.rand(shape, generator=g) * 0.998 + 0.001}, t=(torch.rand(shape, generator=g) > 0.6).float())

    def call(m, a, p, x, stats=False):
        return m.ops.seg_loss(a["p"], x["t"], (bce, pw, tv, alpha, beta, T.SMOOTH), 1, with_stats=stats)

    def ref(a, p, x):
        return (_RefLoss.apply(a["p"], lambda z: T.ref_loss_grad(z, x["t"], ps, False, T.SMOOTH, 1.0)),)

    return Case("seg_loss", build, lambda m, a, p, x: (call(m, a, p, x),), ref, F32,
                stats_call=lambda m, a, p, x: call(m, a, p, x, True))


def _seg_ce(bd):
    import test_boundary as TB
    import test_seg_ce as T
    shape = (2, 3, 7, 9)
    K = shape[1]
    ps = T.PARAM_SETS[2]
    ce, tv, alpha, beta, weighted, bg = ps
    combo = TB.COMBOS[0]

    def build(seed=0):
        z, t = T.make_case(shape, seed=2900 + seed)
        aux = {"t": t}
        if bd:
            aux.update(phi=TB.make_phi(shape, seed=2950 + seed), w_bd=torch.tensor([combo[2]]))
        else:
            aux.update(cw=torch.tensor(T.class_weights(K)))
        return inputs({"z": z}, **aux)

    def call(m, a, p, x, stats=False):
        if bd:
            return m.ops.seg_bd(a["z"], x["t"], x["phi"], x["w_bd"], (combo[0], combo[1], 0.5, 0.5, TB.SMOOTH), None, T.IGNORE,
                                1, True, False, with_stats=stats)
        return m.ops.seg_ce(a["z"], x["t"], (ce, tv, alpha, beta, T.SMOOTH), x["cw"], T.IGNORE, 1, bg, with_stats=stats)

    def ref(a, p, x):
        if bd:
            return (_RefLoss.apply(a["z"], lambda z: TB.ref_bd_loss_grad(z, x["t"], x["phi"], combo, False, False, T.IGNORE,
                                                                         1.0)[:2]),)
        return (_RefLoss.apply(a["z"], lambda z: T.ref_ce_loss_grad(z, x["t"], ps, False, T.IGNORE, T.SMOOTH, 1.0)[:2]),)

    def plain(m, a, p, x):
        r = call(m, a, p, x)
        return (r[0],) if bd else (r,)       # seg_bd also returns its non-differentiable terms

    return Case("seg_bd" if bd else "seg_ce", build, plain, ref, F32, stats_call=lambda m, a, p, x: call(m, a, p, x, True))


# ---------------------------------------------------------------------------------------------
# convolutions, csu.unet, csu.simam
# ---------------------------------------------------------------------------------------------
def _conv2d(name, case, dtype):
    B, H, C, N, k, s, pd = case

    def build(seed=0):
        g = _g(3000 + sum(case) + seed)
        return inputs({"x": _rn(g, B, H, H, C, dtype=dtype)},
                      {"w": _rn(g, N, C, k, k, scale=(C * k * k) ** -0.5), "b": _rn(g, N, scale=0.1)})

    def call(m, a, p, x):
        return (m.ops.conv2d(a["x"], p["w"], p["b"], s, pd),)

    def ref(a, p, x):
        return (F.conv2d(a["x"].permute(0, 3, 1, 2), p["w"], p["b"], stride=s, padding=pd).permute(0, 2, 3, 1),)

    return Case(name, build, call, ref, dtype, autocast=dtype == BF16)


def _conv2d_cat():
    # the smallest geometry csu_conv2d_split_ok accepts (rows of 64 pixels, an even number of them): the
    # two-source kernels run, not the materialised concatenation
    B, H, W, Ca, Cb, N = 1, 4, 64, 64, 64, 64

    def build(seed=0):
        g = _g(3100 + seed)
        return inputs({"xa": _rn(g, B, H, W, Ca, dtype=BF16), "xb": _rn(g, B, H, W, Cb, dtype=BF16)},
                      {"w": _rn(g, N, Ca + Cb, 3, 3, scale=(9 * (Ca + Cb)) ** -0.5), "b": _rn(g, N, scale=0.1)})

    def call(m, a, p, x):
        import ctypes
        gm = m.ops._conv_geom(B, H, W, Ca + Cb, N, 3, 3, 1, 1)
        assert m.ops.lib().csu_conv2d_split_ok(ctypes.byref(gm), Ca), "conv2d_cat would materialise the concatenation"
        return (m.ops.conv2d_cat(a["xa"], a["xb"], p["w"], p["b"], 1),)

    def ref(a, p, x):
        xin = torch.cat([a["xa"], a["xb"]], -1).permute(0, 3, 1, 2)
        return (F.conv2d(xin, p["w"], p["b"], 1, 1).permute(0, 2, 3, 1),)

    return Case("conv2d_cat", build, call, ref, BF16, autocast=True)


def _conv_transpose2d():
    B, H, Cin, Cout = 1, 5, 128, 64

    def build(seed=0):
        g = _g(3200 + seed)
        return inputs({"x": _rn(g, B, H, H, Cin)}, {"w": _rn(g, Cin, Cout, 2, 2, scale=0.1), "b": _rn(g, Cout, scale=0.1)})

    def call(m, a, p, x):
        return (m.ops.conv_transpose2d(a["x"], p["w"], p["b"], 2),)

    def ref(a, p, x):
        return (F.conv_transpose2d(a["x"].permute(0, 3, 1, 2), p["w"], p["b"], stride=2).permute(0, 2, 3, 1),)

    return Case("conv_transpose2d", build, call, ref, F32)


def _bn_relu(training):
    shape = (2, 5, 7, 64)
    C = shape[-1]

    def build(seed=0):
        g = _g(3300 + seed)
        return inputs({"x": _rn(g, *shape, scale=3.0, shift=5.0)},
                      {"gamma": torch.rand(C, generator=g) + 0.5, "beta": _rn(g, C, scale=0.3)},
                      rm=_rn(g, C), rv=torch.rand(C, generator=g) + 0.5)

    def call(m, a, p, x):
        # the running statistics are an in-place input in training: a fresh copy per call
        bn = NS(training=training, track_running_stats=True, momentum=0.1, affine=True, eps=EPS, weight=p["gamma"],
                bias=p["beta"], running_mean=x["rm"].clone(), running_var=x["rv"].clone(),
                num_batches_tracked=torch.zeros((), dtype=torch.int64, device=x["rm"].device))
        return (m.unet.bn_relu_nhwc(a["x"], bn, True),)

    def ref(a, p, x):
        from test_gpu_unet import _ref_bn
        dt = a["x"].dtype
        return (_ref_bn(a["x"], p["gamma"], p["beta"], x["rm"].to(dt).clone(), x["rv"].to(dt).clone(), training, True),)

    return Case("bn_relu_nhwc_train" if training else "bn_relu_nhwc_eval", build, call, ref, F32)


def _max_pool2():
    def build(seed=0):
        return inputs({"x": _rn(_g(3400 + seed), 3, 7, 9, 16)})

    def call(m, a, p, x):
        return (m.unet.max_pool2_nhwc(a["x"]),)

    def ref(a, p, x):
        return (F.max_pool2d(a["x"].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1),)

    return Case("max_pool2_nhwc", build, call, ref, F32)


def _simam(fork):
    shape = (2, 64, 32) if fork else (3, 17, 200)

    def build(seed=0):
        return inputs({"x": _rn(_g(3500 + seed + int(fork)), *shape, scale=1.5, shift=0.3)})

    def call(m, a, p, x):
        return tuple(m.simam.simam_fork(a["x"])) if fork else (m.simam.simam(a["x"]),)

    def ref(a, p, x):
        y = S.simam_ref(a["x"])
        return (a["x"] * 1.0, y) if fork else (y,)

    return Case("simam_fork" if fork else "simam", build, call, ref, BF16 if fork else F32, nout=2 if fork else 1)


CASES = [
    _attn_one("stripe_attention_fp32", (16, 0, 1, 32, 1, 2), F32),
    _attn_one("stripe_attention_bf16", (7, -1, 7, 64, 2, 2), BF16),
    _attn_two("stripe_attention_two_branch", BF16),
    _attn_one("stripe_attention_attn_drop", (7, -1, 7, 64, 2, 2), BF16, drop=True),
    _dropout(),
    _layer_norm(64, F32), _layer_norm(512, BF16),
    _layer_norm_fork(64), _layer_norm_fork(512),
    _carafe_reassemble(), _sigmoid_head(), _carafe_head(), _carafe_head_folded(),
    _linear("linear_bf16", BF16, 37, 64, 72), _linear("linear_fp32", F32, 37, 36, 20),
    _shared_cast(), _concat_linear(),
    _linear_residual(False), _linear_residual(True),
    _mlp_residual("mlp_residual_two_gemm", 64, 37, Hd=128),
    _mlp_residual("mlp_residual_fused_64", 64, 37),
    _mlp_residual("mlp_residual_fused_256", 256, 100),
    _mlp_residual("mlp_residual_c64_wgrad", 64, 37, switches={"SIDE_WGRAD": False}, fused_dx=True),
    _mlp_residual("mlp_residual_drop", 64, 37, drop=True),
    _mlp_residual("mlp_residual_ln_next", 64, 37, ln_next=True),
    _mlp_fp8(), _ln_linear_ws(), _ln_mlp_residual(),
    _bce_loss(), _seg_loss(), _seg_ce(False), _seg_ce(True),
    _conv2d("conv2d_3ch", (2, 32, 3, 64, 7, 4, 2), BF16), _conv2d("conv2d", (2, 9, 32, 36, 3, 1, 1), F32),
    _conv2d_cat(), _conv_transpose2d(),
    _bn_relu(True), _bn_relu(False), _max_pool2(),
    _simam(False), _simam(True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the ops of the issue's list, each covered by at least one entry
OPS = {"stripe_attention": 4, "dropout": 1, "layer_norm": 2, "layer_norm_fork": 2, "carafe_reassemble": 1, "sigmoid_head": 1,
       "carafe_head": 2, "linear": 2, "shared_cast": 1, "concat_linear": 1, "linear_residual": 2, "mlp_residual": 6, "mlp_fp8": 1,
       "ln_linear_ws": 1, "ln_mlp_residual": 1, "bce_loss": 1, "seg_loss": 1, "seg_ce": 1, "seg_bd": 1, "conv2d": 3,
       "conv_transpose2d": 1, "bn_relu_nhwc": 2, "max_pool2_nhwc": 1, "simam": 2}

PATTERNS = {
    "A": "plain", "B": "input layouts", "C_sum": "out.sum().backward()", "C_noncontig": "non-contiguous upstream gradient",
    "C_dtype": "upstream gradient of the other float dtype", "D_acts_only": "parameters frozen",
    "D_params_only": "activations without grad", "D_alternate": "every other parameter frozen, both ways",
    "D_grad_each": "torch.autograd.grad for one input at a time", "E": "one output unused / loss statistics",
    "F_two_calls": "f(x1) + f(x2) with shared parameters", "F_retain_twice": "backward(retain_graph=True) twice",
    "F_existing_grad": "a pre-existing .grad, contiguous and a view into a larger buffer",
    "F_micro_batches": "two forward / backward passes without zeroing", "F_no_grad_between": "a no_grad forward before the backward",
    "G_tensor_hooks": "Tensor.register_hook on each parameter", "G_post_hooks": "post-accumulate-grad hooks",
    "G_autograd_grad": "torch.autograd.grad(out, params)", "H": "backward(create_graph=True)",
    "I_side_on": "a user stream, SIDE_WGRAD on", "I_side_off": "a user stream, SIDE_WGRAD off",
}
_NEEDS_PARAMS = {"D_acts_only", "D_params_only", "D_alternate", "F_two_calls", "F_existing_grad", "F_micro_batches",
                 "G_tensor_hooks", "G_post_hooks", "G_autograd_grad"}


_NPAR = {}


def n_outputs(case):
    """Number of differentiable outputs (``nout``; tests/test_contract_cases.py holds the reference to it)."""
    return case.nout


def not_applicable(case, pattern):
    """Why ``pattern`` does not apply to ``case`` (None: it applies and is a collected test)."""
    if case.name not in _NPAR:
        _NPAR[case.name] = len(case.build(0).params)
    npar = _NPAR[case.name]
    if pattern in _NEEDS_PARAMS and not npar:
        return "the op has no parameters"
    if pattern == "E" and case.stats_call is None and n_outputs(case) < 2:
        return "one differentiable output and no statistics output"
    if pattern == "C_noncontig" and case.stats_call is not None:
        return "the output is a 0-d loss: its gradient has no layout"
    if pattern == "D_alternate" and npar < 2:
        return "a single parameter: freezing it is D_acts_only"
    return None


def applicable(pattern):
    return [c.name for c in CASES if not_applicable(c, pattern) is None]
