"""tests/contract_cases.py on the CPU: the table test_gpu_autograd_contract.py runs on the GPU is itself
right -- deterministic builders, references that agree with torch.nn.functional's fp64 autograd, pattern B's
views equal in value to their contiguous originals and really non-contiguous or offset."""
import pytest
import torch
import torch.nn.functional as F

import contract_cases as CC
import stress_inputs as S
from oracle import cswin_ref as O

NAMES = [c.name for c in CC.CASES]


def _leaves(case, seed=0):
    inp = case.build(seed)
    a = {k: v.double().requires_grad_(True) for k, v in inp.acts.items()}
    p = {k: v.double().requires_grad_(True) for k, v in inp.params.items()}
    return inp, a, p


def test_table_covers_every_op_of_the_list():
    count = dict.fromkeys(CC.OPS, 0)
    for c in NAMES:       # an entry belongs to the op with the longest name it starts with
        count[max((op for op in CC.OPS if c.startswith(op)), key=len)] += 1
    assert count == CC.OPS
    assert set(CC.PATTERNS) >= {"A", "B", "E", "H"}


@pytest.mark.parametrize("name", NAMES)
def test_builders_are_deterministic(name):
    case = CC.BY_NAME[name]
    i0, i1, other = case.build(0), case.build(0), case.build(1)
    assert not set(i0.acts) & set(i0.params), "one name for an activation and a parameter"
    for d0, d1 in ((i0.acts, i1.acts), (i0.params, i1.params)):
        assert list(d0) == list(d1)
        for k in d0:
            assert d0[k].dtype == d1[k].dtype and torch.equal(d0[k], d1[k]), (name, k)
    for k, v in i0.aux.items():
        if torch.is_tensor(v):
            assert torch.equal(v, i1.aux[k]), (name, k)
    for k in i0.acts:       # another seed: other activations of the same shape (patterns F use both)
        assert other.acts[k].shape == i0.acts[k].shape and not torch.equal(other.acts[k], i0.acts[k]), (name, k)
    for t in list(i0.acts.values()) + list(i0.params.values()):
        assert bool(torch.isfinite(t.float()).all())
    assert case.tol in (CC.F32, CC.BF16)


@pytest.mark.parametrize("name", NAMES)
def test_reference_is_differentiable_in_every_input(name):
    case = CC.BY_NAME[name]
    inp, a, p = _leaves(case)
    outs = case.ref(a, p, dict(inp.aux))
    assert isinstance(outs, tuple) and len(outs) == case.nout and all(o.dtype == torch.float64 for o in outs)
    g = torch.Generator().manual_seed(1)
    gs = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in outs]
    grads = torch.autograd.grad(outs, list(a.values()) + list(p.values()), gs)
    for t, gr in zip(list(a.values()) + list(p.values()), grads):
        assert gr.shape == t.shape and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0


# references whose value and gradient are one hand-written pair, or that restate an op torch has: their
# gradient against central differences of their value, along a random direction (the STE of mlp_fp8 is no
# derivative of its forward and is left out)
@pytest.mark.parametrize("name", [n for n in NAMES if n != "mlp_fp8"])
def test_reference_gradient_is_the_derivative_of_its_value(name):
    case = CC.BY_NAME[name]
    inp, a, p = _leaves(case)
    leaves = list(a.values()) + list(p.values())
    g = torch.Generator().manual_seed(2)
    outs = case.ref(a, p, dict(inp.aux))
    gs = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in outs]
    grads = torch.autograd.grad(outs, leaves, gs)
    dirs = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in leaves]
    analytic = sum(float((gr * dv).sum()) for gr, dv in zip(grads, dirs))

    def value(eps):
        a2 = {k: (v.detach() + eps * dv) for (k, v), dv in zip(a.items(), dirs[:len(a)])}
        p2 = {k: (v.detach() + eps * dv) for (k, v), dv in zip(p.items(), dirs[len(a):])}
        with torch.no_grad():
            o2 = case.ref(a2, p2, dict(inp.aux))
        return sum(float((o * gg).sum()) for o, gg in zip(o2, gs))

    scale = max(1.0, max(float(t.detach().abs().max()) for t in leaves))
    eps = 1e-6 / scale
    numeric = (value(eps) - value(-eps)) / (2 * eps)
    assert abs(numeric - analytic) <= 1e-5 * max(1.0, abs(analytic)), (name, numeric, analytic)


def _against(name, torch_form):
    """The case's reference against ``torch_form(a, p, x)`` -- torch.nn.functional / torch.nn in fp64 --
    in value and in every gradient."""
    case = CC.BY_NAME[name]
    inp, a, p = _leaves(case)
    _, a2, p2 = _leaves(case)
    outs, outs2 = case.ref(a, p, dict(inp.aux)), torch_form(a2, p2, dict(inp.aux))
    g = torch.Generator().manual_seed(3)
    gs = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in outs]
    g1 = torch.autograd.grad(outs, list(a.values()) + list(p.values()), gs)
    g2 = torch.autograd.grad(outs2, list(a2.values()) + list(p2.values()), gs)
    for o, o2 in zip(outs, outs2):
        torch.testing.assert_close(o, o2, rtol=1e-10, atol=1e-12)
    for u, v in zip(g1, g2):
        torch.testing.assert_close(u, v, rtol=1e-9, atol=1e-11)


def _sdpa_attention(reso, cb, heads, idx, sw):
    """LePE attention with torch's own scaled_dot_product_attention per stripe window."""
    hs, ws = S.stripe_geometry(reso, idx, sw)

    def form(a, p, x, wkey="lepe_w", bkey="lepe_b", qkv=None, cb_=cb, heads_=heads):
        qkv = a["qkv"] if qkv is None else qkv
        B = qkv.shape[0]
        win = S.window_tokens(reso, hs, ws)              # (nWin, N) token indices
        q, k, v = (qkv[..., i * cb_:(i + 1) * cb_][:, win] for i in range(3))        # (B, nWin, N, cb)
        hd = cb_ // heads_

        def hf(t):
            return t.reshape(B, win.shape[0], hs * ws, heads_, hd).transpose(2, 3)

        o = F.scaled_dot_product_attention(hf(q), hf(k), hf(v)).transpose(2, 3).reshape(B, win.shape[0], hs * ws, cb_)
        img = v.reshape(B * win.shape[0], hs, ws, cb_).permute(0, 3, 1, 2)
        lepe = F.conv2d(img, p[wkey], p[bkey], padding=1, groups=cb_).permute(0, 2, 3, 1).reshape(B, win.shape[0], hs * ws, cb_)
        out = torch.zeros(B, reso * reso, cb_, dtype=qkv.dtype)
        return (out.index_put((torch.arange(B)[:, None, None], win[None]), o + lepe),)
    return form


TORCH_FORMS = {
    "stripe_attention_fp32": _sdpa_attention(16, 32, 1, 0, 1),
    "stripe_attention_bf16": _sdpa_attention(7, 64, 2, -1, 7),
    "layer_norm_64": lambda a, p, x: (torch.nn.functional.layer_norm(a["x"], (64,), p["gamma"], p["beta"], 1e-5),),
    "layer_norm_fork_512": lambda a, p, x: (a["x"] + 0.0, F.layer_norm(a["x"], (512,), p["gamma"], p["beta"], 1e-5)),
    "sigmoid_head": lambda a, p, x: (torch.sigmoid(F.conv2d(a["x"].permute(2, 0, 1)[None], p["w"]))[0, 0],),
    "linear_bf16": lambda a, p, x: (F.linear(a["x"], p["w"], p["b"]),),
    "linear_fp32": lambda a, p, x: (a["x"] @ p["w"].t() + p["b"],),
    "concat_linear": lambda a, p, x: (F.linear(a["a"], p["w"][:, :64]) + F.linear(a["b"], p["w"][:, 64:], p["bias"]),),
    "linear_residual": lambda a, p, x: (a["res"] + F.linear(a["x"], p["w"], p["b"]),),
    "mlp_residual_fused_64": lambda a, p, x: (a["res"] + F.linear(F.gelu(F.linear(a["x"], p["w1"], p["b1"])), p["w2"], p["b2"]),),
    "mlp_residual_two_gemm": lambda a, p, x: (a["res"] + F.linear(F.gelu(F.linear(a["x"], p["w1"], p["b1"])), p["w2"], p["b2"]),),
    "ln_linear_ws": lambda a, p, x: (a["x"] + 0.0, F.linear(F.layer_norm(a["x"], (128,), p["gamma"], p["beta"], 1e-5), p["w"],
                                                          p["b"])),
    "ln_mlp_residual": lambda a, p, x: (a["x"] + F.linear(F.gelu(F.linear(F.layer_norm(a["x"], (128,), p["gamma"], p["beta"],
                                                                                        1e-5), p["w1"], p["b1"])),
                                                          p["w2"], p["b2"]),),
    "bce_loss": lambda a, p, x: (F.binary_cross_entropy(a["p"], x["t"].double()),),
    "conv2d": lambda a, p, x: (F.conv2d(a["x"].permute(0, 3, 1, 2), p["w"], p["b"], stride=1, padding=1).permute(0, 2, 3, 1),),
    "conv2d_3ch": lambda a, p, x: (F.conv2d(a["x"].permute(0, 3, 1, 2), p["w"], p["b"], stride=4, padding=2).permute(0, 2, 3, 1),),
    "conv_transpose2d": lambda a, p, x: (F.conv_transpose2d(a["x"].permute(0, 3, 1, 2), p["w"], p["b"], stride=2)
                                         .permute(0, 2, 3, 1),),
    "bn_relu_nhwc_train": lambda a, p, x: (F.relu(F.batch_norm(a["x"].permute(0, 3, 1, 2), x["rm"].double().clone(),
                                                               x["rv"].double().clone(), p["gamma"], p["beta"], True, 0.1, 1e-5))
                                           .permute(0, 2, 3, 1),),
    "bn_relu_nhwc_eval": lambda a, p, x: (F.relu(F.batch_norm(a["x"].permute(0, 3, 1, 2), x["rm"].double(), x["rv"].double(),
                                                              p["gamma"], p["beta"], False, 0.1, 1e-5)).permute(0, 2, 3, 1),),
    "max_pool2_nhwc": lambda a, p, x: (torch.nn.MaxPool2d(2)(a["x"].permute(0, 3, 1, 2)).permute(0, 2, 3, 1),),
    "simam": lambda a, p, x: (O.simam(a["x"]),),
    "carafe_reassemble": lambda a, p, x: (_carafe_unfold(a["x"], a["enc"], 5, 2),),
    "seg_ce": None,      # filled below
}


def _carafe_unfold(x, enc, H, s):
    """CARAFE reassembly with F.unfold neighbourhoods and F.pixel_shuffle'd softmax kernels."""
    B, _, C = x.shape
    kern = F.pixel_shuffle(enc.permute(0, 3, 1, 2), s).softmax(1)                      # (B, 9, sH, sH)
    xi = x.transpose(1, 2).reshape(B, C, H, H)
    nb = F.unfold(xi, 3, padding=1).reshape(B, C * 9, H, H)
    nb = F.interpolate(nb, scale_factor=s, mode="nearest").reshape(B, C, 9, s * H, s * H)
    return (nb * kern[:, None]).sum(2).reshape(B, C, -1).transpose(1, 2)


def _seg_ce_form(a, p, x):
    """seg_ce's reference with the CE part from F.cross_entropy(mean) and the Tversky part restated with
    one-hot targets (PARAM_SETS[2]: weighted CE, background excluded)."""
    import test_seg_ce as T
    ce, tv, alpha, beta, weighted, bg = T.PARAM_SETS[2]
    z, t = a["z"], x["t"]
    K = z.shape[1]
    w = torch.tensor(T.class_weights(K), dtype=torch.float64)
    ce_term = F.cross_entropy(z, t, weight=w, ignore_index=T.IGNORE)       # mean = sum / sum of the live weights
    live = (t != T.IGNORE)
    prob = torch.softmax(z, 1).permute(0, 2, 3, 1)[live]                   # (n live, K)
    oh = F.one_hot(t[live], K).double()
    tp, sp, st = (prob * oh).sum(0), prob.sum(0), oh.sum(0)
    ti = (tp + T.SMOOTH) / ((1 - alpha - beta) * tp + alpha * sp + beta * st + T.SMOOTH)
    return (ce * ce_term + tv * (1 - ti)[1:].mean(),)


TORCH_FORMS["seg_ce"] = _seg_ce_form


@pytest.mark.parametrize("name", sorted(TORCH_FORMS))
def test_reference_vs_torch_functional(name):
    _against(name, TORCH_FORMS[name])


def test_two_branch_reference_vs_sdpa():
    case = CC.BY_NAME["stripe_attention_two_branch"]

    def form(a, p, x):
        outs = []
        for i in range(2):
            f = _sdpa_attention(16, 32, 1, i, 2)
            qkv = torch.cat([a["qkv"][..., j * 64 + i * 32: j * 64 + (i + 1) * 32] for j in range(3)], -1)
            outs.append(f(a, p, x, f"lepe_w{i}", f"lepe_b{i}", qkv)[0])
        return (torch.cat(outs, -1),)

    _against(case.name, form)


# ---------------------------------------------------------------------------------------------
# pattern B's views
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_layout_views_are_equal_and_really_strided(name):
    case = CC.BY_NAME[name]

    def new(shape, dtype):
        return torch.full(shape, float("nan"), dtype=dtype)

    for k, t in case.build(0).acts.items():
        assert t.is_contiguous() and t.dim() >= 2 and t.shape[-1] > 1 and t.shape[-2] > 1, (name, k)
        for lname, make in CC.LAYOUTS.items():
            v = make(t, new)
            assert v.shape == t.shape and v.dtype == t.dtype and torch.equal(v, t), (name, k, lname)
            assert (not v.is_contiguous()) or v.storage_offset() != 0, (name, k, lname)
            if lname == "offset":
                assert v.is_contiguous() and v.storage_offset() * v.element_size() % 16 == 0
            else:
                assert not v.is_contiguous(), (name, k, lname)
            assert torch.equal(v.contiguous(), t)


def test_step2_runs_along_the_first_dim_longer_than_one():
    assert CC.batch_dim(torch.zeros(1, 37, 64)) == 1 and CC.batch_dim(torch.zeros(2, 5, 8)) == 0


def test_not_applicable_reasons():
    n = 0
    for c in CC.CASES:
        for pat in CC.PATTERNS:
            why = CC.not_applicable(c, pat)
            assert why is None or len(why) > 10
            n += why is None
    assert n > 600        # the table is mostly tests, not reasons
    # the fork ops and the losses are the ones pattern E runs on
    assert set(CC.applicable("E")) >= {"layer_norm_fork_64", "shared_cast", "simam_fork", "bce_loss", "seg_loss", "seg_ce", "seg_bd"}
