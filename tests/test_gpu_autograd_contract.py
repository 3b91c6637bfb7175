"""The autograd contract of the csu ops on the MI355X: every differentiable op of tests/contract_cases.py
under the call patterns autograd allows, not only "contiguous inputs, everything requires grad, one
forward and one backward(randn), default stream, no hooks".

Patterns (PATTERNS of contract_cases; an (op, pattern) pair is a collected test here or has a written reason
in contract_cases.not_applicable -- test_every_pair_is_a_test_or_has_a_reason):
  A  plain: the anchor, against the fp64 reference; two plain calls are bitwise equal.
  B  each activation in turn as a slice of a wider buffer, a step-2 slice, a transposed view, a contiguous
     view at a storage offset.
  C  the upstream gradient as out.sum().backward() (expanded, stride 0), through out.transpose / out[..., ::2]
     (non-contiguous / produced by a slice), and in the other float dtype.
  D  partial differentiation: parameters frozen, activations without grad, every other parameter frozen
     (both ways), torch.autograd.grad for one input at a time.  Frozen tensors keep .grad None.
  E  one output of a two-output op unused (its gradient arrives as zeros); loss statistics stay
     non-differentiable.
  F  f(x1) + f(x2) on shared parameters, backward(retain_graph=True) twice, a pre-existing .grad
     (contiguous and a view into a larger buffer: accumulated into, not replaced), two micro-batches without
     zeroing, a no_grad forward on other inputs between the forward and its backward.
  G  Tensor.register_hook and register_post_accumulate_grad_hook on every parameter (each hook clones what
     it sees, stream-ordered, no synchronise), torch.autograd.grad(out, params).
  H  backward(create_graph=True): first-order values.
  I  forward and backward on a user stream, with SIDE_WGRAD on and off.
  J  the autouse fixture below: no deferred work, late-gradient entry, side-stream event, use count or
     active cast cache outlives a test, no output keeps a stale ``_csu_ln``, and
     ops.STATS["late_grad_fixups"] never rises: no test here makes autograd copy a late gradient (hooks, an
     existing .grad, shared weights and create_graph all switch the op to inline weight gradients, and
     torch.autograd.grad leaves no .grad to repair), so a fix-up anywhere in this file is a finding.
  K  one CSWinBlock and one UNet DoubleConv -> Down -> Up under bf16 autocast with the cast cache active:
     freezing layers and an eval-mode no_grad forward before the backward leave the other gradients bitwise
     unchanged.

Criteria: test_gpu_kernels.assert_close against the fp64 reference on the same (bf16-rounded where the op takes
bf16) inputs -- fp32: rtol 1e-4, atol 1e-5 max(1, max|ref|); bf16: rel-L2 < 2e-2, max-abs < 3e-2 max|ref|.
Where a pattern only changes how the same values arrive (B, C, F, H, I) the results also torch.equal those
of the plain call; in B, F's no_grad forward and I, what is bitwise equal to the plain call's is not compared
with fp64 a second time (the plain call's own comparison is made before anything is compared with it).  Ops exempt from the bitwise rule because two plain calls differ: none (BITWISE_EXEMPT).
One restriction, stated per op in contract_cases (``defers`` / ``fused_dx``): when a pattern forces the
op's weight gradients off the end-of-backward grouped launches or off the side stream (an existing .grad,
shared weights, create_graph, SIDE_WGRAD off), ANOTHER KERNEL with another summation order writes them, so
there the bitwise comparison covers the outputs and the activation gradients and the fp64 criterion the
parameter gradients.

No test here passes a pointer that is not 16-byte aligned to a kernel: every contiguous device tensor
handed to an op is checked first (Run.forward)."""
import contextlib
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import contract_cases as CC
from contract_cases import BF16, F32
from test_gpu_kernels import assert_close

NS = types.SimpleNamespace
BITWISE_EXEMPT = ()        # names of contract_cases entries whose two plain calls are not bitwise equal
_OUTPUTS = []              # every output of this test's forwards (pattern J looks at their ``_csu_ln``)


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def mods():
    import importlib
    ops, rng, simam, unet = (importlib.import_module("csu." + n) for n in ("ops", "rng", "simam", "unet"))
    return NS(ops=ops, rng=rng, simam=simam, unet=unet, dev=dev())      # (csu.simam the module, not csu's function)


# ---------------------------------------------------------------------------------------------
# J. no state left behind
# ---------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def no_state_left_behind():
    if not torch.cuda.is_available():
        yield
        return
    from csu import ops
    fix0 = ops.STATS["late_grad_fixups"]
    _OUTPUTS.clear()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device error: nothing more may be launched in this session
        pytest.exit(f"the device reported an error, the session stops here: {e}", returncode=3)
    try:
        assert not ops.deferred_pending()
        assert not ops._LATE_DEFER and not ops._LATE_SIDE and not ops._SIDE_PENDING
        assert not ops._USES, "forward use counts outlived the backward pass"
        assert ops._LN_QUEUED[0] is False and ops._SIDE_JOIN_QUEUED[0] is False
        assert ops._LN_STASH[0] is None and ops._ACTIVE_CACHE is None and ops._ACTIVE_FP8 is None
        for o in _OUTPUTS:
            pre = getattr(o, "_csu_ln", None)
            assert pre is None or pre[6] == o._version, "an output kept a stale _csu_ln"
        assert ops.STATS["late_grad_fixups"] == fix0, "autograd copied a late gradient"
    finally:        # a failed test must not fail the next one
        for lst in (ops._LN_PENDING, ops._WG_DEFER, ops._WG_PENDING, ops._WG_POST, ops._LEPE_PENDING, ops._LATE_DEFER,
                    ops._LATE_SIDE, ops._SIDE_PENDING):
            lst[:] = []
        ops._USES.clear()
        ops._LN_QUEUED[0] = ops._SIDE_JOIN_QUEUED[0] = False
        ops._LN_STASH[0] = None
        ops.set_cast_cache(None)
        _OUTPUTS.clear()


# ---------------------------------------------------------------------------------------------
# harness
# ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def switched(case, **extra):
    """The op's own csu.ops switches (and ``extra``) for the whole forward + backward."""
    from csu import ops
    want = dict(case.switches, **extra)
    old = {k: getattr(ops, k) for k in want}
    for k, v in want.items():
        setattr(ops, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


_BUILT = {}


def built(case, seed=0):
    """case.build(seed) and its copy on the device, made once: every Run clones from it (the table's inputs
    are seeded, so this only saves the generation and the upload)."""
    key = (case.name, seed)
    if key not in _BUILT:
        m = mods()
        inp = case.build(seed)
        on = lambda dct: {k: (v.to(m.dev) if torch.is_tensor(v) else v) for k, v in dct.items()}
        _BUILT[key] = NS(inp=inp, acts=on(inp.acts), params=on(inp.params), aux=on(inp.aux),
                         extra=case.gpu_aux(m, inp.aux) if case.gpu_aux else {})
    return _BUILT[key]


class Run:
    """One placement of a case's inputs on the device.  The parameters are always those of seed 0 (``params``:
    another Run's, shared); ``seed`` picks the activations.  ``req(name)``: requires_grad of each leaf."""

    def __init__(self, case, seed=0, params=None, req=lambda name: True):
        self.case, self.m = case, mods()
        b = built(case, seed)
        self.a = {k: v.clone().requires_grad_(bool(req(k))) for k, v in b.acts.items()}
        self.p = params if params is not None else {k: v.clone().requires_grad_(bool(req(k)))
                                                    for k, v in built(case, 0).params.items()}
        self.x = dict(b.aux)        # read-only for the ops (bn_relu_nhwc's case copies its running statistics)
        self.x.update(b.extra, log=_OUTPUTS)

    def leaves(self):
        return {**self.a, **self.p}

    def forward(self, a=None):
        case, m = self.case, self.m
        a = self.a if a is None else a
        for k, t in {**a, **self.p}.items():
            if t.is_contiguous():           # what an op's .contiguous() passes on as it is
                assert t.data_ptr() % 16 == 0, f"{case.name}: {k} is not 16-byte aligned; nothing launched"
        ctx = case.setup(m, self.p, self.x) if case.setup else contextlib.nullcontext()
        with ctx, torch.autocast("cuda", dtype=BF16, enabled=case.autocast):
            outs = tuple(case.call(m, a, self.p, self.x))
        _OUTPUTS.extend(outs)
        return outs

    def grads(self):
        return {k: (None if t.grad is None else t.grad.detach()) for k, t in self.leaves().items()}


def upstream(outs, seed=0):
    """Seeded CPU upstream gradients in the outputs' dtypes."""
    g = torch.Generator().manual_seed(4242 + seed)
    return [torch.randn(tuple(o.shape), generator=g).to(o.dtype) for o in outs]


def to_dev(gs):
    return [g.to(dev()) for g in gs]


_REF = {}


def reference(case, seed=0):
    """The fp64 reference graph of (activations of ``seed``, parameters of seed 0), built once and kept."""
    key = (case.name, seed)
    if key not in _REF:
        inp = built(case, seed).inp
        a = {k: v.double().requires_grad_(True) for k, v in inp.acts.items()}
        p = {k: v.double().requires_grad_(True) for k, v in built(case, 0).inp.params.items()}
        x = dict(inp.aux)
        x.update(built(case, seed).extra)       # the masks the device drew, read back
        _REF[key] = NS(a=a, p=p, outs=tuple(case.ref(a, p, x)), grads={})
    return _REF[key]


def ref_grads(ref, gs):
    """{leaf name: fp64 gradient} of the reference for the upstream gradients ``gs`` (any dtype, CPU)."""
    leaves = {**ref.a, **ref.p}
    # most patterns back-propagate the plain call's upstream gradients: one fp64 backward serves them all
    key = tuple((tuple(g.shape), float(g.double().sum()), float(g.double().abs().sum())) for g in gs)
    if key in ref.grads:
        return dict(ref.grads[key])
    ref.grads[key] = out = _ref_grads(ref, leaves, gs)
    return dict(out)


def _ref_grads(ref, leaves, gs):
    grads = torch.autograd.grad(ref.outs, list(leaves.values()), [g.detach().double().cpu() for g in gs], retain_graph=True,
                                allow_unused=True)
    return {k: (torch.zeros_like(t) if g is None else g) for (k, t), g in zip(leaves.items(), grads)}


def crit(case, got, ref, what):
    """The fp64 criterion of the op."""
    assert got is not None, f"{case.name} {what}: no gradient"
    assert tuple(got.shape) == tuple(ref.shape), f"{case.name} {what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    try:
        assert_close(got.detach(), ref.detach(), case.tol)
    except AssertionError as e:
        raise AssertionError(f"{case.name} {what}: {e}") from None


def crit_all(case, outs, grads, ref, rg, what=""):
    for i, (o, r) in enumerate(zip(outs, ref.outs)):
        crit(case, o, r, f"{what} out{i}")
    for k, r in rg.items():
        if k in grads and grads[k] is not None:
            crit(case, grads[k], r, f"{what} d{k}")


def plain_run(case, gs=None, seed=0):
    """Pattern A: one forward, one backward with ``gs`` (default: upstream(seed))."""
    with switched(case):
        run = Run(case, seed)
        outs = run.forward()
        gs = upstream(outs, seed) if gs is None else gs
        torch.autograd.backward(list(outs), to_dev(gs))
    return NS(outs=[o.detach().clone() for o in outs], grads={k: g.clone() for k, g in run.grads().items()}, gs=gs)


_PLAIN = {}


def plain(case, seed=0):
    key = (case.name, seed)
    if key not in _PLAIN:
        r = plain_run(case, None, seed)
        ref = reference(case, seed)       # the anchor itself meets the fp64 criterion, or nothing is compared with it
        crit_all(case, r.outs, r.grads, ref, ref_grads(ref, r.gs), "plain")
        _PLAIN[key] = r
    return _PLAIN[key]


def verify(case, outs, grads, anchor, run, same_path, ref, rg, what):
    """Every output and gradient of a pattern that back-propagates the plain call's upstream gradients:
    torch.equal with the plain call where the pattern keeps the op on the same kernels -- which also is
    the fp64 criterion, met by the anchor (plain()) -- and the fp64 criterion itself for the rest."""
    exempt = case.name in BITWISE_EXEMPT
    for i, (o, r) in enumerate(zip(outs, anchor.outs)):
        if exempt:
            crit(case, o, ref.outs[i], f"{what} out{i}")
        else:
            assert torch.equal(o.detach(), r), f"{case.name} {what}: out{i} differs from the plain call's"
    for k, g in grads.items():
        if g is None:
            continue
        if exempt or (not same_path and case.defers and (k in run.p or case.fused_dx)):
            crit(case, g, rg[k], f"{what} d{k}")
        else:
            assert torch.equal(g, anchor.grads[k]), f"{case.name} {what}: d{k} differs from the plain call's"


def same(case, outs, grads, anchor, run, same_path, what="", scale=1.0, base=None):
    """torch.equal with the plain call ``anchor`` (``scale`` times its gradients, plus ``base``) for what the
    pattern leaves on the same kernels (module docstring)."""
    if case.name in BITWISE_EXEMPT:
        return
    if outs is not None:
        for i, (o, r) in enumerate(zip(outs, anchor.outs)):
            assert torch.equal(o.detach(), r), f"{case.name} {what}: out{i} differs from the plain call's"
    for k, g in grads.items():
        if g is None or anchor.grads.get(k) is None:
            continue
        if not same_path and case.defers and (k in run.p or case.fused_dx):
            continue
        want = anchor.grads[k] * scale
        if base is not None and k in base:
            want = base[k] + want
        assert torch.equal(g, want), f"{case.name} {what}: d{k} differs from the plain call's"


def cases(pattern):
    return CC.applicable(pattern)


def test_every_pair_is_a_test_or_has_a_reason():
    for c in CC.CASES:
        for pat in CC.PATTERNS:
            why = CC.not_applicable(c, pat)
            assert why is None or (isinstance(why, str) and len(why) > 10), (c.name, pat)
    for pat in CC.PATTERNS:       # and every pattern name has its test function below
        assert f"test_{pat}" in globals(), pat


# ---------------------------------------------------------------------------------------------
# A. plain
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases("A"))
def test_A(name):
    case = CC.BY_NAME[name]
    dev()
    r = plain(case)
    ref = reference(case)
    crit_all(case, r.outs, r.grads, ref, ref_grads(ref, r.gs), "plain")
    for k, g in r.grads.items():
        assert g is not None, (name, k)
    again = plain_run(case, r.gs)
    if name not in BITWISE_EXEMPT:
        for i, (o, o2) in enumerate(zip(r.outs, again.outs)):
            assert torch.equal(o, o2), f"{name}: out{i} of two plain calls differs"
        for k in r.grads:
            assert torch.equal(r.grads[k], again.grads[k]), f"{name}: d{k} of two plain calls differs"


# ---------------------------------------------------------------------------------------------
# B. layouts of inputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases("B"))
def test_B(name):
    case = CC.BY_NAME[name]
    d = dev()
    anchor = plain(case)
    ref = reference(case)
    rg = ref_grads(ref, anchor.gs)

    def new(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=d)

    for act in built(case).inp.acts:
        for lname, make in CC.LAYOUTS.items():
            with switched(case):
                run = Run(case)
                v = make(run.a[act].detach(), new)
                assert (not v.is_contiguous()) or v.storage_offset() != 0, (name, act, lname)
                assert torch.equal(v, run.a[act]), (name, act, lname)
                a = dict(run.a)
                a[act] = v.detach().requires_grad_(True)
                outs = run.forward(a)
                torch.autograd.backward(list(outs), to_dev(anchor.gs))
            grads = {k: t.grad for k, t in {**a, **run.p}.items()}
            what = f"{act} as {lname}"
            verify(case, outs, grads, anchor, run, True, ref, rg, what)


# ---------------------------------------------------------------------------------------------
# C. layouts of the upstream gradient
# ---------------------------------------------------------------------------------------------
def _check_c(case, run, outs, gs_equiv, what):
    """After a backward whose upstream gradients equal ``gs_equiv`` in value."""
    ref = reference(case)
    grads = run.grads()
    crit_all(case, outs, grads, ref, ref_grads(ref, gs_equiv), what)
    same(case, outs, grads, plain_run(case, gs_equiv), run, True, what)


@pytest.mark.parametrize("name", cases("C_sum"))
def test_C_sum(name):
    case = CC.BY_NAME[name]
    dev()
    with switched(case):
        run = Run(case)
        outs = run.forward()
        total = outs[0].sum()
        for o in outs[1:]:
            total = total + o.sum()
        total.backward()        # every output's gradient: ones expanded from one element (stride 0)
    _check_c(case, run, outs, [torch.ones(tuple(o.shape), dtype=o.dtype) for o in outs], "sum().backward()")


@pytest.mark.parametrize("name", cases("C_noncontig"))
def test_C_noncontig(name):
    case = CC.BY_NAME[name]
    dev()
    # the outputs consumed through a transpose: the gradient arrives as a transposed (non-contiguous) view
    with switched(case):
        run = Run(case)
        outs = run.forward()
        gs = upstream(outs, 3)
        torch.autograd.backward([o.transpose(-1, -2) for o in outs], to_dev([g.transpose(-1, -2).contiguous() for g in gs]))
    _check_c(case, run, outs, gs, "out.transpose")
    # through out[..., ::2]: the gradient is the slice's backward (zeros between the values)
    with switched(case):
        run = Run(case)
        outs = run.forward()
        gs = upstream(outs, 4)
        torch.autograd.backward([o[..., ::2] for o in outs], to_dev([g[..., ::2].contiguous() for g in gs]))
    full = []
    for g in gs:
        z = torch.zeros_like(g)
        z[..., ::2] = g[..., ::2]
        full.append(z)
    _check_c(case, run, outs, full, "out[..., ::2]")


@pytest.mark.parametrize("name", cases("C_dtype"))
def test_C_dtype(name):
    case = CC.BY_NAME[name]
    dev()
    with switched(case):
        run = Run(case)
        outs = run.forward()
        other = [F32 if o.dtype == BF16 else BF16 for o in outs]
        gs = [g.to(dt) for g, dt in zip(upstream(outs, 5), other)]
        torch.autograd.backward([o.to(dt) for o, dt in zip(outs, other)], to_dev(gs))
    _check_c(case, run, outs, [g.to(o.dtype) for g, o in zip(gs, outs)], "gradient of the other float dtype")


# ---------------------------------------------------------------------------------------------
# D. partial differentiation
# ---------------------------------------------------------------------------------------------
def _partial(case, req, what):
    ref = reference(case)
    with switched(case):
        run = Run(case, req=req)
        outs = run.forward()
        gs = upstream(outs)
        torch.autograd.backward(list(outs), to_dev(gs))
    rg = ref_grads(ref, gs)
    for k, t in run.leaves().items():
        if req(k):
            crit(case, t.grad, rg[k], f"{what} d{k}")
        else:
            assert t.grad is None, f"{case.name} {what}: frozen {k} got a .grad"
    for i, (o, r) in enumerate(zip(outs, ref.outs)):
        crit(case, o, r, f"{what} out{i}")


@pytest.mark.parametrize("name", cases("D_acts_only"))
def test_D_acts_only(name):
    case = CC.BY_NAME[name]
    dev()
    acts = set(built(case).inp.acts)
    _partial(case, lambda k: k in acts, "parameters frozen")


@pytest.mark.parametrize("name", cases("D_params_only"))
def test_D_params_only(name):
    case = CC.BY_NAME[name]
    dev()
    params = set(built(case).inp.params)
    _partial(case, lambda k: k in params, "activations without grad")


@pytest.mark.parametrize("name", cases("D_alternate"))
def test_D_alternate(name):
    """Weight frozen with the bias trainable, and the reverse: every other parameter of the op's signature."""
    case = CC.BY_NAME[name]
    dev()
    params = list(built(case).inp.params)
    for parity in (0, 1):
        frozen = {k for i, k in enumerate(params) if i % 2 == parity}
        _partial(case, lambda k: k not in frozen, f"frozen {sorted(frozen)}")


@pytest.mark.parametrize("name", cases("D_grad_each"))
def test_D_grad_each(name):
    case = CC.BY_NAME[name]
    dev()
    ref = reference(case)
    with switched(case):
        run = Run(case)
        outs = run.forward()
        gs = upstream(outs)
        rg = ref_grads(ref, gs)
        gd = to_dev(gs)
        for k, t in run.leaves().items():
            (g,) = torch.autograd.grad(list(outs), [t], gd, retain_graph=True)
            crit(case, g, rg[k], f"autograd.grad(out, [{k}])")       # complete when the call returns
    for k, t in run.leaves().items():
        assert t.grad is None, (name, k)


# ---------------------------------------------------------------------------------------------
# E. one output unused
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases("E"))
def test_E(name):
    case = CC.BY_NAME[name]
    dev()
    ref = reference(case)
    if case.stats_call is not None:
        with switched(case):
            run = Run(case)
            res = tuple(case.stats_call(run.m, run.a, run.p, run.x))
            gs = upstream(res[:1])
            for extra in res[1:]:      # the statistics (and seg_bd's terms) are not part of the graph
                assert not extra.requires_grad and extra.grad_fn is None, name
            res[0].backward(to_dev(gs)[0])
        crit_all(case, res[:1], run.grads(), ref, ref_grads(ref, gs), "with_stats")
        return
    assert len(ref.outs) == 2
    for used in (0, 1):
        with switched(case):
            run = Run(case)
            outs = run.forward()
            gs = upstream(outs)
            outs[used].backward(to_dev(gs)[used])
        gs_equiv = [g if i == used else torch.zeros_like(g) for i, g in enumerate(gs)]
        crit_all(case, outs, run.grads(), ref, ref_grads(ref, gs_equiv), f"only output {used} used")


# ---------------------------------------------------------------------------------------------
# F. reuse and accumulation
# ---------------------------------------------------------------------------------------------
def _two(case):
    """Two placements sharing the parameters: activations of seed 0 and of seed 1."""
    r1 = Run(case, 0)
    return r1, Run(case, 1, params=r1.p)


def _sum_refs(case, gs1, gs2):
    rg1, rg2 = ref_grads(reference(case, 0), gs1), ref_grads(reference(case, 1), gs2)
    return rg1, rg2


def _check_two(case, r1, r2, o1, o2, gs1, gs2, what):
    """Gradients after both passes: the parameters' are the sum of the two references."""
    rg1, rg2 = _sum_refs(case, gs1, gs2)
    a1, a2 = plain(case, 0), plain(case, 1)
    for run, outs, rg, anchor, tag in ((r1, o1, rg1, a1, "x1"), (r2, o2, rg2, a2, "x2")):
        grads = {k: t.grad for k, t in run.a.items()}
        crit_all(case, outs, grads, reference(case, 0 if tag == "x1" else 1), {k: rg[k] for k in run.a}, f"{what} {tag}")
        same(case, outs, grads, anchor, run, False, f"{what} {tag}")
    for k, t in r1.p.items():
        crit(case, t.grad, rg1[k] + rg2[k], f"{what} d{k}")
        if name_ok(case) and not case.defers:
            assert torch.equal(t.grad, a1.grads[k] + a2.grads[k]), f"{case.name} {what}: d{k} is not the sum of the plain calls'"


def name_ok(case):
    return case.name not in BITWISE_EXEMPT


@pytest.mark.parametrize("name", cases("F_two_calls"))
def test_F_two_calls(name):
    case = CC.BY_NAME[name]
    dev()
    with switched(case):
        r1, r2 = _two(case)
        o1, o2 = r1.forward(), r2.forward()
        gs1, gs2 = upstream(o1, 0), upstream(o2, 1)
        torch.autograd.backward(list(o1) + list(o2), to_dev(gs1) + to_dev(gs2))
    _check_two(case, r1, r2, o1, o2, gs1, gs2, "f(x1) + f(x2)")


@pytest.mark.parametrize("name", cases("F_micro_batches"))
def test_F_micro_batches(name):
    case = CC.BY_NAME[name]
    dev()
    with switched(case):
        r1, r2 = _two(case)
        o1 = r1.forward()
        gs1 = upstream(o1, 0)
        torch.autograd.backward(list(o1), to_dev(gs1))
        o2 = r2.forward()
        gs2 = upstream(o2, 1)
        torch.autograd.backward(list(o2), to_dev(gs2))
    _check_two(case, r1, r2, o1, o2, gs1, gs2, "two micro-batches")


@pytest.mark.parametrize("name", cases("F_retain_twice"))
def test_F_retain_twice(name):
    case = CC.BY_NAME[name]
    dev()
    anchor = plain(case)
    ref = reference(case)
    with switched(case):
        run = Run(case)
        outs = run.forward()
        gd = to_dev(anchor.gs)
        torch.autograd.backward(list(outs), gd, retain_graph=True)
        torch.autograd.backward(list(outs), gd)
    grads = run.grads()
    rg = {k: 2 * g for k, g in ref_grads(ref, anchor.gs).items()}       # the bound applies to the doubled reference
    crit_all(case, outs, grads, ref, rg, "backward twice")
    same(case, outs, grads, anchor, run, False, "backward twice", scale=2.0)


@pytest.mark.parametrize("name", cases("F_existing_grad"))
def test_F_existing_grad(name):
    case = CC.BY_NAME[name]
    d = dev()
    anchor = plain(case)
    ref = reference(case)
    rg = ref_grads(ref, anchor.gs)
    for kind in ("contiguous", "a view into a larger buffer"):
        g = torch.Generator().manual_seed(99)
        with switched(case):
            run = Run(case)
            base, ptrs = {}, {}
            for k, t in run.p.items():
                g0 = torch.randn(tuple(t.shape), generator=g).to(d)
                if kind == "contiguous":
                    t.grad = g0.clone()
                else:
                    buf = torch.zeros(t.numel() + 16, device=d)
                    t.grad = buf[8:8 + t.numel()].view(t.shape)      # 32 B into its allocation
                    t.grad.copy_(g0)
                    assert t.grad.storage_offset() == 8 and t.grad.data_ptr() % 16 == 0
                base[k], ptrs[k] = g0, t.grad.data_ptr()
            outs = run.forward()
            torch.autograd.backward(list(outs), to_dev(anchor.gs))
        grads = run.grads()
        for k, t in run.p.items():
            assert t.grad.data_ptr() == ptrs[k], f"{name}: the existing .grad of {k} ({kind}) was replaced"
            crit(case, t.grad, base[k].double().cpu() + rg[k], f"existing .grad ({kind}) d{k}")
        crit_all(case, outs, {k: grads[k] for k in run.a}, ref, rg, f"existing .grad ({kind})")
        same(case, outs, grads, anchor, run, False, f"existing .grad ({kind})", base=base)


@pytest.mark.parametrize("name", cases("F_no_grad_between"))
def test_F_no_grad_between(name):
    """Validation in the middle of a step: a no_grad forward on other inputs, same parameters, between the
    forward and its backward, changes nothing (the attached LayerNorms, the stash, the cast cache)."""
    case = CC.BY_NAME[name]
    dev()
    anchor = plain(case)
    ref = reference(case)
    with switched(case):
        r1, r2 = _two(case)
        outs = r1.forward()
        with torch.no_grad():
            r2.forward()
        torch.autograd.backward(list(outs), to_dev(anchor.gs))
    grads = r1.grads()
    verify(case, outs, grads, anchor, r1, True, ref, ref_grads(ref, anchor.gs), "no_grad forward between")
    for k, t in r2.a.items():
        assert t.grad is None


# ---------------------------------------------------------------------------------------------
# G. readers of gradients
# ---------------------------------------------------------------------------------------------
def _hooked(case, register, what):
    """Forward + backward with a hook on every parameter that clones what it sees -- stream-ordered, no
    synchronise, so unwritten memory would be cloned as it is.  Hooks force the weight gradients inline:
    no late gradient exists, ops.STATS["late_grad_fixups"] stays (checked after every test)."""
    ref = reference(case)
    seen = {}
    with switched(case):
        run = Run(case)
        handles = [register(t, k, seen) for k, t in run.p.items()]
        outs = run.forward()
        gs = upstream(outs)
        torch.autograd.backward(list(outs), to_dev(gs))
    for h in handles:
        h.remove()
    rg = ref_grads(ref, gs)
    for k in run.p:
        crit(case, seen.get(k), rg[k], f"{what}: what the hook on {k} saw")
    crit_all(case, outs, run.grads(), ref, rg, what)


@pytest.mark.parametrize("name", cases("G_tensor_hooks"))
def test_G_tensor_hooks(name):
    dev()
    _hooked(CC.BY_NAME[name], lambda t, k, seen: t.register_hook(lambda g: seen.__setitem__(k, g.clone())), "register_hook")


@pytest.mark.parametrize("name", cases("G_post_hooks"))
def test_G_post_hooks(name):
    dev()
    _hooked(CC.BY_NAME[name],
            lambda t, k, seen: t.register_post_accumulate_grad_hook(lambda p: seen.__setitem__(k, p.grad.clone())),
            "post-accumulate hook")


@pytest.mark.parametrize("name", cases("G_autograd_grad"))
def test_G_autograd_grad(name):
    """torch.autograd.grad(out, params): deferral and the side stream stay on (no .grad, no hook), the
    returned tensors are the late buffers themselves and must be complete when the call returns.  No .grad
    exists afterwards, so there is nothing to repair: late_grad_fixups stays."""
    case = CC.BY_NAME[name]
    dev()
    ref = reference(case)
    with switched(case):
        run = Run(case)
        outs = run.forward()
        gs = upstream(outs)
        got = torch.autograd.grad(list(outs), list(run.p.values()), to_dev(gs))
    rg = ref_grads(ref, gs)
    for (k, t), g in zip(run.p.items(), got):
        crit(case, g, rg[k], f"autograd.grad(out, params) d{k}")
        assert t.grad is None
    anchor = plain(case)
    if gs_equal(gs, anchor.gs):
        same(case, None, dict(zip(run.p, got)), anchor, run, True, "autograd.grad(out, params)")


def gs_equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------
# H. create_graph=True
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases("H"))
def test_H(name):
    case = CC.BY_NAME[name]
    dev()
    anchor = plain(case)
    ref = reference(case)
    with switched(case):
        run = Run(case)
        outs = run.forward()
        torch.autograd.backward(list(outs), to_dev(anchor.gs), create_graph=True)
    grads = run.grads()
    try:
        crit_all(case, outs, grads, ref, ref_grads(ref, anchor.gs), "create_graph=True")
        same(case, outs, grads, anchor, run, False, "create_graph=True")
    finally:
        for t in run.leaves().values():     # .grad holds the graph: break the cycle
            t.grad = None


# ---------------------------------------------------------------------------------------------
# I. non-default stream
# ---------------------------------------------------------------------------------------------
def _on_stream(name, side):
    case = CC.BY_NAME[name]
    dev()
    anchor = plain(case)
    ref = reference(case)
    with switched(case, SIDE_WGRAD=side):
        run = Run(case)
        gd = to_dev(anchor.gs)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            outs = run.forward()
            torch.autograd.backward(list(outs), gd)
        s.synchronize()
    grads = run.grads()
    what = f"user stream, SIDE_WGRAD {'on' if side else 'off'}"
    same_path = side == case.switches.get("SIDE_WGRAD", True)
    verify(case, outs, grads, anchor, run, same_path, ref, ref_grads(ref, anchor.gs), what)


@pytest.mark.parametrize("name", cases("I_side_on"))
def test_I_side_on(name):
    _on_stream(name, True)


@pytest.mark.parametrize("name", cases("I_side_off"))
def test_I_side_off(name):
    _on_stream(name, False)


# ---------------------------------------------------------------------------------------------
# what the patterns found
# ---------------------------------------------------------------------------------------------
def test_summed_gradient_gets_a_fresh_bf16_copy():
    """A gradient that carries its bf16 copy (``_csu_bf16``, written by the LayerNorm junction's backward)
    and is then summed with a second consumer's gradient: the autograd engine adds INTO it in place, the
    Python attribute survives, and the upstream Linear's backward must not take the copy of the first
    addend for the sum.  h = linear(x) feeds layer_norm_fork and a plain torch consumer."""
    from csu import ops
    d = dev()
    M, K, C = 37, 64, 64
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, M, K, generator=g).bfloat16()
    w, b = torch.randn(C, K, generator=g) * K ** -0.5, torch.randn(C, generator=g) * 0.1
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    g1, g2, g3 = (torch.randn(1, M, C, generator=g) for _ in range(3))
    g2 = g2.bfloat16()
    g3 = g3 * 4.0       # the addend the stale copy would lose dominates
    leaves = [t.to(d).requires_grad_(True) for t in (x, w, b, gam, bet)]
    xd, wd, bd, gd, btd = leaves
    with torch.autocast("cuda", dtype=BF16):
        h = ops.linear(xd, wd, bd, out_dtype=F32)
        t = h * g3.to(d)                                   # created first: its gradient reaches h second
        xa, y = ops.layer_norm_fork(h, gd, btd, CC.EPS, BF16)
    torch.autograd.backward([t.sum(), xa, y], [None, g1.to(d), g2.to(d)])
    r = [v.double().requires_grad_(True) for v in (x, w, b, gam, bet)]
    h64 = torch.nn.functional.linear(r[0], r[1], r[2])
    y64 = torch.nn.functional.layer_norm(h64, (C,), r[3], r[4], CC.EPS)
    torch.autograd.backward([(h64 * g3.double()).sum(), h64, y64], [None, g1.double(), g2.double()])
    for name, got, ref in zip(("dx", "dW", "db", "dgamma", "dbeta"), leaves, r):
        try:
            assert_close(got.grad, ref.grad, BF16)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None


@pytest.mark.parametrize("name", ["linear_residual_ln_next", "mlp_residual_ln_next"])
def test_in_place_change_invalidates_the_attached_layer_norm(name):
    """An output that carries the next LayerNorm (``_csu_ln``) and is then changed in place (no_grad): the
    junction must normalise the new values, not hand out the attached ones, and the stale attachment goes."""
    case = CC.BY_NAME[name]
    d = dev()
    C = case.build(0).params["gamma"].numel()
    held = []
    with switched(case), torch.no_grad():
        run = Run(case)
        run.x["log"] = held
        run.forward()                          # producing launch + junction on the attached values
        y = held[0]
        assert getattr(y, "_csu_ln", None) is not None
        noise = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)).to(d)
        y.add_(noise)
        _, hn = run.m.ops.layer_norm_fork(y, run.p["gamma"], run.p["beta"], CC.EPS, BF16)
    _OUTPUTS.append(y)
    assert getattr(y, "_csu_ln", None) is None
    want = torch.nn.functional.layer_norm(y.double().cpu(), (C,), run.p["gamma"].double().cpu(), run.p["beta"].double().cpu(),
                                          CC.EPS)
    assert_close(hn, want, BF16)


# ---------------------------------------------------------------------------------------------
# K. module level
# ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _active_cache(linears=(), convs=()):
    """The cast cache as CSWinTransformer.forward activates it around its forward (bf16 shadows of the Linear
    weights and biases, their fragment-ordered copies, the conv layouts)."""
    from csu import ops
    cache = ops.CastCache()
    cache.refresh(list(linears), BF16, list(convs))
    cache.refresh_frag()
    ops.set_cast_cache(cache)
    try:
        yield
    finally:
        ops.set_cast_cache(None)


def _block(dim, reso, heads, split, last):
    from csu.model import CSWinBlock
    torch.manual_seed(dim + reso)
    m = CSWinBlock(dim=dim, reso=reso, num_heads=heads, split_size=split, qkv_bias=True, last_stage=last).to(dev())
    lin = [p for mod in m.modules() if isinstance(mod, torch.nn.Linear) for p in (mod.weight, mod.bias)]
    first = [m.norm1.weight, m.norm1.bias]
    last_ = [m.mlp.fc2.weight, m.mlp.fc2.bias]
    return m, (lambda: _active_cache(lin)), first, last_


class _UNetPath(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from csu.unet import DoubleConv, Down, Up
        self.inc, self.down, self.up = DoubleConv(16, 32), Down(32, 64), Up(64, 32)

    def forward(self, x):
        x1 = self.inc(x)
        return self.up(self.down(x1), x1)


def _unet_path():
    torch.manual_seed(11)
    m = _UNetPath().to(dev())
    convs = [mod.weight for mod in m.modules() if isinstance(mod, torch.nn.Conv2d)]
    c0 = m.inc.double_conv[0]
    bn = m.up.conv.double_conv[4]
    return m, (lambda: _active_cache((), convs)), [c0.weight, c0.bias], [bn.weight, bn.bias]


MODULES = {
    # the smallest geometry of test_gpu_model.py::test_cswin_block_vs_golden (C = 64: the unfused junctions)
    "cswin_block_64": (lambda: _block(64, 4, 2, 4, True), (2, 16, 64)),
    # and the narrowest one whose junctions run fused (ln_linear_ws, linear_residual + norm2, ln_mlp_residual)
    "cswin_block_128": (lambda: _block(128, 8, 4, 2, False), (1, 64, 128)),
    "unet_doubleconv_down_up": (_unet_path, (2, 8, 8, 16)),
}


def _module_step(m, cache, x, gy, between=None):
    """One train-mode forward + backward under bf16 autocast with the cast cache active: {name: .grad}."""
    for p in m.parameters():
        p.grad = None
    m.train()
    with cache(), torch.autocast("cuda", dtype=BF16):
        y = m(x)
    _OUTPUTS.append(y)
    if between is not None:
        m.eval()
        with torch.no_grad(), cache(), torch.autocast("cuda", dtype=BF16):
            m(between)
        m.train()
    y.backward(gy.to(y.dtype))
    return {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}


@pytest.mark.parametrize("which", list(MODULES))
def test_K(which):
    make, shape = MODULES[which]
    d = dev()
    m, cache, first, last = make()
    g = torch.Generator().manual_seed(21)
    x, x2 = torch.randn(shape, generator=g).to(d), torch.randn(shape, generator=g).to(d)
    with torch.no_grad(), cache(), torch.autocast("cuda", dtype=BF16):
        yshape = m(x).shape
    gy = torch.randn(tuple(yshape), generator=g).to(d)
    full = _module_step(m, cache, x, gy)
    assert all(v is not None and bool(torch.isfinite(v).all()) for v in full.values())
    ids = {id(p): k for k, p in m.named_parameters()}
    # everything frozen but the last layer
    for p in m.parameters():
        p.requires_grad_(False)
    for p in last:
        p.requires_grad_(True)
    got = _module_step(m, cache, x, gy)
    for k, v in got.items():
        if k in {ids[id(p)] for p in last}:
            assert torch.equal(v, full[k]), f"{which}: {k} changed when the other layers were frozen"
        else:
            assert v is None, f"{which}: frozen {k} got a .grad"
    # only the first layer frozen
    for p in m.parameters():
        p.requires_grad_(True)
    for p in first:
        p.requires_grad_(False)
    got = _module_step(m, cache, x, gy)
    for k, v in got.items():
        if k in {ids[id(p)] for p in first}:
            assert v is None, f"{which}: frozen {k} got a .grad"
        else:
            assert torch.equal(v, full[k]), f"{which}: {k} changed when the first layer was frozen"
    # an eval-mode no_grad forward between the train forward and its backward
    for p in m.parameters():
        p.requires_grad_(True)
    got = _module_step(m, cache, x, gy, between=x2)
    for k, v in got.items():
        assert torch.equal(v, full[k]), f"{which}: {k} changed by a no_grad forward before the backward"
