"""The group-aware weight-gradient planner (csu_linear_wgrad_group_plan_all): host code, no GPU.
Every list x every CU count: the plan covers each Linear's tokens exactly once in 64-row multiples,
stays inside the slab cap, keeps csu_linear_wgrad_group_plan's tile shapes, fits the launch limits,
and depends on (cus, shapes in order) alone.  On the headline list an independent dispatch simulator
(per XCD, greedy over slots, fixed + steps x per-step cost per workgroup) must find the planned
launches no longer than the per-Linear plan's."""
import ctypes
import heapq

import pytest

from csu import _lib

PASSES = [(256, 128), (128, 128), (128, 64), (64, 128), (64, 64)]
WGG_MAX = 48


def _block(M, C):
    return [(M, 3 * C, C), (M, C, C), (M, 4 * C, C), (M, C, 4 * C)]


def _headline():
    s = []
    for _ in range(18):
        s += _block(16384, 256)
    for _ in range(2):
        s += _block(4096, 512)
    for _ in range(4):
        s += _block(65536, 128)
    return s + [(262144, 192, 64), (262144, 64, 64)]


LISTS = {
    "headline": _headline(),
    "one": [(16384, 768, 256)],
    "fifty": [(256, 64, 64)] * 50,
    "ragged": [(100, 64, 64), (4097, 256, 128), (65537, 128, 128), (99999, 192, 64), (4097, 64, 192), (65537, 768, 256),
               (99999, 128, 512), (100, 256, 256)],
}
CUS = (2, 8, 256)


def _plan(shapes, cus, base=0):
    n = len(shapes)
    items = (_lib.WgradGroupItem * n)()
    for i, (M, N, K) in enumerate(shapes):   # plan_all must not look at the pointers: any values will do
        p = base + 4096 * i if base else None
        items[i].dy, items[i].x, items[i].dw_db, items[i].slab, items[i].M, items[i].N, items[i].K = p, p, p, p, M, N, K
    out = (_lib.WgradGroupPlan * n)()
    assert _lib.lib().csu_linear_wgrad_group_plan_all(items, n, cus, out) == 0
    return [(p.tn, p.tk, p.chunks, p.rpc, p.slab_bytes, p.launch, p.pos) for p in out]


def _legacy(M, N, K):
    """csu_linear_wgrad_group_plan's (tn, tk, chunks) and the rows per chunk its launch uses."""
    tn, tk, ch = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.lib().csu_linear_wgrad_group_plan(M, N, K, ctypes.byref(tn), ctypes.byref(tk), ctypes.byref(ch))
    c = int(M * (N + K) / (32.0 * N * K) + 0.5)
    c = max(min(c, max(M // 1024, 1)), 1)
    r = -(-(-(-M // c)) // 64) * 64
    assert -(-M // r) == ch.value
    return tn.value, tk.value, ch.value, r


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("name", list(LISTS))
def test_plan_properties(name, cus):
    shapes = LISTS[name]
    plans = _plan(shapes, cus)
    slab_total, operand_total = 0, 0
    launches = {}
    for (M, N, K), (tn, tk, chunks, rpc, slab, launch, pos) in zip(shapes, plans):
        assert (tn, tk) == _legacy(M, N, K)[:2]
        assert chunks >= 1 and rpc >= 64 and rpc % 64 == 0
        assert (chunks - 1) * rpc < M <= chunks * rpc          # every token in exactly one chunk, no empty chunk
        nt, kt = -(-N // tn), -(-K // tk)
        written = (nt * kt * tn * tk + nt * tn) * chunks * 4 if chunks > 1 else 0
        assert slab >= written
        slab_total += slab
        operand_total += M * (N + K) * 2
        launches.setdefault(launch, []).append((pos, tn, tk, nt * kt * chunks))
    assert slab_total * 16 <= operand_total * 2
    order = []
    for launch in sorted(launches):
        members = sorted(launches[launch])
        assert [m[0] for m in members] == list(range(len(members))) and len(members) <= WGG_MAX
        assert len({m[1:3] for m in members}) == 1 and sum(m[3] for m in members) < 2 ** 30
        order.append(PASSES.index(members[0][1:3]))
    assert order == sorted(order)   # tile shapes go out in csu_linear_wgrad_group's order
    if name == "fifty":
        assert len(launches) >= 2
    if name == "one":
        assert len(launches) == 1


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("name", list(LISTS))
def test_plan_is_a_function_of_the_shapes(name, cus):
    shapes = LISTS[name]
    a = _plan(shapes, cus)
    assert a == _plan(shapes, cus)
    assert a == _plan(shapes, cus, base=0x7f0000000000) == _plan(shapes, cus, base=0x10000)
    if len(shapes) > 1:   # the same Linears behind another list still cover their tokens (another key, another plan)
        assert len(_plan(shapes[::-1], cus)) == len(shapes)
        assert a == _plan(shapes, cus)


def _model(tn, tk):
    f, s, w = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    _lib.lib().csu_linear_wgrad_group_model(tn, tk, ctypes.byref(f), ctypes.byref(s), ctypes.byref(w))
    return f.value, s.value, w.value


def _makespan(costs, cus, per_cu):
    """Workgroup id i runs on XCD i % 8, which walks a contiguous eighth of the logical ids; each
    workgroup goes to the slot of its XCD that is free first."""
    xcds = min(8, cus)
    slots = max(1, cus // xcds) * per_cu
    free = [[0.0] * slots for _ in range(xcds)]
    q, rem = divmod(len(costs), 8)
    worst, b = 0.0, 0
    for x in range(8):
        n = q + 1 if x < rem else q
        h = free[x % xcds]
        heapq.heapify(h)
        for c in costs[b:b + n]:
            t = heapq.heappop(h) + c
            heapq.heappush(h, t)
            worst = max(worst, t)
        b += n
    return worst


def _launch_costs(members):
    """members: [(M, N, K, tn, tk, chunks, rpc)] in launch order -> cost per logical workgroup."""
    costs = []
    for M, N, K, tn, tk, chunks, rpc in members:
        fixed, step, _ = _model(tn, tk)
        tiles = -(-N // tn) * -(-K // tk)
        for ch in range(chunks):
            rows = min(rpc, M - ch * rpc)
            costs += [fixed + step * -(-rows // 64)] * tiles
    return costs


def test_model_constants():
    for tn, tk in PASSES:
        fixed, step, per_cu = _model(tn, tk)
        assert fixed > 0 and step > 0
        assert per_cu == (1 if tn == 256 else 2)   # the launch bounds of wgrad_group<tn, tk>


def test_headline_plan_beats_per_linear_plan_on_the_simulator():
    shapes, cus = LISTS["headline"], 256
    plans = _plan(shapes, cus)
    new = 0.0
    for launch in sorted({p[5] for p in plans}):
        members = sorted((p[6], s + p[:4]) for s, p in zip(shapes, plans) if p[5] == launch)
        tn, tk = members[0][1][3:5]
        new += _makespan(_launch_costs([m[1] for m in members]), cus, _model(tn, tk)[2])
    old = 0.0
    legacy = [_legacy(*s) for s in shapes]
    for tn, tk in PASSES:
        members = [s + l for s, l in zip(shapes, legacy) if l[:2] == (tn, tk)]
        for j in range(0, len(members), WGG_MAX):
            old += _makespan(_launch_costs(members[j:j + WGG_MAX]), cus, _model(tn, tk)[2])
    print(f"simulated grouped launches: per-Linear plan {old:.1f} us, group plan {new:.1f} us")
    assert new <= old
