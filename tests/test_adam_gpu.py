"""GPU: the Adam step of csrc/adam.hip (``inerf_adam_step``, ``optim.Adam``) against ``torch.optim.Adam`` itself - on the CPU in
fp64 (the mathematics) and in fp32 (what the reference's trainer computes).

One step, per element, with eps = 2^-24 and from the same fp32 state:
    |m - m64| <= 4 eps max|g|       |v - v64| <= 4 eps max|g|^2       |p - p64| <= 8 eps (|p0| + |p64 - p0|)
(torch's own fp32 Adam sits at 0.12, 0.004 and 3.99 of those units; the kernel has the same number of roundings, the bound is
twice the reference's own distance).  A trajectory of 200 steps on a recorded gradient sequence: the project's plain 1e-4 per
tensor, ``max|p - p64| <= 1e-4 max(max|p64|, 1e-3)`` (torch's fp32 run ends 3.2e-7 from fp64 on parameters of scale 0.06: a
failure means a wrong formula, not rounding).  Measured on an MI355X: m 0.18, v 0.004, p 2.17 / 3.48 / 4.58 of those units at
steps 1 / 42 / 200 000 (torch's fp32 CPU Adam on the same inputs: 0.18, 0.004, 2.20 / 3.58 / 3.67); the trajectories end at
0.0095 / 0.0105 of their bound; three training steps in place of torch.optim.Adam at 0.48 of it.  Every test prints its worst figures before it asserts (``pytest -s``)."""
import copy
import ctypes as C
import types
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 2.0 ** -24
COUNTS = (1, 3, 63, 64, 65, 255, 257, 256 * 319)
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8


def lr_at(i, base=5e-4, decay=250):
    return base * 0.1 ** (i / (decay * 1000))            # run_nerf.py:1023-1025


# ---- helpers: the C ABI on lists of device tensors, and torch.optim.Adam on the CPU from a given state ----
def hip_step(P, G, M, V, S, lr, lr_dev=None, betas=BETAS, eps=ADAM_EPS):
    from intrinsicnerf_amd import _capi
    n = len(P)
    ptrs = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    keep = [ptrs(P), ptrs(G), ptrs(M), ptrs(V), ptrs(S), (C.c_int64 * n)(*[t.numel() for t in P])]
    a = _capi.AdamArgs()
    a.n_tensors = n
    a.params, a.grads, a.exp_avg, a.exp_avg_sq, a.steps, a.counts = (C.cast(x, C.c_void_p) for x in keep)
    a.lr, a.lr_dev = float(lr), None if lr_dev is None else lr_dev.data_ptr()
    a.beta1, a.beta2, a.eps = betas[0], betas[1], eps
    stream = C.c_void_p(torch.cuda.current_stream(P[0].device).cuda_stream)
    _capi.check(_capi.lib().inerf_adam_step(C.byref(a), stream), "inerf_adam_step")


def cpu_adam(p0, grads, m0, v0, t0, lrs, dtype):
    """``torch.optim.Adam`` on the CPU in ``dtype`` from the fp32 state (p0, m0, v0, step t0), one step per entry of ``grads``
    (each a list of tensors) with the rates ``lrs``: returns (params, exp_avg, exp_avg_sq, step counts)."""
    params = [torch.nn.Parameter(x.detach().cpu().to(dtype).clone()) for x in p0]
    opt = torch.optim.Adam(params, lr=lrs[0], betas=BETAS, eps=ADAM_EPS)
    for p, m, v, t in zip(params, m0, v0, t0):
        opt.state[p] = {"step": torch.tensor(float(t), dtype=torch.float32), "exp_avg": m.detach().cpu().to(dtype).clone(),
                        "exp_avg_sq": v.detach().cpu().to(dtype).clone()}
    for gs, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        for p, g in zip(params, gs):
            p.grad = None if g is None else g.detach().cpu().to(dtype)
        opt.step()
    st = [opt.state[p] for p in params]
    return [p.detach() for p in params], [s["exp_avg"] for s in st], [s["exp_avg_sq"] for s in st], [float(s["step"]) for s in st]


def units(got, want64, scale):
    """max over elements of |got - want64| / (eps * scale); an element whose scale is 0 must match exactly."""
    err = (got.detach().cpu().double() - want64).abs()
    scale = torch.as_tensor(scale, dtype=torch.float64).expand_as(err)
    assert bool((err[scale == 0] == 0).all())
    live = scale > 0
    return float((err[live] / (EPS * scale[live])).max()) if bool(live.any()) else 0.0


def assert_one_step(tag, P, M, V, p0, G, ref64, gmax_of=None):
    """The three one-step bounds of the module docstring, per element; returns the worst figures in their units.  max|g| of a
    tensor is taken over the step's gradient and, where the state before the step came from earlier steps, over theirs too
    (``gmax_of``): the moments' rounding scales with the gradients they were formed from."""
    p64, m64, v64, _ = ref64
    worst = [0.0, 0.0, 0.0]
    for i in range(len(P)):
        gmax = float(G[i].detach().abs().max().cpu()) if gmax_of is None else gmax_of[i]
        assert torch.isfinite(P[i]).all() and torch.isfinite(M[i]).all() and torch.isfinite(V[i]).all(), (tag, i)
        um = units(M[i], m64[i], gmax)
        uv = units(V[i], v64[i], gmax * gmax)
        up = units(P[i], p64[i], p0[i].detach().cpu().double().abs() + (p64[i] - p0[i].detach().cpu().double()).abs())
        worst = [max(a, b) for a, b in zip(worst, (um, uv, up))]
    print(f"\n{tag}: worst m {worst[0]:.3f} of 4, v {worst[1]:.4f} of 4, p {worst[2]:.3f} of 8 (units of eps)")
    assert worst[0] <= 4.0 and worst[1] <= 4.0 and worst[2] <= 8.0, (tag, worst)
    return worst


def issue_gradient(shape, gen):
    """Magnitudes 2^k per element, k uniform in [-40, 10], random sign, 5 % exactly zero."""
    k = torch.randint(-40, 11, shape, generator=gen).float()
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
    g = sign * torch.exp2(k)
    zero = torch.rand(shape, generator=gen) < 0.05
    if bool(zero.all()):                                              # (a one-element tensor: keep its gradient, max|g| = 0 bounds nothing)
        zero[...] = False
    g[zero] = 0.0
    return g


LAYOUTS = ("own", "view_all", "view_param")


def laid_out(values, layout, dev):
    """[p, g, m, v] on the device: each its own allocation; all four as views one float past a 16-byte boundary of flat buffers
    (the vector path with a scalar head); or only the parameter such a view (the four arrays disagree: one float per access)."""
    out = []
    for j, x in enumerate(values):
        if layout == "view_all" or (layout == "view_param" and j == 0):
            flat = torch.zeros(x.numel() + 8, dtype=torch.float32, device=dev)
            off = 1 + (j % 3 if layout == "view_param" else 0)
            t = flat[off:off + x.numel()]
            t.copy_(x.reshape(-1))
            assert t.data_ptr() % 16 == 4 * off
        else:
            t = x.reshape(-1).to(dev).clone()
        out.append(t)
    return out


def one_step_case(t0, seed, dev):
    """Every count of COUNTS in every layout, in one call; the state before the step is zero (t0 = 0) or what two steps of torch's
    fp32 Adam on gradients of the same magnitudes left, with the step count set to t0."""
    gen = torch.Generator().manual_seed(seed)
    P, G, M, V, S, p0, gmax = [], [], [], [], [], [], []
    for n in COUNTS:
        for layout in LAYOUTS:
            p = torch.randn(n, generator=gen) * 0.06
            m, v = torch.zeros(n), torch.zeros(n)
            warm = []
            if t0 > 0:
                warm = [[issue_gradient((n,), gen)] for _ in range(2)]
                ps, ms, vs, _ = cpu_adam([p], warm, [m], [v], [0], [5e-4, 5e-4], torch.float32)
                p, m, v = ps[0].clone(), ms[0].clone(), vs[0].clone()
            g = issue_gradient((n,), gen)
            gmax.append(max(float(x.abs().max()) for x in [g] + [w[0] for w in warm]))
            tp, tg, tm, tv = laid_out([p, g, m, v], layout, dev)
            P.append(tp); G.append(tg); M.append(tm); V.append(tv); p0.append(p)
            S.append(torch.tensor(float(t0), dtype=torch.float32, device=dev))
    return P, G, M, V, S, p0, gmax


@pytest.mark.parametrize("t0", [0, 41, 199999], ids=["first_step", "step_42", "step_200000"])
def test_one_step_against_fp64_on_every_count_and_alignment(t0):
    dev = torch.device(DEV)
    P, G, M, V, S, p0, gmax = one_step_case(t0, 100 + t0 % 7, dev)
    m0, v0 = [m.clone() for m in M], [v.clone() for v in V]
    lr = lr_at(t0)
    ref64 = cpu_adam(p0, [G], m0, v0, [t0] * len(P), [lr], torch.float64)
    hip_step(P, G, M, V, S, lr)
    torch.cuda.synchronize()
    assert all(float(s) == t0 + 1 for s in S)
    if t0 == 199999:
        # 1 - 0.9^200000 is 1 and 1 - 0.999^200000 is 1 - 1.4e-87 in fp64: the scalars must be exactly lr and 1, never 0 or NaN
        assert all(torch.isfinite(p).all() for p in P)
    assert_one_step(f"one step from t0 = {t0}", P, M, V, p0, G, ref64, gmax)
    # a zero gradient on zero state leaves the parameter bit-unchanged (torch's behaviour: 0 / (0 + eps) = 0)
    if t0 == 0:
        for p, g, q in zip(P, G, p0):
            zero = (g == 0).cpu()
            assert torch.equal(p.cpu()[zero], q[zero])
    # the same call with the rate on the device is the same arithmetic, bit for bit
    P2, G2, M2, V2, S2, _, _ = one_step_case(t0, 100 + t0 % 7, dev)
    hip_step(P2, G2, M2, V2, S2, 123.0, lr_dev=torch.tensor(lr, dtype=torch.float32, device=dev))
    for a, b in zip(P + M + V + S, P2 + M2 + V2 + S2):
        assert torch.equal(a, b)


def test_special_values_element_by_element_against_torch_fp32():
    dev = torch.device(DEV)
    g = torch.tensor([2.0 ** 70, -2.0 ** 70, float("inf"), float("nan"), 2.0 ** -80, 0.0, 1e-30])
    p0 = torch.ones(7)
    ps, ms, vs, _ = cpu_adam([p0], [[g], [g]], [torch.zeros(7)], [torch.zeros(7)], [0], [5e-4, 5e-4], torch.float32)
    ps64, ms64, _, _ = cpu_adam([p0], [[g], [g]], [torch.zeros(7)], [torch.zeros(7)], [0], [5e-4, 5e-4], torch.float64)
    P, G, M, V = [p0.to(dev)], [g.to(dev)], [torch.zeros(7, device=dev)], [torch.zeros(7, device=dev)]
    S = [torch.zeros((), device=dev)]
    hip_step(P, G, M, V, S, 5e-4)
    hip_step(P, G, M, V, S, 5e-4)
    p, m, v = P[0].cpu(), M[0].cpu(), V[0].cpu()
    print(f"\nspecial values: p {p.tolist()}\n  m {m.tolist()}\n  v {v.tolist()}\n  torch p {ps[0].tolist()}\n  torch m {ms[0].tolist()}\n  torch v {vs[0].tolist()}")
    nan, inf = float("nan"), float("inf")
    same = lambda a, b: all((x == y) or (x != x and y != y) for x, y in zip(a.tolist(), b))
    assert same(p, [1.0, 1.0, nan, nan, 1.0, 1.0, 1.0]) and same(ps[0], [1.0, 1.0, nan, nan, 1.0, 1.0, 1.0])
    assert same(v, [inf, inf, inf, nan, 0.0, 0.0, 0.0]) and same(vs[0], [inf, inf, inf, nan, 0.0, 0.0, 0.0])
    cls = lambda t: ["nan" if x != x else "inf" if abs(x) == inf else "zero" if x == 0 else "finite" for x in t.tolist()]
    assert cls(m) == cls(ms[0]), (cls(m), cls(ms[0]))
    assert float(S[0]) == 2.0
    fin = torch.isfinite(ms[0])
    gmax = g.abs()                                                     # per element here: the gradients span 150 binades
    err = (m[fin].double() - ms64[0][fin]).abs()
    assert bool((err <= 4 * EPS * gmax[fin].double()).all()), err


def network_shapes(which):
    from intrinsicnerf_amd import object_level as ol, ssr
    e, ch = ol.get_embedder(10, 0)
    ed, chd = ol.get_embedder(4, 0)
    if which == "object":
        net = ol.NeRF(D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=chd, use_viewdirs=True)
    else:
        net = ssr.Semantic_NeRF(True, 28, D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=chd, use_viewdirs=True)
    return [tuple(p.shape) for p in net.parameters()] * 2              # coarse + fine


@pytest.mark.parametrize("which,n_tensors", [("object", 64), ("ssr", 72)])
def test_trajectory_of_200_steps_on_a_recorded_gradient_sequence(which, n_tensors):
    from intrinsicnerf_amd import optim
    dev = torch.device(DEV)
    shapes = network_shapes(which)
    assert len(shapes) == n_tensors
    gen = torch.Generator().manual_seed(5)
    p0 = [torch.randn(s, generator=gen) * 0.06 for s in shapes]
    base = [[torch.randn(s, generator=gen) * 1e-3 for s in shapes] for _ in range(3)]
    steps = 200
    # the recorded sequence: three gradient sets, cycled, each step scaled by a power of two (exact in fp32 and fp64 alike)
    scale = [2.0 ** ((k * 7) % 5 - 2) for k in range(steps)]
    lrs = [lr_at(k) for k in range(steps)]

    def run_hip():
        params = [torch.nn.Parameter(x.to(dev).clone()) for x in p0]
        gs = [[g.to(dev) for g in b] for b in base]
        opt = optim.Adam(params, lr=lrs[0], betas=BETAS)
        for k in range(steps):
            opt.param_groups[0]["lr"] = lrs[k]
            for p, g in zip(params, gs[k % 3]):
                p.grad = g * scale[k]
            opt.step()
        torch.cuda.synchronize()
        return params, opt

    params, opt = run_hip()
    ref = [torch.nn.Parameter(x.double().clone()) for x in p0]
    ropt = torch.optim.Adam(ref, lr=lrs[0], betas=BETAS)
    b64 = [[g.double() for g in b] for b in base]
    for k in range(steps):
        ropt.param_groups[0]["lr"] = lrs[k]
        for p, g in zip(ref, b64[k % 3]):
            p.grad = g * scale[k]
        ropt.step()
    worst = 0.0
    for i, (p, q) in enumerate(zip(params, ref)):
        err = float((p.detach().cpu().double() - q.detach()).abs().max())
        bound = 1e-4 * max(float(q.detach().abs().max()), 1e-3)
        worst = max(worst, err / bound)
        assert err <= bound, (which, i, err, bound)
    print(f"\ntrajectory {which}: worst max|p - p64| = {worst:.2e} of the 1e-4 bound")
    assert all(float(opt.state[p]["step"]) == steps for p in params)
    again, _ = run_hip()
    assert all(torch.equal(a, b) for a, b in zip(params, again))                      # bit-identical run to run


def test_zero_gradients_leave_parameters_bit_unchanged():
    from intrinsicnerf_amd import optim
    dev = torch.device(DEV)
    gen = torch.Generator().manual_seed(2)
    params = [torch.nn.Parameter((torch.randn(n, generator=gen) * 0.06).to(dev)) for n in (1, 5, 4099)]
    before = [p.detach().clone() for p in params]
    opt = optim.Adam(params, lr=5e-4)
    for _ in range(3):
        for p in params:
            p.grad = torch.zeros_like(p)
        opt.step()
    assert all(torch.equal(p.detach(), b) for p, b in zip(params, before))
    assert all(float(opt.state[p]["step"]) == 3 and not opt.state[p]["exp_avg"].any() for p in params)


def _small_params(dev, seed, sizes):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(n, generator=gen) * 0.06).to(dev)) for n in sizes]


def test_parameters_without_a_gradient_are_skipped_entirely():
    from intrinsicnerf_amd import optim
    dev = torch.device(DEV)
    sizes = (1, 7, 64, 65, 300, 2049, 5, 4096, 33)
    gen = torch.Generator().manual_seed(3)
    grads = [[torch.randn(n, generator=gen).to(dev) * 1e-2 for n in sizes] for _ in range(2)]
    runs = {}
    for mode in ("full", "skip"):
        params = _small_params(dev, 1, sizes)
        opt = optim.Adam(params, lr=5e-4)
        for k in range(2):
            for i, p in enumerate(params):
                p.grad = None if (mode == "skip" and k == 1 and i % 3 == 0) else grads[k][i].clone()
            if k == 1:
                snap = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), opt.state[p]["step"].clone(), p._version)
                        for p in params]
            opt.step()
        runs[mode] = (params, opt, snap)
    params, opt, snap = runs["skip"]
    full, fopt, _ = runs["full"]
    for i, p in enumerate(params):
        st = opt.state[p]
        if i % 3 == 0:
            assert torch.equal(p.detach(), snap[i][0]) and torch.equal(st["exp_avg"], snap[i][1]) and torch.equal(st["exp_avg_sq"], snap[i][2])
            assert float(st["step"]) == 1.0 == float(snap[i][3]) and p._version == snap[i][4]
        else:
            fs = fopt.state[full[i]]
            assert torch.equal(p.detach(), full[i].detach()) and torch.equal(st["exp_avg"], fs["exp_avg"]) and torch.equal(st["exp_avg_sq"], fs["exp_avg_sq"])
            assert float(st["step"]) == 2.0 and p._version > snap[i][4]
    # a parameter that never had a gradient has no state at all, as in torch
    lone = _small_params(dev, 4, (3, 3))
    lopt = optim.Adam(lone, lr=5e-4)
    lone[0].grad = torch.ones_like(lone[0])
    lopt.step()
    assert "exp_avg" in lopt.state[lone[0]] and not lopt.state.get(lone[1])


def test_200_tensors_in_one_call_equal_200_single_calls():
    from intrinsicnerf_amd import _capi
    dev = torch.device(DEV)
    assert 200 > 2 * _capi.ADAM_TABLE_TENSORS                                           # three tables: 72 + 72 + 56
    gen = torch.Generator().manual_seed(6)
    sizes = [int(x) for x in torch.randint(1, 700, (200,), generator=gen)]
    sizes[71], sizes[72], sizes[143], sizes[144] = 4097, 1, 2048, 2049                    # across the table boundaries
    mk = lambda: ([(torch.randn(n, generator=torch.Generator().manual_seed(n + i)) * 0.06).to(dev) for i, n in enumerate(sizes)])
    G = [(torch.randn(n, generator=gen) * 1e-2).to(dev) for n in sizes]
    runs = []
    for single in (False, True):
        P = mk()
        M, V = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]
        S = [torch.full((), float(i % 5), device=dev) for i in range(200)]
        for _ in range(2):
            if single:
                for i in range(200):
                    hip_step(P[i:i + 1], G[i:i + 1], M[i:i + 1], V[i:i + 1], S[i:i + 1], 5e-4)
            else:
                hip_step(P, G, M, V, S, 5e-4)
        torch.cuda.synchronize()
        runs.append(P + M + V + S)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert [float(s) for s in runs[0][600:]] == [float(i % 5) + 2 for i in range(200)]


def _sync_from(src_params, src_opt, dst_params, dst_opt):
    with torch.no_grad():
        for d, s in zip(dst_params, src_params):
            d.copy_(s)
    dst_opt.load_state_dict(copy.deepcopy(src_opt.state_dict()))


@pytest.mark.parametrize("direction", ["inerf_to_torch", "torch_to_inerf"])
def test_state_dict_interop_on_the_device(direction):
    """20 steps with one class, its state_dict() loaded into the other over clones, then 5 steps on both with the same gradients:
    every one of them from the same fp32 state (re-loaded through state_dict each time), within the one-step bounds of fp64."""
    from intrinsicnerf_amd import optim
    dev = torch.device(DEV)
    sizes = (1, 28, 384, 3584, 65)
    gen = torch.Generator().manual_seed(8)
    grads = [[(torch.randn(n, generator=gen) * 10.0 ** -i).to(dev) for i, n in enumerate(sizes)] for _ in range(25)]        # a scale per tensor
    gmax = [max(float(grads[k][i].abs().max()) for k in range(25)) for i in range(len(sizes))]
    a_params, b_params = _small_params(dev, 9, sizes), _small_params(dev, 9, sizes)
    mk = {"inerf": lambda ps: optim.Adam(ps, lr=5e-4, betas=BETAS), "torch": lambda ps: torch.optim.Adam(ps, lr=5e-4, betas=BETAS)}
    first, second = direction.split("_to_")
    a, b = mk[first](a_params), mk[second](b_params)
    for k in range(20):
        a.param_groups[0]["lr"] = lr_at(k)
        for p, g in zip(a_params, grads[k]):
            p.grad = g.clone()
        a.step()
    worst = [0.0, 0.0, 0.0]
    for k in range(20, 25):
        _sync_from(a_params, a, b_params, b)
        sd = a.state_dict()["state"]
        assert all(float(sd[i]["step"]) == k and sd[i]["step"].device.type == "cpu" for i in range(len(sizes)))
        p0 = [p.detach().clone() for p in a_params]
        m0, v0 = [sd[i]["exp_avg"].clone() for i in range(len(sizes))], [sd[i]["exp_avg_sq"].clone() for i in range(len(sizes))]
        ref64 = cpu_adam(p0, [grads[k]], m0, v0, [k] * len(sizes), [lr_at(k)], torch.float64)
        for opt, params in ((a, a_params), (b, b_params)):
            opt.param_groups[0]["lr"] = lr_at(k)
            for p, g in zip(params, grads[k]):
                p.grad = g.clone()
            opt.step()
            st = [opt.state[p] for p in params]
            assert all(float(s["step"]) == k + 1 for s in st)
            w = assert_one_step(f"{direction} step {k + 1} ({type(opt).__module__})", [p.detach() for p in params], [s["exp_avg"] for s in st],
                                [s["exp_avg_sq"] for s in st], p0, grads[k], ref64, gmax)
            worst = [max(x, y) for x, y in zip(worst, w)]
    assert type(b.state_dict()["param_groups"][0]["lr"]) is float


def test_version_counters_move_and_the_packed_weights_follow():
    from intrinsicnerf_amd import _capi, object_level as ol, optim, packing
    dev = torch.device(DEV)
    e, ch = ol.get_embedder(10, 0)
    ed, chd = ol.get_embedder(4, 0)
    torch.manual_seed(0)
    net = ol.NeRF(D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=chd, use_viewdirs=True).to(dev)
    desc = _capi.net_desc(_capi.VARIANT_OBJECT)
    params = list(net.parameters())
    before = packing.packed_for_module(net, desc, dev).clone()
    versions = [p._version for p in params]
    opt = optim.Adam(params, lr=5e-4)
    gen = torch.Generator().manual_seed(1)
    for p in params:
        p.grad = (torch.randn(p.shape, generator=gen) * 1e-3).to(dev)
    opt.step()
    assert all(p._version > v for p, v in zip(params, versions))
    after = packing.packed_for_module(net, desc, dev).clone()
    assert not torch.equal(before, after)
    packing.invalidate(net)
    fresh = packing.packed_for_module(net, desc, dev)
    assert torch.equal(after, fresh)
    # autograd's saved-tensor check sees the update, as after torch's Adam
    w = params[0]
    y = (w * w).sum()
    for p in params:
        p.grad = torch.zeros_like(p)
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward()


# ---- through the render: the graphed step and the reference-style construction ----
def _object_setup(dev):
    from _cases import case_weights
    from intrinsicnerf_amd import object_level as ol
    fx = load_golden("object_chair_det")
    embed, ch = ol.get_embedder(10, 0); embed_d, ch_d = ol.get_embedder(4, 0)
    mk = lambda: ol.NeRF(D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=ch_d, use_viewdirs=True).to(dev)
    net_c, net_f = mk(), mk()
    sd_c, sd_f = case_weights(fx)
    net_c.load_state_dict(sd_c); net_f.load_state_dict(sd_f)
    return ol, net_c, net_f, ol.NetworkQuery(embed, embed_d), torch.from_numpy(fx["rays"]).to(dev)


OBJECT_WEIGHTS = {"image": 1.0, "chroma": 1.0, "sparsity": 0.01, "far": 0.01, "shading": 1.0, "residual": 1.0, "intensity": 0.1, "cluster": 0.5}


class _AtenLog(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
        self.ops.append(str(func))
        return func(*args, **(kwargs or {}))


def test_graphed_step_with_inerf_adam_equals_its_eager_step(monkeypatch):
    """Five replayed steps with a decaying param_group['lr'] written every iteration: parameters, moments and step counts
    bit-identical to five eager steps of optim.Adam from the same state; graph B holds the library's launch and no ATen one."""
    from intrinsicnerf_amd import graphs, optim
    monkeypatch.setenv("INERF_PRECISION", "f16x3")
    dev = torch.device(DEV)
    results, captured_ops = {}, []
    for mode in ("eager", "graph"):
        ol, net_c, net_f, query, rays = _object_setup(dev)
        n = 12
        batches = [rays[i:i + n] for i in (0, 7, 3, 11, 5)]
        assert all(b.shape[0] == n for b in batches)
        gen = torch.Generator().manual_seed(11)
        targets = [torch.rand(n, 3, generator=gen).to(dev) for _ in batches]
        masks = [(torch.rand(n, 1, generator=gen) > 0.3).float().to(dev) for _ in batches]
        clusters = [torch.rand(n, 3, generator=gen).to(dev) for _ in batches]
        params = list(net_c.parameters()) + list(net_f.parameters())
        opt = optim.Adam(params, lr=5e-4, betas=BETAS)

        def loss_fn(r, t, m, c):
            out = ol.render(1, n, None, chunk=1024 * 32, rays=(r[:, 0:3], r[:, 3:6]), ndc=False, near=2., far=6., use_viewdirs=True,
                            network_fn=net_c, network_query_fn=query, N_samples=64, retraw=True, perturb=0.0, N_importance=64, network_fine=net_f,
                            white_bkgd=True)
            return ol.object_step_loss(out, t, m, OBJECT_WEIGHTS, c)[0]

        losses = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if mode == "graph":
                inner = opt.step

                def logged_step(*a, **k):                           # what optimizer.step() dispatches to ATen while graph B is captured
                    if torch.cuda.is_current_stream_capturing():
                        with _AtenLog() as log:
                            out = inner(*a, **k)
                        captured_ops.append(log.ops)
                        return out
                    return inner(*a, **k)
                opt.step = logged_step
                step = graphs.GraphedTrainStep(loss_fn, (batches[0], targets[0], masks[0], clusters[0]), opt)
            for i, (r, t, m, c) in enumerate(zip(batches, targets, masks, clusters)):
                for group in opt.param_groups:                      # run_nerf.py:1026-1027
                    group["lr"] = lr_at(150000 + i)
                if mode == "eager":
                    opt.zero_grad(set_to_none=True)
                    loss = loss_fn(r, t, m, c)
                    loss.backward()
                    opt.step()
                else:
                    loss = step(r, t, m, c)
                losses.append(float(loss))
        state = [opt.state[p] for p in params]
        results[mode] = (losses, [p.detach().clone() for p in params], [s["exp_avg"].clone() for s in state],
                         [s["exp_avg_sq"].clone() for s in state], [s["step"].detach().cpu().clone() for s in state])
        if mode == "graph":
            assert step.fallbacks == 0
            # checked on the dispatcher: while graph B was captured, optimizer.step() issued no ATen operator at all (torch's Adam issues
            # _foreach_* / _fused_adam_, the multi_tensor_apply launches) - only the library's own launch is in the graph.  What the
            # Optimizer base class brackets every step() with (profiler.record_function) launches nothing.
            assert len(captured_ops) == 1
            aten = [o for o in captured_ops[0] if not o.startswith("profiler.")]
            assert aten == [], aten
            sd = step.optimizer_state_dict()
            assert all(type(g["lr"]) is float and g["capturable"] is False for g in sd["param_groups"])
            assert sd["param_groups"][0]["lr"] == pytest.approx(lr_at(150004), rel=1e-6)
            clones = [p.detach().cpu().clone().requires_grad_(True) for p in params]
            fresh = torch.optim.Adam(clones, lr=1e-3)
            fresh.load_state_dict(sd)
            assert all(float(fresh.state[c]["step"]) == 5.0 and fresh.state[c]["step"].device.type == "cpu" for c in clones)
            assert all(torch.equal(fresh.state[c]["exp_avg"], opt.state[p]["exp_avg"].cpu()) for c, p in zip(clones, params))
            for c in clones:
                c.grad = torch.zeros_like(c)
            fresh.step()
            step.close()
            assert all(type(g["lr"]) is float and not g["capturable"] for g in opt.param_groups)
            for p in params:
                p.grad = torch.zeros_like(p)
            opt.step()                                              # eager use works again (step counts move back to the device)
            assert all(float(opt.state[p]["step"]) == 6.0 for p in params)
    assert np.isfinite(results["graph"][0]).all()
    assert results["eager"][0] == results["graph"][0], (results["eager"][0], results["graph"][0])
    for k in range(1, 5):
        for a, b in zip(results["eager"][k], results["graph"][k]):
            assert torch.equal(a, b), k
    assert all(float(s) == 5.0 for s in results["graph"][4])


def chair_args(**over):
    a = dict(dataset_type="blender", use_viewdirs=True, white_bkgd=True, N_samples=64, N_importance=128, netdepth=8, netwidth=256,
             netdepth_fine=8, netwidth_fine=256, lrate=5e-4, chunk=1024 * 32, netchunk=1024 * 64, perturb=1., i_embed=0, multires=10,
             multires_views=4, raw_noise_std=0., lindisp=False, no_ndc=False)
    a.update(over)
    return types.SimpleNamespace(**a)


def reference_style_create_nerf(args, dev, adam):
    """run_nerf.py:275-356 with this package's symbols imported over the reference's, as tests/test_dropin_gpu.py restates it -
    here with the optimizer line (run_nerf.py:304) and its place in the return value."""
    from intrinsicnerf_amd.object_level import NeRF, get_embedder, run_network
    embed_fn, input_ch = get_embedder(args.multires, args.i_embed)
    embeddirs_fn, input_ch_views = get_embedder(args.multires_views, args.i_embed)
    output_ch = 5 if args.N_importance > 0 else 4
    model = NeRF(D=args.netdepth, W=args.netwidth, input_ch=input_ch, output_ch=output_ch, skips=[4],
                 input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs).to(dev)
    grad_vars = list(model.parameters())
    model_fine = NeRF(D=args.netdepth_fine, W=args.netwidth_fine, input_ch=input_ch, output_ch=output_ch, skips=[4],
                      input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs).to(dev)
    grad_vars += list(model_fine.parameters())
    network_query_fn = lambda inputs, viewdirs, network_fn: run_network(inputs, viewdirs, network_fn,      # noqa: E731
                                                                        embed_fn=embed_fn,
                                                                        embeddirs_fn=embeddirs_fn,
                                                                        netchunk=args.netchunk)
    optimizer = adam(params=grad_vars, lr=args.lrate, betas=(0.9, 0.999))
    train = {"network_query_fn": network_query_fn, "perturb": args.perturb, "N_importance": args.N_importance,
             "network_fine": model_fine, "N_samples": args.N_samples, "network_fn": model, "use_viewdirs": args.use_viewdirs,
             "white_bkgd": args.white_bkgd, "raw_noise_std": args.raw_noise_std, "ndc": False, "lindisp": args.lindisp}
    return train, grad_vars, optimizer


def test_three_training_steps_in_place_of_torch_adam(monkeypatch):
    from intrinsicnerf_amd import object_level as ol, optim
    monkeypatch.setenv("INERF_PRECISION", "f16x3")
    dev = torch.device(DEV)
    fx = load_golden("object_chair_det")
    from _cases import case_weights
    sd_c, sd_f = case_weights(fx)
    rays = torch.from_numpy(fx["rays"]).to(dev)
    n = rays.shape[0]
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(4)).to(dev)
    args = chair_args()
    ends = {}
    for name, adam in (("inerf", optim.Adam), ("torch", torch.optim.Adam)):
        train_kw, grad_vars, optimizer = reference_style_create_nerf(args, dev, adam)
        train_kw["network_fn"].load_state_dict(sd_c); train_kw["network_fine"].load_state_dict(sd_f)
        torch.manual_seed(1234)
        for i in range(3):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out = ol.render(1, n, None, chunk=args.chunk, rays=(rays[:, 0:3], rays[:, 3:6]), verbose=False, retraw=True, near=2., far=6., **train_kw)
            optimizer.zero_grad()
            loss = ((out[0] - target) ** 2).mean() + ((out[6]["rgb0"] - target) ** 2).mean()           # run_nerf.py:976,1006
            loss.backward()
            optimizer.step()
            for group in optimizer.param_groups:
                group["lr"] = lr_at(i + 1)
        ends[name] = ([p.detach().cpu().double() for p in grad_vars], float(loss))
    worst = 0.0
    for i, (a, b) in enumerate(zip(*[ends[k][0] for k in ("inerf", "torch")])):
        err, bound = float((a - b).abs().max()), 1e-4 * max(float(b.abs().max()), 1e-3)
        worst = max(worst, err / bound)
    print(f"\nthree training steps, optim.Adam against torch.optim.Adam: worst per-tensor distance {worst:.3e} of the 1e-4 bound; "
          f"losses {ends['inerf'][1]:.6f} / {ends['torch'][1]:.6f}")
    assert worst <= 1.0, worst
