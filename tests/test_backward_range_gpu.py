"""The network backward (inerf_mlp_backward: the input-gradient chain of csrc/mlp_bwd.hip, the weight-gradient products of
csrc/mlp_wgrad.hip) over the RANGE of cotangents a trained scene gives it: d loss / d raw from 2^-140 (fp32 denormals: the
build has no flush-to-zero) to 2^100, several magnitudes inside one 64-point tile, channels and points that are exactly zero,
the compositing backward's own output on opaque rays - and the backward's f16 range guard from both sides.

Judge throughout: fp64 torch autograd through the module's own forward on the fp32 sample positions
(test_backward_golden._torch_reference_grads), fed the same fp32 cotangent; per parameter tensor
|got - want|_2 <= 2e-4 |want|_2 with NO absolute term (a tensor whose reference gradient is exactly zero must come out exactly
zero).  ReLU ties (test_backward_golden._relu_tie_points, from the fp64 network alone) get no cotangent; below 1 % of the points.

Every case prints its worst relative error; these are records, not thresholds."""
import copy

import pytest
import torch

import _chain
import _cotangents as ct
import oracle
from test_backward_golden import _torch_reference_grads

pytestmark = pytest.mark.gpu

RTOL = 2e-4                       # the project's bound on a parameter gradient (test_backward_golden._check_network_backward)
K_F16_SAFE = 6.0e4                # csrc/mlp_f16_dev.h kF16Safe, on the stored value: kActScale (8) x the normalised gradient
NETWORKS = {"object": ("object", 0, False), "ssr28": ("ssr", 28, False), "ssr5e": ("ssr", 5, True)}
SMALL = (37, 5)                   # 185 points: two tiles and a ragged third
BIG = {"object": (1024, 192), "ssr28": (512, 192), "ssr5e": (512, 192)}       # >= 3 tiles per workgroup of the chain
# (network, chain form, training forward): both chain forms; for the object-level network both training forwards
FORMS = [("object", "dual", None), ("object", "single", None), ("object", "dual", "t128"), ("object", "single", "t128"),
         ("ssr28", "dual", None), ("ssr28", "single", None), ("ssr5e", "dual", None), ("ssr5e", "single", None)]
FORM_IDS = [f"{n}-{c}-{f or 'fwd64'}" for n, c, f in FORMS]

# The sweep's k at which got(k) * 2^-k must equal got(0) bit for bit, element by element.  Not -120: below a largest gradient of
# 2^-112 the weight-gradient products' operand scale stops at 2^126 (a larger one has no finite reciprocal), the operands then
# sit lower in their f16 hi / lo pair than at k = 0 and round differently.
EXACT_LOG2 = (-100, -60, -20, 20, 60, 100)
# At k = -100 underflow is within reach although the fp64 result passes _cotangents.scaling_stays_normal: a parameter gradient is
# the fp32 sum, in a fixed order, of up to R = inerf_wgrad_grid(points) per-workgroup partial tiles stored at their true scale,
# and with the gradients' norms near 2^-95 a partial (or an element itself) 2^-30 of that scale - ordinary for sums of 1e5
# cancelling products - lies below 2^-126 and is rounded to the denormal grid, 2^-149.  Each such rounding moves the sum by at
# most 2^-150, R of them by R 2^-150, which can also tip the element's final rounding: so there, and only there, an element may
# differ by one spacing of its own value plus R 2^-149 (in units of k = 0: times 2^100).  Every other element, and every element
# at the other k, must be identical.
UNDERFLOW_LOG2 = (-100,)


class _Case:
    """One network on one batch: module, fp64 copy, rays / depths (the recipe of _check_network_backward), the tie mask."""

    def __init__(self, key, n, s):
        from intrinsicnerf_amd import _capi, object_level as ol, ssr
        variant, c, endpoint = NETWORKS[key]
        dev = torch.device("cuda:0")
        self.key, self.n, self.s, self.endpoint, self.dev, self.classes = key, n, s, endpoint, dev, c
        g = torch.Generator().manual_seed(7 + n)
        sd = oracle.lcg_state_dict(variant, c, seed=21, sigma_gain_log2=3, freq_decay=True)
        if variant == "object":
            self.embed, ch = ol.get_embedder(10, 0); self.embed_d, ch_d = ol.get_embedder(4, 0)
            net = ol.NeRF(D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=ch_d, use_viewdirs=True).to(dev)
        else:
            self.embed, ch = ssr.get_embedder(10, 0, scalar_factor=10); self.embed_d, ch_d = ssr.get_embedder(4, 0, scalar_factor=1)
            net = ssr.Semantic_NeRF(c > 0, c, D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=ch_d, use_viewdirs=True).to(dev)
        net.load_state_dict(sd)
        self.net = net
        o = torch.rand(n, 3, generator=g) * 2 - 1
        d = torch.randn(n, 3, generator=g)
        self.rays = torch.cat([o, d, torch.zeros(n, 2), d / d.norm(dim=-1, keepdim=True)], -1).to(dev)
        self.z = torch.sort(torch.rand(n, s, generator=g) * 3 + 0.5, -1)[0].to(dev)
        self.channels = 11 + c + (128 if endpoint else 0)
        self.p = n * s
        desc = net.fused_desc()
        self.desc = _capi.NetDesc(desc.variant, desc.n_classes, desc.l_xyz, desc.l_dir, self.embed.scalar_factor, _capi.PREC_F16X3)
        ties = []
        self.reference(torch.zeros(n, s, self.channels), ties_out=ties)
        self.live = ~ties[0].reshape(-1).cpu()                  # from the fp64 network alone
        assert 100 * int((~self.live).sum()) < self.p, int((~self.live).sum())          # below 1 % of the points
        self.refs = {}

    def reference(self, cot, ties_out=None, net=None):
        """fp64 autograd of the fp32 cotangent ``cot`` ([n, s, channels] or [p, channels], CPU or device): name -> fp64 CPU."""
        net64 = copy.deepcopy(self.net if net is None else net).double()
        c = cot.to(self.dev).double().reshape(self.n, self.s, self.channels)
        _, grads = _torch_reference_grads(net64, self.embed, self.embed_d, self.rays.double(), self.z.double(), c, self.endpoint, ties_out=ties_out)
        return {k: v.detach().cpu() for k, v in grads.items()}

    def forward(self, net=None):
        """The fused training forward -> (raw [p, channels], save, act_max, packed transposed weights); its status word is 0."""
        from intrinsicnerf_amd import kernels, packing
        named = {k: v.detach() for k, v in (self.net if net is None else net).named_parameters()}
        status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        act_max = torch.zeros(1, dtype=torch.float32, device=self.dev)
        raw, save = kernels.encode_mlp_train(self.desc, packing.device_packer(self.desc, False, self.dev)(named), self.rays, self.z,
                                             self.endpoint, status, act_max)
        pb = packing.device_packer(self.desc, True, self.dev)(named)
        assert int(status.item()) == 0, "the training forward left the f16 range"
        return raw.view(self.p, self.channels), save, act_max, pb

    def backward(self, fwd, cot):
        """inerf_mlp_backward on the cotangent ``cot`` (fp32, CPU: copied bit for bit) -> (name -> fp32 gradient, status word)."""
        from intrinsicnerf_amd import kernels
        raw, save, act_max, pb = fwd
        d_raw = cot.reshape(self.p, self.channels).to(self.dev)
        status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        flat = kernels.mlp_backward(self.desc, pb, raw, d_raw, save, act_max, self.endpoint, status)
        return kernels.param_views(self.desc, flat), int(status.item())

    def chain(self, fwd, cot):
        """inerf_mlp_backward_inputs alone -> the gradient buffer dz."""
        from intrinsicnerf_amd import kernels
        raw, save, act_max, pb = fwd
        return kernels.mlp_backward_inputs(self.desc, pb, raw, cot.reshape(self.p, self.channels).to(self.dev), save, endpoint=self.endpoint)


@pytest.fixture(scope="module")
def cases():
    """(network, shape) -> _Case, built once per module run and dropped with it (device tensors and fp64 references)."""
    store = {}

    def get(key, shape):
        if (key, shape) not in store:
            store[(key, shape)] = _Case(key, *shape)
        return store[(key, shape)]

    yield get
    store.clear()
    torch.cuda.empty_cache()


def _select(monkeypatch, chain, fwd):
    monkeypatch.setenv("INERF_DGRAD_KERNEL", chain)          # two workgroups per CU (default) | the eight-wave chain
    if fwd:
        monkeypatch.setenv("INERF_TRAIN_FWD", fwd)
    else:
        monkeypatch.delenv("INERF_TRAIN_FWD", raising=False)


def _judge(got, want, what):
    """Non-finite tensors and tensors beyond 2e-4 of their reference's norm (no absolute term); prints the worst ratio."""
    bad, worst = {}, (0.0, "")
    for name, w in want.items():
        gt = got[name].detach().double().cpu()
        if not bool(torch.isfinite(gt).all()):
            bad[name] = f"{int((~torch.isfinite(gt)).sum())} non-finite of {gt.numel()}"
            continue
        e, wn = float((gt - w.double()).norm()), float(w.double().norm())
        if not e <= RTOL * wn:
            bad[name] = f"{e:.3e} vs norm {wn:.3e}"
        if wn > 0 and e / wn > worst[0]:
            worst = (e / wn, name)
    print(f"RANGE {what}: worst {worst[0]:.2e} of a tensor's norm ({worst[1]}){'  BAD: ' + str(bad) if bad else ''}")
    return bad


def _masked(case, c0):
    """c0 with the ReLU ties' rows zeroed."""
    return c0 * case.live[:, None].to(c0.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# 1. uniform scale sweep
# ---------------------------------------------------------------------------------------------------------------------
def _sweep_reference(case):
    """(c0 with the ties masked, fp64 gradients of c0): one autograd pass serves the whole sweep - see the test below."""
    c0 = _masked(case, ct.base_cotangent(case.p, case.channels, seed=100 + case.n))
    if "sweep" not in case.refs:
        case.refs["sweep"] = case.reference(ct.scaled(c0, 0))
    return c0, case.refs["sweep"]


@pytest.mark.parametrize("key", list(NETWORKS))
def test_fp64_reference_scales_exactly(key, cases):
    """The fp64 gradient of c0 * 2^k is the fp64 gradient of c0 times 2^k (fp64 has 900 binades of room): an autograd pass on
    the scaled cotangent agrees with the scaled pass to fp64 rounding, towards both ends of the sweep."""
    case = cases(key, SMALL)
    c0, want0 = _sweep_reference(case)
    for k in (-100, 100):
        cot = ct.scaled(c0, k)
        assert not bool(ct.is_denormal(cot).any())
        direct = case.reference(cot)
        for name, w in want0.items():
            assert float((direct[name] * 2.0 ** -k - w).norm()) <= 1e-12 * float(w.norm()), (k, name)


@pytest.mark.parametrize("size", ["small", "big"])
@pytest.mark.parametrize("key,chain,fwd", FORMS, ids=FORM_IDS)
def test_uniform_scale_sweep(key, chain, fwd, size, monkeypatch, cases):
    """c0 * 2^k, k = -120 .. 100 (every channel live): finite, status 0, each within 2e-4 of fp64 autograd per tensor (the fp64
    gradient of c0 * 2^k is that of c0 times 2^k: test_fp64_reference_scales_exactly), and got(k) * 2^-k == got(0) bit for bit
    for EXACT_LOG2, element by element (UNDERFLOW_LOG2: what may differ at k = -100, and by how much)."""
    from intrinsicnerf_amd import _capi
    case = cases(key, SMALL if size == "small" else BIG[key])
    _select(monkeypatch, chain, fwd)
    c0, want0 = _sweep_reference(case)
    assert all(float(w.norm()) > 0 for w in want0.values())
    for k in EXACT_LOG2:             # the precondition of the bit-for-bit check, from the fp64 reference: it must hold, not lapse
        assert ct.scaling_stays_normal(want0, k), f"k = {k}: the fp64 result leaves fp32's normal range"
    fwd_out = case.forward()
    rows = int(_capi.lib().inerf_wgrad_grid(case.p))          # partial tiles per gradient element, at most
    got, bad = {}, {}
    for k in ct.SWEEP_LOG2:
        grads, status = case.backward(fwd_out, ct.scaled(c0, k))
        got[k] = {name: t.detach().double().cpu() for name, t in grads.items()}
        if status != 0:
            bad[(k, "status")] = status
        for name, why in _judge(got[k], {name: w * 2.0 ** k for name, w in want0.items()}, f"sweep {key} {chain} {fwd} {size} k={k}").items():
            bad[(k, name)] = why
    exact, inexact = [], {}
    for k in ct.SWEEP_LOG2:
        if k == 0:
            continue
        differ, left_out = {}, 0
        for name in want0:
            a, b = got[k][name] * 2.0 ** -k, got[0][name]
            d = a != b
            if k in UNDERFLOW_LOG2:          # explained by partials on the denormal grid: see UNDERFLOW_LOG2
                spacing = torch.nextafter(b.float().abs(), torch.full((), float("inf"))).double() - b.abs()
                explained = d & ((a - b).abs() <= spacing + rows * 2.0 ** -149 * 2.0 ** -k)
                left_out += int(explained.sum())
                d = d & ~explained
            if bool(d.any()):
                differ[name] = int(d.sum())
        if differ and k in EXACT_LOG2:
            inexact[k] = differ
        elif differ:
            print(f"RANGE sweep {key} {chain} {fwd} {size}: k={k} not bit-exact under scaling in {differ}")
        else:
            exact.append(k)
        if left_out:
            print(f"RANGE sweep {key} {chain} {fwd} {size}: k={k}: {left_out} of {sum(w.numel() for w in want0.values())} elements differ by one "
                  f"spacing, explained by partial sums on the denormal grid")
    print(f"RANGE sweep {key} {chain} {fwd} {size}: bit-exact under scaling at k = {exact}")
    assert not bad, bad
    assert not inexact, inexact


# ---------------------------------------------------------------------------------------------------------------------
# 2. mixed scales inside one tile
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,chain,fwd", FORMS, ids=FORM_IDS)
def test_mixed_scales_inside_one_tile(key, chain, fwd, monkeypatch, cases):
    """Eight groups by point index mod 8 (2^-140, 2^-130, 2^-120, 2^-40, 1, 2^30, zero, sigma only at 2^-10) at the small shape:
    each accurate group alone against fp64 at 2e-4 of ITS run's norms; the denormal groups alone finite; the zero batch
    exactly zero; all together finite, status 0 and within 2e-4 of the whole cotangent's fp64 result - one point whose
    normaliser has no finite reciprocal would turn every sum into NaN; the normalisers and fragments themselves."""
    from intrinsicnerf_amd import kernels
    case = cases(key, SMALL)
    _select(monkeypatch, chain, fwd)
    groups = ct.group_index(case.p, case.live)
    assert ct.tiles_hold_every_group(groups)
    c0 = ct.base_cotangent(case.p, case.channels, seed=200 + case.n)
    fwd_out = case.forward()
    raw = fwd_out[0]
    bad = {}

    def ref(tag, cot):
        if tag not in case.refs:
            case.refs[tag] = case.reference(cot)
        return case.refs[tag]

    for g in ct.ACCURATE_GROUPS:                      # isolated runs
        cot = ct.grouped_cotangent(c0, groups, only=g)
        grads, status = case.backward(fwd_out, cot)
        if status != 0:
            bad[(g, "status")] = status
        for name, why in _judge(grads, ref(("group", g), cot), f"group {key} {chain} {fwd} [{ct.GROUP_NAMES[g]}] alone").items():
            bad[(ct.GROUP_NAMES[g], name)] = why
    for g in ct.DENORMAL_GROUPS:                      # finite; no accuracy bound: the fp32 result is itself made of denormals
        grads, status = case.backward(fwd_out, ct.grouped_cotangent(c0, groups, only=g))
        for name, t in grads.items():
            if not bool(torch.isfinite(t).all()):
                bad[(ct.GROUP_NAMES[g], name)] = "non-finite"
        if status != 0:
            bad[(ct.GROUP_NAMES[g], "status")] = status
    # the zero batch: exactly 0.0 everywhere, normalisers 1.0
    zero = torch.zeros(case.p, case.channels)
    grads, status = case.backward(fwd_out, zero)
    assert status == 0
    for name, t in grads.items():
        if float(t.abs().max()) != 0.0:
            bad[("zero", name)] = float(t.abs().max())
    padded = (case.p + 63) // 64 * 64
    norm = kernels.save_slot_views(case.desc, case.chain(fwd_out, zero), case.p, gradient=True)[kernels.SAVE_ENC]
    assert norm.shape == (padded,) and bool((norm == 1.0).all()), "a point without gradient has the normaliser 1"
    # all groups together
    cot = ct.grouped_cotangent(c0, groups)
    grads, status = case.backward(fwd_out, cot)
    if status != 0:
        bad[("all", "status")] = status
    for name, why in _judge(grads, ref("all groups", cot), f"group {key} {chain} {fwd} all together").items():
        bad[("all", name)] = why
    # the normalisers: finite powers of two, not below the point's largest head gradient (by head_gradients' formula in fp64,
    # rounded to fp32, less one ulp for the kernel's own fp32 evaluation), 1 where there is no gradient; every f16 half of the
    # fragments finite
    dz = case.chain(fwd_out, cot)
    s = kernels.save_slot_views(case.desc, dz, case.p, gradient=True)[kernels.SAVE_ENC].cpu()
    m = ct.head_gradient_max(raw.cpu(), cot, case.classes, 128 if case.endpoint else 0)
    assert bool(torch.isfinite(s).all()) and bool((s > 0).all())
    assert bool((torch.frexp(s)[0] == 0.5).all()), "normalisers are powers of two"
    assert bool((s[:case.p] >= torch.nextafter(m.float(), torch.zeros(()))).all()), "a normaliser below its point's largest head gradient"
    assert bool((1.0 / s).isfinite().all()), "a normaliser without a finite reciprocal"
    assert bool((s[:case.p][m == 0] == 1.0).all()) and bool((s[case.p:] == 1.0).all())
    for g in ct.DENORMAL_GROUPS:
        assert float(m[groups == g].max()) < ct.F32_MIN_NORMAL
    assert float(m[groups == 1].min()) < 2.0 ** -128
    words = _chain.chain_words(case.desc, dz, case.p)
    for name, slot, first, n_words, width in _chain.chain_layout(case.desc, case.p):
        if name in ("dpre", "norm"):
            assert bool(torch.isfinite(words[first:first + n_words].view(torch.float32)).all()), name
        else:
            halves = words[first:first + n_words].view(torch.float16)
            if not bool(torch.isfinite(halves).all()):
                bad[("fragments", name)] = f"{int((~torch.isfinite(halves)).sum())} non-finite f16 halves"
    assert not bad, bad


@pytest.mark.parametrize("chain", ["dual", "single"])
@pytest.mark.parametrize("key", list(NETWORKS))
def test_normaliser_at_the_top_of_fp32(key, chain, monkeypatch, cases):
    """Two points with 2^127 on the sigma channel, nothing elsewhere: the power of two above that does not exist in fp32, so
    the normaliser stops at 2^126 (its reciprocal 2^-126 is still normal) and the normalised gradient is 2 instead of <= 1.
    Normalisers as stated, fragments and gradients finite, gradients within 2e-4 of fp64."""
    from intrinsicnerf_amd import kernels
    case = cases(key, SMALL)
    _select(monkeypatch, chain, None)
    points = [int(q) for q in case.live.nonzero().flatten()[[3, 70]]]
    cot = torch.zeros(case.p, case.channels)
    cot[points, ct.SIGMA_CHANNEL] = torch.tensor([2.0 ** 127, -(2.0 ** 127)])
    fwd_out = case.forward()
    dz = case.chain(fwd_out, cot)
    s = kernels.save_slot_views(case.desc, dz, case.p, gradient=True)[kernels.SAVE_ENC].cpu()
    assert s[points].tolist() == [2.0 ** 126] * 2 and bool((s[[q for q in range(s.numel()) if q not in points]] == 1.0).all())
    words = _chain.chain_words(case.desc, dz, case.p)
    for name, slot, first, n_words, width in _chain.chain_layout(case.desc, case.p):
        view = torch.float32 if name in ("dpre", "norm") else torch.float16
        assert bool(torch.isfinite(words[first:first + n_words].view(view)).all()), name
    grads, status = case.backward(fwd_out, cot)
    want = case.reference(cot)
    assert all(bool(torch.isfinite(w.float()).all()) for w in want.values()), "the fp64 result fits fp32"
    bad = _judge(grads, want, f"top of fp32 {key} {chain}")
    assert status == 0 and not bad, (status, bad)


# ---------------------------------------------------------------------------------------------------------------------
# 3. cotangents from the compositing backward on opaque rays
# ---------------------------------------------------------------------------------------------------------------------
COMPOSITE_FORMS = [("object", "dual", None), ("object", "single", None), ("object", "dual", "t128"),
                   ("ssr28", "dual", None), ("ssr28", "single", None), ("ssr5e", "dual", None), ("ssr5e", "single", None)]


@pytest.mark.parametrize("key,chain,fwd", COMPOSITE_FORMS, ids=[f"{n}-{c}-{f or 'fwd64'}" for n, c, f in COMPOSITE_FORMS])
def test_cotangent_of_the_composite_backward_on_opaque_rays(key, chain, fwd, monkeypatch, cases):
    """d_raw from k_composite_bwd (kernels.composite(...).backward()) on 1024 rays x 192 samples whose density makes
    sigma * delta = 1 per sample from sample 20 on, loss = mean((rgb - target)^2): the transmittance runs through fp32's
    denormal window into exact zeros.  The fp64 compositing confirms that first: of the entries in the channels the loss reaches
    (rgb and sigma; the SSR logits and the endpoint feature stay exactly zero beside them, which is the point of running the SSR
    networks here) >= 1 % are denormal-sized and >= 10 % zeros - for the object-level network also counted over every entry.
    Then the network gradients are finite, status 0 and within 2e-4 per tensor of fp64 autograd fed the SAME fp32 d_raw."""
    from intrinsicnerf_amd import kernels
    case = cases(key, (1024, 192))
    _select(monkeypatch, chain, fwd)
    feat = 128 if case.endpoint else 0
    fwd_out = case.forward()
    raw = fwd_out[0].view(case.n, case.s, case.channels)
    rays_d = case.rays[:, 3:6].contiguous()
    comp = raw.detach().clone()
    comp[..., 3] = ct.opaque_sigma(case.z.cpu(), rays_d.cpu()).to(case.dev)
    target = torch.rand(case.n, 3, generator=torch.Generator().manual_seed(9)).to(case.dev)
    # the fp64 compositing on the CPU: the case is what it claims to be
    r64 = comp.cpu().double().requires_grad_(True)
    cfg = oracle.RenderConfig(variant="ssr" if case.classes else "object", n_classes=case.classes)
    out64 = oracle.composite(r64, case.z.cpu().double(), rays_d.cpu().double(), cfg, feat=case.endpoint)
    ((out64["rgb"] - target.cpu().double()) ** 2).mean().backward()
    reached = (r64.grad != 0).reshape(-1, case.channels).any(0)
    assert reached.tolist() == [True] * 4 + [False] * (case.channels - 4), "an rgb loss reaches rgb and sigma only"
    denormal, zero = ct.magnitude_classes(r64.grad[..., reached])
    assert denormal >= 0.01 and zero >= 0.10, (denormal, zero)
    if key == "object":
        assert ct.magnitude_classes(r64.grad)[0] >= 0.01
    # the project's own compositing backward
    leaf = comp.clone().requires_grad_(True)
    out = kernels.composite(leaf, case.z, rays_d, None, False, case.classes, feat)
    ((out["rgb"] - target) ** 2).mean().backward()
    d_raw = (leaf.grad * case.live.view(case.n, case.s, 1).to(case.dev)).cpu()          # (ReLU ties: no cotangent)
    assert bool(torch.isfinite(d_raw).all())
    assert float(d_raw[..., ~reached].abs().max()) == 0.0
    got_denormal = float(ct.is_denormal(d_raw[..., reached]).float().mean())
    print(f"RANGE composite {key}: of the reached channels, fp64 d_raw {denormal:.1%} denormal-sized, {zero:.1%} zeros; the kernel's "
          f"d_raw {got_denormal:.1%} denormal, {float((d_raw[..., reached] == 0).float().mean()):.1%} zero, largest {float(d_raw.abs().max()):.2e}")
    assert got_denormal >= 0.01, "the compositing kernel's cotangent holds denormals"
    tag = "composite"
    if tag not in case.refs:
        case.refs[tag] = (d_raw, case.reference(d_raw))
    assert torch.equal(case.refs[tag][0], d_raw)
    grads, status = case.backward(fwd_out, d_raw)
    bad = _judge(grads, case.refs[tag][1], f"composite {key} {chain} {fwd}")
    assert status == 0 and not bad, (status, bad)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the backward's f16 range guard, both sides
# ---------------------------------------------------------------------------------------------------------------------
def _predicted_chain_max(case, net, cot):
    """max over every layer and point of 8 x |pre-activation gradient| / s_point - what the chain stores as f16 - and the
    largest forward activation, from the fp64 network (hooks on every nn.Linear)."""
    net64 = copy.deepcopy(net).double()
    m = cot[:, ct.SIGMA_CHANNEL].abs().double()                # sigma only: the point's largest head gradient is |g3|
    frac, e = torch.frexp(m)                                   # m = frac 2^e, frac in [0.5, 1): s = 2^e (a power of two m gets s = 2 m)
    s = torch.where(m > 0, torch.ldexp(torch.ones_like(m), e), torch.ones_like(m)).to(case.dev)
    peak = {"dz": 0.0, "act": 0.0}

    def fwd(mod, inputs, out):          # every hidden layer's pre-activation (128 or 256 wide): its size, and its gradient's
        if out.dim() == 2 and out.shape[0] == case.p and out.shape[1] >= 128:
            peak["act"] = max(peak["act"], float(out.detach().abs().max()))
            if out.requires_grad:
                out.register_hook(lambda grad: peak.__setitem__("dz", max(peak["dz"], float((grad.abs() / s[:, None]).max()) * 8.0)))

    hooks = [m.register_forward_hook(fwd) for m in net64.modules() if isinstance(m, torch.nn.Linear)]
    _torch_reference_grads(net64, case.embed, case.embed_d, case.rays.double(), case.z.double(),
                           cot.to(case.dev).double().reshape(case.n, case.s, case.channels), case.endpoint)
    for h in hooks:
        h.remove()
    return peak["dz"], peak["act"]


@pytest.mark.parametrize("chain", ["dual", "single"])
@pytest.mark.parametrize("key", ["object", "ssr28", "ssr5e"])
def test_backward_range_guard_from_both_sides(key, chain, monkeypatch, cases):
    """alpha_linear.weight times a factor, cotangent 1 on the sigma channel only: sigma leaves the network as fp32 and is never
    split, so the forward stays in range, while d h7 = W_alpha^T d sigma grows with the factor.  From the fp64 network: a factor
    that puts the largest stored gradient (8 x the normalised value) at 0.5 x kF16Safe and one at 2 x.  Below: status 0 and 2e-4
    against fp64.  Above: inerf_mlp_backward sets INERF_STATUS_F16_RANGE, and a training step through kernels.mlp_train raises
    FloatingPointError without writing any .grad."""
    from intrinsicnerf_amd import _capi, kernels
    case = cases(key, SMALL)
    _select(monkeypatch, chain, None)
    cot = torch.zeros(case.p, case.channels)
    cot[:, ct.SIGMA_CHANNEL] = case.live.float()
    base, _ = _predicted_chain_max(case, case.net, cot)
    assert 0 < base < 0.25 * K_F16_SAFE
    nets = {}
    for side, aim in (("below", 0.5), ("above", 2.0)):
        net = copy.deepcopy(case.net)
        with torch.no_grad():
            net.alpha_linear.weight.mul_(aim * K_F16_SAFE / base)
        dz, act = _predicted_chain_max(case, net, cot)
        print(f"RANGE guard {key} {side}: factor {aim * K_F16_SAFE / base:.4g}, predicted largest stored gradient {dz:.4g} "
              f"({dz / K_F16_SAFE:.2f} x kF16Safe), largest hidden activation {act:.3g}")
        assert 0.8 * aim <= dz / K_F16_SAFE <= 1.2 * aim and act < 7.5e3
        nets[side] = net
    # below: unflagged and accurate
    fwd_out = case.forward(nets["below"])
    grads, status = case.backward(fwd_out, cot)
    bad = _judge(grads, case.reference(cot, net=nets["below"]), f"guard {key} {chain} below")
    assert status == 0 and not bad, (status, bad)
    # above: the C call reports it ...
    fwd_out = case.forward(nets["above"])                   # (asserts that the forward's own word stays 0)
    grads, status = case.backward(fwd_out, cot)
    assert status & _capi.STATUS_F16_RANGE, status
    # ... and the training step raises, leaving no gradient behind
    net = nets["above"]
    net.zero_grad()
    desc = net.fused_desc()
    desc.xyz_div = case.embed.scalar_factor
    raw = kernels.mlp_train(desc, net, case.rays, case.z, case.endpoint)
    with pytest.raises(FloatingPointError, match="training backward"):
        (raw * cot.to(case.dev).view(case.n, case.s, case.channels)).sum().backward()
    for name, p in net.named_parameters():
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), name
