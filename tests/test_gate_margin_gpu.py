"""GPU: the gate probe's cull margin per packed network (include/inerf.h INERF_FLAG_GATE_PROBE).

With a margin state the probe lists its candidates' (s, S), the listed trunk measures r = |s - sigma| / S on every one of them, and
the NEXT launch on that state culls with kappa = max(2^-9, 8 r_max) instead of 2^-6 - once the state has seen INERF_PROBE_MIN_OBS
points (1 here unless a test says otherwise).  Without a state the launches are the constant's.  Equality is on the bits.

Shapes: 37 rays x 64 (one sub-range), 37 x 192 in sub-ranges of 4 rays, 171 x 193 in sub-ranges of 40 rays - no point count a
multiple of the 128-point tile, several sub-ranges per launch, the last one short.  The ungated reference of a (network, shape) is
computed once and shared."""
import pytest
import torch

import _gate_probe as gp

pytestmark = pytest.mark.gpu

COLOURS = [0, 1, 2, 4, 5, 6, 7, 8, 9, 10]
S_C, S_I = 64, 128
FLOOR = 2.0 ** -9
SHAPES = {"37x64": (37, 64, None, "sd_c"), "37x192": (37, 192, 4, "sd_f"), "171x193": (171, 193, 40, "sd_f")}      # rays, samples, rays per sub-range, network


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("INERF_PRECISION", "INERF_F16_KERNEL", "INERF_GATE", "INERF_PROBE", "INERF_PROBE_WG", "INERF_GATE_LOG", "INERF_ENC_CACHE",
              "INERF_GATE_BYTES", "INERF_PROBE_ADAPT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("INERF_PROBE_MIN_OBS", "1")


_cache = {}


def _setup():
    if not _cache:
        from intrinsicnerf_amd import _capi
        dev = torch.device("cuda:0")
        sd_c, rays = gp.network("bench_coarse")
        sd_f, _ = gp.network("bench_fine")
        _cache.update(dev=dev, rays=rays.to(dev), sd_c=sd_c, sd_f=sd_f, desc=_capi.net_desc(_capi.VARIANT_OBJECT, precision=_capi.PREC_F16X3),
                      cases={})
    return _cache


def _pack(c, sd):
    from intrinsicnerf_amd import packing
    return packing.pack_state_dict(c["desc"], sd).to(c["dev"])


def _frame_rays(c, n_rays):
    return c["rays"][:: c["rays"].shape[0] // n_rays][:n_rays].contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _new_state(c, r_max=0.0, observed=0):
    """A margin state as the front-end makes it (eight zeroed int32 words), optionally seeded: float r_max at word 0, uint64 observed
    at byte 8."""
    st = torch.zeros(8, dtype=torch.int32, device=c["dev"])
    st.view(torch.float32)[0] = r_max
    st.view(torch.int64)[1] = observed
    return st


def _probed(c, case, state=None):
    """Gate with probe on ``case`` -> (raw rows [n, 11], (s, S) [n, 2])."""
    from intrinsicnerf_amd import kernels
    po = torch.full((case["z"].numel(), 2), float("nan"), device=c["dev"])
    raw = kernels.encode_mlp(c["desc"], case["packed"], case["rays"], case["z"], gate_colour=True, gate_probe=True, probe_out=po, gate_state=state)
    torch.cuda.synchronize()
    return raw.reshape(-1, 11), po


def _case(c, key, monkeypatch, sd=None, rays=None, z=None, rays_per_sub=None):
    """packed weights, rays, depths, and - computed once per key - the ungated rows, the gate's rows, the constant's rows and (s, S).
    Sets INERF_GATE_BYTES for the case's sub-ranges."""
    if key in SHAPES:
        n_rays, n_samples, rays_per_sub, net = SHAPES[key]
    if key not in c["cases"]:
        from intrinsicnerf_amd import kernels
        if key in SHAPES:
            sd, rays = c[net], _frame_rays(c, n_rays)
            z = gp.sample_depths(rays.cpu(), n_samples, seed=23).to(c["dev"])
        case = dict(packed=_pack(c, sd), rays=rays, z=z, rays_per_sub=rays_per_sub)
        if rays_per_sub is not None:
            monkeypatch.setenv("INERF_GATE_BYTES", str(rays_per_sub * z.shape[1] * 1028))
        case["plain"] = kernels.encode_mlp(c["desc"], case["packed"], rays, z).reshape(-1, 11)
        case["gated"] = kernels.encode_mlp(c["desc"], case["packed"], rays, z, gate_colour=True).reshape(-1, 11)
        case["constant"], case["po"] = _probed(c, case)
        c["cases"][key] = case
    case = c["cases"][key]
    if case["rays_per_sub"] is not None:
        monkeypatch.setenv("INERF_GATE_BYTES", str(case["rays_per_sub"] * case["z"].shape[1] * 1028))
    return case


def _candidates(po, kappa):
    return ~(po[:, 0] < -kappa * po[:, 1])


def _r_fp32(case, cand):
    """(max of |s - sigma| / S in fp32 over the finite candidates with S > 0 - correctly rounded operations, on the CPU -, their number)"""
    s, big_s, sigma = case["po"][:, 0].cpu(), case["po"][:, 1].cpu(), case["plain"][:, 3].cpu()
    e = (s - sigma).abs() / big_s
    ok = cand.cpu() & torch.isfinite(e) & (big_s > 0)
    return (float(e[ok].max()) if bool(ok.any()) else 0.0), int(ok.sum())


def _assert_rows(case, probed, po, kappa):
    """The issue's statements about a launch that culled with ``kappa`` (a float32 value): every point of positive (or NaN) density has
    the ungated row, every other row zero colours and channel 3 <= 0, a culled row's channel 3 is s - and a candidate's row is the
    gate's, so the candidates are exactly !(s < -kappa S), point by point in every sub-range.  Returns the candidate mask."""
    plain, gated = case["plain"], case["gated"]
    assert torch.equal(_bits(po), _bits(case["po"]))                    # (s, S) do not depend on the margin
    live = ~(plain[:, 3] <= 0)
    assert torch.equal(_bits(probed[live]), _bits(plain[live]))
    assert int((probed[~live][:, COLOURS] != 0).sum()) == 0
    assert bool((probed[~live][:, 3] <= 0).all())
    cand = _candidates(po, torch.tensor(kappa, dtype=torch.float32, device=po.device))
    assert torch.equal(_bits(probed[~cand][:, 3]), _bits(po[~cand][:, 0]))
    assert torch.equal(_bits(probed[cand]), _bits(gated[cand]))
    return cand


@pytest.mark.parametrize("key", list(SHAPES))
def test_first_and_second_launch(monkeypatch, key):
    """A fresh state: the first launch is the constant's and measures every candidate; the second culls with max(2^-9, 8 r_max)."""
    from intrinsicnerf_amd import kernels
    c = _setup()
    case = _case(c, key, monkeypatch)
    state = _new_state(c)
    first, po = _probed(c, case, state)
    assert torch.equal(_bits(first), _bits(case["constant"])) and torch.equal(_bits(po), _bits(case["po"]))
    cand1 = _assert_rows(case, first, po, gp.KAPPA)
    m1 = kernels.gate_margin(state)
    r_ref, n_ref = _r_fp32(case, cand1)
    print(f"{key} first launch: {m1}, candidates {int(cand1.sum())} of {cand1.numel()}, fp32 r over them {r_ref:.6e}")
    assert m1["launches"] == 1 and m1["kappa_in_use"] == gp.KAPPA
    assert m1["observed"] == int(cand1.sum()) == n_ref
    assert m1["r_max"] == r_ref and r_ref > 0.0

    second, po2 = _probed(c, case, state)
    m2 = kernels.gate_margin(state)
    want = max(FLOOR, 8.0 * m1["r_max"])
    print(f"{key} second launch: {m2}")
    assert m2["launches"] == 2 and m2["kappa_in_use"] == want
    cand2 = _assert_rows(case, second, po2, m2["kappa_in_use"])
    assert m2["observed"] - m1["observed"] == int(cand2.sum())
    assert int(cand2.sum()) < int(cand1.sum())
    assert bool((cand1 | ~cand2).all())                                   # (a smaller margin lists a subset)
    assert m2["r_max"] >= m1["r_max"]


@pytest.mark.parametrize("key", ["37x192", "171x193"])
def test_a_seeded_state_widens_the_margin(monkeypatch, key):
    """r_max = 2^-4 with enough observations: 8 r_max = 0.5 is used although it is above 2^-6."""
    from intrinsicnerf_amd import kernels
    c = _setup()
    case = _case(c, key, monkeypatch)
    state = _new_state(c, r_max=2.0 ** -4, observed=1 << 30)
    probed, po = _probed(c, case, state)
    m = kernels.gate_margin(state)
    print(f"{key} seeded: {m}")
    assert m["kappa_in_use"] == 0.5 and m["launches"] == 1
    cand = _assert_rows(case, probed, po, 0.5)
    n_const = int(_candidates(case["po"], gp.KAPPA).sum())
    assert int(cand.sum()) > n_const
    assert m["observed"] == (1 << 30) + int(cand.sum()) and m["r_max"] == 2.0 ** -4


def test_few_points_keep_the_constant(monkeypatch):
    """The built-in INERF_PROBE_MIN_OBS: ten launches of 37 x 192 do not move the margin."""
    from intrinsicnerf_amd import kernels
    c = _setup()
    case = _case(c, "37x192", monkeypatch)
    monkeypatch.delenv("INERF_PROBE_MIN_OBS")
    state = _new_state(c)
    n_cand = int(_candidates(case["po"], gp.KAPPA).sum())
    for i in range(10):
        probed, _ = _probed(c, case, state)
        m = kernels.gate_margin(state)
        assert m["kappa_in_use"] == gp.KAPPA and m["launches"] == i + 1 and m["observed"] == (i + 1) * n_cand, m
        assert torch.equal(_bits(probed), _bits(case["constant"]))
    print(f"ten launches: {m}")


@pytest.mark.parametrize("level", ["coarse", "fine"])
@pytest.mark.parametrize("family", gp.HOLDOUT_FAMILIES)
def test_trained_and_held_out_networks_adapt_safely(monkeypatch, family, level):
    """The lightly trained fixture and both hold-out fits on the depths their passes see (171 rays: 64 linspace depths / the fine pass's
    own 192): after adapting, no culled point has positive exact sigma."""
    from intrinsicnerf_amd import kernels
    c = _setup()
    rays = gp.family_rays(family)[:171].contiguous().to(c["dev"])
    if level == "coarse":
        t = torch.linspace(0., 1., S_C, device=c["dev"])
        z = (rays[:, 6:7] * (1 - t) + rays[:, 7:8] * t).contiguous()
    else:
        z = gp.fine_depths(family)[:171].contiguous().to(c["dev"])
    case = _case(c, f"{family}_{level}", monkeypatch, sd=gp.network(f"{family}_{level}")[0], rays=rays, z=z)
    state = _new_state(c)
    _probed(c, case, state)
    m1 = kernels.gate_margin(state)
    probed, po = _probed(c, case, state)
    m = kernels.gate_margin(state)
    assert m["kappa_in_use"] == max(FLOOR, 8.0 * m1["r_max"]) and m["launches"] == 2
    cand = _assert_rows(case, probed, po, m["kappa_in_use"])
    sigma = case["plain"][:, 3]
    r_all = float(((po[:, 0].double() - sigma.double()).abs() / po[:, 1].double()).max())
    print(f"{family} {level}: margin in use {m['kappa_in_use']:.4e}, r_max {m['r_max']:.4e} over {m['observed']} listed points, r over all points {r_all:.4e}, "
          f"reserve {m['kappa_in_use'] / r_all:.2f}, candidates {float(cand.float().mean()):.4f} (constant: {float(_candidates(po, gp.KAPPA).float().mean()):.4f})")
    assert int((~cand & (sigma > 0)).sum()) == 0
    assert 0.0 < float(cand.float().mean()) < 1.0


def test_a_nan_density_is_not_measured(monkeypatch):
    """A NaN weight in alpha_linear (as tests/test_gate_probe_gpu.py builds it): every sigma and s is NaN, every point a candidate and a
    survivor; r_max stays finite - no such row is counted."""
    from intrinsicnerf_amd import kernels
    c = _setup()
    sd = {k: v.clone() for k, v in c["sd_f"].items()}
    sd["alpha_linear.weight"][0, 5] = float("nan")
    rays = _frame_rays(c, 37)
    z = gp.sample_depths(rays.cpu(), 64, seed=9).to(c["dev"])
    case = _case(c, "nan", monkeypatch, sd=sd, rays=rays, z=z, rays_per_sub=12)
    assert bool(torch.isnan(case["plain"][:, 3]).all())
    state = _new_state(c)
    for launch in (1, 2):
        probed, po = _probed(c, case, state)
        m = kernels.gate_margin(state)
        cand = _assert_rows(case, probed, po, m["kappa_in_use"])
        assert bool(cand.all()) and bool(torch.isnan(probed[:, 3]).all())
        assert m["r_max"] == 0.0 and m["observed"] == 0 and m["kappa_in_use"] == gp.KAPPA and m["launches"] == launch, m


def test_the_eight_wave_probe_measures_the_same(monkeypatch):
    """INERF_PROBE_WG=1: the state's words and the raw rows of two launches are the default form's, bit for bit."""
    c = _setup()
    case = _case(c, "171x193", monkeypatch)
    got = {}
    for form in ("", "1"):
        if form:
            monkeypatch.setenv("INERF_PROBE_WG", form)
        state = _new_state(c)
        rows = []
        words = []
        for _ in range(2):
            probed, po = _probed(c, case, state)
            rows.append(probed)
            words.append(state.clone())
        got[form] = (rows, words)
    for launch in range(2):
        assert torch.equal(_bits(got[""][0][launch]), _bits(got["1"][0][launch])), launch
        assert torch.equal(got[""][1][launch], got["1"][1][launch]), (launch, got[""][1][launch].tolist(), got["1"][1][launch].tolist())
    assert int(got["1"][1][1][4]) == 2 and float(got["1"][1][1].view(torch.float32)[1]) < gp.KAPPA      # two launches, the second adapted


def test_a_network_without_candidates(monkeypatch):
    """alpha bias -1e4: nothing is listed, nothing measured, the margin stays the constant."""
    from intrinsicnerf_amd import kernels
    c = _setup()
    sd = {k: v.clone() for k, v in c["sd_f"].items()}
    sd["alpha_linear.bias"] = sd["alpha_linear.bias"] - 1.0e4
    rays = _frame_rays(c, 37)
    z = gp.sample_depths(rays.cpu(), 64, seed=5).to(c["dev"])
    case = _case(c, "none", monkeypatch, sd=sd, rays=rays, z=z, rays_per_sub=12)
    state = _new_state(c)
    for launch in (1, 2, 3):
        probed, po = _probed(c, case, state)
        m = kernels.gate_margin(state)
        cand = _assert_rows(case, probed, po, gp.KAPPA)
        assert int(cand.sum()) == 0
        assert m["observed"] == 0 and m["r_max"] == 0.0 and m["kappa_in_use"] == gp.KAPPA and m["launches"] == launch, m


MAPS = [f"{k}_{lvl}" for lvl in ("coarse", "fine") for k in ("rgb", "disp", "acc", "depth", "albedo", "shading", "residual")] + ["z_std"]


def _assert_maps_equal(a, b):
    for k in MAPS:
        assert torch.equal(torch.isnan(a[k]), torch.isnan(b[k])), k
        assert torch.equal(_bits(torch.nan_to_num(a[k], nan=0.0)), _bits(torch.nan_to_num(b[k], nan=0.0))), k


def test_the_front_end_keeps_a_state_per_packed_blob(monkeypatch):
    """render_rays_fused, 37 rays, 64 + 128, three calls on the same blobs: the state of a blob is found again, the second and third
    call cull with the adapted margin, and all maps are those of INERF_PROBE_ADAPT=0 and of INERF_PROBE=0.  A module's state is made
    with its blob: packing.invalidate and load_state_dict start a new one."""
    from intrinsicnerf_amd import kernels, object_level as ol, packing
    c = _setup()
    monkeypatch.setenv("INERF_GATE_BYTES", str(12 * 64 * 1028))      # 4 coarse sub-ranges, 10 fine ones
    embed, ch = ol.get_embedder(10, 0)
    embed_d, ch_d = ol.get_embedder(4, 0)
    mk = lambda: ol.NeRF(D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=ch_d, use_viewdirs=True).to(c["dev"])
    net_c, net_f = mk(), mk()
    net_c.load_state_dict(c["sd_c"]); net_f.load_state_dict(c["sd_f"])
    rays = _frame_rays(c, 37)
    u = torch.rand(37, S_I, generator=torch.Generator().manual_seed(5)).to(c["dev"])
    t = torch.linspace(0., 1., S_C, device=c["dev"])

    def render():
        pc, pf = packing.packed_for_module(net_c, c["desc"], c["dev"]), packing.packed_for_module(net_f, c["desc"], c["dev"])
        out = kernels.render_rays_fused(c["desc"], pc, pf, rays, S_C, S_I, t, u=u, white_bkgd=True)
        torch.cuda.synchronize()
        return out, kernels.gate_margin(packing.gate_state_of(pc)), kernels.gate_margin(packing.gate_state_of(pf))

    outs = [render() for _ in range(3)]
    for i, (_, mc, mf) in enumerate(outs):
        print(f"call {i + 1}: coarse {mc}, fine {mf}")
        assert mc["launches"] == mf["launches"] == i + 1
        assert mc["kappa_in_use"] == (gp.KAPPA if i == 0 else max(FLOOR, 8.0 * outs[i - 1][1]["r_max"]))
        assert mf["kappa_in_use"] == (gp.KAPPA if i == 0 else max(FLOOR, 8.0 * outs[i - 1][2]["r_max"]))
    assert 0 < outs[0][1]["observed"] and outs[1][1]["observed"] - outs[0][1]["observed"] < outs[0][1]["observed"]
    _assert_maps_equal(outs[0][0], outs[1][0])
    _assert_maps_equal(outs[0][0], outs[2][0])
    launches = outs[2][1]["launches"]
    monkeypatch.setenv("INERF_PROBE_ADAPT", "0")
    constant, mc, _ = render()
    assert mc["launches"] == launches                                 # the state was not passed
    monkeypatch.setenv("INERF_PROBE", "0")
    gate, mc, _ = render()
    assert mc["launches"] == launches
    _assert_maps_equal(outs[2][0], constant)
    _assert_maps_equal(outs[2][0], gate)
    assert int(outs[2][0]["status"].max()) == 0
    monkeypatch.delenv("INERF_PROBE_ADAPT")
    monkeypatch.delenv("INERF_PROBE")
    # a repack starts from zero
    old = packing.gate_state_of(packing.packed_for_module(net_c, c["desc"], c["dev"]))
    packing.invalidate(net_c)
    new = packing.gate_state_of(packing.packed_for_module(net_c, c["desc"], c["dev"]))
    assert new is not old and kernels.gate_margin(new) == dict(r_max=0.0, observed=0, kappa_in_use=0.0, launches=0)
    assert kernels.gate_margin(old)["launches"] == launches
    net_f.load_state_dict(c["sd_c"])
    new_f = packing.gate_state_of(packing.packed_for_module(net_f, c["desc"], c["dev"]))
    assert kernels.gate_margin(new_f)["observed"] == 0 and kernels.gate_margin(new_f)["launches"] == 0
