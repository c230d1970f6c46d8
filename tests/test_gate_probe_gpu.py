"""GPU: the density gate with its one-product probe (INERF_FLAG_GATE_PROBE): probe kernel -> listed trunk -> heads.

The probe culls a point when s < -kappa S on hi-only arithmetic; every other point goes through the exact trunk as an entry of a
candidate list.  So the raw rows of points with positive (or NaN) density are the ungated kernel's bit for bit, the others carry
zero colours and a non-positive sigma, and the rendered maps are those of the gate alone and of the ungated path.  Equality is
``torch.equal`` on the bits.

kappa was fitted on the bench networks and the lightly trained fixture.  ``test_trained_and_held_out_networks`` runs every trained
network the project has - that fixture and the two hold-out fits (tests/golden/probe_holdout_*.npz) - through the probe kernel on
the depths their passes see, and holds the kernel's own (s, S) against the exact kernel's sigma and against the torch restatement
that the CPU derivation (tests/test_gate_probe_cpu.py) speaks for."""
import pytest
import torch

import _gate_probe as gp

pytestmark = pytest.mark.gpu

COLOURS = [0, 1, 2, 4, 5, 6, 7, 8, 9, 10]
S_C, S_I = 64, 128


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("INERF_PRECISION", "INERF_F16_KERNEL", "INERF_GATE", "INERF_PROBE", "INERF_PROBE_WG", "INERF_GATE_LOG", "INERF_ENC_CACHE",
              "INERF_GATE_BYTES"):
        monkeypatch.delenv(k, raising=False)


_cache = {}


def _setup():
    if not _cache:
        from intrinsicnerf_amd import _capi
        dev = torch.device("cuda:0")
        sd_c, rays = gp.network("bench_coarse")
        sd_f, _ = gp.network("bench_fine")
        _cache.update(dev=dev, rays=rays.to(dev), sd_c=sd_c, sd_f=sd_f, desc=_capi.net_desc(_capi.VARIANT_OBJECT, precision=_capi.PREC_F16X3))
    return _cache


def _pack(c, sd):
    from intrinsicnerf_amd import packing
    return packing.pack_state_dict(c["desc"], sd).to(c["dev"])


def _frame_rays(c, n_rays):
    """``n_rays`` of the 4096-ray sample, spread over the frame."""
    return c["rays"][:: c["rays"].shape[0] // n_rays][:n_rays].contiguous()


def _three_ways(c, packed, rays, z, **kw):
    """(ungated, gate alone, gate with probe, probe_out [n, 2])"""
    from intrinsicnerf_amd import kernels
    plain = kernels.encode_mlp(c["desc"], packed, rays, z)
    gated = kernels.encode_mlp(c["desc"], packed, rays, z, gate_colour=True)
    po = torch.full((z.numel(), 2), float("nan"), device=c["dev"])
    probed = kernels.encode_mlp(c["desc"], packed, rays, z, gate_colour=True, gate_probe=True, probe_out=po, **kw)
    torch.cuda.synchronize()
    return plain.reshape(-1, 11), gated.reshape(-1, 11), probed.reshape(-1, 11), po


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_rows(plain, gated, probed, po):
    """The issue's three statements about the raw rows, and that a candidate's row is the gate's.  Returns the candidate mask."""
    s, big_s = po[:, 0], po[:, 1]
    live = ~(plain[:, 3] <= 0)                                       # positive or NaN
    assert torch.equal(_bits(probed[live]), _bits(plain[live]))      # all eleven channels
    assert int((probed[~live][:, COLOURS] != 0).sum()) == 0
    assert bool((probed[~live][:, 3] <= 0).all())
    culled = s < -gp.KAPPA * big_s
    differs = _bits(probed[:, 3]) != _bits(plain[:, 3])
    assert bool(culled[differs].all())
    assert torch.equal(_bits(probed[~culled]), _bits(gated[~culled]))
    assert torch.equal(probed[culled][:, 3], s[culled])
    return ~culled


@pytest.mark.parametrize("n_rays,n_samples,rays_per_sub", [(171, 193, 40), (37, 64, 12), (37, 192, 4)])
def test_raw_rows_at_the_kernel(monkeypatch, n_rays, n_samples, rays_per_sub):
    """171 x 193: 258 tiles with a ragged last one, in five sub-ranges (the last of 11 rays); 37 rays: neither point count is a multiple
    of the tile."""
    c = _setup()
    monkeypatch.setenv("INERF_GATE_BYTES", str(rays_per_sub * n_samples * 1028))
    rays = _frame_rays(c, n_rays)
    z = gp.sample_depths(rays.cpu(), n_samples, seed=23).to(c["dev"])
    plain, gated, probed, po = _three_ways(c, _pack(c, c["sd_f"]), rays, z)
    cand = _assert_rows(plain, gated, probed, po)
    r = float(((po[:, 0].double() - plain[:, 3].double()).abs() / po[:, 1].double()).max())
    share = float(cand.float().mean())
    print(f"{n_rays} x {n_samples}: sigma > 0 on {float((plain[:, 3] > 0).float().mean()):.4f}, candidates {share:.4f}, r = {r:.3e}, 8 r / kappa = {8 * r / gp.KAPPA:.3f}")
    assert 0.0 < share < 1.0                                          # both sides of the probe are exercised
    assert 8.0 * r <= gp.KAPPA


def test_r_of_the_coarse_network():
    c = _setup()
    rays = _frame_rays(c, 128)
    t = torch.linspace(0., 1., S_C, device=c["dev"])
    z = (rays[:, 6:7] * (1 - t) + rays[:, 7:8] * t).contiguous()
    plain, gated, probed, po = _three_ways(c, _pack(c, c["sd_c"]), rays, z)
    _assert_rows(plain, gated, probed, po)
    r = float(((po[:, 0].double() - plain[:, 3].double()).abs() / po[:, 1].double()).max())
    print(f"coarse network: r = {r:.3e}, 8 r / kappa = {8 * r / gp.KAPPA:.3f}")
    assert 8.0 * r <= gp.KAPPA


HELD_OUT_SHAPES = {"coarse": (171, None), "fine_sub_ranges": (37, 4), "fine_ragged": (171, None)}       # (rays, rays per sub-range)


def _held_out_case(c, family, shape):
    """(state dict, rays, depths) of one case: the coarse network on 64 linspace depths, or the fine network on the fine pass's own
    192 depths (``gp.fine_depths``), on 171 of the family's 256 rays (171 x 192 = 256.5 tiles) or on 37 spread over them."""
    n_rays, _ = HELD_OUT_SHAPES[shape]
    rays, z_fine = gp.family_rays(family), gp.fine_depths(family)
    sel = torch.arange(n_rays) if n_rays == 171 else torch.arange(0, rays.shape[0], rays.shape[0] // n_rays)[:n_rays]
    rays = rays[sel].contiguous().to(c["dev"])
    if shape == "coarse":
        t = torch.linspace(0., 1., S_C, device=c["dev"])
        return gp.network(family + "_coarse")[0], rays, (rays[:, 6:7] * (1 - t) + rays[:, 7:8] * t).contiguous()
    return gp.network(family + "_fine")[0], rays, z_fine[sel].contiguous().to(c["dev"])


def _held_out_figures(tag, sd, rays, z, plain, po, cand):
    """Prints and returns (r of the kernel, kernel-to-model distance in S, candidate share)."""
    s, big_s = po[:, 0].double().cpu(), po[:, 1].double().cpu()
    with torch.no_grad():
        s_model, _ = gp.probe_model(sd, gp.positions(rays.cpu(), z.cpu()))
    r = float(((s - plain[:, 3].double().cpu()).abs() / big_s).max())
    dist = float(((s - s_model).abs() / big_s).max())
    share = float(cand.float().mean())
    print(f"{tag}: {tuple(z.shape)}, sigma > 0 on {float((plain[:, 3] > 0).float().mean()):.4f}, candidates {share:.4f}, r = {r:.3e}, "
          f"kappa / r = {gp.KAPPA / r:.2f}, kernel vs model {dist:.3e} S")
    return r, dist, share


@pytest.mark.parametrize("shape", list(HELD_OUT_SHAPES))
@pytest.mark.parametrize("family", gp.HOLDOUT_FAMILIES)
def test_trained_and_held_out_networks(monkeypatch, family, shape):
    """37 x 192 in ten sub-ranges of 4 rays (the last of one); 171 x 192: 257 tiles, the last one half full."""
    c = _setup()
    sd, rays, z = _held_out_case(c, family, shape)
    n_rays, rays_per_sub = HELD_OUT_SHAPES[shape]
    if rays_per_sub is not None:
        monkeypatch.setenv("INERF_GATE_BYTES", str(rays_per_sub * z.shape[1] * 1028))
    words = -(-n_rays // 8)
    status = torch.zeros(words, dtype=torch.int32, device=c["dev"])
    plain, gated, probed, po = _three_ways(c, _pack(c, sd), rays, z, status=status, status_rays=8)
    r, dist, share = _held_out_figures(f"{family} {shape}", sd, rays, z, plain, po, ~(po[:, 0] < -gp.KAPPA * po[:, 1]))
    assert not bool(torch.isnan(po).any()) and int(status.max()) == 0          # every point was probed, none left the f16 range
    cand = _assert_rows(plain, gated, probed, po)
    assert r <= gp.KAPPA                                  # the kernel cannot cull a positive density
    assert dist <= gp.KAPPA / 8                           # ... and stays where the CPU derivation on the model speaks for it
    assert 0.0 < share < 1.0 and share == float(cand.float().mean())


def test_a_held_out_network_in_the_eight_wave_form(monkeypatch):
    """INERF_PROBE_WG=1 (tests/test_gate_probe_wg2_gpu.py) on a network neither form was tuned or tested on: (s, S) and the raw rows
    are the default form's bit for bit."""
    c = _setup()
    sd, rays, z = _held_out_case(c, "holdout_sharp", "fine_ragged")
    packed = _pack(c, sd)
    _, _, probed, po = _three_ways(c, packed, rays, z)
    monkeypatch.setenv("INERF_PROBE_WG", "1")
    _, _, probed1, po1 = _three_ways(c, packed, rays, z)
    print(f"holdout_sharp fine, two forms: candidates {float((~(po[:, 0] < -gp.KAPPA * po[:, 1])).float().mean()):.4f}")
    assert not bool(torch.isnan(po).any())
    assert torch.equal(_bits(po), _bits(po1))
    assert torch.equal(_bits(probed), _bits(probed1))


def _with_alpha_bias(sd, shift):
    sd = {k: v.clone() for k, v in sd.items()}
    sd["alpha_linear.bias"] = sd["alpha_linear.bias"] + shift
    return sd


def _point_rays(c, n):
    """``n`` sample points as ``n`` rays of ONE sample each (so that any prefix of them is a launch), one sub-range."""
    rays = _frame_rays(c, 64).repeat_interleave(48, 0)[:n].contiguous()
    g = torch.Generator().manual_seed(3)
    z = (2.0 + 4.0 * torch.rand(n, 1, generator=g)).to(c["dev"])
    return rays, z


@pytest.mark.parametrize("case", ["none", "all"])
def test_no_candidate_and_all_candidates(monkeypatch, case):
    c = _setup()
    monkeypatch.setenv("INERF_GATE_BYTES", str(12 * 64 * 1028))
    rays = _frame_rays(c, 37)
    z = gp.sample_depths(rays.cpu(), 64, seed=5).to(c["dev"])
    packed = _pack(c, _with_alpha_bias(c["sd_f"], -1.0e4 if case == "none" else 1.0e4))
    plain, gated, probed, po = _three_ways(c, packed, rays, z)
    cand = _assert_rows(plain, gated, probed, po)
    assert int(cand.sum()) == (0 if case == "none" else cand.numel())


@pytest.mark.parametrize("target", [255, 256, 257])
def test_candidate_count_at_the_tile_boundary(target):
    """A count of exactly two listed tiles, and one candidate less and more: the network's alpha bias is shifted so that about half
    of the points are candidates, and the launch is the prefix of 3 072 one-sample rays that holds exactly ``target`` of them."""
    c = _setup()
    packed = _pack(c, _with_alpha_bias(c["sd_f"], 1.0))
    rays, z = _point_rays(c, 3072)
    if "prefix" not in _cache:
        _, _, _, po = _three_ways(c, packed, rays, z)
        _cache["prefix"] = (~(po[:, 0] < -gp.KAPPA * po[:, 1])).long().cumsum(0)
    count = _cache["prefix"]
    assert int(count[-1]) >= 257, int(count[-1])
    n = int(torch.nonzero(count == target)[0]) + 1
    plain, gated, probed, po = _three_ways(c, packed, rays[:n].contiguous(), z[:n].contiguous())
    cand = _assert_rows(plain, gated, probed, po)
    assert int(cand.sum()) == target and bool(cand[-1])


@pytest.mark.parametrize("n_rays,n_samples", [(1, 1), (37, 64)])
def test_a_nan_density_survives(monkeypatch, n_rays, n_samples):
    """A NaN weight in alpha_linear: sigma is NaN (behind the trunk's ReLUs, which turn a NaN into 0, the density head is the one place
    a NaN can come from), the probe's s is NaN too, and !(s < -kappa S) makes the point a candidate, !(sigma <= 0) a survivor.  A
    launch of ONE point, and 37 x 64 in four sub-ranges where every point is one."""
    c = _setup()
    monkeypatch.setenv("INERF_GATE_BYTES", str(12 * 64 * 1028))
    sd = {k: v.clone() for k, v in c["sd_f"].items()}
    sd["alpha_linear.weight"][0, 5] = float("nan")
    rays = _frame_rays(c, 37)[:n_rays].contiguous()
    z = gp.sample_depths(rays.cpu(), n_samples, seed=9).to(c["dev"])
    plain, gated, probed, po = _three_ways(c, _pack(c, sd), rays, z)
    assert bool(torch.isnan(plain[:, 3]).all()) and not bool(torch.isnan(plain[:, COLOURS]).any())
    cand = _assert_rows(plain, gated, probed, po)
    assert bool(cand.all()) and bool(torch.isnan(probed[:, 3]).all())


def _render(c, white=True, sd_c=None, sd_f=None, desc=None, **kw):
    from intrinsicnerf_amd import kernels
    desc = desc or c["desc"]
    if "u" not in _cache:
        g = torch.Generator().manual_seed(5)
        _cache["u"] = torch.rand(37, S_I, generator=g).to(c["dev"])
        _cache["rays37"] = _frame_rays(c, 37)
    t = torch.linspace(0., 1., S_C, device=c["dev"])
    pc = _pack({**c, "desc": desc}, sd_c or c["sd_c"])
    pf = _pack({**c, "desc": desc}, sd_f or c["sd_f"])
    out = kernels.render_rays_fused(desc, pc, pf, _cache["rays37"], S_C, S_I, t, u=_cache["u"], white_bkgd=white, **kw)
    torch.cuda.synchronize()
    return out


MAPS = [f"{k}_{lvl}" for lvl in ("coarse", "fine") for k in ("rgb", "disp", "acc", "depth", "albedo", "shading", "residual")] + ["z_std"]


def _assert_maps_equal(a, b):
    for k in MAPS:
        assert torch.equal(torch.isnan(a[k]), torch.isnan(b[k])), k
        assert torch.equal(torch.nan_to_num(a[k], nan=0.0), torch.nan_to_num(b[k], nan=0.0)), k


@pytest.mark.parametrize("white", [True, False])
def test_rendered_maps_with_the_probe_the_gate_alone_and_ungated(monkeypatch, white):
    c = _setup()
    monkeypatch.setenv("INERF_GATE_BYTES", str(12 * 64 * 1028))      # 4 coarse sub-ranges, 10 fine ones
    probe = _render(c, white=white)
    again = _render(c, white=white)
    monkeypatch.setenv("INERF_PROBE", "0")
    gate = _render(c, white=white)
    monkeypatch.setenv("INERF_GATE", "0")
    plain = _render(c, white=white)
    _assert_maps_equal(probe, gate)
    _assert_maps_equal(probe, plain)
    _assert_maps_equal(probe, again)
    assert int(probe["status"].max()) == 0 and int(plain["status"].max()) == 0


def test_range_flag(monkeypatch):
    """h0's unit j becomes G relu(x - x0) with G = 1e5: 8 h0[j] passes the guard's 6e4 for every point with x - x0 > 0.075 - on the
    hi-only values as on the exact ones, whose relative distance (1e-3) is far inside the margin left here (x - x0 > 0.1).  One
    status word per 8 rays: the words of the rays that hold such a point are set at least; the unchanged network sets none."""
    from intrinsicnerf_amd import kernels
    c = _setup()
    monkeypatch.setenv("INERF_GATE_BYTES", str(12 * 64 * 1028))
    rays = _frame_rays(c, 37)
    z = gp.sample_depths(rays.cpu(), 64, seed=11).to(c["dev"])
    x = gp.positions(rays, z)[:, 0].reshape(37, 64)
    x0 = float(torch.quantile(x.flatten(), 0.9))
    hot = ((x - x0) > 0.1).any(-1)
    words = -(-37 // 8)
    expect = torch.zeros(words, dtype=torch.bool, device=c["dev"])
    expect[torch.nonzero(hot).flatten() // 8] = True
    assert bool(expect.any()) and not bool(hot.all())
    sd = {k: v.clone() for k, v in c["sd_f"].items()}
    sd["pts_linears.0.weight"][7].zero_()
    sd["pts_linears.0.weight"][7, 0] = 1.0e5
    sd["pts_linears.0.bias"][7] = -1.0e5 * x0
    for net, want in ((sd, expect), (c["sd_f"], torch.zeros_like(expect))):
        status = torch.zeros(words, dtype=torch.int32, device=c["dev"])
        kernels.encode_mlp(c["desc"], _pack(c, net), rays, z, gate_colour=True, gate_probe=True, status=status, status_rays=8)
        torch.cuda.synchronize()
        got = status != 0
        print("status words:", got.tolist(), "expected at least:", want.tolist())
        assert bool(got[want].all())
        if not bool(want.any()):
            assert not bool(got.any())


def _gate_lines(capfd):
    return [l for l in capfd.readouterr().err.splitlines() if l.startswith("inerf gate:")]


def test_automatic_gating(monkeypatch, capfd):
    """What runs is read from INERF_GATE_LOG's line per gated launch (it names the probe's candidates only when the probe ran)."""
    import oracle
    from intrinsicnerf_amd import _capi, kernels, packing
    c = _setup()
    monkeypatch.setenv("INERF_GATE_LOG", "1")
    _render(c)
    lines = _gate_lines(capfd)
    assert len(lines) == 2 and all("candidates" in l for l in lines), lines
    monkeypatch.setenv("INERF_PROBE", "0")
    _render(c)
    lines = _gate_lines(capfd)
    assert len(lines) == 2 and not any("candidates" in l for l in lines), lines
    monkeypatch.setenv("INERF_GATE", "0")
    _render(c)
    assert _gate_lines(capfd) == []
    monkeypatch.delenv("INERF_PROBE")
    monkeypatch.delenv("INERF_GATE")
    # the caller takes raw_fine: only the coarse pass is gated
    _render(c, want_raw_fine=True)
    lines = _gate_lines(capfd)
    assert len(lines) == 1 and f"x {S_C} samples" in lines[0], lines
    # noise is added to sigma before the ReLU; exact fp32; SSR
    g = torch.Generator().manual_seed(3)
    _render(c, noise_coarse=torch.randn(37, S_C, generator=g).to(c["dev"]), noise_fine=torch.randn(37, S_C + S_I, generator=g).to(c["dev"]))
    assert _gate_lines(capfd) == []
    _render(c, desc=_capi.net_desc(_capi.VARIANT_OBJECT, precision=_capi.PREC_F32))
    assert _gate_lines(capfd) == []
    desc = _capi.net_desc(_capi.VARIANT_SSR, n_classes=5, xyz_div=10.0, precision=_capi.PREC_F16X3)
    packed = packing.pack_state_dict(desc, oracle.make_state_dict("ssr", 5, seed=1)).to(c["dev"])
    t = torch.linspace(0., 1., S_C, device=c["dev"])
    kernels.render_rays_fused(desc, packed, packed, _cache["rays37"], S_C, S_I, t, u=_cache["u"])
    torch.cuda.synchronize()
    assert _gate_lines(capfd) == []


def test_the_probe_flag_needs_the_gate():
    from intrinsicnerf_amd import kernels
    c = _setup()
    rays = _frame_rays(c, 4)
    z = gp.sample_depths(rays.cpu(), 8, seed=1).to(c["dev"])
    with pytest.raises(RuntimeError):
        kernels.encode_mlp(c["desc"], _pack(c, c["sd_f"]), rays, z, gate_probe=True)
