"""GPU: the two forms of the density gate's probe kernel compute the same bits.

The default is ``k_mlp_gate_probe_wg2_f16`` - two four-wave workgroups per CU, a wave on 64 channels x 128 points
(csrc/mlp_f16_probe.h); ``INERF_PROBE_WG=1`` selects ``k_mlp_gate_probe_f16``, the eight-wave workgroup it was derived from.  Every
output element's products are summed in the same k order with the same instruction and go through the same epilogue, so (s, S) per
point, the raw rows behind the listed trunk and the heads, and the range status words are equal bit for bit."""
import pytest
import torch

import _gate_probe as gp

pytestmark = pytest.mark.gpu


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


def _bits(t):
    return t.contiguous().view(torch.int32)


def _probed(c, packed, rays, z, **kw):
    """(raw rows [n, 11], probe_out [n, 2]) of the gate with its probe, in whichever form the environment selects."""
    from intrinsicnerf_amd import kernels
    po = torch.full((z.numel(), 2), float("nan"), device=c["dev"])
    raw = kernels.encode_mlp(c["desc"], packed, rays, z, gate_colour=True, gate_probe=True, probe_out=po, **kw)
    torch.cuda.synchronize()
    return raw.reshape(-1, 11), po


def _both_forms(monkeypatch, c, packed, rays, z):
    """Runs the two forms and asserts equality of (s, S) and the raw rows; returns the default form's (raw, probe_out)."""
    raw2, po2 = _probed(c, packed, rays, z)
    monkeypatch.setenv("INERF_PROBE_WG", "1")
    raw1, po1 = _probed(c, packed, rays, z)
    monkeypatch.delenv("INERF_PROBE_WG")
    assert not bool(torch.isnan(po2).any())                      # every point of the launch was written
    assert torch.equal(_bits(po2), _bits(po1))
    assert torch.equal(_bits(raw2), _bits(raw1))
    return raw2, po2


def _assert_live_rows_are_the_ungated_kernels(c, packed, rays, z, raw):
    from intrinsicnerf_amd import kernels
    plain = kernels.encode_mlp(c["desc"], packed, rays, z).reshape(-1, 11)
    torch.cuda.synchronize()
    live = plain[:, 3] > 0
    assert bool(live.any()) and not bool(live.all())
    assert torch.equal(_bits(raw[live]), _bits(plain[live]))      # all eleven channels


@pytest.mark.parametrize("n_rays,n_samples,rays_per_sub", [(171, 193, 40), (37, 64, 12), (1, 64, None), (700, 192, None)])
def test_both_forms_give_the_same_bits(monkeypatch, n_rays, n_samples, rays_per_sub):
    """171 x 193: 258 tiles with a ragged last one, in five sub-ranges (the last of 11 rays); 37 x 64 in four; 1 x 64: half a tile, one
    workgroup; 700 x 192: 1 050 tiles - more than two per CU's pair of workgroups, so every workgroup walks more than one tile."""
    c = _setup()
    if rays_per_sub is not None:
        monkeypatch.setenv("INERF_GATE_BYTES", str(rays_per_sub * n_samples * 1028))
    rays = _frame_rays(c, n_rays)
    z = gp.sample_depths(rays.cpu(), n_samples, seed=23).to(c["dev"])
    packed = _pack(c, c["sd_f"])
    raw, po = _both_forms(monkeypatch, c, packed, rays, z)
    cand = ~(po[:, 0] < -gp.KAPPA * po[:, 1])
    print(f"{n_rays} x {n_samples}: candidates {float(cand.float().mean()):.4f}")
    if n_rays > 1:
        assert 0.0 < float(cand.float().mean()) < 1.0             # both sides of the probe are exercised
        _assert_live_rows_are_the_ungated_kernels(c, packed, rays, z, raw)


def test_the_coarse_network(monkeypatch):
    c = _setup()
    rays = _frame_rays(c, 128)
    t = torch.linspace(0., 1., 64, device=c["dev"])
    z = (rays[:, 6:7] * (1 - t) + rays[:, 7:8] * t).contiguous()
    packed = _pack(c, c["sd_c"])
    raw, _ = _both_forms(monkeypatch, c, packed, rays, z)
    _assert_live_rows_are_the_ungated_kernels(c, packed, rays, z, raw)


def test_range_status_words(monkeypatch):
    """h0's unit 7 becomes G relu(x - x0) with G = 1e5 (tests/test_gate_probe_gpu.py::test_range_flag): the rays that reach
    x - x0 > 0.1 leave the f16 range, the others do not.  One status word per 8 rays; the flag is per tile of 128 consecutive points
    in both forms, so the words are equal - and some are set, some are not."""
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
    packed = _pack(c, sd)
    got = {}
    for form in (None, "1"):
        if form:
            monkeypatch.setenv("INERF_PROBE_WG", form)
        status = torch.zeros(words, dtype=torch.int32, device=c["dev"])
        kernels.encode_mlp(c["desc"], packed, rays, z, gate_colour=True, gate_probe=True, status=status, status_rays=8)
        torch.cuda.synchronize()
        got[form] = status.clone()
    print("status words:", got[None].tolist(), "eight-wave form:", got["1"].tolist(), "expected at least:", expect.tolist())
    assert torch.equal(got[None], got["1"])
    assert bool((got[None] != 0)[expect].all())
