"""GPU: the equalities that need no tolerance, at REDUCED encodings - (l_xyz, l_dir) = (6, 2) and (0, 0), where the encoding's pad
columns start at 39 / 15 and at 3 / 3 instead of 63 / 27.  The gated trunk parks the skip layer's encoding in LDS and drops the
direction encoding; the grid kernel encodes lattice points itself: all of that is held bit for bit at (10, 4) by
test_density_gate_gpu.py, test_raw_rows_gpu.py and test_grid_gpu.py, and here on the descriptions a user who trains with
--multires 6 --multires_views 2 gets.

Weights: oracle.lcg_state_dict(seed 21, sigma_gain_log2 3, freq_decay) as in tests/_descs.py, alpha_linear.bias moved by minus the
median sigma of the case's points so that both signs occur (asserted: a share of sigma <= 0 between 0.2 and 0.9)."""
import pytest
import torch

import _descs
import oracle
from test_density_gate_gpu import GATE_BYTES, N_RAYS, S_C, S_I, _assert_maps_equal, _rays
from test_gate_probe_gpu import _assert_rows
from test_grid_gpu import bits, encode_mlp_sigma

pytestmark = pytest.mark.gpu

TAG = "backward_descs | equalities"
DEV = "cuda:0"
ENCODINGS = [(6, 2), (0, 0)]
COLOUR = [0, 1, 2, 4, 5, 6, 7, 8, 9, 10]


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("INERF_PRECISION", "INERF_F16_KERNEL", "INERF_GATE", "INERF_PROBE", "INERF_PROBE_WG", "INERF_GATE_LOG", "INERF_ENC_CACHE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("INERF_GATE_BYTES", GATE_BYTES)


def _pack(desc, sd):
    from intrinsicnerf_amd import packing
    return packing.pack_state_dict(desc, sd).to(DEV)


def _centred(desc, sd, rays, z):
    """``sd`` with alpha_linear.bias moved by minus the median of the plain kernel's sigma on (rays, z); the share of sigma <= 0 after."""
    from intrinsicnerf_amd import kernels
    sigma = kernels.encode_mlp(desc, _pack(desc, sd), rays, z)[..., 3]
    sd = {k: v.clone() for k, v in sd.items()}
    sd["alpha_linear.bias"] = sd["alpha_linear.bias"] - float(sigma.flatten().median())
    share = float((kernels.encode_mlp(desc, _pack(desc, sd), rays, z)[..., 3] <= 0).float().mean())
    return sd, share


@pytest.mark.parametrize("probe", [False, True], ids=["probe-off", "probe-on"])
@pytest.mark.parametrize("enc", ENCODINGS, ids=lambda e: f"x{e[0]}d{e[1]}")
def test_gated_rows_equal_plain_rows(enc, probe):
    """encode_mlp(gate_colour=True) against the plain call at 1, 127, 129 and 703 points: surviving rows equal on all 11 channels,
    culled rows equal sigma and zero colour (what test_density_gate_gpu.test_raw_rows_at_the_kernel asserts at (10, 4)).  With the
    probe on top, what test_gate_probe_gpu.test_raw_rows_at_the_kernel asserts at (10, 4): rows of positive density are the plain
    kernel's, the others have zero colours and sigma <= 0 - the probe's own s where it culled, the gate's row elsewhere."""
    from intrinsicnerf_amd import kernels
    desc = _descs.capi_desc("object", 0, *enc)
    rays = _rays(torch.device(DEV))
    g = torch.Generator().manual_seed(703)
    z_all = (2.0 + 4.0 * torch.rand(N_RAYS, 19, generator=g).sort(-1).values).to(DEV)          # 37 x 19 = 703 points
    sd, share = _centred(desc, oracle.lcg_state_dict("object", 0, l_xyz=enc[0], l_dir=enc[1], **_descs.WEIGHTS), rays, z_all)
    print(f"{TAG} gate x{enc[0]}d{enc[1]} probe {probe}: share of sigma <= 0 at 703 points {share:.3f}")
    assert 0.2 <= share <= 0.9, share
    packed = _pack(desc, sd)
    shares = []
    for n_points in (1, 127, 129, 703):
        if n_points == 703:
            r, z = rays, z_all
        else:              # n_points rays of one sample each, drawn like the 703 points the bias was centred on
            r = rays[torch.arange(n_points, device=DEV) % N_RAYS].contiguous()
            z = (2.0 + 4.0 * torch.rand(n_points, 1, generator=torch.Generator().manual_seed(n_points))).to(DEV)
        plain = kernels.encode_mlp(desc, packed, r, z).reshape(-1, 11)
        gated = kernels.encode_mlp(desc, packed, r, z, gate_colour=True).reshape(-1, 11)
        torch.cuda.synchronize()
        keep = plain[:, 3] > 0
        if n_points >= 127:
            assert 0 < int(keep.sum()) < n_points, (n_points, int(keep.sum()))
        assert torch.equal(gated[keep], plain[keep]), n_points
        assert torch.equal(gated[~keep][:, 3], plain[~keep][:, 3]), n_points
        assert int((gated[~keep][:, COLOUR] != 0).sum()) == 0, n_points
        if probe:          # a point the probe culls carries the probe's s <= 0 for sigma, not the trunk's: test_gate_probe_gpu._assert_rows
            po = torch.full((n_points, 2), float("nan"), device=DEV)
            probed = kernels.encode_mlp(desc, packed, r, z, gate_colour=True, gate_probe=True, probe_out=po).reshape(-1, 11)
            torch.cuda.synchronize()
            candidates = _assert_rows(plain, gated, probed, po)
            shares.append(float(candidates.float().mean()))
    if probe:
        print(f"{TAG} gate x{enc[0]}d{enc[1]}: candidates of the probe at 1 / 127 / 129 / 703 points {shares}")
        assert 0.0 < shares[-1] < 1.0          # both sides of the probe are exercised at 703 points


@pytest.mark.parametrize("enc", ENCODINGS, ids=lambda e: f"x{e[0]}d{e[1]}")
def test_gated_maps_equal_ungated_maps(enc, monkeypatch):
    """render_rays_fused at 37 rays x (64 + 128) samples with and without INERF_GATE=0: the same maps."""
    from intrinsicnerf_amd import kernels
    desc = _descs.capi_desc("object", 0, *enc)
    rays = _rays(torch.device(DEV))
    t = torch.linspace(0., 1., S_C, device=DEV)
    u = torch.rand(N_RAYS, S_I, generator=torch.Generator().manual_seed(5)).to(DEV)
    z = (2.0 + 4.0 * t).expand(N_RAYS, S_C).contiguous()
    sds, shares = [], []
    for seed in (21, 22):
        weights = dict(_descs.WEIGHTS, seed=seed)
        sd, share = _centred(desc, oracle.lcg_state_dict("object", 0, l_xyz=enc[0], l_dir=enc[1], **weights), rays, z)
        sds.append(_pack(desc, sd)); shares.append(share)
    print(f"{TAG} maps x{enc[0]}d{enc[1]}: share of sigma <= 0 on the coarse samples (coarse, fine network) {shares}")
    assert all(0.2 <= s <= 0.9 for s in shares), shares

    def run():
        out = kernels.render_rays_fused(desc, sds[0], sds[1], rays, S_C, S_I, t, u=u, white_bkgd=True)
        torch.cuda.synchronize()
        return out
    on = run()
    monkeypatch.setenv("INERF_GATE", "0")
    off = run()
    _assert_maps_equal(on, off)
    assert int(on["status"].max()) == 0 and int(off["status"].max()) == 0


@pytest.mark.parametrize("count", [129, 2197])
@pytest.mark.parametrize("variant,classes,enc", [("object", 0, (6, 2)), ("ssr", 5, (3, 0))], ids=["object-x6d2", "ssr5-x3d0"])
def test_grid_sigma_has_the_bits_of_encode_mlp(variant, classes, enc, count):
    """occupancy_grid(..., sigma=True) against inerf_encode_mlp channel 3 on the same lattice points (test_grid_gpu.py at (10, 4))."""
    import _grid
    from intrinsicnerf_amd import kernels
    desc = _descs.capi_desc(variant, classes, *enc)
    sd = oracle.lcg_state_dict(variant, classes, l_xyz=enc[0], l_dir=enc[1], **_descs.WEIGHTS)
    t, dim, scale, m, _ = _grid.box("d13" if variant == "ssr" else "object")
    n = dict(desc=desc, packed=_pack(desc, sd))
    t = t.to(DEV)
    pts = kernels.grid_points(t, scale, m, 0, count)
    want = encode_mlp_sigma(n, pts)
    shift = float(want.median())
    sd["alpha_linear.bias"] = sd["alpha_linear.bias"] - shift
    n["packed"] = _pack(desc, sd)
    want = encode_mlp_sigma(n, pts)
    share = float((want <= 0).float().mean())
    print(f"{TAG} grid {variant} x{enc[0]}d{enc[1]} count {count}: share of sigma <= 0 {share:.3f}")
    assert 0.2 <= share <= 0.9, share
    dist = float(_grid.fixture()[("ssr" if variant == "ssr" else "object") + "/dist"])
    occ, sigma = kernels.occupancy_grid(desc, n["packed"], t, scale, m, dist, 0, count, sigma=True)
    assert torch.isfinite(sigma).all()
    assert torch.equal(bits(sigma), bits(want))
    assert bool((occ[sigma <= 0] == 0).all())
