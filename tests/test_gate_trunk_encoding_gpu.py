"""GPU: the gated trunk kernel's position encoding - it is evaluated once per tile, parked in LDS while the in-place
layers overwrite columns 0..63, and copied back for the skip layer pts_linears[5]; the view direction is encoded by the heads kernel
alone.  The parked values are copies of what the same code computed, so every case compares the gated pass's raw rows BIT FOR BIT
with the ungated kernel's (INERF_GATE=0) on the same inputs: all eleven channels of a surviving point, sigma and ten zeros of the
others."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# 258 tiles of 128 points, the last one ragged (107 points): two more tiles than the chip has CUs, so two workgroups walk their tile
# loop twice and could restore the tile before's parked copy.  (172 x 192 would be 258 tiles exactly: no ragged tile.)
N_RAYS, N_SAMPLES = 171, 193
N_TILES = -(-N_RAYS * N_SAMPLES // 128)
COLOURS = [0, 1, 2, 4, 5, 6, 7, 8, 9, 10]


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("INERF_PRECISION", "INERF_F16_KERNEL", "INERF_GATE", "INERF_GATE_LOG", "INERF_ENC_CACHE", "INERF_GATE_BYTES"):
        monkeypatch.delenv(k, raising=False)          # (default record budget: the 258 tiles are ONE trunk launch)


def _frame_rays(dev):
    """171 rays of the 800 x 800 chair frame bench.py renders (spread over the image), near 2, far 6."""
    from intrinsicnerf_amd import object_level as ol
    import bench
    ro, rd = ol.get_rays(bench.H, bench.W, bench.chair_intrinsics(), bench.chair_pose().to(dev))
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    sel = torch.arange(N_RAYS, device=dev) * (bench.W * 4 + 3) + 40 * bench.W + 17
    vd = rd[sel] / rd[sel].norm(dim=-1, keepdim=True)
    one = torch.ones_like(vd[:, :1])
    return torch.cat([ro[sel], rd[sel], 2.0 * one, 6.0 * one, vd], -1).contiguous()


_cache = {}


def _setup():
    """The calibrated default-init fine network (seed 1, as bench.py builds it), the rays and depths: computed once, left unchanged."""
    if not _cache:
        from oracle import calibration as cal
        from intrinsicnerf_amd import _capi
        assert N_TILES == 258 and N_RAYS * N_SAMPLES % 128 != 0
        dev = torch.device("cuda:0")
        rays = _frame_rays(dev)
        g = torch.Generator().manual_seed(23)
        z = (2.0 + 4.0 * torch.rand(N_RAYS, N_SAMPLES, generator=g).sort(-1).values).to(dev)
        _cache.update(dev=dev, rays=rays, z=z, desc=_capi.net_desc(_capi.VARIANT_OBJECT, precision=_capi.PREC_F16X3),
                      sd_f=cal.calibrated_default_init("object", 0, 1, rays.cpu()))
    return _cache


def _pack(c, sd):
    from intrinsicnerf_amd import packing
    return packing.pack_state_dict(c["desc"], sd).to(c["dev"])


def _gated_and_plain(monkeypatch, c, packed, rays, z):
    from intrinsicnerf_amd import kernels
    gated = kernels.encode_mlp(c["desc"], packed, rays, z, gate_colour=True)
    monkeypatch.setenv("INERF_GATE", "0")
    plain = kernels.encode_mlp(c["desc"], packed, rays, z)
    monkeypatch.delenv("INERF_GATE")
    torch.cuda.synchronize()
    return gated, plain


def _assert_rows_equal(gated, plain):
    """Returns the survivor mask."""
    keep = ~(plain[..., 3] <= 0)                                  # (a NaN survives)
    assert torch.equal(gated[..., 3].view(torch.int32), plain[..., 3].view(torch.int32))      # sigma of EVERY point, bit for bit
    assert torch.equal(gated[keep].view(torch.int32), plain[keep].view(torch.int32))          # all 11 channels
    assert int((gated[~keep][:, COLOURS] != 0).sum()) == 0
    return keep


@pytest.mark.parametrize("n_points", [64, 128, 129])
def test_skip_layer_sees_the_restored_encoding(monkeypatch, n_points):
    """pts_linears[5] with its h-part (input columns 63..318) zeroed: h5, and so sigma and everything behind it, depends on the
    encoding that the skip layer reads alone - a wrong restored column is not diluted by 256 channels of h4.  Half a tile, a whole
    tile, a tile and one point."""
    c = _setup()
    sd = {k: v.clone() for k, v in c["sd_f"].items()}
    assert sd["pts_linears.5.weight"].shape == (256, 63 + 256)
    sd["pts_linears.5.weight"][:, 63:] = 0.0
    g = torch.Generator().manual_seed(n_points)
    z = (2.0 + 4.0 * torch.rand(1, n_points, generator=g).sort(-1).values).to(c["dev"])
    gated, plain = _gated_and_plain(monkeypatch, c, _pack(c, sd), c["rays"][:1], z)
    sigma = plain[..., 3]
    assert int(sigma.unique().numel()) > n_points // 2            # the encoding reaches sigma: it varies from point to point
    keep = _assert_rows_equal(gated, plain)
    print(f"{n_points} points: {int(keep.sum())} survive")


def test_no_stale_parking_across_tiles(monkeypatch):
    c = _setup()
    gated, plain = _gated_and_plain(monkeypatch, c, _pack(c, c["sd_f"]), c["rays"], c["z"])
    share = float((~(plain[..., 3] <= 0)).float().mean())
    print("survivor share:", share)
    assert 0.0 < share < 1.0
    _assert_rows_equal(gated, plain)


def test_directions_still_reach_the_heads(monkeypatch):
    """The trunk kernel no longer encodes the view direction: the heads kernel's own encoding is what the colours see.  Two view
    directions per ray origin (the ray's own, and a tilted one): each gated run equals its ungated run, and the two gated runs
    differ on surviving points."""
    c = _setup()
    packed = _pack(c, c["sd_f"])
    tilted = c["rays"].clone()
    vd = tilted[:, 8:11] + torch.tensor([0.3, -0.2, 0.1], device=c["dev"])
    tilted[:, 8:11] = vd / vd.norm(dim=-1, keepdim=True)
    got = []
    for rays in (c["rays"], tilted):
        gated, plain = _gated_and_plain(monkeypatch, c, packed, rays, c["z"])
        keep = _assert_rows_equal(gated, plain)
        assert 0 < int(keep.sum()) < keep.numel()
        got.append((gated, keep))
    (a, keep_a), (b, keep_b) = got
    assert torch.equal(keep_a, keep_b) and torch.equal(a[..., 3], b[..., 3])      # density does not depend on the direction
    differ = (a[keep_a][:, COLOURS] != b[keep_a][:, COLOURS]).any(-1)
    print("surviving points whose colours differ between the two directions:", int(differ.sum()), "of", int(keep_a.sum()))
    assert int(differ.sum()) >= 1
