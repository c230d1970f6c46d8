"""GPU: mesh extraction's grid query - inerf_grid_points and inerf_occupancy_grid (the kGridTrunk mode of the 128-point tile body,
csrc/mlp_f16_t128.hip) and their front-ends (geometry.occupancy_grid, SSRRenderMixin.occupancy_grid).

The lattice is the reference's, bit for bit (tests/golden/grid_query.npz); sigma has the bits of channel 3 of inerf_encode_mlp on the same
points (it is the same device code: this is the test that fails when the shared tile body is disturbed); sigma and occupancy are within
rtol 1e-4 / atol 1e-5 (tests/_cases.py) of what the reference recorded on both fixture networks."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import _grid

pytestmark = pytest.mark.gpu

DEV = "cuda"


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def nets():
    """per fixture network: module on the device, encoders, descriptor (f16x3), packed weights, its box (device table), voxel size"""
    from intrinsicnerf_amd import _capi, packing
    out = {}
    for tag, box_tag in (("ssr", "d13"), ("object", "object")):
        net, embed, embed_d = _grid.network(tag, DEV)
        desc = net.fused_desc()
        desc.precision = _capi.PREC_F16X3
        desc.xyz_div = embed.scalar_factor
        t, dim, scale, m, pts = _grid.box(box_tag)
        out[tag] = dict(net=net, embed=embed, embed_d=embed_d, desc=desc, packed=packing.packed_for_module(net, desc, torch.device(DEV)),
                        t=t.to(DEV), scale=scale, m=m, dist=float(_grid.fixture()[tag + "/dist"]), box=box_tag)
    return out


@pytest.fixture(scope="module")
def whole(nets):
    """(occ, sigma) of the whole dim-13 lattice per network, one C call each: computed once, shared, never written"""
    from intrinsicnerf_amd import kernels
    return {tag: kernels.occupancy_grid(n["desc"], n["packed"], n["t"], n["scale"], n["m"], n["dist"], sigma=True) for tag, n in nets.items()}


def encode_mlp_sigma(n, pts):
    """channel 3 of inerf_encode_mlp on rays (o = pts, d = 0, z = 0)"""
    from intrinsicnerf_amd import _capi
    count = pts.shape[0]
    rays = torch.zeros(count, _capi.RAY_FLOATS, device=DEV)
    rays[:, 0:3] = pts
    z = torch.zeros(count, 1, device=DEV)
    ch = _capi.lib().inerf_raw_channels(n["desc"], 0, 1)
    raw = torch.empty(count, ch, device=DEV)
    rc = _capi.lib().inerf_encode_mlp(n["desc"], C.c_void_p(n["packed"].data_ptr()), C.c_void_p(rays.data_ptr()), C.c_void_p(z.data_ptr()),
                                      count, 1, 0, C.c_void_p(raw.data_ptr()), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _capi.OK
    return raw[:, 3]


@pytest.mark.parametrize("tag", ["d2", "d5", "d16", "d13", "object"])
def test_device_points_are_the_reference_bits(tag):
    from intrinsicnerf_amd import kernels
    t, dim, scale, m, want = _grid.box(tag)
    got = kernels.grid_points(t.to(DEV), scale, m)
    assert tuple(got.shape) == (dim ** 3, 3) and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    got = kernels.grid_points(t.to(DEV), scale, m, dim ** 3 - 5, 5)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want[-5:].view(np.uint32))


def test_device_points_equal_the_host_entry_point_at_dim_33():
    from intrinsicnerf_amd import geometry, kernels
    _, _, scale, m, _ = _grid.box("d16")
    t = torch.linspace(-1.0, 1.0, steps=33)
    host = kernels.grid_points(t, scale, m)
    assert tuple(host.shape) == (33 ** 3, 3) and torch.equal(bits(kernels.grid_points(t.to(DEV), scale, m)), bits(host))
    assert torch.equal(bits(kernels.grid_points(t.to(DEV), scale, m, 77, 300)), bits(host[77:377]))
    fx = _grid.fixture()
    pts, sc = geometry.grid_within_bound([-1.0, 1.0], fx["extents_d16"], fx["transform_d16"], 33, device=DEV)
    assert pts.is_cuda and tuple(pts.shape) == (33 ** 3, 1, 3) and torch.equal(bits(pts.reshape(-1, 3)), bits(host))


@pytest.mark.parametrize("count", [1, 127, 128, 129, 2197, 35937])
@pytest.mark.parametrize("tag", ["object", "ssr"])
def test_sigma_has_the_bits_of_encode_mlp(nets, tag, count):
    """ragged last tiles, one tile exactly, and 281 tiles - more than the persistent workgroups, so the tile loop takes a second trip"""
    from intrinsicnerf_amd import kernels
    n = nets[tag]
    t = n["t"] if count <= 2197 else torch.linspace(-1.0, 1.0, steps=33).to(DEV)
    pts = kernels.grid_points(t, n["scale"], n["m"], 0, count)
    occ, sigma = kernels.occupancy_grid(n["desc"], n["packed"], t, n["scale"], n["m"], n["dist"], 0, count, sigma=True)
    want = encode_mlp_sigma(n, pts)
    assert torch.isfinite(sigma).all()
    assert torch.equal(bits(sigma), bits(want))
    # the activation on those bits: relu, times the voxel size, exponential
    ref = 1.0 - torch.exp(-torch.relu(sigma.double()) * float(np.float32(n["dist"])))
    assert float((occ.double() - ref).abs().max()) <= 2.0 ** -22 and bool((occ[sigma <= 0] == 0).all())


@pytest.mark.parametrize("tag", ["object", "ssr"])
def test_values_against_the_reference(whole, tag):
    fx = _grid.fixture()
    occ, sigma = whole[tag]
    _grid.within(sigma.cpu().numpy(), fx[tag + "/sigma32"], f"{tag}: sigma against the reference's fp32")
    _grid.within(occ.cpu().numpy(), fx[tag + "/occ32"], f"{tag}: occupancy against the reference's fp32")
    _grid.within(sigma.cpu().numpy(), fx[tag + "/sigma64"], f"{tag}: sigma against fp64")
    _grid.within(occ.cpu().numpy(), fx[tag + "/occ64"], f"{tag}: occupancy against fp64")


@pytest.mark.parametrize("first,count", [(77, 300), (13 ** 3 - 5, 5)])
@pytest.mark.parametrize("tag", ["object", "ssr"])
def test_sub_ranges_are_slices_of_the_whole_grid(nets, whole, tag, first, count):
    from intrinsicnerf_amd import kernels
    n = nets[tag]
    guard = 16
    occ_buf = torch.full((count + 2 * guard,), -7.0, device=DEV)
    sig_buf = torch.full((count + 2 * guard,), -9.0, device=DEV)
    kernels.occupancy_grid(n["desc"], n["packed"], n["t"], n["scale"], n["m"], n["dist"], first, count,
                           occ=occ_buf[guard:guard + count], sigma=sig_buf[guard:guard + count])
    assert torch.equal(bits(occ_buf[guard:guard + count]), bits(whole[tag][0][first:first + count]))
    assert torch.equal(bits(sig_buf[guard:guard + count]), bits(whole[tag][1][first:first + count]))
    for buf, fill in ((occ_buf, -7.0), (sig_buf, -9.0)):
        assert bool((buf[:guard] == fill).all()) and bool((buf[guard + count:] == fill).all())
    # without sigma_out: the same occupancy
    occ, none = kernels.occupancy_grid(n["desc"], n["packed"], n["t"], n["scale"], n["m"], n["dist"], first, count)
    assert none is None and torch.equal(bits(occ), bits(whole[tag][0][first:first + count]))


@pytest.mark.parametrize("tag", ["object", "ssr"])
def test_nan_density_gives_nan_occupancy(nets, tag):
    import copy
    from intrinsicnerf_amd import kernels, packing
    n = nets[tag]
    net = copy.deepcopy(n["net"])
    with torch.no_grad():
        net.alpha_linear.bias.fill_(float("nan"))
    packed = packing.packed_for_module(net, n["desc"], torch.device(DEV))
    occ, sigma = kernels.occupancy_grid(n["desc"], packed, n["t"], n["scale"], n["m"], n["dist"], 0, 300, sigma=True)
    assert bool(torch.isnan(sigma).all()) and bool(torch.isnan(occ).all())


def far_box():
    """an axis-aligned dim-16 box whose x runs from 0 to 2e4 (the existing range tests' magnitude): lattice slabs i >= 6 lie beyond
    |8 x| = 6e4, slab 5 (x = 6 667) and everything below stay inside - by a factor 4 for the layer outputs of a default-init trunk"""
    t = torch.linspace(-1.0, 1.0, steps=16)
    scale, m = [1.0e4, 1.0, 1.0], [1.0, 0.0, 0.0, 1.0e4, 0.0, 1.0, 0.0, 0.3, 0.0, 0.0, 1.0, -0.2]
    return t, scale, m


@pytest.mark.parametrize("tag", ["object", "ssr"])
def test_range_guard_flags_the_chunks_that_leave_the_range(nets, tag):
    from intrinsicnerf_amd import _capi, kernels
    n = nets[tag]
    t, scale, m = far_box()
    div = n["desc"].xyz_div if tag == "ssr" else 1.0
    scale, m = [scale[0] * div, scale[1], scale[2]], [m[0], m[1], m[2], m[3] * div] + m[4:]      # (the SSR encoder divides first)
    pts = kernels.grid_points(t, scale, m)
    beyond = (pts.abs().max(dim=1)[0] / div * 8.0 > 6.0e4).reshape(-1, 512).any(dim=1)              # per word of 512 points = 4 tiles
    assert beyond.tolist() == [False] * 3 + [True] * 5
    status = torch.zeros(8, dtype=torch.int32, device=DEV)
    kernels.occupancy_grid(n["desc"], n["packed"], t.to(DEV), scale, m, n["dist"], status=status, status_points=512)
    assert [bool(int(w) & _capi.STATUS_F16_RANGE) for w in status.cpu().tolist()] == beyond.tolist()
    # a sub-range: the words are those of the LATTICE index; one word for all: status_points = 0
    status = torch.zeros(8, dtype=torch.int32, device=DEV)
    kernels.occupancy_grid(n["desc"], n["packed"], t.to(DEV), scale, m, n["dist"], 1024, 1024, status=status, status_points=512)
    assert [int(w) for w in status.cpu().tolist()] == [0, 0, 0, 1, 0, 0, 0, 0]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    kernels.occupancy_grid(n["desc"], n["packed"], t.to(DEV), scale, m, n["dist"], 0, 1536, status=status)
    assert int(status.item()) == 0
    kernels.occupancy_grid(n["desc"], n["packed"], t.to(DEV), scale, m, n["dist"], 1536, 128, status=status)
    assert int(status.item()) & _capi.STATUS_F16_RANGE


def test_front_end_evaluates_flagged_chunks_in_exact_fp32(nets, monkeypatch):
    from intrinsicnerf_amd import geometry, kernels
    n = nets["object"]
    t, scale, m = far_box()
    extents = np.array(scale) * 2.0 * 0.9                  # grid_within_bound's scale = extents / (0.9 * 2)
    T = np.eye(4)
    T[:3] = np.array(m).reshape(3, 4)
    assert geometry._scene_scale([-1.0, 1.0], extents).tolist() == scale
    monkeypatch.setattr(geometry, "STATUS_POINTS", 512)
    monkeypatch.setattr(kernels, "_warned_fallback", False)
    with warnings.catch_warnings(record=True) as said:
        warnings.simplefilter("always")
        occ, sigma = geometry.occupancy_grid(n["net"], n["embed"], [-1.0, 1.0], extents, T, 16, n["dist"], return_sigma=True)
    assert any("5 of 8 chunks left the f16 range" in str(w.message) for w in said)
    fused = kernels.occupancy_grid(n["desc"], n["packed"], t.to(DEV), scale, m, n["dist"], sigma=True)
    exact = geometry._sigma_exact(n["net"], n["embed"], None, n["desc"], kernels.grid_points(t.to(DEV), scale, m))
    assert tuple(occ.shape) == (16, 16, 16) and torch.isfinite(occ).all()
    assert torch.equal(bits(sigma.reshape(-1)[:1536]), bits(fused[1][:1536])) and torch.equal(bits(occ.reshape(-1)[:1536]), bits(fused[0][:1536]))
    assert torch.equal(bits(sigma.reshape(-1)[1536:]), bits(exact[1536:]))
    assert torch.equal(bits(occ.reshape(-1)[1536:]), bits(geometry.occupancy_activation(exact[1536:], n["dist"])))


def test_front_ends_return_the_c_call(nets, whole):
    from intrinsicnerf_amd import geometry, ssr
    fx = _grid.fixture()
    for tag, box in (("ssr", "d13"), ("object", "object")):
        n = nets[tag]
        T, extents = (fx["transform_d13"], fx["extents_d13"]) if box == "d13" else (fx["object/transform"], fx["object/extents"])
        occ, sigma = geometry.occupancy_grid(n["net"], n["embed"], [-1.0, 1.0], extents, T, 13, n["dist"], return_sigma=True)
        assert tuple(occ.shape) == tuple(sigma.shape) == (13, 13, 13) and occ.is_cuda
        assert torch.equal(bits(occ.reshape(-1)), bits(whole[tag][0])) and torch.equal(bits(sigma.reshape(-1)), bits(whole[tag][1]))
        chunked = geometry.occupancy_grid(n["net"], n["embed"], [-1.0, 1.0], extents, T, 13, n["dist"], chunk_points=1000)
        assert torch.equal(bits(chunked.reshape(-1)), bits(whole[tag][0]))

    class Trainer(ssr.SSRRenderMixin):
        pass

    tr, n = Trainer(), nets["ssr"]
    tr.ssr_net_fine, tr.embed_fn, tr.embeddirs_fn = n["net"], n["embed"], n["embed_d"]
    tr.near, tr.far, tr.N_importance = float(fx["ssr/near"]), float(fx["ssr/far"]), int(fx["ssr/n_importance"])
    occ = tr.occupancy_grid(fx["extents_d13"], fx["transform_d13"], grid_dim=13)
    assert tuple(occ.shape) == (13, 13, 13) and torch.equal(bits(occ.reshape(-1)), bits(whole["ssr"][0]))


@pytest.mark.parametrize("tag", ["object", "ssr"])
def test_exact_fp32_front_end(nets, tag, monkeypatch):
    """INERF_PRECISION=f32: inerf_grid_points, the exact-fp32 kernel, channel 3, the same activation"""
    from intrinsicnerf_amd import geometry
    monkeypatch.setenv("INERF_PRECISION", "f32")
    fx, n = _grid.fixture(), nets[tag]
    T, extents = (fx["transform_d13"], fx["extents_d13"]) if tag == "ssr" else (fx["object/transform"], fx["object/extents"])
    occ, sigma = geometry.occupancy_grid(n["net"], n["embed"], [-1.0, 1.0], extents, T, 13, n["dist"], return_sigma=True, chunk_points=1000)
    _grid.within(sigma.cpu().numpy(), fx[tag + "/sigma32"], f"{tag}, f32: sigma against the reference's fp32")
    _grid.within(occ.cpu().numpy(), fx[tag + "/occ32"], f"{tag}, f32: occupancy against the reference's fp32")


def test_other_width_goes_layer_by_layer():
    """W = 128 is outside the fused kernels: the layer kernels on inerf_grid_points' lattice, against the module's own forward in fp64"""
    import copy
    from intrinsicnerf_amd import geometry, object_level as ol
    fx = _grid.fixture()
    embed, ch = ol.get_embedder(10, 0)
    embed_d, ch_d = ol.get_embedder(4, 0)
    torch.manual_seed(5)
    net = ol.NeRF(D=8, W=128, input_ch=ch, input_ch_views=ch_d, output_ch=5, skips=[4], use_viewdirs=True).requires_grad_(False)
    with torch.no_grad():
        net.alpha_linear.weight.mul_(4.0)
    assert net.fused_desc() is None
    dist = float(fx["object/dist"])
    occ, sigma = geometry.occupancy_grid(copy.deepcopy(net).to(DEV), embed, [-1.0, 1.0], fx["object/extents"], fx["object/transform"], 13, dist,
                                         return_sigma=True)
    pts = torch.from_numpy(fx["object/points"]).double()
    with torch.no_grad():
        want = net.double()(torch.cat([embed(pts), embed_d(torch.zeros_like(pts))], -1))[:, 3]
    assert tuple(occ.shape) == (13, 13, 13)
    _grid.within(sigma.cpu().numpy(), want.numpy(), "W = 128: sigma against fp64")
    _grid.within(occ.cpu().numpy(), geometry.occupancy_activation(want, dist).numpy(), "W = 128: occupancy against fp64")


def test_two_launches_give_the_same_bits(nets, whole):
    from intrinsicnerf_amd import kernels
    for tag, n in nets.items():
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            again = kernels.occupancy_grid(n["desc"], n["packed"], n["t"], n["scale"], n["m"], n["dist"], sigma=True)
        stream.synchronize()
        assert torch.equal(bits(again[0]), bits(whole[tag][0])) and torch.equal(bits(again[1]), bits(whole[tag][1]))
