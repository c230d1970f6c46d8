"""CPU: mesh extraction's grid entry points (inerf_grid_points, inerf_grid_points_host, inerf_occupancy_grid) - the host evaluation of
grid_point() reproduces the reference's lattice bit for bit (tests/golden/grid_query.npz), geometry.make_3D_grid / grid_within_bound on
CPU tensors return the reference's tensors, arguments are validated before anything touches a device, and header, binding and library
agree on the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
import _grid

NEW = ("inerf_grid_points", "inerf_grid_points_host", "inerf_occupancy_grid")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__
    __graft_entry__.build()
    from intrinsicnerf_amd import _capi
    return _capi


def host_points(capi, tag, first=0, count=None):
    t, dim, scale, m, want = _grid.box(tag)
    count = dim ** 3 - first if count is None else count
    out = np.full((count + 2, 3), 7.0, np.float32)                 # (a guard row on either side)
    sc, mm = _grid.c_arrays(scale, m)
    rc = capi.lib().inerf_grid_points_host(C.c_void_p(t.data_ptr()), dim, sc, mm, first, count, C.c_void_p(out[1:].ctypes.data))
    assert rc == capi.OK
    assert (out[0] == 7.0).all() and (out[-1] == 7.0).all()
    return out[1:-1], want


def test_header_binding_and_library_agree_on_the_abi(capi):
    text = open(os.path.join(REPO, "include", "inerf.h")).read()
    header = int(re.search(r"#define INERF_ABI_VERSION (\d+)", text).group(1))
    assert header == capi.ABI_VERSION == capi.lib().inerf_abi_version()


def test_header_and_binding_declare_the_grid_entry_points(capi):
    text = open(os.path.join(REPO, "include", "inerf.h")).read()
    assert int(re.search(r"#define INERF_ABI_VERSION (\d+)", text).group(1)) >= 40018
    assert int(re.search(r"#define INERF_MAX_GRID_DIM (\d+)", text).group(1)) == capi.MAX_GRID_DIM == 1024
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert decl, f"{name} is not declared in include/inerf.h"
        assert name in capi.SYMBOLS and len(capi.SYMBOLS[name][1]) == len(decl.group(1).split(",")), name
        assert getattr(capi.lib(), name) is not None


@pytest.mark.parametrize("tag", ["d2", "d5", "d16", "d13", "object"])
def test_host_points_are_the_reference_bits(capi, tag):
    got, want = host_points(capi, tag)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_host_points_of_a_sub_range(capi):
    got, want = host_points(capi, "d16", 77, 300)
    assert np.array_equal(got.view(np.uint32), want[77:377].view(np.uint32))
    got, want = host_points(capi, "d16", 16 ** 3 - 5, 5)
    assert np.array_equal(got.view(np.uint32), want[-5:].view(np.uint32))


def test_make_3D_grid_on_the_cpu_is_the_reference(capi):
    from intrinsicnerf_amd import geometry
    fx = _grid.fixture()
    for tag in ("d2", "d5", "d16", "d13"):
        dim = int(tag[1:])
        rng = [float(v) for v in fx["occ_range"]]
        pts, scale = geometry.grid_within_bound(rng, fx["extents_" + tag], fx["transform_" + tag], dim)
        assert tuple(pts.shape) == (dim ** 3, 1, 3) and pts.dtype == torch.float32 and pts.device.type == "cpu"
        assert np.array_equal(pts.numpy().reshape(-1, 3).view(np.uint32), fx["points_" + tag].view(np.uint32))
        assert np.array_equal(scale.numpy(), fx["scale_" + tag]) and scale.dtype == torch.float32
        grid = geometry.make_3D_grid(rng, dim, transform=torch.from_numpy(fx["transform_" + tag]).float(), scale=torch.from_numpy(fx["scale_" + tag]))
        assert tuple(grid.shape) == (dim, dim, dim, 3)
        assert np.array_equal(grid.numpy().reshape(-1, 3).view(np.uint32), fx["points_" + tag].view(np.uint32))
    # without a transform: the scaled lattice itself, 'ij' order
    t = torch.linspace(-1.0, 1.0, steps=5)
    s = torch.tensor([2.0, 3.0, 0.5])
    grid = geometry.make_3D_grid([-1.0, 1.0], 5, scale=s)
    want = torch.stack(torch.meshgrid(t, t, t, indexing="ij"), dim=3) * s
    assert torch.equal(grid, want)


def test_argument_rules(capi):
    lib = capi.lib()
    buf = (C.c_float * 64)()                      # never dereferenced by a device: every device call below returns before a launch
    p = C.cast(buf, C.c_void_p)
    sc, m = (C.c_float * 3)(1., 1., 1.), (C.c_float * 12)(1., 0., 0., 0., 0., 1., 0., 0., 0., 0., 1., 0.)
    for fn, tail in ((lib.inerf_grid_points, (None,)), (lib.inerf_grid_points_host, ())):
        assert fn(p, 4, sc, m, 0, 0, None, *tail) == capi.OK                       # an empty range needs no output
        assert fn(p, 4, sc, m, 64, 0, None, *tail) == capi.OK
        assert fn(None, 4, sc, m, 0, 8, p, *tail) == capi.E_INVALID
        assert fn(p, 4, None, m, 0, 8, p, *tail) == capi.E_INVALID
        assert fn(p, 4, sc, None, 0, 8, p, *tail) == capi.E_INVALID
        assert fn(p, 4, sc, m, 0, 8, None, *tail) == capi.E_INVALID
        assert fn(p, 1, sc, m, 0, 1, p, *tail) == capi.E_INVALID                   # 2 <= dim <= 1024
        assert fn(p, 1025, sc, m, 0, 8, p, *tail) == capi.E_INVALID
        assert fn(p, 4, sc, m, -1, 8, p, *tail) == capi.E_INVALID
        assert fn(p, 4, sc, m, 0, -1, p, *tail) == capi.E_INVALID
        assert fn(p, 4, sc, m, 60, 5, p, *tail) == capi.E_INVALID                  # first + count <= dim^3
        assert fn(p, 4, sc, m, 1, (1 << 63) - 1, p, *tail) == capi.E_INVALID       # (no overflow into range)
    f16, f32 = capi.net_desc(capi.VARIANT_OBJECT, precision=capi.PREC_F16X3), capi.net_desc(capi.VARIANT_OBJECT, precision=capi.PREC_F32)
    ssr = capi.net_desc(capi.VARIANT_SSR, 28, xyz_div=10.0, precision=capi.PREC_F16X3)
    occ = lib.inerf_occupancy_grid
    for d in (f16, ssr):
        assert occ(d, p, p, 4, sc, m, 0.1, 0, 0, None, None, None, 0, None) == capi.OK
        assert occ(d, None, p, 4, sc, m, 0.1, 0, 8, p, None, None, 0, None) == capi.E_INVALID
        assert occ(d, p, None, 4, sc, m, 0.1, 0, 8, p, None, None, 0, None) == capi.E_INVALID
        assert occ(d, p, p, 4, None, m, 0.1, 0, 8, p, None, None, 0, None) == capi.E_INVALID
        assert occ(d, p, p, 4, sc, None, 0.1, 0, 8, p, None, None, 0, None) == capi.E_INVALID
        assert occ(d, p, p, 4, sc, m, 0.1, 0, 8, None, p, None, 0, None) == capi.E_INVALID
        assert occ(d, p, p, 1, sc, m, 0.1, 0, 1, p, None, None, 0, None) == capi.E_INVALID
        assert occ(d, p, p, 1025, sc, m, 0.1, 0, 8, p, None, None, 0, None) == capi.E_INVALID
        assert occ(d, p, p, 4, sc, m, 0.1, -1, 8, p, None, None, 0, None) == capi.E_INVALID
        assert occ(d, p, p, 4, sc, m, 0.1, 0, -8, p, None, None, 0, None) == capi.E_INVALID
        assert occ(d, p, p, 4, sc, m, 0.1, 57, 8, p, None, None, 0, None) == capi.E_INVALID
        assert occ(d, p, p, 4, sc, m, 0.1, 0, 8, p, None, p, -1, None) == capi.E_INVALID
    assert occ(None, p, p, 4, sc, m, 0.1, 0, 8, p, None, None, 0, None) == capi.E_INVALID
    assert occ(f32, p, p, 4, sc, m, 0.1, 0, 8, p, None, None, 0, None) == capi.E_UNSUPPORTED      # the exact-fp32 kernels have no such mode
    bad = capi.net_desc(capi.VARIANT_OBJECT, l_xyz=11, precision=capi.PREC_F16X3)
    assert occ(bad, p, p, 4, sc, m, 0.1, 0, 8, p, None, None, 0, None) == capi.E_UNSUPPORTED


def test_launchers_refuse_what_they_cannot_take():
    from intrinsicnerf_amd import geometry, kernels, object_level as ol
    t = torch.linspace(-1.0, 1.0, steps=4)
    with pytest.raises(ValueError):
        kernels.grid_points(t, [1.0, 1.0], [0.0] * 12)
    with pytest.raises(ValueError):
        kernels.grid_points(t.double(), [1.0] * 3, [0.0] * 12)
    with pytest.raises(RuntimeError, match="HIP device"):
        kernels.occupancy_grid(None, t, t, [1.0] * 3, [0.0] * 12, 0.1)
    embed, ch = ol.get_embedder(10, 0)
    net = ol.NeRF(input_ch=ch, input_ch_views=27, use_viewdirs=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        geometry.occupancy_grid(net, embed, [-1.0, 1.0], np.ones(3), np.eye(4), 4, 0.1)
    with pytest.raises(ValueError):
        geometry.occupancy_grid(net, embed, [-1.0, 1.0], np.ones(3), np.eye(4), 1, 0.1)
