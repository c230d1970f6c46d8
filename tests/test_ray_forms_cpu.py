"""CPU: the ray-form entry points (inerf_gen_rays_ndc, inerf_assemble_rays, inerf_ndc_rays) - header, binding and library agree,
arguments are validated before anything touches a device, the front-end's NDC coefficients are the reference's two scalar
expressions, and render() / ndc_rays() on CPU tensors still are the reference's expressions, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

NEW = ("inerf_gen_rays_ndc", "inerf_assemble_rays", "inerf_ndc_rays")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__
    __graft_entry__.build()
    from intrinsicnerf_amd import _capi
    return _capi


def test_header_binding_and_library_agree_on_the_ray_forms(capi):
    text = open(os.path.join(REPO, "include", "inerf.h")).read()
    header = int(re.search(r"#define INERF_ABI_VERSION (\d+)", text).group(1))
    assert header == capi.ABI_VERSION == capi.lib().inerf_abi_version() and header >= 40017
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = capi.lib()
    for name in NEW:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert decl, f"{name} is not declared in include/inerf.h"
        n_args = len(decl.group(1).split(","))
        assert name in capi.SYMBOLS and len(capi.SYMBOLS[name][1]) == n_args, name
        assert getattr(lib, name) is not None
    body = code[code.index("typedef struct inerf_ndc"):code.index("} inerf_ndc;")]
    assert re.findall(r"([a-z_]+)\s*[,;]", body[body.index("{"):] + ";") == [f[0] for f in capi.Ndc._fields_]
    assert C.sizeof(capi.Ndc) == 12 and all(f[1] is C.c_float for f in capi.Ndc._fields_)


def test_argument_rules(capi):
    lib = capi.lib()
    ndc = C.byref(capi.Ndc(-1.0, -1.5, 1.0))
    buf = (C.c_float * 64)()                      # never dereferenced: every call below returns before a launch
    p = C.cast(buf, C.c_void_p)
    # an empty batch is fine, whatever the pointers
    assert lib.inerf_gen_rays_ndc(None, 12, None, 0, 4, 4, 1., 1., 2., 2., 0., 1., 1, ndc, None, None) == capi.OK
    assert lib.inerf_gen_rays_ndc(None, 12, None, 1, 0, 4, 1., 1., 2., 2., 0., 1., 1, None, None, None) == capi.OK
    assert lib.inerf_assemble_rays(None, 3, None, 3, 0, 0., 1., None, None, None) == capi.OK
    assert lib.inerf_ndc_rays(None, 3, None, 3, 0, None, None, None, None) == capi.OK
    # null pointers, negative sizes, strides below one row
    assert lib.inerf_gen_rays_ndc(None, 12, None, 1, 4, 4, 1., 1., 2., 2., 0., 1., 1, ndc, p, None) == capi.E_INVALID
    assert lib.inerf_gen_rays_ndc(p, 12, None, 1, 4, 4, 1., 1., 2., 2., 0., 1., 1, ndc, None, None) == capi.E_INVALID
    assert lib.inerf_gen_rays_ndc(p, 12, None, -1, 4, 4, 1., 1., 2., 2., 0., 1., 1, ndc, p, None) == capi.E_INVALID
    assert lib.inerf_gen_rays_ndc(p, 11, None, 1, 4, 4, 1., 1., 2., 2., 0., 1., 1, ndc, p, None) == capi.E_INVALID
    assert lib.inerf_assemble_rays(None, 3, p, 3, 4, 0., 1., None, p, None) == capi.E_INVALID
    assert lib.inerf_assemble_rays(p, 3, None, 3, 4, 0., 1., None, p, None) == capi.E_INVALID
    assert lib.inerf_assemble_rays(p, 3, p, 3, 4, 0., 1., ndc, None, None) == capi.E_INVALID
    assert lib.inerf_assemble_rays(p, 3, p, 3, -4, 0., 1., None, p, None) == capi.E_INVALID
    assert lib.inerf_assemble_rays(p, 2, p, 3, 4, 0., 1., None, p, None) == capi.E_INVALID
    assert lib.inerf_assemble_rays(p, 11, p, 0, 4, 0., 1., None, p, None) == capi.E_INVALID
    assert lib.inerf_ndc_rays(p, 3, p, 3, 4, None, p, p, None) == capi.E_INVALID                     # ndc_rays without coefficients
    assert lib.inerf_ndc_rays(None, 3, p, 3, 4, ndc, p, p, None) == capi.E_INVALID
    assert lib.inerf_ndc_rays(p, 3, p, 3, 4, ndc, p, None, None) == capi.E_INVALID
    assert lib.inerf_ndc_rays(p, 3, p, 3, 4, ndc, None, p, None) == capi.E_INVALID
    assert lib.inerf_ndc_rays(p, 3, p, 2, 4, ndc, p, p, None) == capi.E_INVALID
    assert lib.inerf_ndc_rays(p, 3, p, 3, -1, ndc, p, p, None) == capi.E_INVALID
    # more workgroups of 256 rays than a grid holds
    too_many = ((1 << 31) - 1) * 256 + 1
    assert lib.inerf_assemble_rays(p, 3, p, 3, too_many, 0., 1., None, p, None) == capi.E_UNSUPPORTED
    assert lib.inerf_ndc_rays(p, 3, p, 3, too_many, ndc, p, p, None) == capi.E_UNSUPPORTED
    assert lib.inerf_gen_rays_ndc(p, 12, None, (1 << 31) - 1, 1 << 15, 1 << 15, 1., 1., 2., 2., 0., 1., 1, ndc, p, None) == capi.E_UNSUPPORTED
    assert lib.inerf_gen_rays(p, 12, None, (1 << 31) - 1, 1 << 15, 1 << 15, 1., 1., 2., 2., 0., 1., 1, p, None) == capi.E_UNSUPPORTED


def test_launchers_refuse_cpu_tensors():
    from intrinsicnerf_amd import kernels
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        kernels.assemble_rays(o, d, 0., 1.)
    with pytest.raises(RuntimeError, match="HIP device"):
        kernels.ndc_rays(o, d, (-1., -1., 1.))
    with pytest.raises(ValueError):
        kernels.ndc_rays(o, d, None)
    assert not kernels.rows3_viewable(o)


@pytest.mark.parametrize("W,H", [(504, 378), (16, 12)])
@pytest.mark.parametrize("kind", [float, np.float32, np.float64])
def test_ndc_coefficients_are_the_reference_expressions(capi, kind, W, H):
    """run_nerf_helpers.py:387-393 with the caller's own objects, then ONE rounding to fp32 - what ATen does with the scalar."""
    from intrinsicnerf_amd import kernels, object_level as ol
    focal = kind(407.5653) if W == 504 else kind(12.93859683)
    sx, sy, near = ol._ndc_coefficients(H, W, focal, 1.)
    want_x, want_y = -1. / (W / (2. * focal)), -1. / (H / (2. * focal))
    assert type(sx) is type(want_x) and type(sy) is type(want_y)
    assert sx == want_x and sy == want_y and near == 1.
    coeff = kernels._ndc_arg((sx, sy, 0.7))
    x = torch.tensor([1.0, 3.0, -0.3333333])
    assert (x * coeff.sx).tolist() == (want_x * x).tolist() and (x * coeff.sy).tolist() == (want_y * x).tolist()
    assert coeff.near_plane == np.float32(0.7) and 2.0 * coeff.near_plane == float(np.float32(2. * 0.7))


def test_cpu_tensors_keep_the_reference_expressions(monkeypatch):
    """render() and ndc_rays() on CPU tensors: rays_generators.npz's render_rays_ndc, render_rays_given, ndc_o, ndc_d bit for bit,
    and no launcher is called."""
    from intrinsicnerf_amd import kernels, object_level as ol
    fx = load_golden("rays_generators")
    H, W, K, focal = int(fx["H"]), int(fx["W"]), fx["K"], float(fx["focal"])
    c2w = torch.from_numpy(fx["c2w"])

    def forbidden(*a, **k):
        raise AssertionError("a HIP launcher was called for CPU tensors")

    for name in ("gen_rays", "assemble_rays", "ndc_rays"):
        monkeypatch.setattr(kernels, name, forbidden)
    ro, rd = torch.from_numpy(fx["get_rays_o"]), torch.from_numpy(fx["get_rays_d"])
    o2, d2 = ol.ndc_rays(H, W, focal, 1.0, ro + torch.tensor([0.0, 0.0, 4.0]), rd)
    assert np.array_equal(o2.numpy(), fx["ndc_o"]) and np.array_equal(d2.numpy(), fx["ndc_d"])
    captured = {}

    def spy(rays_flat, chunk=1024 * 32, **kw):
        captured["rays"] = rays_flat.clone()
        n = rays_flat.shape[0]
        z3, z1 = torch.zeros(n, 3), torch.zeros(n)
        return {"rgb_map": z3, "disp_map": z1, "acc_map": z1, "albedo_map": z3, "shading_map": z1, "residual_map": z3}

    monkeypatch.setattr(ol, "batchify_rays", spy)
    out = ol.render(H, W, K, chunk=64, c2w=c2w, near=2.0, far=6.0, use_viewdirs=True, ndc=True)
    assert np.array_equal(captured["rays"].numpy(), fx["render_rays_ndc"]) and tuple(out[0].shape) == (H, W, 3)
    given = (torch.from_numpy(fx["given_o"]), torch.from_numpy(fx["given_d"]))
    out = ol.render(H, W, K, chunk=64, rays=given, ndc=False, near=0.5, far=3.0, use_viewdirs=True)
    assert np.array_equal(captured["rays"].numpy(), fx["render_rays_given"]) and tuple(out[0].shape) == (10, 3)
    ol.render(H, W, K, chunk=64, rays=torch.stack(given), ndc=False, near=0.5, far=3.0, use_viewdirs=True)      # batch_rays [2, N, 3]
    assert np.array_equal(captured["rays"].numpy(), fx["render_rays_given"])
