"""CPU: the vertex-colour pass of mesh extraction (inerf_vertex_rays, inerf_vertex_rays_host, inerf_vertex_colours and their Python
front-ends).  The host evaluation of the vertex ray form reproduces torch's CPU tensors bit for bit (tests/golden/vertex_rays.npz:
float64 and float32 inputs, near_t = 2.0, 0.0, 0.3), arguments are validated before anything touches a device, and the mixin's
vertex_colours refuses training mode and restores the attributes it changes."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

NEW = ("inerf_vertex_rays", "inerf_vertex_rays_host", "inerf_vertex_colours")
SENTINEL = 7.0


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__
    __graft_entry__.build()
    from intrinsicnerf_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def fx():
    return load_golden("vertex_rays")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host_rays(capi, vertices, normals, near, far, near_t):
    """inerf_vertex_rays_host on numpy arrays [n, 3] of any row stride, into a buffer with a guard row on either side."""
    n = vertices.shape[0]
    assert vertices.dtype == normals.dtype and vertices.strides[1] == vertices.itemsize and normals.strides[1] == normals.itemsize
    dtype = capi.DTYPE_F64 if vertices.dtype == np.float64 else capi.DTYPE_F32
    stride = lambda a: max(a.strides[0] // a.itemsize, 3) if n > 1 else 3
    out = np.full((n + 2, 11), SENTINEL, np.float32)
    rc = capi.lib().inerf_vertex_rays_host(C.c_void_p(vertices.ctypes.data), stride(vertices), C.c_void_p(normals.ctypes.data), stride(normals),
                                           n, dtype, near, far, near_t, C.c_void_p(out[1:].ctypes.data))
    assert rc == capi.OK
    assert (out[0] == SENTINEL).all() and (out[-1] == SENTINEL).all()
    return out[1:-1]


def test_header_binding_and_library_declare_the_entry_points(capi):
    text = open(os.path.join(REPO, "include", "inerf.h")).read()
    header = int(re.search(r"#define INERF_ABI_VERSION (\d+)", text).group(1))
    assert header == capi.ABI_VERSION == capi.lib().inerf_abi_version() and header >= 40021
    assert int(re.search(r"#define INERF_DTYPE_F32 (\d+)", text).group(1)) == capi.DTYPE_F32
    assert int(re.search(r"#define INERF_DTYPE_F64 (\d+)", text).group(1)) == capi.DTYPE_F64
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert decl, f"{name} is not declared in include/inerf.h"
        assert name in capi.SYMBOLS and len(capi.SYMBOLS[name][1]) == len(decl.group(1).split(",")), name
        assert getattr(capi.lib(), name) is not None


def test_new_sources_and_their_headers_are_in_the_build_digest(capi):
    """(tests/test_capi_cpu.py walks every #include of csrc/; here: the two files this entry point added are among what it walks)"""
    from intrinsicnerf_amd import _build
    headers = {os.path.realpath(h) for h in _build.HEADERS}
    assert "mesh.hip" in _build.SOURCES and os.path.realpath(os.path.join(_build.CSRC, "sem_label.h")) in headers
    for src in ("mesh.hip", "eval.hip", "frame_ops.hip"):
        for name in re.findall(r'#include "([^"]+)"', open(os.path.join(_build.CSRC, src)).read()):
            assert os.path.realpath(os.path.join(_build.CSRC, name)) in headers, (src, name)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [0, 1, 3, 100])
def test_host_rays_are_the_reference_bits(capi, fx, dt, n):
    v, m = fx["vertices_" + dt][:n], fx["normals_" + dt][:n]
    for i, near_t in enumerate(fx["near_t"]):
        got = host_rays(capi, v, m, float(fx["near"]), float(fx["far"]), float(near_t))
        want = fx[f"rays_{dt}_{i}"][:n]
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (dt, n, near_t)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_host_rays_of_strided_rows(capi, fx, dt):
    """vertices as columns 1:4 of a [n, 5] array, normals as columns 2:5 of a [n, 7] one: row strides 5 and 7 elements."""
    v, m = fx["vertices_" + dt], fx["normals_" + dt]
    n = v.shape[0]
    wide_v, wide_m = np.full((n, 5), 99.0, v.dtype), np.full((n, 7), -99.0, m.dtype)
    wide_v[:, 1:4], wide_m[:, 2:5] = v, m
    for k in (1, 3, n):
        got = host_rays(capi, wide_v[:k, 1:4], wide_m[:k, 2:5], float(fx["near"]), float(fx["far"]), 2.0)
        assert np.array_equal(bits(got), bits(fx[f"rays_{dt}_0"][:k])), (dt, k)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("n", [0, 1, 3, 100])
def test_geometry_vertex_rays_on_the_cpu(capi, fx, dt, n):
    from intrinsicnerf_amd import geometry
    v, m = fx["vertices_" + dt][:n], fx["normals_" + dt][:n]
    for i, near_t in enumerate(fx["near_t"]):
        want = fx[f"rays_{dt}_{i}"][:n]
        for vv, mm in ((v, m), (torch.from_numpy(v.copy()), torch.from_numpy(m.copy()))):            # numpy and torch inputs
            got = geometry.vertex_rays(vv, mm, near_t=float(near_t))
            assert got.dtype == torch.float32 and got.device.type == "cpu" and tuple(got.shape) == (n, 11)
            assert np.array_equal(bits(got.numpy()), bits(want)), (dt, n, near_t)
    if n == 100:                                                                                     # strided views, and mixed dtypes
        wide = np.full((n, 6), 5.0, v.dtype)
        wide[:, 0:3], wide[:, 3:6] = v, m
        got = geometry.vertex_rays(wide[:, 0:3], torch.from_numpy(wide)[:, 3:6])
        assert np.array_equal(bits(got.numpy()), bits(fx[f"rays_{dt}_0"]))
        got = geometry.vertex_rays(fx["vertices_f64"], fx["normals_f32"])
        assert np.array_equal(bits(got.numpy()), bits(fx["rays_f32_0"]))


def test_vertex_rays_argument_rules(capi):
    lib = capi.lib()
    buf = (C.c_double * 64)()                     # never dereferenced by a device: every device call below returns before a launch
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)
    for fn, tail in ((lib.inerf_vertex_rays, (None,)), (lib.inerf_vertex_rays_host, ())):
        for dtype in (capi.DTYPE_F32, capi.DTYPE_F64):
            assert fn(None, 3, None, 3, 0, dtype, 0.1, 10.0, 2.0, None, *tail) == capi.OK                # n == 0: nothing to do
            assert fn(p, 3, p, 3, -1, dtype, 0.1, 10.0, 2.0, p, *tail) == capi.E_INVALID
            assert fn(None, 3, p, 3, 4, dtype, 0.1, 10.0, 2.0, p, *tail) == capi.E_INVALID
            assert fn(p, 3, None, 3, 4, dtype, 0.1, 10.0, 2.0, p, *tail) == capi.E_INVALID
            assert fn(p, 3, p, 3, 4, dtype, 0.1, 10.0, 2.0, None, *tail) == capi.E_INVALID
            assert fn(p, 2, p, 3, 4, dtype, 0.1, 10.0, 2.0, p, *tail) == capi.E_INVALID                 # rows of three
            assert fn(p, 3, p, 2, 4, dtype, 0.1, 10.0, 2.0, p, *tail) == capi.E_INVALID
        for dtype in (-1, 2, 7):
            assert fn(p, 3, p, 3, 4, dtype, 0.1, 10.0, 2.0, p, *tail) == capi.E_INVALID                 # neither INERF_DTYPE_*
        assert fn(odd, 3, p, 3, 4, capi.DTYPE_F64, 0.1, 10.0, 2.0, p, *tail) == capi.E_INVALID          # doubles at an odd float
        assert fn(p, 3, odd, 3, 4, capi.DTYPE_F64, 0.1, 10.0, 2.0, p, *tail) == capi.E_INVALID
    assert lib.inerf_vertex_rays(p, 3, p, 3, ((1 << 31) - 1) * 256 + 1, capi.DTYPE_F32, 0.1, 10.0, 2.0, p, None) == capi.E_UNSUPPORTED
    out = (C.c_float * 12)()
    assert lib.inerf_vertex_rays_host(odd, 3, odd, 3, 1, capi.DTYPE_F32, 0.1, 10.0, 2.0, C.cast(out, C.c_void_p)) == capi.OK    # floats: 4 bytes


def test_vertex_colours_argument_rules(capi):
    fn = capi.lib().inerf_vertex_colours
    buf = (C.c_float * 64)()                      # never dereferenced: every call below returns before a launch
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 2)
    assert fn(p, 3, p, 28, 8, 28, p, p, None, None) == capi.E_INVALID                  # both sources
    assert fn(None, 3, None, 28, 8, 28, p, p, None, None) == capi.E_INVALID            # neither
    assert fn(None, 0, None, 0, 0, 28, p, p, None, None) == capi.E_INVALID             # ... also for an empty batch
    assert fn(p, 3, None, 0, -1, 0, None, p, None, None) == capi.E_INVALID             # n < 0, either mode
    assert fn(None, 0, p, 28, -1, 28, p, p, None, None) == capi.E_INVALID
    assert fn(p, 2, None, 0, 8, 0, None, p, None, None) == capi.E_INVALID              # rows of three
    assert fn(None, 0, p, 27, 8, 28, p, p, None, None) == capi.E_INVALID               # a row narrower than its classes
    for c in (0, -3, capi.MAX_CLASSES + 1):
        assert fn(None, 0, p, 512, 8, c, p, p, None, None) == capi.E_UNSUPPORTED       # 1 <= n_classes <= INERF_MAX_CLASSES
        assert fn(None, 0, p, 512, 0, c, p, p, None, None) == capi.E_UNSUPPORTED       # checked for an empty batch too
    assert fn(p, 3, None, 0, 0, 0, None, None, None, None) == capi.OK                  # n == 0: nothing to do, whatever the outputs
    assert fn(None, 0, p, 28, 0, 28, None, None, None, None) == capi.OK
    assert fn(p, 3, None, 0, 8, 0, None, None, None, None) == capi.E_INVALID           # no output
    assert fn(None, 0, p, 28, 8, 28, p, None, None, None) == capi.E_INVALID
    assert fn(None, 0, p, 28, 8, 28, None, p, None, None) == capi.E_INVALID            # semantic mode without a map
    assert fn(odd, 3, None, 0, 8, 0, None, p, None, None) == capi.E_INVALID            # misaligned floats / labels
    assert fn(None, 0, odd, 28, 8, 28, p, p, None, None) == capi.E_INVALID
    assert fn(None, 0, p, 28, 8, 28, p, p, odd, None) == capi.E_INVALID


def test_python_front_ends_validate_before_a_device(capi, fx):
    from intrinsicnerf_amd import geometry, kernels
    v, m = fx["vertices_f32"], fx["normals_f32"]

    def never(rays):
        raise AssertionError("render_rays must not be reached")

    for bad_v, bad_m in ((v, m[:50]), (v[:, :2], m[:, :2]), (v.reshape(-1), m.reshape(-1)), (v[None], m[None])):
        with pytest.raises(ValueError):
            geometry.vertex_rays(bad_v, bad_m)
        with pytest.raises(ValueError):
            geometry.vertex_colours(never, bad_v, bad_m)
    with pytest.raises(ValueError):
        geometry.vertex_rays(np.ones((4, 3), np.float16), np.ones((4, 3), np.float16))
    with pytest.raises(ValueError):
        geometry.vertex_rays(v.astype(np.int64), m.astype(np.int64))
    with pytest.raises(ValueError, match="colour_map"):
        geometry.vertex_colours(never, v, m, sem=True)                                  # sem without a map
    for bad_map in (np.zeros((5, 4), np.uint8), np.zeros(15, np.uint8), np.zeros((0, 3), np.uint8), np.zeros((2, 5, 3), np.uint8),
                    torch.zeros(capi.MAX_CLASSES + 1, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="colour_map"):
            geometry.vertex_colours(never, v, m, sem=True, colour_map=bad_map)
    with pytest.raises(ValueError):
        geometry.vertex_colours(never, v, m, chunk=0)
    with pytest.raises(ValueError):
        geometry.vertex_colours(never, v, m, return_labels=True)                        # labels exist in semantic mode only
    # the tensor launchers
    tv, tm = torch.from_numpy(v.copy()), torch.from_numpy(m.copy())
    with pytest.raises(ValueError):
        kernels.vertex_rays(tv, tm[:7])
    with pytest.raises(ValueError):
        kernels.vertex_rays(tv, tm.double())
    with pytest.raises(ValueError):
        kernels.vertex_rays(tv.t().contiguous().t(), tm)                                 # rows without unit stride
    with pytest.raises(ValueError):
        kernels.vertex_rays(tv.half(), tm.half())
    rgb, logits, cmap = torch.zeros(8, 3), torch.zeros(8, 5), torch.zeros(5, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        kernels.vertex_colours(rgb=rgb, logits=logits, colour_map=cmap)
    with pytest.raises(ValueError):
        kernels.vertex_colours()
    with pytest.raises(ValueError):
        kernels.vertex_colours(rgb=torch.zeros(8, 4))
    with pytest.raises(ValueError):
        kernels.vertex_colours(rgb=rgb.double())
    with pytest.raises(ValueError):
        kernels.vertex_colours(rgb=rgb, out=torch.zeros(7, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        kernels.vertex_colours(rgb=rgb, out=torch.zeros(8, 3))
    with pytest.raises(ValueError):
        kernels.vertex_colours(logits=logits)                                            # no map
    with pytest.raises(ValueError):
        kernels.vertex_colours(logits=logits, colour_map=torch.zeros(4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        kernels.vertex_colours(logits=logits, colour_map=cmap.float())
    with pytest.raises(ValueError):
        kernels.vertex_colours(logits=logits, colour_map=cmap, labels=torch.zeros(8, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        kernels.vertex_colours(rgb=rgb)                                                  # valid, but on the CPU: no eager fallback


def test_mixin_refuses_training_mode_and_restores_its_attributes(capi, fx, monkeypatch):
    from intrinsicnerf_amd import geometry, ssr
    v, m = fx["vertices_f64"], fx["normals_f64"]

    class Stub(ssr.SSRRenderMixin):
        """a render_rays that records the two attributes it is called under, then raises"""
        seen = []

        def render_rays(self, rays):
            assert tuple(rays.shape) == (100, 11)
            self.seen.append((self.return_raw, self.check_numerics))
            raise FloatingPointError("render failed")

    t = Stub()
    t.training = True
    with pytest.raises(RuntimeError, match="eval mode"):
        t.vertex_colours(v, m)
    assert t.seen == []
    t.training = False
    # the device half of geometry.vertex_colours is replaced: rays on the CPU, straight into render_rays
    calls = []

    def cpu_pass(render_rays, vertices, normals, **kw):
        calls.append(kw)
        return render_rays(geometry.vertex_rays(vertices, normals, kw["near"], kw["far"], kw["near_t"]))

    monkeypatch.setattr(geometry, "vertex_colours", cpu_pass)
    for raw, numerics in ((True, True), (False, True), (True, False)):
        t.return_raw, t.check_numerics = raw, numerics
        with pytest.raises(FloatingPointError):
            t.vertex_colours(v, m, near_t=0.3)
        assert (t.return_raw, t.check_numerics) == (raw, numerics)
        assert t.seen[-1] == (False, False)
    assert calls[-1]["near"] == 0.1 and calls[-1]["far"] == 10.0 and calls[-1]["near_t"] == 0.3 and calls[-1]["sem"] is False
    # the map defaults to self.valid_colour_map, and an explicit one wins
    t.valid_colour_map = torch.arange(15, dtype=torch.uint8).reshape(5, 3)
    with pytest.raises(FloatingPointError):
        t.vertex_colours(v, m, sem=True)
    assert calls[-1]["sem"] is True and calls[-1]["colour_map"] is t.valid_colour_map
    other = np.zeros((5, 3), np.uint8)
    with pytest.raises(FloatingPointError):
        t.vertex_colours(v, m, sem=True, colour_map=other)
    assert calls[-1]["colour_map"] is other
    del t.valid_colour_map
    monkeypatch.undo()
    with pytest.raises(ValueError, match="colour_map"):
        t.vertex_colours(v, m, sem=True)
    assert (t.return_raw, t.check_numerics) == (True, False)
