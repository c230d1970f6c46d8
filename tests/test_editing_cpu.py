"""CPU side of scene editing (csrc/edit.hip, intrinsicnerf_amd/editing.py), through the real library: the three entry points
validate their arguments before any HIP call, the ABI number moved in the header, the binding and the library together, the new
sources are in the build digest, and the session's host logic - argument validation, the slot -> (semantic, class) inversion
over ``center_begin``, the refusal of a host device - needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _editing as E
from conftest import REPO, load_golden
from test_cluster import Manager, fixture_clusters


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__
    __graft_entry__.build()
    from intrinsicnerf_amd import _capi
    return _capi


def _buf(n_bytes=64, align=16):
    """(keep-alive, address): host memory with the wanted alignment; never dereferenced by the calls below."""
    raw = (C.c_char * (n_bytes + align))()
    addr = C.addressof(raw)
    return raw, addr + (-addr) % align


def test_abi_version_and_symbols(capi):
    text = open(os.path.join(REPO, "include", "inerf.h")).read()
    header = int(re.search(r"#define INERF_ABI_VERSION (\d+)", text).group(1))
    assert header == capi.ABI_VERSION == capi.lib().inerf_abi_version() and header >= 40019
    assert "inerf_edit_params" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("inerf_edit_frame", "inerf_edit_recompose", "inerf_edit_recompose_u8"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in capi.SYMBOLS and getattr(capi.lib(), name) is not None
    assert [f[0] for f in capi.EditParams._fields_] == ["edit_centers", "shading_mode", "residual_mode", "shading_scale", "residual_scale"]
    assert C.sizeof(capi.EditParams) == 24


def test_edit_sources_are_in_the_build_digest():
    from intrinsicnerf_amd import _build
    assert "edit.hip" in _build.SOURCES
    headers = {os.path.realpath(h) for h in _build.HEADERS}
    for src in ("edit.hip", "refresh.hip"):
        text = open(os.path.join(_build.CSRC, src)).read()
        includes = re.findall(r'^\s*#\s*include\s*"([^"]+)"', text, flags=re.M)
        assert "to_u8.h" in includes                                    # one to_u8, shared
        assert not re.search(r"unsigned\s+to_u8\s*\(", text)
        for name in includes:
            assert os.path.realpath(os.path.join(_build.CSRC, name)) in headers, (src, name)
    assert "cluster_search.h" in open(os.path.join(_build.CSRC, "edit.hip")).read()


def _params(capi, centers, smode=0, rmode=0, gs=1.0, gr=1.0):
    return capi.EditParams(centers, smode, rmode, gs, gr)


def test_edit_frame_validates_before_any_launch(capi):
    lib = capi.lib()
    keep, a = _buf()
    P = C.c_void_p
    names = ("albedo", "label", "shading", "residual", "anchors", "links", "anchor_begin", "factor", "center_begin",
             "out_result", "out_c", "out_f32", "out_slot")

    def call(n=100, stride=8, k=5, flags=0, params="default", **ptr):
        v = {name: ptr.get(name, a) for name in names}
        p = {name: (P(x) if x else None) for name, x in v.items()}
        par = _params(capi, a) if params == "default" else params
        return lib.inerf_edit_frame(p["albedo"], p["label"], p["shading"], p["residual"], stride, n, p["anchors"], p["links"],
                                    p["anchor_begin"], p["factor"], p["center_begin"], k, flags, None if par is None else C.byref(par),
                                    p["out_result"], p["out_c"], p["out_f32"], p["out_slot"], None)
    assert call(n=0, params=None, **{name: 0 for name in names}) == capi.OK            # an empty frame, whatever the pointers
    assert call(n=-1) == capi.E_INVALID and call(stride=2) == capi.E_INVALID and call(k=0) == capi.E_INVALID
    for name in names[:-3]:                                                            # every pointer but the optional outputs
        assert call(**{name: 0}) == capi.E_INVALID, name
    assert call(params=None) == capi.E_INVALID and call(params=_params(capi, None)) == capi.E_INVALID
    for bad in (-1, 2):
        assert call(params=_params(capi, a, smode=bad)) == capi.E_INVALID and call(params=_params(capi, a, rmode=bad)) == capi.E_INVALID
    assert call(params=_params(capi, a + 2)) == capi.E_INVALID
    assert call(anchors=a + 4) == capi.E_INVALID                                       # float4 loads
    for name in ("albedo", "label", "shading", "residual", "out_f32", "out_slot", "out_result", "out_c"):
        assert call(**{name: a + 2}) == capi.E_INVALID, name
    # valid but for its size: 2^32 blocks of 32 pixels - with and without the optional outputs, and with the ignore-label flag
    assert call(n=1 << 37) == capi.E_UNSUPPORTED and call(n=1 << 37, out_c=0, out_f32=0, out_slot=0) == capi.E_UNSUPPORTED
    assert call(label=0, flags=capi.CLUSTER_IGNORE_LABEL, n=1 << 37) == capi.E_UNSUPPORTED
    assert call(params=_params(capi, a, 1, 1, 0.37, 1.63), n=1 << 37) == capi.E_UNSUPPORTED
    del keep


@pytest.mark.parametrize("form", ["f32", "u8"])
def test_edit_recompose_validates_before_any_launch(capi, form):
    lib = capi.lib()
    keep, a = _buf()
    P = C.c_void_p
    names = ("albedo", "shading", "residual", "slot", "out_result", "out_c", "out_f32")

    def call(n=100, stride=8, params="default", **ptr):
        v = {name: ptr.get(name, a) for name in names}
        p = {name: (P(x) if x else None) for name, x in v.items()}
        par = C.byref(_params(capi, a) if params == "default" else params) if params is not None else None
        if form == "f32":
            return lib.inerf_edit_recompose(p["albedo"], p["shading"], p["residual"], stride, p["slot"], n, par, p["out_result"], p["out_c"],
                                            p["out_f32"], None)
        return lib.inerf_edit_recompose_u8(p["albedo"], p["shading"], p["residual"], p["slot"], n, par, p["out_result"], p["out_c"],
                                           p["out_f32"], None)
    assert call(n=0, params=None, **{name: 0 for name in names}) == capi.OK
    assert call(n=-1) == capi.E_INVALID
    for name in names[:-2]:
        assert call(**{name: 0}) == capi.E_INVALID, name
    assert call(params=None) == capi.E_INVALID and call(params=_params(capi, None)) == capi.E_INVALID
    for bad in (-1, 2):
        assert call(params=_params(capi, a, smode=bad)) == capi.E_INVALID and call(params=_params(capi, a, rmode=bad)) == capi.E_INVALID
    assert call(params=_params(capi, a + 1)) == capi.E_INVALID
    for name in ("slot", "out_f32"):
        assert call(**{name: a + 2}) == capi.E_INVALID, name
    big = 1 << 43                                                                      # 2^32 blocks of 2048 pixels
    if form == "f32":
        assert call(stride=2) == capi.E_INVALID
        for name in ("albedo", "shading", "residual"):
            assert call(**{name: a + 2}) == capi.E_INVALID, name
    else:                                                                              # 8-bit sources at any byte alignment
        for off in (1, 2, 3):
            assert call(n=big, albedo=a + off, shading=a + (off + 1) % 4, residual=a + (off + 2) % 4) == capi.E_UNSUPPORTED
    for off in (0, 1, 2, 3):                                                           # ... and the 8-bit outputs of both forms
        assert call(n=big, out_result=a + off, out_c=a + (off + 1) % 4) == capi.E_UNSUPPORTED
    assert call(n=big, out_c=0, out_f32=0) == capi.E_UNSUPPORTED
    del keep


# ---- the session's host logic ------------------------------------------------------------------------------------------------------
def test_slot_inversion_over_center_begin():
    from intrinsicnerf_amd import editing
    fx = load_golden("cluster_lookup")
    begin = editing.center_ranges(fixture_clusters(fx))
    assert tuple(begin) == E.CENTER_BEGIN
    assert editing.slot_to_class(begin, -1) is None
    seen = []
    for sem in range(5):
        for cls in range(begin[sem + 1] - begin[sem]):
            slot = editing.class_to_slot(begin, sem, cls)
            assert editing.slot_to_class(begin, slot) == (sem, cls)
            seen.append(slot)
    assert seen == list(range(17))                                                     # every row once, class 3 owns none
    assert editing.slot_to_class(begin, 12) == (4, 0) and editing.slot_to_class(begin, 11) == (2, 3)
    for bad in (-2, 17, 100):
        with pytest.raises(ValueError):
            editing.slot_to_class(begin, bad)
    for sem, cls in ((-1, 0), (5, 0), (3, 0), (0, 4), (0, -1), (4, 5)):
        with pytest.raises(ValueError):
            editing.class_to_slot(begin, sem, cls)
    assert editing.center_ranges([fixture_clusters(fx)[4]]) == [0, 5]


def test_slider_colours_follow_the_reference():
    from intrinsicnerf_amd import editing
    assert editing.slider_color(255, 16, 0) == (float(255) / 255.0, float(16) / 255.0, float(0) / 255.0)
    for bad in ((-1, 0, 0), (0, 256, 0), (0, 0, float("nan"))):
        with pytest.raises(ValueError):
            editing.slider_color(*bad)


def test_u8_frames_are_validated_on_the_host():
    from intrinsicnerf_amd import editing
    F, H, W = 2, 3, 5
    a = np.zeros((F, H, W, 3), np.uint8)
    s = np.zeros((F, H, W), np.uint8)
    lab = np.zeros((F, H, W), np.int64)
    out = editing.check_frames_u8(a, s, a, lab)
    assert out[4] == (F, H, W) and out[3].shape == (F, H, W)
    assert editing.check_frames_u8(a, s[..., None], a, lab[..., None])[3].shape == (F, H, W)          # load_all_image's label shape
    assert editing.check_frames_u8(a, s, a, None)[3] is None
    with pytest.raises(ValueError):
        editing.check_frames_u8(a.astype(np.float32), s, a, lab)                       # the division already done
    with pytest.raises(ValueError):
        editing.check_frames_u8(a, s[:1], a, lab)
    with pytest.raises(ValueError):
        editing.check_frames_u8(a[..., :2], s, a, lab)
    with pytest.raises(ValueError):
        editing.check_frames_u8(a, s, a, lab.astype(np.float32))
    with pytest.raises(ValueError):
        editing.check_frames_u8(a, s, a, lab[:, :2])


def test_session_refuses_the_host():
    """No CPU path: a session on the host raises before it touches the manager, like every front-end of the package."""
    from intrinsicnerf_amd import editing, kernels
    import torch
    mgr = Manager(fixture_clusters(load_golden("cluster_lookup")))
    with pytest.raises(RuntimeError, match="HIP device"):
        editing.EditSession(mgr, device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        kernels.edit_recompose_u8(type("T", (), {"device": torch.device("cpu")})(), None, torch.zeros(4, 3, dtype=torch.uint8),
                                  torch.zeros(4, dtype=torch.uint8), torch.zeros(4, 3, dtype=torch.uint8), None)
