"""Frame images without a device: the ABI number and the new symbols, the argument checks of the C entry points through the built
library, the plane layout (host-only function), the committed jet table against its header, against matplotlib and - where it
imports - against imgviz, the restatement of the integer casts (_frame_vis.py) against numpy's, ``frames.depth2rgb`` on host
arrays, and the launcher switch."""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

import _frame_vis as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANCHORS = {0: (0, 0, 128), 127: (122, 255, 125), 128: (125, 255, 122), 255: (128, 0, 0)}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__
    __graft_entry__.build()
    from intrinsicnerf_amd import _capi
    return _capi


def test_header_binding_and_names_agree(capi):
    with open(os.path.join(REPO, "include", "inerf.h")) as fh:
        text = fh.read()
    header = int(re.search(r"#define INERF_ABI_VERSION (\d+)", text).group(1))
    assert header == capi.ABI_VERSION == capi.lib().inerf_abi_version() and header >= 40024
    for name in ("inerf_frame_products", "inerf_frame_products_layout", "inerf_frame_range", "inerf_frame_range_workspace_bytes",
                 "inerf_jet_table"):
        assert name in capi.SYMBOLS and re.search(r"\b%s\(" % name, text)
        assert getattr(capi.lib(), name) is not None
    for i, name in enumerate(capi.FRAME_KIND_NAMES):
        assert re.search(r"#define INERF_FRAME_%s\s+%d\b" % (name.upper(), i), text), name
        assert getattr(capi, "FRAME_" + name.upper()) == i == getattr(V, "JET_KIND" if name == "jet" else name.upper())
    assert re.search(r"#define INERF_FRAME_MAX_PRODUCTS\s+%d\b" % capi.FRAME_MAX_PRODUCTS, text) and capi.FRAME_MAX_PRODUCTS == 16
    # the ctypes mirrors in header field order
    for struct, mirror in (("inerf_frame_product", capi.FrameProduct), ("inerf_frame_products_args", capi.FrameProductsArgs)):
        body = text[text.index("typedef struct %s {" % struct):text.index("} %s;" % struct)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"([a-z_0-9]+)(?:\[INERF_FRAME_MAX_PRODUCTS\])?\s*;", body) == [f[0] for f in mirror._fields_]
    assert C.sizeof(capi.FrameProduct) == 40 and C.sizeof(capi.FrameProductsArgs) == 56 + 16 * 40


def _args(capi, n, products, stride=8, frame=0x10000, out=0x100000, out_bytes=1 << 20, palette=0x20000, n_colours=4):
    a = capi.FrameProductsArgs()
    a.frame, a.stride, a.n, a.n_products, a.n_colours = frame, stride, n, len(products), n_colours
    a.palette, a.out, a.out_bytes = palette, out, out_bytes
    for k, (kind, column, width) in enumerate(products):
        a.products[k].kind, a.products[k].column, a.products[k].width = kind, column, width
    return a


ALL_KINDS = [(V.TO8B, 0, 3), (V.TO8B, 3, 1), (V.U16, 4, 1), (V.U8_CAST, 5, 1), (V.THRESH, 6, 1), (V.PALETTE, 5, 1), (V.JET_KIND, 4, 1)]


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 16, 17, 1021, 76800, 640000])
def test_layout_offsets_are_multiples_of_16_and_planes_do_not_overlap(capi, n):
    lib = capi.lib()
    a = _args(capi, n, ALL_KINDS)
    total = lib.inerf_frame_products_layout(C.byref(a))
    want, want_total = V.layout(n, [(k, c, w) for k, c, w in ALL_KINDS])
    assert total == want_total
    end = 0
    for k, (kind, _, width) in enumerate(ALL_KINDS):
        off = a.products[k].offset
        assert off % 16 == 0 and off >= end and (off, n * V.bytes_per_pixel(kind, width)) == want[k]
        end = off + n * V.bytes_per_pixel(kind, width)
    assert end <= total and total % 16 == 0 and total - end < 16
    # 16 products at once; the launcher's plan says the same
    from intrinsicnerf_amd import kernels
    sixteen = [(V.TO8B, 0, 3)] * 5 + [(V.U16, 4, 1)] * 5 + [(V.JET_KIND, 4, 1)] * 6
    _, planes, total16 = kernels.frame_products_plan(n, [(k, c, w, 0.0, 1.0, None) for k, c, w in sixteen])
    assert (planes, total16) == V.layout(n, sixteen)
    with pytest.raises(ValueError):
        kernels.frame_products_plan(n, [(V.TO8B, 0, 1, 0.0, 0.0, None)] * 17)


def test_validation_codes_come_back_without_a_device(capi):
    """Every refusal below is decided before any HIP call: the pointers are made up and never dereferenced."""
    lib = capi.lib()
    E = capi.E_INVALID

    def run(a, lay=True):
        if lay:
            assert lib.inerf_frame_products_layout(C.byref(a)) >= 0
        return lib.inerf_frame_products(C.byref(a), None)

    assert lib.inerf_frame_products(None, None) == E and lib.inerf_frame_products_layout(None) == E
    assert run(_args(capi, 0, ALL_KINDS)) == capi.OK                                       # n == 0: a no-op, whatever the pointers
    assert run(_args(capi, 0, ALL_KINDS, frame=None, out=None, palette=None)) == capi.OK
    assert run(_args(capi, 100, [])) == capi.OK                                           # no product: a no-op
    for field in ("frame", "out", "palette"):
        assert run(_args(capi, 100, ALL_KINDS, **{field: None})) == E, field
    for bad in ([(6, 0, 1)], [(-1, 0, 1)], [(V.TO8B, 0, 2)], [(V.TO8B, 0, 4)], [(V.U16, 0, 3)], [(V.JET_KIND, 0, 3)], [(V.PALETTE, 0, 0)],
                [(V.THRESH, 0, 3)], [(V.U8_CAST, 0, 2)]):
        a = _args(capi, 100, bad)
        assert lib.inerf_frame_products_layout(C.byref(a)) == E and run(a, lay=False) == E, bad
    a = _args(capi, 100, ALL_KINDS)
    a.n_products = 17
    assert lib.inerf_frame_products_layout(C.byref(a)) == E and run(a, lay=False) == E
    assert run(_args(capi, -1, ALL_KINDS), lay=False) == E
    assert run(_args(capi, 100, [(V.TO8B, 6, 3)])) == E                                   # reads beyond the stride
    assert run(_args(capi, 100, [(V.TO8B, -1, 1)])) == E
    assert run(_args(capi, 100, ALL_KINDS, stride=0)) == E
    assert run(_args(capi, 100, ALL_KINDS), lay=False) == E                               # offsets that are not the layout's
    assert run(_args(capi, 100, ALL_KINDS, out_bytes=100)) == E
    assert run(_args(capi, 100, ALL_KINDS, out=0x100004)) == E                            # out: 16-byte aligned
    assert run(_args(capi, 100, ALL_KINDS, frame=0x10002)) == E
    a = _args(capi, 100, ALL_KINDS)
    a.products[0].range = 0x30000                                                         # a range on a product that is no JET
    assert run(a) == E
    # overlaps: out against the frame, the palette and a jet range
    assert run(_args(capi, 100, ALL_KINDS, frame=0x100000 + 64)) == E
    assert run(_args(capi, 100, ALL_KINDS, frame=0x100000 - 100 * 8 * 4 + 8)) == E
    assert run(_args(capi, 100, ALL_KINDS, palette=0x100000 + 1440)) == E
    a = _args(capi, 100, ALL_KINDS)
    a.products[6].range = 0x100000 + 32
    assert run(a) == E
    assert run(_args(capi, 100, [(V.TO8B, 31, 1)], stride=40)) == capi.E_UNSUPPORTED      # a column beyond the 31st
    # inerf_frame_range
    assert lib.inerf_frame_range_workspace_bytes(0) == 0 and lib.inerf_frame_range_workspace_bytes(1) == 8
    assert lib.inerf_frame_range_workspace_bytes(65) == 8 and lib.inerf_frame_range_workspace_bytes(4097) == 17 * 8
    assert lib.inerf_frame_range_workspace_bytes(1 << 30) == 256 * 8
    rng = lambda values, stride, n, minmax, ws, ws_bytes: lib.inerf_frame_range(values, stride, n, minmax, ws, ws_bytes, 0, None)
    assert rng(None, 1, 0, None, None, 0) == capi.OK
    assert rng(None, 1, 10, 0x2000, 0x3000, 64) == E and rng(0x1000, 1, 10, None, 0x3000, 64) == E
    assert rng(0x1000, 0, 10, 0x2000, 0x3000, 64) == E and rng(0x1000, 1, -1, 0x2000, 0x3000, 64) == E
    assert rng(0x1002, 1, 10, 0x2000, 0x3000, 64) == E
    assert rng(0x1000, 1, 10, 0x2000, None, 64) == capi.E_WORKSPACE and rng(0x1000, 1, 10, 0x2000, 0x3000, 4) == capi.E_WORKSPACE
    assert rng(0x1000, 1, 10, 0x1008, 0x3000, 64) == E and rng(0x1000, 4, 10, 0x2000, 0x1010, 64) == E


def test_jet_header_golden_and_library_hold_the_same_bytes(capi):
    with open(os.path.join(REPO, "intrinsicnerf_amd", "csrc", "jet_table.h")) as fh:
        words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{6})u", fh.read())]
    assert len(words) == 256
    header = np.array([[w & 0xff, w >> 8 & 0xff, w >> 16] for w in words], np.uint8)
    assert V.JET.shape == (256, 3) and V.JET.dtype == np.uint8 and np.array_equal(header, V.JET)
    from intrinsicnerf_amd import kernels
    assert np.array_equal(kernels.jet_table(), V.JET)
    for i, rgb in ANCHORS.items():
        assert tuple(int(v) for v in V.JET[i]) == rgb


def test_jet_table_and_rule_equal_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    table = (matplotlib.colormaps["jet"](np.arange(256))[:, :3] * 255).round().astype(np.uint8)
    assert np.array_equal(table, V.JET)
    x = V.edge_frame()
    assert x.shape == (37, 53) and np.isnan(x).sum() == 40 and np.isinf(x).sum() == 20
    assert np.array_equal(V.jet(x, 0.1, 10.0), V.mpl_depth2rgb(x, 0.1, 10.0))
    lo, hi = V.frame_range(np.where(np.isinf(x), np.nan, x))               # its own (finite) range
    assert np.array_equal(V.jet(x, lo, hi), V.mpl_depth2rgb(x, lo, hi))
    lo, hi = V.frame_range(x)                                               # +-inf take part: every finite t is NaN or +-inf / inf
    assert (lo, hi) == (-np.inf, np.inf) and np.array_equal(V.jet(x, lo, hi), V.mpl_depth2rgb(x, lo, hi))
    assert np.array_equal(V.jet(x, 3.0, 3.0), V.mpl_depth2rgb(x, 3.0, 3.0))               # hi == lo


@pytest.mark.skipif(importlib.util.find_spec("imgviz") is None, reason="imgviz is not installed")
def test_rule_equals_imgviz_depth2rgb():
    import imgviz
    x = V.edge_frame()
    finite = np.where(np.isinf(x), np.nan, x)
    assert np.array_equal(V.jet(finite, 0.1, 10.0), imgviz.depth2rgb(finite.copy(), min_value=0.1, max_value=10.0))
    lo, hi = V.frame_range(finite)
    assert np.array_equal(V.jet(finite, lo, hi), imgviz.depth2rgb(finite.copy()))


def test_integer_cast_restatements_equal_numpy():
    x = np.array([v for v, _ in V.U16_EDGES], np.float32)
    want = np.array([w for _, w in V.U16_EDGES], np.uint16)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(x.astype(np.uint16), want)                    # what numpy does, as the issue recorded it
        assert np.array_equal(V.u16(x, 1.0), want)
        assert np.array_equal(V.u8_cast(x), x.astype(np.uint8))
        y = np.array([0.0, 1.0, 27.0, 100.9, 255.0, 255.9, 256.0, 300.0, -1.0, -0.5, -255.0, -256.0, -257.0], np.float32)
        assert np.array_equal(V.u8_cast(y), y.astype(np.uint8))
        g = np.random.default_rng(3)
        z = np.concatenate([g.uniform(-70000, 140000, 4096), g.uniform(-2, 2, 512)]).astype(np.float32)
        assert np.array_equal(V.u16(z, 1.0), z.astype(np.uint16)) and np.array_equal(V.u8_cast(z), z.astype(np.uint8))
        d = g.uniform(0, 12, 4096).astype(np.float32)
        assert np.array_equal(V.u16(d, 1000.0), (d * 1000).astype(np.uint16))              # depth in mm, trainer.py:1345
    assert V.u16(np.float32(1.0005), 1000.0) == 1000 == (np.float32([1.0005]) * 1000).astype(np.uint16)[0]
    # to8b, the mask and the palette against the host expressions they replace
    t = np.concatenate([g.uniform(-0.2, 1.2, 4096), np.arange(256) / 255.0, [0.0, 1.0, -0.0, np.inf, -np.inf]]).astype(np.float32)
    assert np.array_equal(V.to8b(t), (255 * np.clip(t, 0, 1)).astype(np.uint8)) and V.to8b(np.float32("nan")) == 0
    acc = np.array([0.0, 9.999, 10.0, 10.000001, 11.0, np.inf, -np.inf, np.nan], np.float32)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(V.thresh(acc, 10.0), (255 * np.clip((acc > 10).astype(np.float32), 0, 1)).astype(np.uint8))
    colours = g.integers(0, 256, (28, 3)).astype(np.uint8)
    labels = g.integers(0, 28, 500).astype(np.float32)
    assert np.array_equal(V.palette(labels, colours), colours[labels.astype(np.uint8).astype(np.int64)])
    assert np.array_equal(V.palette(np.array([28.0, -1.0, np.nan, 3e9, -0.5], np.float32), colours),
                          np.stack([np.zeros(3, np.uint8)] * 4 + [colours[0]]))


def test_depth2rgb_on_host_arrays(capi):
    import torch
    from intrinsicnerf_amd import frames
    x = V.edge_frame()
    got = frames.depth2rgb(x, min_value=0.1, max_value=10.0)
    assert got.shape == (37, 53, 3) and got.dtype == np.uint8 and np.array_equal(got, V.jet(x, 0.1, 10.0))
    finite = np.where(np.isinf(x), np.nan, x)
    assert np.array_equal(frames.depth2rgb(finite), V.jet(finite, *V.frame_range(finite)))
    assert np.array_equal(frames.depth2rgb(finite, min_value=1.0), V.jet(finite, 1.0, V.frame_range(finite)[1]))
    assert np.array_equal(frames.depth2rgb(torch.from_numpy(finite), max_value=7.0), V.jet(finite, V.frame_range(finite)[0], 7.0))
    assert not frames.depth2rgb(np.full((3, 4), np.nan, np.float32)).any()                 # all NaN: black
    assert np.array_equal(frames.depth2rgb(x.astype(np.float64), 0.1, 10.0), got)          # float64 in: rounded to fp32 first
    assert np.array_equal(frames.depth2rgb(np.float32([[2.0, 2.0]]))[0, 0], [0, 0, 0])    # hi == lo: 0 / 0


def test_frame_products_object_refuses_host_tensors(capi):
    import torch
    from intrinsicnerf_amd import frames, kernels
    fp = frames.FrameProducts()
    with pytest.raises(RuntimeError, match="before begin"):
        fp.add_frame(0, torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        fp.begin([("x", "to8b", "a")], ["a"], [1], (2, 2), "cpu")
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        kernels.frame_products(torch.zeros(4, 2), [(V.TO8B, 0, 1, 0.0, 0.0, None)])
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        kernels.frame_range(torch.zeros(4))


def test_launcher_switch_is_parsed(monkeypatch):
    from intrinsicnerf_amd import _capi, launch
    seen = []

    def fake(*a, **kw):
        seen.append((a, kw))
        import types
        return types.ModuleType("m"), compile("", "x", "exec")

    monkeypatch.setattr(launch, "prepare", fake)
    monkeypatch.setattr(_capi, "lib", lambda: None)
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    launch.main(["train_SSR_main.py", "--inerf-render-path", "--inerf-frame-products", "--config_file", "x.yaml"])
    assert seen[-1] == (("train_SSR_main.py", True, False, False), {"frame_products": True}) and sys.argv[1:] == ["--config_file", "x.yaml"]
    launch.main(["run_nerf.py", "--inerf-frame-products"])
    assert seen[-1] == (("run_nerf.py", False, False, False), {"frame_products": True})
    launch.main(["run_nerf.py", "--inerf-render-path"])
    assert seen[-1] == (("run_nerf.py", True, False), {})                                  # without the switch the call is what it was
    assert "--inerf-frame-products" in launch.__doc__


def test_launcher_binds_a_frame_products_object(monkeypatch):
    """rebind_object_level hands the mirror's render_path a FrameProducts only with the switch and the render path."""
    from intrinsicnerf_amd import frames, launch
    ns = {"create_nerf": lambda: None}
    launch.rebind_object_level(ns, with_render_path=True, frame_products=True)
    assert isinstance(ns["render_path"].keywords["products"], frames.FrameProducts)
    ns = {"create_nerf": lambda: None, "Cluster_Manager": object}
    launch.rebind_object_level(ns, with_render_path=True, frame_products=True)
    assert isinstance(ns["render_path"].keywords["products"], frames.FrameProducts) and "cluster_manager_factory" in ns["render_path"].keywords
    ns = {"create_nerf": lambda: None, "Cluster_Manager": object}
    launch.rebind_object_level(ns, with_render_path=True)
    assert "products" not in ns["render_path"].keywords
    ns = {"create_nerf": lambda: None}
    launch.rebind_object_level(ns, with_render_path=False, frame_products=True)
    assert "render_path" not in ns
    from intrinsicnerf_amd import ssr
    assert ssr.SSRRenderMixin.frame_products is None


def test_cluster_refresh_says_whether_it_will_keep_every_pack():
    """What object_level.render_path(products=, refresh=) asks before it lets only rgb and disp travel as floats: the refresh
    pass's own budget rule on the pack's real size - 12 floats per pixel at the object level, not the 11 columns the images read."""
    from intrinsicnerf_amd import refresh
    n, frames_ = 800 * 800, 145
    r = refresh.ClusterRefresh()                                                           # 4 GiB
    assert r.keeps_all(frames_, n * 44) and not r.keeps_all(frames_, n * 48)
    assert refresh.ClusterRefresh(keep_bytes=3 * 100 * 48).keeps_all(3, 100 * 48)
    assert not refresh.ClusterRefresh(keep_bytes=3 * 100 * 48 - 1).keeps_all(3, 100 * 48)
    assert not refresh.ClusterRefresh(keep_bytes=1).keeps_all(1, 48) and r.keeps_all(0, 48)
