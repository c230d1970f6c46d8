"""CPU side of the cluster-refresh pass: the two entry points of csrc/refresh.hip validate their arguments before any HIP call
(as test_capi_cpu.py shows for their neighbours), the ABI number moved in the header, the binding and the library together, the
new sources are in the build digest, and ``--inerf-cluster-refresh`` binds a ``ClusterRefresh`` where the mirrors read it.
Same stand-in entry scripts and subprocess as test_launch_cpu.py."""
import ctypes as C
import os
import re

import pytest

from conftest import REPO
from test_launch_cpu import PRELUDE, _run, ref  # noqa: F401  (ref: the stand-in tree fixture)


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


def test_frame_subsample_validates_before_any_launch(capi):
    lib = capi.lib()
    keep, a = _buf()
    P = C.c_void_p
    call = lambda frame=a, stride=9, acol=2, lcol=6, h=4, w=4, step=2, px=a, lab=a, cnt=a, k=5: lib.inerf_frame_subsample(
        P(frame) if frame else None, stride, acol, lcol, h, w, step, P(px) if px else None, P(lab) if lab else None,
        P(cnt) if cnt else None, k, None)
    # zero-sized frames are fine whatever the pointers
    assert call(frame=0, px=0, lab=0, cnt=0, h=0) == capi.OK and call(frame=0, px=0, w=0) == capi.OK
    # negative sizes, a step below 1
    assert call(h=-1) == capi.E_INVALID and call(w=-4) == capi.E_INVALID and call(h=0, w=-1) == capi.E_INVALID
    assert call(step=0) == capi.E_INVALID and call(step=-2) == capi.E_INVALID
    # null pointers: the labels only with a label column
    assert call(frame=0) == capi.E_INVALID and call(px=0) == capi.E_INVALID and call(lab=0) == capi.E_INVALID
    # columns outside the row, no classes to count into
    assert call(acol=7) == capi.E_INVALID and call(acol=-1) == capi.E_INVALID and call(lcol=9) == capi.E_INVALID
    assert call(k=0) == capi.E_INVALID
    # misaligned: floats and counts to 4 bytes, labels to 8
    assert call(frame=a + 2) == capi.E_INVALID and call(px=a + 1) == capi.E_INVALID
    assert call(lab=a + 4) == capi.E_INVALID and call(cnt=a + 2) == capi.E_INVALID
    # 2^40 rows: 2^32 blocks of 256
    assert call(h=1 << 20, w=1 << 20, step=1) == capi.E_UNSUPPORTED
    del keep


def test_cluster_snap_compose_validates_before_any_launch(capi):
    lib = capi.lib()
    keep, a = _buf()
    P = C.c_void_p
    names = ("albedo", "label", "shading", "residual", "anchors", "links", "anchor_begin", "factor", "centers", "center_begin",
             "out_c", "out_edit", "out_color")

    def call(n=100, stride=8, k=5, flags=0, **ptr):
        v = {name: ptr.get(name, a) for name in names}
        p = {name: (P(x) if x else None) for name, x in v.items()}
        return lib.inerf_cluster_snap_compose(p["albedo"], p["label"], p["shading"], p["residual"], stride, n, p["anchors"], p["links"],
                                              p["anchor_begin"], p["factor"], p["centers"], p["center_begin"], k, flags, p["out_c"],
                                              p["out_edit"], p["out_color"], None)
    assert call(n=0, **{name: 0 for name in names}) == capi.OK                     # an empty batch, whatever the pointers
    assert call(n=-1) == capi.E_INVALID and call(stride=2) == capi.E_INVALID and call(k=0) == capi.E_INVALID
    for name in names[:-1]:                                                        # every pointer but the optional colour output
        assert call(**{name: 0}) == capi.E_INVALID, name
    assert call(label=0, flags=capi.CLUSTER_IGNORE_LABEL, n=1 << 37) == capi.E_UNSUPPORTED      # (valid but for its size: see below)
    assert call(anchors=a + 4) == capi.E_INVALID                                   # float4 loads
    for name in ("albedo", "label", "shading", "residual", "out_color"):
        assert call(**{name: a + 2}) == capi.E_INVALID, name
    for name in ("out_c", "out_edit"):                                             # whole tiles go out as dwords
        assert call(**{name: a + 1}) == capi.E_INVALID and call(**{name: a + 2}) == capi.E_INVALID, name
    assert call(n=1 << 37) == capi.E_UNSUPPORTED and call(n=1 << 37, out_color=0) == capi.E_UNSUPPORTED       # 2^32 blocks of 32 pixels
    del keep


def test_abi_version_moved_everywhere(capi):
    text = open(os.path.join(REPO, "include", "inerf.h")).read()
    header = int(re.search(r"#define INERF_ABI_VERSION (\d+)", text).group(1))
    assert header == capi.ABI_VERSION == capi.lib().inerf_abi_version() and header >= 40015
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("inerf_frame_subsample", "inerf_cluster_snap_compose"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in capi.SYMBOLS and getattr(capi.lib(), name) is not None


def test_refresh_sources_are_in_the_build_digest():
    """Every #include "..." of refresh.hip and of the search header it shares with cluster.hip is hashed into the build digest."""
    from intrinsicnerf_amd import _build
    assert "refresh.hip" in _build.SOURCES
    headers = {os.path.realpath(h) for h in _build.HEADERS}
    shared = os.path.join(_build.CSRC, "cluster_search.h")
    assert os.path.realpath(shared) in headers
    for path in (os.path.join(_build.CSRC, "refresh.hip"), shared, os.path.join(_build.CSRC, "cluster.hip")):
        includes = re.findall(r'^\s*#\s*include\s*"([^"]+)"', open(path).read(), flags=re.M)
        assert includes or path == shared
        for name in includes:
            assert os.path.realpath(os.path.join(_build.CSRC, name)) in headers, (path, name)
    assert "cluster_search.h" in open(os.path.join(_build.CSRC, "refresh.hip")).read()
    assert "cluster_search.h" in open(os.path.join(_build.CSRC, "cluster.hip")).read()


OBJECT_REFRESH = PRELUDE + r'''
from intrinsicnerf_amd import cluster as ic, refresh
mod, main = launch.prepare(%(ref)r + "/object_level/run_nerf.py", with_render_path=True, cluster_refresh=True)
rp = mod.render_path
assert rp.func is ol.render_path and isinstance(rp.keywords["refresh"], refresh.ClusterRefresh)
assert rp.keywords["refresh"].manager_factory is ic.Cluster_Manager and rp.keywords["cluster_manager_factory"] is ic.Cluster_Manager
assert sys.modules["cluster"].Cluster_Manager.update_center is ic.update_center          # the switch implies the GPU fit
print("object-level cluster refresh ok")
'''

SSR_REFRESH = PRELUDE + r'''
from intrinsicnerf_amd import cluster as ic, refresh
mod, main = launch.prepare(%(ref)r + "/train_SSR_main.py", with_render_path=True, cluster_refresh=True)
trainer, cl = sys.modules["SSR.training.trainer"], sys.modules["SSR.training.cluster"]
t = trainer.SSRTrainer.__new__(trainer.SSRTrainer)
assert trainer.SSRTrainer.render_path is ssr.SSRRenderMixin.render_path
assert isinstance(t.cluster_refresh, refresh.ClusterRefresh) and t.cluster_refresh.manager_factory is ic.Cluster_Manager
assert t.cluster_manager_factory is ic.Cluster_Manager and cl.Cluster_Manager.update_center is ic.update_center
print("ssr cluster refresh ok")
'''

NO_SWITCH = PRELUDE + r'''
# the switch alone, without the render-path mirrors, binds nothing of its own
mod, main = launch.prepare(%(ref)r + "/object_level/run_nerf.py", cluster_refresh=True)
assert mod.render_path.__code__.co_filename.endswith("object_level/run_nerf.py")
assert getattr(sys.modules["cluster"].Cluster_Manager, "update_center", None) is not __import__("intrinsicnerf_amd.cluster", fromlist=["x"]).update_center
mod, main = launch.prepare(%(ref)r + "/object_level/run_nerf.py", with_render_path=True, cluster_fit=True)
assert "refresh" not in mod.render_path.keywords
mod, main = launch.prepare(%(ref)r + "/train_SSR_main.py", with_render_path=True, cluster_fit=True)
trainer = sys.modules["SSR.training.trainer"]
assert getattr(trainer.SSRTrainer.__new__(trainer.SSRTrainer), "cluster_refresh", None) is None
assert ssr.SSRRenderMixin.cluster_refresh is None and ssr.SSRRenderer.cluster_refresh is None
print("no refresh without the switch ok")
'''


def test_switch_binds_object_level(ref):
    assert "object-level cluster refresh ok" in _run(OBJECT_REFRESH, ref)


def test_switch_binds_ssr(ref):
    assert "ssr cluster refresh ok" in _run(SSR_REFRESH, ref)


def test_without_the_switch_nothing_is_bound(ref):
    assert "no refresh without the switch ok" in _run(NO_SWITCH, ref)


def test_switch_is_parsed_and_removed(monkeypatch):
    from intrinsicnerf_amd import launch
    seen = {}
    monkeypatch.setattr(launch, "prepare", lambda script, rp, cf, *a, **kw: seen.update(script=script, rp=rp, kw=kw)
                        or (type("M", (), {"__dict__": {}})(), compile("", "x", "exec")))
    import sys
    monkeypatch.setattr(sys, "argv", sys.argv[:])
    try:
        launch.main(["run_nerf.py", "--inerf-render-path", "--inerf-cluster-refresh", "--config", "x"])
    except Exception:
        pass
    assert seen.get("rp") is True and seen["kw"].get("cluster_refresh") is True
    assert "--inerf-cluster-refresh" not in sys.argv


def test_refresh_object_refuses_the_host():
    """No CPU path: a ClusterRefresh begun on the host raises, like every launcher of the package."""
    from intrinsicnerf_amd import refresh
    r = refresh.ClusterRefresh(keep_bytes=1, step=2)
    with pytest.raises(RuntimeError, match="HIP device"):
        r.begin(2, 4, 4, 1, "cpu")
    with pytest.raises(RuntimeError):
        r.snap(0)
    with pytest.raises(ValueError):
        refresh.ClusterRefresh(step=0)
