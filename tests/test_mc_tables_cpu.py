"""CPU: the marching-cubes case table (scripts/gen_mc_tables.py -> csrc/mc_tables.h), the argument checks of the new entry points and
geometry.write_ply.

The watertightness proof uses the table alone: over all 2^12 states of a 3 x 2 x 2 lattice the two cubes draw exactly opposite edges in
the face they share; the faces towards j and k follow from the same check on the transposed lattices."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _mc

REPO = _mc.REPO


def test_regenerating_the_header_reproduces_the_committed_file():
    gen = _mc.generator()
    text, max_tris, max_edge_tris = gen.render()
    with open(gen.HEADER, "rb") as fh:
        assert fh.read() == text.encode()
    assert f"constexpr int kMcMaxTriangles = {max_tris};" in text and f"constexpr int kMcMaxEdgeTriangles = {max_edge_tris};" in text
    out = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "gen_mc_tables.py"), "--check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert f"max triangles per cube: {max_tris}; max triangles at one edge of one cube: {max_edge_tris}" in out.stderr


def test_edge_numbering():
    """edges by axis, then by low corner"""
    assert [(a, lo) for a, lo, _ in _mc.EDGES] == [(0, 0), (0, 2), (0, 4), (0, 6), (1, 0), (1, 1), (1, 4), (1, 5), (2, 0), (2, 1), (2, 2), (2, 3)]
    assert all(hi == lo | 1 << a for a, lo, hi in _mc.EDGES)


def edge_face(e):
    """the set of cube faces (axis, side) a cube edge lies in"""
    axis, lo, _ = _mc.EDGES[e]
    return {(a, (lo >> a) & 1) for a in range(3) if a != axis}


@pytest.mark.parametrize("case", range(256))
def test_every_case(case):
    tris = _mc.TABLE[case]
    active = {e for e, (_, lo, hi) in enumerate(_mc.EDGES) if (case >> lo & 1) != (case >> hi & 1)}
    used = {e for t in tris for e in t}
    assert used == active                                                      # every active edge is used, and no other
    assert all(len(set(t)) == 3 for t in tris)
    directed = [(t[n], t[(n + 1) % 3]) for t in tris for n in range(3)]
    assert len(set(directed)) == len(directed)                                 # no directed edge twice
    for a, b in directed:
        if (b, a) in directed:
            continue                                                           # inside the cube: matched by its reverse
        assert edge_face(a) & edge_face(b), (case, a, b)                       # else it lies in a face of the cube
    assert {e for t in _mc.TABLE[255 - case] for e in t} == used               # the complement: the same edges
    assert len(tris) <= _mc.MAX_TRIANGLES and max([sum(e in t for t in tris) for e in range(12)]) <= _mc.MAX_EDGE_TRIANGLES


def boundary_edges(case):
    """directed triangle edges of one cube that no reverse matches, as pairs of (axis, low corner)"""
    directed = [(t[n], t[(n + 1) % 3]) for t in _mc.TABLE[case] for n in range(3)]
    return [(a, b) for a, b in directed if (b, a) not in directed]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_two_cubes_agree_on_their_shared_face(axis):
    """all 2^12 states of two cubes stacked along ``axis``: in the shared face their edges are exact reverses"""
    def lattice_edge(cube, e):
        """(axis, lattice point of the low corner) of cube edge e, cube 1 shifted by one along ``axis``"""
        a, lo, _ = _mc.EDGES[e]
        p = [lo & 1, (lo >> 1) & 1, lo >> 2]
        p[axis] += cube
        return (a, tuple(p))

    shape = [2, 2, 2]
    shape[axis] = 3
    points = list(itertools.product(*[range(n) for n in shape]))
    for state in range(1 << 12):
        ins = {p: state >> n & 1 for n, p in enumerate(points)}
        per_cube = []
        for cube in (0, 1):
            case = 0
            for c in range(8):
                p = [c & 1, (c >> 1) & 1, c >> 2]
                p[axis] += cube
                case |= ins[tuple(p)] << c
            shared = []
            for a, b in boundary_edges(case):
                ea, eb = lattice_edge(cube, a), lattice_edge(cube, b)
                if all(e[0] != axis and e[1][axis] == 1 for e in (ea, eb)):    # both ends in the plane between the cubes
                    shared.append((ea, eb))
            per_cube.append(shared)
        assert sorted(per_cube[0]) == sorted((b, a) for a, b in per_cube[1]), (axis, state)


def test_counts_in_the_header():
    assert _mc.MAX_TRIANGLES == 5 and _mc.MAX_EDGE_TRIANGLES == 5 and sum(len(t) for t in _mc.TABLE) > 0


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: answered before any HIP call, so without a device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from intrinsicnerf_amd import _capi
    return _capi, _capi.lib()


def test_new_symbols_are_declared_bound_and_built(lib):
    import re
    from intrinsicnerf_amd import _build
    capi, l = lib
    text = open(os.path.join(REPO, "include", "inerf.h")).read()
    for name in ("inerf_mc_workspace_bytes", "inerf_mc_count", "inerf_mc_emit", "inerf_mesh_workspace_bytes", "inerf_mesh_normals", "inerf_mesh_clean"):
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S))
        assert decl and name in capi.SYMBOLS and len(capi.SYMBOLS[name][1]) == len(decl.group(1).split(",")), name
        assert getattr(l, name) is not None
    assert "mcubes.hip" in _build.SOURCES and os.path.join(_build.CSRC, "mc_tables.h") in _build.HEADERS
    assert "stays with the caller" not in text and "stay with the caller (skimage" not in text


def test_shape_limits(lib):
    capi, l = lib
    assert l.inerf_mc_workspace_bytes(2, 2, 2) > 0 and l.inerf_mc_workspace_bytes(2, 5, 2) > 0
    assert l.inerf_mc_workspace_bytes(1024, 1024, 1024) >= 10 * 2 ** 30
    for shape in ((1, 2, 2), (2, 0, 2), (2, 2, -3)):
        assert l.inerf_mc_workspace_bytes(*shape) == capi.E_INVALID
    assert l.inerf_mc_workspace_bytes(1025, 2, 2) == capi.E_UNSUPPORTED
    assert l.inerf_mesh_workspace_bytes(-1, 0) == capi.E_INVALID and l.inerf_mesh_workspace_bytes(0, -1) == capi.E_INVALID
    assert l.inerf_mesh_workspace_bytes(2 ** 31, 1) == capi.E_UNSUPPORTED and l.inerf_mesh_workspace_bytes(1, 2 ** 31 // 3 + 1) == capi.E_UNSUPPORTED
    assert l.inerf_mesh_workspace_bytes(0, 0) > 0


def test_argument_checks_answer_without_a_device(lib):
    """host addresses stand in for device pointers: every call below must return before it touches them"""
    capi, l = lib
    buf = (C.c_char * 8192)()
    base = (C.addressof(buf) + 255) & ~255
    p = lambda off=0: C.c_void_p(base + off)
    affine = (C.c_double * 12)()
    need = l.inerf_mc_workspace_bytes(2, 2, 2)
    # inerf_mc_count
    assert l.inerf_mc_count(None, 2, 2, 2, 0.5, p(256), need, p(4096), None) == capi.E_INVALID
    assert l.inerf_mc_count(p(), 2, 2, 2, 0.5, None, need, p(4096), None) == capi.E_INVALID
    assert l.inerf_mc_count(p(), 2, 2, 2, 0.5, p(256), need, None, None) == capi.E_INVALID
    assert l.inerf_mc_count(p(2), 2, 2, 2, 0.5, p(256), need, p(4096), None) == capi.E_INVALID          # occ not 4-byte aligned
    assert l.inerf_mc_count(p(), 2, 2, 2, 0.5, p(256 + 8), need, p(4096), None) == capi.E_INVALID       # workspace not 256-byte aligned
    assert l.inerf_mc_count(p(), 2, 2, 2, 0.5, p(256), need, p(4096 + 4), None) == capi.E_INVALID       # totals not 8-byte aligned
    assert l.inerf_mc_count(p(), 1, 2, 2, 0.5, p(256), need, p(4096), None) == capi.E_INVALID
    assert l.inerf_mc_count(p(), 2, 2, 1025, 0.5, p(256), need, p(4096), None) == capi.E_UNSUPPORTED
    assert l.inerf_mc_count(p(), 2, 2, 2, 0.5, p(256), need - 1, p(4096), None) == capi.E_WORKSPACE
    # inerf_mc_emit
    ok = dict(occ=p(), ws=p(256), aff=affine, nv=1, nt=1, vl=p(4096), vs=p(4608), f=p(5120))

    def emit(**kw):
        a = dict(ok, **kw)
        return l.inerf_mc_emit(a["occ"], 2, 2, 2, 0.5, a["ws"], a.get("wsb", need), a["aff"], a["nv"], a["nt"], a["vl"], a["vs"], a["f"], None)

    assert emit(occ=None) == capi.E_INVALID and emit(ws=None) == capi.E_INVALID
    assert emit(nv=-1) == capi.E_INVALID and emit(nt=-1) == capi.E_INVALID
    assert emit(nv=2 ** 31) == capi.E_UNSUPPORTED and emit(nt=2 ** 31 // 3 + 1) == capi.E_UNSUPPORTED
    assert emit(aff=None) == capi.E_INVALID and emit(vs=None) == capi.E_INVALID                         # the map and its output: both or neither
    assert emit(f=None) == capi.E_INVALID and emit(vl=None, vs=None, aff=None) == capi.E_INVALID
    assert emit(vl=p(4096 + 2)) == capi.E_INVALID and emit(vs=p(4608 + 4)) == capi.E_INVALID and emit(f=p(5120 + 2)) == capi.E_INVALID
    assert emit(wsb=need - 1) == capi.E_WORKSPACE
    # inerf_mesh_normals
    mneed = l.inerf_mesh_workspace_bytes(3, 1)
    assert l.inerf_mesh_normals(None, 3, p(2048), 1, p(256), mneed, p(4096), None) == capi.E_INVALID
    assert l.inerf_mesh_normals(p(), 3, None, 1, p(256), mneed, p(4096), None) == capi.E_INVALID
    assert l.inerf_mesh_normals(p(), 3, p(2048), 1, None, mneed, p(4096), None) == capi.E_INVALID
    assert l.inerf_mesh_normals(p(), 3, p(2048), 1, p(256), mneed, None, None) == capi.E_INVALID
    assert l.inerf_mesh_normals(p(4), 3, p(2048), 1, p(256), mneed, p(4096), None) == capi.E_INVALID
    assert l.inerf_mesh_normals(p(), -3, p(2048), 1, p(256), mneed, p(4096), None) == capi.E_INVALID
    assert l.inerf_mesh_normals(p(), 3, p(2048), -1, p(256), mneed, p(4096), None) == capi.E_INVALID
    assert l.inerf_mesh_normals(p(), 3, p(2048), 1, p(256), mneed - 1, p(4096), None) == capi.E_WORKSPACE
    assert l.inerf_mesh_normals(None, 0, None, 0, None, 0, None, None) == capi.OK                      # no vertex: nothing to do

    # inerf_mesh_clean
    def clean(faces=p(), nv=3, nt=1, min_t=1, f32=None, a=None, b=None, ws=p(256), wsb=mneed, fo=p(2048), o32=None, oa=None, ob=None, tot=p(4096)):
        return l.inerf_mesh_clean(faces, nv, nt, min_t, 0, f32, a, b, ws, wsb, fo, o32, oa, ob, tot, None)

    assert clean(faces=None) == capi.E_INVALID and clean(fo=None) == capi.E_INVALID and clean(tot=None) == capi.E_INVALID
    assert clean(nv=-1) == capi.E_INVALID and clean(nt=-1) == capi.E_INVALID and clean(min_t=-1) == capi.E_INVALID
    assert clean(ws=None) == capi.E_INVALID and clean(wsb=mneed - 1) == capi.E_WORKSPACE
    assert clean(f32=p(5120)) == capi.E_INVALID and clean(oa=p(5120)) == capi.E_INVALID and clean(b=p(5120)) == capi.E_INVALID
    assert clean(faces=p(2)) == capi.E_INVALID and clean(tot=p(4096 + 4)) == capi.E_INVALID and clean(a=p(5120 + 4), oa=p(6144)) == capi.E_INVALID
    assert clean(nv=2 ** 31) == capi.E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------
# the PLY writer
# ---------------------------------------------------------------------------------------------------------------------
def test_write_ply_round_trips(tmp_path):
    from intrinsicnerf_amd import geometry
    rng = np.random.default_rng(1)
    v = rng.standard_normal((7, 3))
    n = rng.standard_normal((7, 3))
    c = rng.integers(0, 256, (7, 3), dtype=np.uint8)
    f = rng.integers(0, 7, (5, 3)).astype(np.int32)
    path = tmp_path / "mesh.ply"
    geometry.write_ply(str(path), v, f, colours=c, normals=n)
    props, faces = _mc.read_ply(str(path))
    assert list(props) == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(np.stack([props["x"], props["y"], props["z"]], 1), v)
    assert np.array_equal(np.stack([props["nx"], props["ny"], props["nz"]], 1), n)
    assert np.array_equal(np.stack([props["red"], props["green"], props["blue"]], 1), c) and np.array_equal(faces, f)
    geometry.write_ply(str(path), v.astype(np.float32), f)                     # bare: positions and faces
    props, faces = _mc.read_ply(str(path))
    assert list(props) == ["x", "y", "z"] and np.array_equal(props["x"], v.astype(np.float32)[:, 0].astype(np.float64)) and np.array_equal(faces, f)
    geometry.write_ply(str(path), np.zeros((0, 3)), np.zeros((0, 3), np.int32), colours=np.zeros((0, 3), np.uint8))
    props, faces = _mc.read_ply(str(path))
    assert props["x"].shape == (0,) and faces.shape == (0, 3)
    with pytest.raises(ValueError):
        geometry.write_ply(str(path), v, f, colours=c[:5])


def test_lattice_to_scene_is_the_chain_of_the_tool():
    from intrinsicnerf_amd import geometry
    rng = np.random.default_rng(2)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, [0.3, -1.2, 2.5]
    extents = np.array([3.0, 1.5, 2.25])
    x = rng.uniform(0, 12, (50, 3))
    a = geometry.lattice_to_scene(13, extents, T)
    want = (((x / 12.0) - 0.5) * 2.0 * (extents / 2.0)) @ q.T + T[:3, 3]
    assert a.shape == (3, 4) and a.dtype == np.float64
    assert np.abs(x @ a[:, :3].T + a[:, 3] - want).max() <= 1e-12 * np.abs(want).max()
    a = geometry.lattice_to_scene((13, 7, 3), extents, T[:3])
    want = (((x / np.array([12.0, 6.0, 2.0])) - 0.5) * 2.0 * (extents / 2.0)) @ q.T + T[:3, 3]
    assert np.abs(x @ a[:, :3].T + a[:, 3] - want).max() <= 1e-12 * np.abs(want).max()
