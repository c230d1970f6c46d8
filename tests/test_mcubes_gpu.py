"""GPU: marching cubes, scene coordinates, vertex normals and mesh cleaning on the device (csrc/mcubes.hip) and their front-ends
(geometry.marching_cubes / vertex_normals / clean_mesh / extract_mesh, SSRRenderMixin.extract_colour_mesh).

Bit equality with skimage is not the aim (its table is not ours).  The mesh is pinned to what any correct isosurface mesh has - the
vertex set (enumerated independently in numpy, bit for bit), closedness, orientation, Euler characteristic, enclosed volume - and the
faces to a numpy restatement that applies the generator's table cube by cube (tests/_mc.py).

Sizes: the classify kernel works on tiles of 4 x 8 x 32 lattice points and the scans on blocks of 1 024, so 16^3 (4 096 points: 4 x 2 x 1
tiles, ragged along k; four scan blocks) and 24^3 (13 824 points: 6 x 3 x 1 tiles, 14 scan blocks with a ragged last one) cross every
boundary; 2 x 2 x 2 up to 2 x 5 x 2 sit inside one tile; 128 x 96 x 92 has more than 1 024 scan blocks, where the scan of the block
sums takes its other path."""
import numpy as np
import pytest
import torch

import _mc

pytestmark = pytest.mark.gpu

DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def run_mc(occ, level, affine=None):
    from intrinsicnerf_amd import geometry
    v, s, f = geometry.marching_cubes(dev(np.asarray(occ, np.float32)), level, affine)
    assert v.is_cuda and f.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int32 and (s is None) == (affine is None)
    return host(v), host(s), host(f)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# one cube, minimal shapes
# ---------------------------------------------------------------------------------------------------------------------
def test_one_cube_every_case():
    rng = np.random.default_rng(11)
    level = 0.5
    for case in range(256):
        mag = rng.uniform(0.05, 0.45, 8).astype(np.float32)
        occ = np.empty((2, 2, 2), np.float32)
        for c in range(8):
            occ[c & 1, (c >> 1) & 1, c >> 2] = level + mag[c] if case >> c & 1 else level - mag[c]
        v, _, f = run_mc(occ, level)
        want_v, ids = _mc.vertices(occ, level)
        assert int(_mc.cases(occ, level)[0, 0, 0]) == case
        assert same_bits(v, want_v), case
        assert np.array_equal(f, _mc.faces(occ, level, ids)), case
        assert len(f) == len(_mc.TABLE[case])


@pytest.mark.parametrize("shape", [(2, 2, 3), (3, 2, 2), (2, 5, 2)])
def test_minimal_shapes(shape):
    rng = np.random.default_rng(sum(shape))
    for trial in range(8):
        occ = rng.uniform(0, 1, shape).astype(np.float32)
        v, _, f = run_mc(occ, 0.5)
        want_v, ids = _mc.vertices(occ, 0.5)
        assert same_bits(v, want_v) and np.array_equal(f, _mc.faces(occ, 0.5, ids)), (shape, trial)


def test_no_crossing_gives_an_empty_mesh():
    from intrinsicnerf_amd import geometry
    for value in (0.0, 1.0):
        occ = torch.full((3, 4, 5), value, device=DEV)
        v, s, f = geometry.marching_cubes(occ, 0.5, np.eye(4)[:3])
        assert tuple(v.shape) == (0, 3) and tuple(s.shape) == (0, 3) and tuple(f.shape) == (0, 3)
        n = geometry.vertex_normals(s, f)
        assert tuple(n.shape) == (0, 3)
        cv, cf, cn, cl = geometry.clean_mesh(s, f, n, v)
        assert tuple(cv.shape) == (0, 3) and tuple(cf.shape) == (0, 3) and tuple(cn.shape) == (0, 3) and tuple(cl.shape) == (0, 3)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_a_non_finite_lattice_raises(bad):
    from intrinsicnerf_amd import geometry, kernels
    occ = np.random.default_rng(3).uniform(0, 1, (5, 9, 34)).astype(np.float32)           # two tiles along j and along k
    occ[4, 8, 33] = bad
    with pytest.raises(ValueError, match="non-finite"):
        geometry.marching_cubes(dev(occ), 0.5)
    occ[0, 0, 0] = bad
    _, totals = kernels.mc_count(dev(occ), 0.5)
    assert int(totals[2]) == 2
    # a NaN counts as outside: the other totals are those of the lattice with the NaN replaced by a low value
    if bad != bad:
        _, clean = kernels.mc_count(dev(np.where(np.isnan(occ), np.float32(-1), occ)), 0.5)
        assert totals[:2].tolist() == clean[:2].tolist()


# ---------------------------------------------------------------------------------------------------------------------
# 16^3 of independent uniform values: every case, the vertex order, two triangles per interior edge, the same bytes twice
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noise():
    occ = np.random.default_rng(2024).uniform(0, 1, (16, 16, 16)).astype(np.float32)
    v, _, f = run_mc(occ, 0.5)
    return occ, v, f


def test_noise_field_holds_every_case_and_the_enumerated_vertices(noise):
    occ, v, f = noise
    assert len(np.unique(_mc.cases(occ, 0.5))) == 256
    want_v, ids = _mc.vertices(occ, 0.5)
    assert same_bits(v, want_v)
    assert np.array_equal(f, _mc.faces(occ, 0.5, ids))


def test_noise_mesh_is_watertight_inside_the_volume(noise):
    occ, v, f = noise
    keys, fwd, back = _mc.edge_table(f)
    a, b = v[keys[:, 0]], v[keys[:, 1]]
    on_boundary = np.zeros(len(keys), bool)
    for axis in range(3):
        for wall in (0.0, float(occ.shape[axis] - 1)):
            on_boundary |= (a[:, axis] == wall) & (b[:, axis] == wall)
    inner = ~on_boundary
    assert inner.sum() > 1000 and on_boundary.sum() > 100
    assert (fwd[inner] == 1).all() and (back[inner] == 1).all()                # two triangles, opposite directions
    assert (fwd[on_boundary] + back[on_boundary] == 1).all()                   # a boundary edge of the open surface: one triangle


def test_two_runs_give_the_same_bytes(noise):
    occ, v, f = noise
    v2, _, f2 = run_mc(occ, 0.5)
    assert same_bits(v, v2) and same_bits(f, f2)


# ---------------------------------------------------------------------------------------------------------------------
# sphere and torus
# ---------------------------------------------------------------------------------------------------------------------
CENTRE, RADIUS = np.array([11.3, 12.1, 11.7]), 8.0
EXTENTS = np.array([3.0, 1.5, 2.25])


def box_to_scene():
    q, _ = np.linalg.qr(np.random.default_rng(5).standard_normal((3, 3)))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, [0.3, -1.2, 2.5]
    return T


@pytest.fixture(scope="module")
def sphere():
    from intrinsicnerf_amd import geometry
    occ = _mc.sphere_field((24, 24, 24), CENTRE, RADIUS)
    affine = geometry.lattice_to_scene(24, EXTENTS, box_to_scene())
    v, s, f = run_mc(occ, 0.0, affine)
    return occ, v, s, f, affine


def test_sphere_is_closed_oriented_and_of_genus_zero(sphere):
    occ, v, s, f, _ = sphere
    keys, fwd, back = _mc.edge_table(f)
    assert (fwd == 1).all() and (back == 1).all()
    assert _mc.euler(f) == 2 and len(np.unique(f)) == len(v)
    v64 = v.astype(np.float64)
    a, b, c = v64[f[:, 0]], v64[f[:, 1]], v64[f[:, 2]]
    normal = np.cross(b - a, c - a)
    solid = np.linalg.norm(normal, axis=1) > 0
    assert solid.sum() > 0.9 * len(f)
    assert (np.einsum("ij,ij->i", normal, (a + b + c) / 3.0 - CENTRE)[solid] > 0).all()


def test_sphere_volume_lies_between_its_bounds(sphere):
    """below: the cubes with all eight corners inside are enclosed by the mesh; above: the field is concave along any line, so every
    interpolated vertex lies inside the ball and the mesh (the boundary of a polyhedron with its vertices in the ball) with it"""
    occ, v, _, f, _ = sphere
    vol = _mc.volume(v, f)
    lower = int((_mc.cases(occ, 0.0) == 255).sum())
    upper = 4.0 / 3.0 * np.pi * RADIUS ** 3
    print(f"sphere volume: {lower} <= {vol:.3f} <= {upper:.3f}")
    assert lower <= vol <= upper


def test_torus_has_euler_characteristic_zero():
    occ = _mc.torus_field((24, 24, 16), (11.4, 11.8, 7.6), 7.0, 3.2)
    v, _, f = run_mc(occ, 0.0)
    keys, fwd, back = _mc.edge_table(f)
    assert (fwd == 1).all() and (back == 1).all()
    assert _mc.euler(f) == 0
    want_v, ids = _mc.vertices(occ, 0.0)
    assert same_bits(v, want_v) and np.array_equal(f, _mc.faces(occ, 0.0, ids))


def test_lattice_beyond_1024_scan_blocks():
    """128 x 96 x 92 = 1 130 496 points are 1 104 scan blocks: the one workgroup that scans the block sums then takes two sums per
    thread instead of one.  Two spheres, one in the first blocks and one in the last, so that offsets cross the whole range."""
    shape = (128, 96, 92)
    occ = np.maximum(_mc.sphere_field(shape, (9.3, 10.1, 8.7), 6.0), _mc.sphere_field(shape, (117.2, 85.4, 81.1), 7.5))
    v, _, f = run_mc(occ, 0.0)
    want_v, ids = _mc.vertices(occ, 0.0)
    assert len(v) > 1000 and same_bits(v, want_v) and np.array_equal(f, _mc.faces(occ, 0.0, ids))
    assert _mc.euler(f) == 4


def test_scene_vertices_follow_lattice_to_scene(sphere):
    """the kernel applies the composed 3 x 4 map; numpy walks the tool's chain (/ (dim - 1), - 0.5, x 2, x extents / 2, transform).  Both
    round a handful of fp64 operations on numbers no larger than the scene's: 1e-12 of that magnitude is four thousand ulps"""
    occ, v, s, f, affine = sphere
    T = box_to_scene()
    x = v.astype(np.float64)
    want = (((x / 23.0) - 0.5) * 2.0 * (EXTENTS / 2.0)) @ T[:3, :3].T + T[:3, 3]
    assert s.dtype == np.float64 and s.shape == want.shape
    assert np.abs(s - want).max() <= 1e-12 * np.abs(want).max()
    composed = (affine[:, 0] * x[:, :1] + affine[:, 1] * x[:, 1:2]) + affine[:, 2] * x[:, 2:3] + affine[:, 3]
    assert same_bits(s, composed)                                              # and the documented operation order, bit for bit


# ---------------------------------------------------------------------------------------------------------------------
# normals
# ---------------------------------------------------------------------------------------------------------------------
def test_normals_are_the_ordered_fp64_sum(sphere):
    from intrinsicnerf_amd import geometry
    occ, v, s, f, _ = sphere
    got = geometry.vertex_normals(dev(s), dev(f))
    assert got.is_cuda and got.dtype == torch.float64
    want = _mc.normals_reference(s, f)
    assert same_bits(host(got), want)
    assert same_bits(host(geometry.vertex_normals(dev(s), dev(f))), want)       # again: the same bytes
    assert np.abs(np.linalg.norm(want, axis=1) - 1.0).max() < 1e-12
    # from float32 lattice vertices: promoted, the same function
    assert same_bits(host(geometry.vertex_normals(dev(v), dev(f))), _mc.normals_reference(v.astype(np.float64), f))


def test_normals_of_a_mesh_from_elsewhere():
    """a fan of 40 triangles about vertex 0 (beyond the 20 slots held in registers), a vertex no triangle names, a triangle that names
    a vertex twice and one whose index is out of range"""
    from intrinsicnerf_amd import geometry
    rng = np.random.default_rng(9)
    v = rng.standard_normal((43, 3))
    f = np.array([[0, 1 + n, 1 + (n + 1) % 40] for n in range(40)] + [[5, 5, 6]], np.int32)
    f = f[rng.permutation(len(f))]
    got = host(geometry.vertex_normals(dev(v), dev(f)))
    want = _mc.normals_reference(v, f)
    assert same_bits(got, want) and (got[41:] == 0).all()
    bad = np.concatenate([f, np.array([[0, 1, 43]], np.int32)])
    assert same_bits(host(geometry.vertex_normals(dev(v), dev(bad))), want)


# ---------------------------------------------------------------------------------------------------------------------
# cleaning
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def islands():
    """two disjoint spheres and three single-voxel blobs in 24 x 20 x 36, as a scene-space mesh with normals"""
    from intrinsicnerf_amd import geometry
    shape = (24, 20, 36)
    occ = np.maximum(_mc.sphere_field(shape, (7.3, 9.1, 8.7), 5.2), _mc.sphere_field(shape, (15.2, 10.4, 25.1), 6.4))
    for p in ((2, 2, 33), (21, 17, 3), (20, 3, 2)):
        occ[p] = 0.6
    affine = geometry.lattice_to_scene(shape, EXTENTS, box_to_scene())
    v, s, f = geometry.marching_cubes(dev(occ), 0.0, affine)
    n = geometry.vertex_normals(s, f)
    return v, s, f, n


def test_components_are_those_of_the_shared_edge_graph(islands):
    from intrinsicnerf_amd import geometry
    v, s, f, n = islands
    count, label = _mc.edge_components(host(f))
    sizes = np.sort(np.bincount(label))
    assert count == 5 and sizes[:3].tolist() == [8, 8, 8] and sizes[3] > 400
    *_, counts = geometry.clean_mesh(s, f, n, v, min_num_cluster=1, return_counts=True)
    assert counts == {"vertices": len(v), "triangles": len(f), "components": 5, "kept_components": 5}
    # per component: the device's counts are scipy's (keep everything with at least k triangles, for every k that matters)
    for k in sorted(set(sizes.tolist())):
        *_, counts = geometry.clean_mesh(s, f, None, None, min_num_cluster=k, return_counts=True)
        assert counts["kept_components"] == int((sizes >= k).sum()) and counts["triangles"] == int(sizes[sizes >= k].sum()), k


@pytest.mark.parametrize("k,single", [(8, False), (9, False), (400, False), (100000, False), (400, True)])
def test_clean_mesh_keeps_the_expected_part_in_order(islands, k, single):
    from intrinsicnerf_amd import geometry
    v, s, f, n = islands
    keep_t, keep_v, want_f, sizes = _mc.clean_reference(host(f), len(v), k, single)
    cv, cf, cn, cl = geometry.clean_mesh(s, f, n, v, min_num_cluster=k, keep_single_cluster=single)
    assert np.array_equal(host(cf), want_f)
    assert same_bits(host(cv), host(s)[keep_v]) and same_bits(host(cn), host(n)[keep_v]) and same_bits(host(cl), host(v)[keep_v])
    if single:
        assert len(want_f) == sizes.max()
    elif k == 9:
        assert len(want_f) == len(f) - 24                                      # the three blobs of eight triangles are gone
    elif k == 8:
        assert len(want_f) == len(f)
    elif k == 100000:
        assert len(want_f) == 0 and tuple(cv.shape) == (0, 3)


def test_keep_single_cluster_breaks_a_tie_by_the_lowest_label():
    from intrinsicnerf_amd import geometry
    occ = np.zeros((6, 6, 6), np.float32)
    occ[1, 1, 1] = occ[4, 4, 4] = 1.0
    v, s, f = geometry.marching_cubes(dev(occ), 0.5, np.eye(4)[:3])
    assert len(f) == 16
    cv, cf, _, _ = geometry.clean_mesh(s, f, keep_single_cluster=True)
    assert len(cf) == 8 and np.array_equal(host(cv), host(s)[:6]) and np.array_equal(host(cf), host(f)[host(f).max(1) < 6])


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_extract_colour_mesh_end_to_end(tmp_path):
    import _grid
    from intrinsicnerf_amd import geometry, ssr
    fx = _grid.fixture()
    n_classes = int(fx["ssr/n_classes"])
    torch.manual_seed(7)
    t = ssr.SSRRenderer(n_classes, N_samples=8, N_importance=8, perturb=0., raw_noise_std=0., device=DEV)
    assert t.embed_fn.scalar_factor == float(fx["ssr/xyz_div"])
    with torch.no_grad():                                                      # the grid tests' calibration of the density head
        for net in (t.ssr_net_coarse, t.ssr_net_fine):
            net.alpha_linear.weight.copy_(torch.from_numpy(fx["ssr/alpha_weight"]))
            net.alpha_linear.bias.copy_(torch.from_numpy(fx["ssr/alpha_bias"]))
            net.requires_grad_(False)
    t.near, t.far, t.return_raw = float(fx["ssr/near"]), float(fx["ssr/far"]), False
    extents, T = fx["extents_d16"], fx["transform_d16"]
    occ = t.occupancy_grid(extents, T, grid_dim=16)
    level = 0.45
    if not (bool((occ > level).any()) and bool((occ <= level).any())):
        level = float(occ.median())                                            # the grid's own median: something on either side
    print("occupancy range:", float(occ.min()), float(occ.max()), " level:", level)
    cmap = np.random.default_rng(3).integers(0, 256, (n_classes, 3), dtype=np.uint8)
    for sem in (False, True):
        path = tmp_path / f"mesh_{int(sem)}.ply"
        v, f, n, colours = t.extract_colour_mesh(extents, T, grid_dim=16, level=level, sem=sem, colour_map=cmap, save_path=str(path),
                                                 min_num_cluster=2)
        print("vertices, faces:", len(v), len(f))
        assert v.is_cuda and f.is_cuda and n.is_cuda and v.dtype == torch.float64 and f.dtype == torch.int32
        assert len(v) > 0 and len(f) > 0 and len(n) == len(v) and colours.shape == (len(v), 3) and colours.dtype == np.uint8
        assert int(f.min()) == 0 and int(f.max()) == len(v) - 1
        props, faces = _mc.read_ply(str(path))
        assert len(props["x"]) == len(props["red"]) == len(v) and np.array_equal(faces, host(f))
        assert np.array_equal(np.stack([props["x"], props["y"], props["z"]], 1), host(v))
        assert np.array_equal(np.stack([props["red"], props["green"], props["blue"]], 1), colours)
        want = geometry.vertex_colours(t.render_rays, v, n, near=0.1, far=10.0, near_t=2.0, sem=sem, colour_map=cmap if sem else None)
        assert np.array_equal(colours, want)
        # the stages one by one give the same mesh
        occ_again = t.occupancy_grid(extents, T, grid_dim=16)
        _, s, f0 = geometry.marching_cubes(occ_again, level, geometry.lattice_to_scene(16, extents, T))
        cv, cf, cn, _ = geometry.clean_mesh(s, f0, geometry.vertex_normals(s, f0), min_num_cluster=2)
        assert torch.equal(cv, v) and torch.equal(cf, f) and torch.equal(cn, n)
