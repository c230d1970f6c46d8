"""CPU: what tests/test_mcubes_edges_gpu.py relies on, checked on the numpy / scipy restatements of tests/_mc.py alone (no device).

Each lattice of the GPU file is chosen for a property; were the property absent, the GPU test would pass without having tried
anything.  The GPU tests repeat the assertions on the meshes they compare.  Values as obtained with
``np.random.default_rng(seed).uniform(0, 1, shape).astype(np.float32)`` at level 0.5 unless stated otherwise (numpy 2):

  field                                        properties asserted
  -------------------------------------------  -------------------------------------------------------------------------------------
  (9, 17, 67), seed 1                          all 256 cases; V = 14 374, F = 27 096; 142 shared-edge components; the vertex graph splits
                                               the triangles as the shared-edge graph does; largest valence exactly 20
                                               (= 4 * MAX_EDGE_TRIANGLES); no zero-area triangle; 3 x 3 x 3 ragged classify tiles with
                                               straddling edges across the tile faces: 1 117 along i (owner i % 4 == 3), 609 along j
                                               (j % 8 == 7), 140 along k (k % 32 == 31).  At level 0.45: 256 cases, and 0.45 is not a
                                               float32; at level 0.3: 247 cases
  (40, 40, 70), seed 8                         V = 164 621, F = 337 016; 1 180 components, the largest of 326 717 triangles, the second
                                               of 72; the two partitions are equal
  uniform(0, 1, (13, 19, 41)) ** 3, seed 4     892 components of 40 distinct sizes, the largest of 200; partitions equal
  rng(5).integers(0, 4, (9, 17, 35)) as fp32   level 1.0 (a lattice value): 256 cases, 3 057 zero-area triangles, 195 vertices whose
                                               normal sum is zero, valence up to 20, partitions still equal (64 components).
                                               Level 2.0: 456 components of 43 distinct sizes, partitions equal
  rng(6).uniform(0, 1, (9, 17, 35)) > 0.7      every t is exactly 0.5; 425 components; partitions equal
  noise - 0.5 on (7, 11, 37), seed 2, level 0  scaled by 2^100 and 2^-100: no value denormal, the reference mesh is bit-identical to the
                                               unscaled one (V = 3 914, F = 6 885); by 2^-140: 2 846 denormal values and three zeros,
                                               finite vertices, another mesh (F = 6 881)
  (5, 9, 34), (4, 8, 32), (5, 8, 33), (4, 9, 32)   seeded by the sum of the shape: each has straddling edges on all three axes
  fans of 20 and 21 triangles                  vertex 0 has valence exactly 20 and 21
"""
import numpy as np
import pytest

import _mc


def reference_mesh(occ, level):
    v, ids = _mc.vertices(occ, level)
    return v, _mc.faces(occ, level, ids)


def n_cases(occ, level):
    return len(np.unique(_mc.cases(occ, level)))


def test_tile_field_crosses_every_tile_face_with_every_case_and_valence_twenty():
    occ = _mc.tile_field()
    assert occ.shape == (9, 17, 67) and n_cases(occ, 0.5) == 256
    v, f = reference_mesh(occ, 0.5)
    facts = _mc.mesh_facts(v, f)
    assert (facts["V"], facts["F"]) == (14374, 27096)
    assert facts["components"][0] == 142 and facts["partitions_equal"]
    assert facts["max_valence"] == 20 == 4 * _mc.MAX_EDGE_TRIANGLES
    assert facts["zero_area"] == 0
    crossing = _mc.tile_face_crossings(occ, 0.5)
    assert crossing == [1117, 609, 140] and min(crossing) > 0
    # three tiles along every axis, the last one ragged
    assert [-(-n // t) for n, t in zip(occ.shape, (4, 8, 32))] == [3, 3, 3] and all(n % t for n, t in zip(occ.shape, (4, 8, 32)))


@pytest.mark.parametrize("level,cases", [(0.45, 256), (0.3, 247)])
def test_tile_field_at_levels_that_are_not_float32(level, cases):
    occ = _mc.tile_field()
    assert float(np.float32(level)) != level                                   # the level itself is rounded on its way to the kernel
    assert n_cases(occ, level) == cases and min(_mc.tile_face_crossings(occ, level)) > 0
    assert not (occ == np.float32(level)).any()


@pytest.mark.parametrize("shape", [(5, 9, 34), (4, 8, 32), (5, 8, 33), (4, 9, 32)])
def test_small_tile_shapes_have_crossings_on_every_axis(shape):
    flag, _ = _mc.crossings(_mc.noise_field(sum(shape), shape), 0.5)
    assert flag.reshape(-1, 3).sum(0).min() > 100


def test_big_field_has_one_huge_component_among_many():
    occ = _mc.big_field()
    v, f = reference_mesh(occ, 0.5)
    facts = _mc.mesh_facts(v, f)
    assert (facts["V"], facts["F"]) == (164621, 337016)
    assert facts["components"][0] == 1180 and facts["sizes"][-1] == 326717 and facts["sizes"][-2] == 72
    assert facts["partitions_equal"]


def test_sparse_field_has_components_of_many_sizes():
    v, f = reference_mesh(_mc.sparse_field(), 0.5)
    facts = _mc.mesh_facts(v, f)
    assert facts["components"][0] == 892 and len(np.unique(facts["sizes"])) == 40 and facts["sizes"][-1] == 200
    assert facts["partitions_equal"]


def test_integer_field_puts_the_level_on_lattice_values():
    occ = _mc.integer_field()
    assert (occ == 1.0).sum() > 1000 and n_cases(occ, 1.0) == 256
    v, f = reference_mesh(occ, 1.0)
    facts = _mc.mesh_facts(v, f)
    assert facts["zero_area"] == 3057 and facts["partitions_equal"] and facts["components"][0] == 64 and facts["max_valence"] == 20
    flag, t = _mc.crossings(occ, 1.0)
    assert (t[flag] == 0).any() and (t[flag] == 1).any()                        # vertices ON lattice points, from either end
    normals = _mc.normals_reference(v, f)
    assert int((~normals.any(1)).sum()) == 195                                  # vertices whose cross products sum to zero
    v2, f2 = reference_mesh(occ, 2.0)
    facts2 = _mc.mesh_facts(v2, f2)
    assert facts2["components"][0] == 456 and len(np.unique(facts2["sizes"])) == 43 and facts2["partitions_equal"]


def test_binary_field_has_every_vertex_at_a_midpoint():
    occ = _mc.binary_field()
    assert set(np.unique(occ).tolist()) == {0.0, 1.0}
    flag, t = _mc.crossings(occ, 0.5)
    assert flag.sum() > 1000 and (t[flag] == 0.5).all()
    v, f = reference_mesh(occ, 0.5)
    facts = _mc.mesh_facts(v, f)
    assert facts["components"][0] == 425 and facts["partitions_equal"]


def test_power_of_two_scaling_is_exact_until_the_values_turn_denormal():
    base = _mc.scale_base()
    v, f = reference_mesh(base, 0.0)
    assert (len(v), len(f)) == (3914, 6885)
    tiny = np.float32(2.0 ** -126)
    for exponent in (100, -100):
        occ = _mc.scaled(base, exponent)
        assert np.isfinite(occ).all() and not ((np.abs(occ) < tiny) & (occ != 0)).any()
        assert np.array_equal(np.ldexp(occ.astype(np.float64), -exponent), base.astype(np.float64))        # nothing was rounded
        vs, fs = reference_mesh(occ, 0.0)
        assert vs.tobytes() == v.tobytes() and np.array_equal(fs, f)
    occ = _mc.scaled(base, -140)
    assert int(((np.abs(occ) < tiny) & (occ != 0)).sum()) == 2846 and int((occ == 0).sum()) == 3
    assert occ[occ != 0].size and np.abs(occ).max() < tiny                      # every value denormal or zero - and numpy kept them
    vs, fs = reference_mesh(occ, 0.0)
    assert np.isfinite(vs).all() and len(vs) > 3000 and len(fs) == 6881


@pytest.mark.parametrize("n", [20, 21])
def test_fan_valence(n):
    f, nv = _mc.fan(n)
    assert nv == n + 1 and _mc.valence(f, nv)[0] == n and (_mc.valence(f, nv)[1:] == 2).all()
    assert 4 * _mc.MAX_EDGE_TRIANGLES == 20


# ---------------------------------------------------------------------------------------------------------------------
# the vertex-graph reference on meshes small enough to work out by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_vertex_components_ignore_faces_out_of_range_and_keep_lone_vertices():
    f = np.array([[0, 1, 2], [2, 3, 4], [6, 7, 8], [0, 6, 9], [-1, 6, 0]], np.int32)
    n, label = _mc.vertex_components(f, 9)
    assert n == 3 and len(set(label[:5])) == 1 and label[5] not in (label[0], label[6]) and len(set(label[6:])) == 1


def test_vertex_clean_reference_on_a_bow_tie():
    f, nv = _mc.bow_tie()
    keep_t, keep_v, out, sizes = _mc.clean_reference(f, nv, 2, False, graph="vertex")
    assert keep_t.all() and keep_v.all() and np.array_equal(out, f) and sizes.tolist() == [2]
    keep_t, keep_v, out, _ = _mc.clean_reference(f, nv, 3, False, graph="vertex")
    assert not keep_t.any() and not keep_v.any() and out.shape == (0, 3)
    assert _mc.edge_components(f)[0] == 2                                       # while no edge is shared


def test_vertex_clean_reference_breaks_a_tie_by_the_lowest_label():
    f, nv = _mc.two_equal_strips(5)
    keep_t, keep_v, out, sizes = _mc.clean_reference(f, nv, 0, True, graph="vertex")
    assert sizes.tolist() == [5, 5] and keep_t.tolist() == [False] * 5 + [True] * 5 and keep_v.tolist() == [True] * 7 + [False] * 7
    assert np.array_equal(out, f[5:])


def test_vertex_clean_reference_drops_bad_faces_and_unreferenced_vertices():
    f, nv = _mc.disjoint_triangles(4)
    f = np.concatenate([f[:2], [[-1, 0, 1]], f[2:], [[0, 1, nv + 3]]]).astype(np.int32)
    keep_t, keep_v, out, sizes = _mc.clean_reference(f, nv + 3, 1, False, graph="vertex")
    assert keep_t.tolist() == [True, True, False, True, True, False] and keep_v.tolist() == [True] * 12 + [False] * 3
    assert sizes.tolist() == [1, 1, 1, 1] and np.array_equal(out, _mc.disjoint_triangles(4)[0])


def test_foreign_mesh_builders():
    f, nv = _mc.strip(6, descending=True)
    assert f[0].tolist() == [7, 6, 5] and f[-1].tolist() == [2, 1, 0] and nv == 8
    f, nv = _mc.hub(7)
    assert nv == 15 and (f == 14).sum(1).tolist() == [1] * 7 and {int(np.argmax(row == 14)) for row in f} == {0, 1, 2}
    assert _mc.vertex_components(f, nv)[0] == 1 and _mc.edge_components(f)[0] == 7
    rng = np.random.default_rng(0)
    g = _mc.relabel(_mc.strip(50)[0], 52, rng)
    assert sorted(np.unique(g).tolist()) == list(range(52)) and _mc.vertex_components(g, 52)[0] == 1 and _mc.edge_components(g)[0] == 1
