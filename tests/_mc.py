"""numpy / scipy restatements for the marching-cubes and mesh-cleaning tests (no torch, no device).

  vertices(occ, level)        the straddling lattice edges enumerated independently of the kernels: float32 [V, 3] in the order owner
                              lattice point (linear index), then axis, and the vertex id of every (point, axis)
  faces(occ, level)           the case table (scripts/gen_mc_tables.py, imported - not the C header) applied cube by cube
  analytic fields, edge bookkeeping (directed edge multiplicities, Euler characteristic), enclosed volume, the shared-edge triangle graph
  the seeded lattices of the boundary tests (tile_field, big_field, ...), the vertex graph (vertex_components) and the cleaning contract
  on it (clean_reference(graph="vertex")), mesh_facts, and small meshes no marching cubes made (fan, strip, hub, bow_tie, ...)
"""
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def generator():
    spec = importlib.util.spec_from_file_location("gen_mc_tables", os.path.join(REPO, "scripts", "gen_mc_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GEN = generator()
TABLE, MAX_TRIANGLES, MAX_EDGE_TRIANGLES = _GEN.build()
EDGES = _GEN.EDGES                                        # [(axis, low corner, high corner)]


def inside(occ, level):
    with np.errstate(invalid="ignore"):
        return occ > np.float32(level)


def crossings(occ, level):
    """(bool [nx, ny, nz, 3]: the owned edge towards +axis straddles the level, float32 [nx, ny, nz, 3]: its t = (level - v0) / (v1 - v0))"""
    occ = np.asarray(occ, np.float32)
    level = np.float32(level)
    ins = inside(occ, level)
    shape = occ.shape
    flag = np.zeros(shape + (3,), bool)
    t = np.zeros(shape + (3,), np.float32)
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        flag[lo + (axis,)] = ins[lo] != ins[hi]
        with np.errstate(all="ignore"):
            t[lo + (axis,)] = (level - occ[lo]) / (occ[hi] - occ[lo])            # float32 throughout
    return flag, t


def vertices(occ, level):
    """(float32 [V, 3], int64 [nx, ny, nz, 3] vertex id or -1)"""
    flag, t = crossings(occ, level)
    ids = np.full(flag.shape, -1, np.int64)
    ids[flag] = np.arange(int(flag.sum()))                                       # C order: point linear index, then axis
    idx = np.argwhere(flag)                                                      # same order
    verts = idx[:, :3].astype(np.float32)
    rows = np.arange(idx.shape[0])
    verts[rows, idx[:, 3]] = verts[rows, idx[:, 3]] + t[flag]
    return verts, ids


def cases(occ, level):
    """uint8 [nx - 1, ny - 1, nz - 1]: bit c = di | dj << 1 | dk << 2 set iff that corner is inside"""
    ins = inside(np.asarray(occ, np.float32), level)
    nx, ny, nz = ins.shape
    out = np.zeros((nx - 1, ny - 1, nz - 1), np.uint8)
    for c in range(8):
        di, dj, dk = c & 1, (c >> 1) & 1, c >> 2
        out |= ins[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk].astype(np.uint8) << c
    return out


def faces(occ, level, ids=None):
    """int32 [F, 3]: cube by cube in linear order, the table's triangles, vertex ids of the edges' owners"""
    if ids is None:
        ids = vertices(occ, level)[1]
    cs = cases(occ, level)
    out = []
    for i, j, k in np.argwhere(cs > 0):
        for tri in TABLE[int(cs[i, j, k])]:
            row = []
            for e in tri:
                axis, lo, _ = EDGES[e]
                row.append(ids[i + (lo & 1), j + ((lo >> 1) & 1), k + (lo >> 2), axis])
            out.append(row)
    return np.asarray(out, np.int32).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------------------------
def lattice(shape):
    return np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1)


def sphere_field(shape, centre, radius):
    return (radius - np.linalg.norm(lattice(shape) - np.asarray(centre, np.float64), axis=-1)).astype(np.float32)


def torus_field(shape, centre, major, minor):
    p = lattice(shape) - np.asarray(centre, np.float64)
    q = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - major
    return (minor - np.sqrt(q ** 2 + p[..., 2] ** 2)).astype(np.float32)


def noise_field(seed, shape):
    return np.random.default_rng(seed).uniform(0, 1, shape).astype(np.float32)


# The lattices of tests/test_mcubes_edges_gpu.py; tests/test_mc_reference_cpu.py holds what each is chosen for and checks it.
TILE_SHAPE = (9, 17, 67)                                 # three ragged classify tiles (4 x 8 x 32 lattice points) along every axis
BIG_SHAPE = (40, 40, 70)


def tile_field():
    return noise_field(1, TILE_SHAPE)


def big_field():
    return noise_field(8, BIG_SHAPE)


def sparse_field():
    return noise_field(4, (13, 19, 41)) ** 3


def integer_field():
    return np.random.default_rng(5).integers(0, 4, (9, 17, 35)).astype(np.float32)


def binary_field():
    return (np.random.default_rng(6).uniform(0, 1, (9, 17, 35)) > 0.7).astype(np.float32)


def scale_base():
    return noise_field(2, (7, 11, 37)) - np.float32(0.5)


def scaled(occ, exponent):
    """occ * 2^exponent, rounded once to float32 (exact unless the result is denormal)"""
    return np.ldexp(np.asarray(occ, np.float64), exponent).astype(np.float32)


def tile_face_crossings(occ, level, tile=(4, 8, 32)):
    """per axis: the straddling edges whose owner is the last point of a classify tile along that axis - its far end is a halo value"""
    flag, _ = crossings(occ, level)
    index = np.meshgrid(*[np.arange(n) for n in flag.shape[:3]], indexing="ij")
    return [int(flag[..., axis][index[axis] % tile[axis] == tile[axis] - 1].sum()) for axis in range(3)]


# ---------------------------------------------------------------------------------------------------------------------
# mesh bookkeeping
# ---------------------------------------------------------------------------------------------------------------------
def mesh_facts(v, f):
    """what the boundary tests rely on, of a mesh (vertices [V, 3], faces [F, 3]): V, F, the shared-edge components (scipy's result and
    their sizes in ascending order), whether the vertex graph splits the triangles the same way, the largest valence, the number of
    zero-area triangles"""
    f = np.asarray(f, np.int64)
    components = edge_components(f)
    by_vertex = vertex_components(f, len(v))[1][f[:, 0]]
    return {"V": len(v), "F": len(f), "components": components, "sizes": np.sort(np.bincount(components[1])),
            "partitions_equal": same_partition(components[1], by_vertex), "max_valence": int(valence(f, len(v)).max()),
            "zero_area": int(zero_area(v, f).sum())}


def directed_edges(f):
    f = np.asarray(f, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)


def edge_table(f):
    """per undirected edge (a < b): (keys [E, 2], count a -> b, count b -> a)"""
    d = directed_edges(f)
    fwd = d[:, 0] < d[:, 1]
    und = np.where(fwd[:, None], d, d[:, ::-1])
    keys, inv = np.unique(und, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    return keys, np.bincount(inv[fwd], minlength=len(keys)), np.bincount(inv[~fwd], minlength=len(keys))


def euler(f):
    f = np.asarray(f, np.int64)
    keys, _, _ = edge_table(f)
    return len(np.unique(f)) - len(keys) + len(f)


def volume(v, f):
    """enclosed volume by the divergence theorem: sum over triangles of a . (b x c) / 6 (normals outward = positive)"""
    v = np.asarray(v, np.float64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def edge_components(f):
    """(number of components, label per triangle) of the graph whose nodes are triangles and whose links are shared undirected edges -
    open3d's cluster_connected_triangles"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(f, np.int64)
    d = directed_edges(f)
    und = np.sort(d, axis=1)
    tri = np.tile(np.arange(len(f)), 3)
    _, inv = np.unique(und[:, 0] * (int(und.max(initial=0)) + 1) + und[:, 1], return_inverse=True)      # one int64 key per undirected edge
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    inv_s, tri_s = inv[order], tri[order]
    same = inv_s[1:] == inv_s[:-1]                                              # consecutive triangles of one edge: a chain links them all
    g = coo_matrix((np.ones(int(same.sum())), (tri_s[:-1][same], tri_s[1:][same])), shape=(len(f), len(f)))
    return connected_components(g, directed=False)


def vertex_components(f, n_vertices):
    """(number of components, label per vertex) of the graph whose nodes are the n_vertices vertices and whose links are triangle
    sides; a face with an index outside [0, n_vertices) is ignored, a vertex no face names is a component of its own"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(f, np.int64).reshape(-1, 3)
    f = f[((f >= 0) & (f < n_vertices)).all(1)]
    d = directed_edges(f)
    g = coo_matrix((np.ones(len(d)), (d[:, 0], d[:, 1])), shape=(n_vertices, n_vertices))
    return connected_components(g, directed=False)


def same_partition(a, b):
    """two label arrays split their items into the same groups"""
    a, b = np.asarray(a), np.asarray(b)
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return a.shape == b.shape and len(pairs) == len(np.unique(a)) == len(np.unique(b))


def clean_reference(f, n_vertices, min_triangles, keep_single, graph="edge", components=None):
    """(kept triangle mask, kept vertex mask, re-indexed faces, triangles per component).

    graph="edge": by the shared-edge components (``components``: a result of edge_components(f) computed earlier).
    graph="vertex": the contract of inerf_mesh_clean - components of the vertex graph, each labelled by its smallest vertex index,
    its triangles counted by their first vertex; keep_single keeps the component with the most triangles, a tie going to the lowest
    label; faces with an index outside [0, n_vertices) are dropped, and so are the vertices no kept triangle names.  The sizes are
    those of the components that own a triangle, in ascending label."""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    if graph == "vertex":
        valid = ((f >= 0) & (f < n_vertices)).all(1)
        _, comp = vertex_components(f, n_vertices)
        smallest = np.full(comp.max() + 1 if n_vertices else 0, n_vertices, np.int64)
        np.minimum.at(smallest, comp, np.arange(n_vertices))
        label = smallest[comp]                                                  # per vertex: the smallest index of its component
        tri_label = np.where(valid, label[np.where(valid, f[:, 0], 0)], -1)
        count = np.bincount(tri_label[valid], minlength=n_vertices)             # per label
        if keep_single:
            best = min(np.flatnonzero(count > 0), key=lambda c: (-count[c], c)) if valid.any() else -2
            keep_t = tri_label == best
        else:
            keep_t = valid & (count[np.where(valid, tri_label, 0)] >= min_triangles)
        sizes = count[count > 0]
    elif graph == "edge":
        n, label = edge_components(f) if components is None else components
        sizes = np.bincount(label, minlength=n)
        if keep_single:
            first_vertex = np.full(n, n_vertices, np.int64)
            np.minimum.at(first_vertex, label, f.min(1))
            best = sorted(range(n), key=lambda c: (-sizes[c], first_vertex[c]))[0]
            keep_t = label == best
        else:
            keep_t = sizes[label] >= min_triangles
    else:
        raise ValueError(graph)
    keep_v = np.zeros(n_vertices, bool)
    keep_v[f[keep_t].reshape(-1)] = True
    new = np.cumsum(keep_v) - 1
    return keep_t, keep_v, new[f[keep_t]].astype(np.int32), sizes


def valence(f, n_vertices):
    """triangles that name each vertex (a triangle that names it twice counts twice, as the kernels' slots do)"""
    return np.bincount(np.asarray(f, np.int64).reshape(-1), minlength=n_vertices)


def zero_area(v, f):
    """bool per triangle: the fp64 cross product (b - a) x (c - a) is the zero vector"""
    v = np.asarray(v, np.float64)
    f = np.asarray(f, np.int64)
    return ~np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).any(1)


# ---------------------------------------------------------------------------------------------------------------------
# small meshes from elsewhere: (int32 faces [F, 3], number of vertices)
# ---------------------------------------------------------------------------------------------------------------------
def fan(n):
    """n triangles about vertex 0 (a closed umbrella over the rim 1 .. n)"""
    return np.array([[0, 1 + t, 1 + (t + 1) % n] for t in range(n)], np.int32), n + 1


def strip(n, descending=False):
    """a strip of n triangles (t, t + 1, t + 2) over n + 2 vertices; descending: vertex v renamed n + 1 - v, so that indices fall
    along the strip and every union hooks the vertex met earlier under the one met later"""
    f = np.arange(n, dtype=np.int64)[:, None] + np.arange(3)
    if descending:
        f = n + 1 - f
    return f.astype(np.int32), n + 2


def relabel(f, n_vertices, rng):
    """the same mesh with its vertices renamed by a random permutation and its triangles in a random order"""
    perm = rng.permutation(n_vertices)
    return perm[np.asarray(f, np.int64)][rng.permutation(len(f))].astype(np.int32)


def hub(n):
    """n triangles that share nothing but the LAST vertex (2 n), which takes each of the three positions in turn"""
    t = np.arange(n, dtype=np.int64)
    f = np.stack([np.full(n, 2 * n), 2 * t, 2 * t + 1], 1)
    cols = (np.arange(3)[None, :] - (t % 3)[:, None]) % 3                       # row t rolled by t % 3: a cyclic shift keeps the winding
    return np.take_along_axis(f, cols, 1).astype(np.int32), 2 * n + 1


def bow_tie():
    """two triangles that share one vertex and no edge"""
    return np.array([[0, 1, 2], [2, 3, 4]], np.int32), 5


def disjoint_triangles(n):
    return np.arange(3 * n, dtype=np.int32).reshape(n, 3), 3 * n


def two_equal_strips(n):
    """two strips of n triangles each; the one whose triangles come SECOND holds vertex 0, so the lowest label is not the first met"""
    a, nv = strip(n)
    return np.concatenate([a + nv, a]).astype(np.int32), 2 * nv


def normals_reference(v, f):
    """fp64: np.add.at of the cross products in ascending triangle order (triangle by triangle, its three corners), then the division
    by sqrt((x x + y y) + z z); a zero sum stays zero"""
    v = np.asarray(v, np.float64)
    f = np.asarray(f, np.int64)
    u, w = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    cr = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    n = np.zeros_like(v)
    np.add.at(n, f.reshape(-1), np.repeat(cr, 3, axis=0))
    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    ok = length > 0
    n[ok] = n[ok] / length[ok, None]
    return n


def read_ply(path):
    """a small reader for the binary little-endian PLY files geometry.write_ply writes: {property name: array}, faces int32 [F, 3]"""
    types = {"double": "<f8", "float": "<f4", "uchar": "u1", "int": "<i4"}
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    counts, props, element = {}, {}, None
    for line in lines[2:]:
        w = line.split()
        if w[:1] == ["element"]:
            element = w[1]
            counts[element] = int(w[2])
            props[element] = []
        elif w[:1] == ["property"]:
            props[element].append(w[1:])
    vdtype = np.dtype([(p[1], types[p[0]]) for p in props["vertex"]])
    nv, nf = counts["vertex"], counts["face"]
    verts = np.frombuffer(data, vdtype, nv, end)
    assert props["face"] == [["list", "uchar", "int", "vertex_indices"]]
    fdtype = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    tris = np.frombuffer(data, fdtype, nf, end + nv * vdtype.itemsize)
    assert end + nv * vdtype.itemsize + nf * fdtype.itemsize == len(data) and (tris["n"] == 3).all()
    return {name: verts[name] for name in vdtype.names}, tris["v"].copy()
