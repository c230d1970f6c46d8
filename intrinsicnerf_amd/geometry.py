"""Geometry out of a trained scene: the query lattice of mesh extraction and the occupancy of a network on it.

Mirrors, with the reference's names, arguments and returned tensors (citations relative to ``/root/reference/SSR``):
  grid_within_bound, make_3D_grid      geometry/occupancy.py:5-48
  occupancy_grid                       extract_colour_mesh.py:149-185 (lattice, chunk loop over run_network, raw[..., 3],
                                       occupancy_activation) - one launch of ``inerf_occupancy_grid`` on the fused networks
  vertex_rays                          extract_colour_mesh.py:232-238 (one ray per mesh vertex, against its normal) - one launch of
                                       ``inerf_vertex_rays``
  vertex_colours                       extract_colour_mesh.py:27-41, 232-257 (the rays, the chunk loop over render_rays, to8b or
                                       valid_colour_map[label]) - three bytes per vertex reach the host, once
  marching_cubes, lattice_to_scene     extract_colour_mesh.py:186-201 (skimage.measure.marching_cubes, /(dim - 1), -0.5, x2, x extents / 2,
                                       transform) - ``inerf_mc_count`` + ``inerf_mc_emit``: welded vertices, fp64 scene coordinates, int32 faces
  vertex_normals                       open3d's compute_vertex_normals (open3d_utils.trimesh_to_open3d) - ``inerf_mesh_normals``
  clean_mesh                           open3d_utils.clean_mesh, :214 - ``inerf_mesh_clean``
  extract_mesh                         :149-219 chained on the device: two host reads of a few counters, nothing else leaves it
  write_ply                            o3d.io.write_triangle_mesh, :263-266 - binary little-endian PLY, numpy on the host
The triangulation is this project's own (csrc/mc_tables.h), not skimage's: DESIGN.md section 3, INTEGRATION.md.
"""
import numpy as np
import torch

from . import _capi, kernels, layered, packing
from .object_level import Embedder

__all__ = ["grid_within_bound", "make_3D_grid", "occupancy_grid", "occupancy_activation", "vertex_rays", "vertex_colours",
           "marching_cubes", "lattice_to_scene", "vertex_normals", "clean_mesh", "extract_mesh", "write_ply"]

STATUS_POINTS = 1 << 20        # lattice points per f16 range word of the fused launch - and per launch of the other paths
VERTEX_CHUNK = 1 << 16         # vertices per render_rays call of vertex_colours


def _rows34(transform):
    """rows 0..2 of a [3 | 4, 4] matrix as twelve fp32-rounded numbers (occupancy.py:9: from_numpy(...).float())"""
    m = torch.as_tensor(np.asarray(transform.detach().cpu() if isinstance(transform, torch.Tensor) else transform)).float()
    if m.dim() != 2 or m.shape[0] < 3 or m.shape[1] != 4:
        raise ValueError(f"transform has shape {tuple(m.shape)}, expected [4, 4] (or its first three rows)")
    return m[:3].reshape(-1).tolist()


def _scale3(scale):
    s = torch.as_tensor(np.asarray(scale.detach().cpu() if isinstance(scale, torch.Tensor) else scale)).float().reshape(-1)
    if s.numel() == 1:
        s = s.expand(3)
    if s.numel() != 3:
        raise ValueError(f"scale holds {s.numel()} numbers, expected 3")
    return s.tolist()


def _axis(occ_range, dim, device):
    """torch.linspace on the CPU, as occupancy.py:25 evaluates it (its roundings are what the lattice's bits start from)"""
    t = torch.linspace(occ_range[0], occ_range[1], steps=int(dim))
    return t if device is None or torch.device(device).type == "cpu" else t.to(device)


def make_3D_grid(occ_range, dim, transform=None, scale=None, device=None):
    """``[dim, dim, dim, 3]`` lattice of occupancy.py:24-48: linspace(occ_range) per axis, times ``scale``, through the rotation and
    translation of ``transform`` - the reference's CPU bits, produced by ``inerf_grid_points`` on ``device`` or, without one, by
    ``inerf_grid_points_host``.  ``scale`` None: no scaling; ``transform`` None: the scaled lattice itself (occupancy.py:33-35)."""
    dim = int(dim)
    t = _axis(occ_range, dim, device)
    sc = [1.0, 1.0, 1.0] if scale is None else _scale3(scale)
    if transform is None:
        g = torch.stack(torch.meshgrid(t, t, t, indexing="ij"), dim=3)
        return g if scale is None else g * torch.tensor(sc, device=t.device)
    return kernels.grid_points(t, sc, _rows34(transform)).reshape(dim, dim, dim, 3)


def _scene_scale(occ_range, extents):
    return torch.from_numpy(np.asarray(extents) / ((occ_range[1] - occ_range[0]) * 0.9)).float()      # occupancy.py:6-11


def grid_within_bound(occ_range, extents, transform, grid_dim, device=None):
    """``(grid_pc [-1, 1, 3], scene_scale [3])`` of occupancy.py:5-22: the lattice inside the oriented bounding box
    (``extents``, ``transform`` = box to scene, numpy as trimesh gives them)."""
    scene_scale = _scene_scale(occ_range, extents)
    grid_pc = make_3D_grid(occ_range, grid_dim, transform=transform, scale=scene_scale, device=device)
    return grid_pc.view(-1, 1, 3), scene_scale


def occupancy_activation(alpha, distances):
    """extract_colour_mesh.py:172-175 (relu before the exponential; a NaN stays one)"""
    return 1.0 - torch.exp(-torch.relu(alpha) * distances)


def _fused_desc(net, embed_fn):
    """Descriptor when ``inerf_occupancy_grid`` takes (net, embed_fn), else None.  (The density needs neither the direction
    encoder nor the class count to be the kernels' own.)"""
    if not hasattr(net, "fused_desc") or not isinstance(embed_fn, Embedder):
        return None
    desc = net.fused_desc()
    if desc is None or embed_fn.n_freqs != desc.l_xyz or embed_fn.input_dims != 3:
        return None
    if desc.variant != _capi.VARIANT_SSR and embed_fn.scalar_factor != 1.0:
        return None
    desc.xyz_div = embed_fn.scalar_factor
    return desc


def _dirs_encoder(net, embeddirs_fn):
    if embeddirs_fn is not None or not getattr(net, "use_viewdirs", False):
        return embeddirs_fn
    n, r = divmod(int(getattr(net, "input_ch_views", 3)) - 3, 6)
    return Embedder(n) if r == 0 and n >= 0 else None


def _sigma_exact(net, embed_fn, embeddirs_fn, desc, pts):
    """channel 3 of the network on ``pts`` [n, 3] along the existing paths: the fused kernels in exact fp32, the layer kernels for other
    depths and widths, a foreign callable through its own forward (run_network with zero view directions, as the reference calls it)"""
    n = pts.shape[0]
    if desc is not None:
        d32 = _capi.NetDesc(desc.variant, desc.n_classes, desc.l_xyz, desc.l_dir, desc.xyz_div, _capi.PREC_F32)
        rays = torch.zeros(n, _capi.RAY_FLOATS, dtype=torch.float32, device=pts.device)
        rays[:, 0:3] = pts
        z = torch.zeros(n, 1, dtype=torch.float32, device=pts.device)
        return kernels.encode_mlp(d32, packing.packed_for_module(net, d32, pts.device), rays, z)[:, 0, 3]
    dirs_fn = _dirs_encoder(net, embeddirs_fn)
    dirs = torch.zeros(n, 3, dtype=torch.float32, device=pts.device) if dirs_fn is not None else None
    spec = layered.spec_for(net, embed_fn, dirs_fn)
    if spec is not None and spec.use_viewdirs == (dirs is not None):
        return layered.evaluate_points(spec, net, pts[:, None, :], dirs)[:, 0, 3]
    emb = embed_fn(pts)
    if dirs is not None:
        emb = torch.cat([emb, dirs_fn(dirs)], -1)
    return net(emb)[..., 3]


def occupancy_grid(net, embed_fn, occ_range, extents, transform, grid_dim, distances, return_sigma=False, chunk_points=None,
                   embeddirs_fn=None):
    """``occ[dim, dim, dim] = 1 - exp(-relu(sigma) * distances)`` of ``net`` on the lattice of ``grid_within_bound`` - what
    extract_colour_mesh.py:149-185 hands to marching cubes - on the device of ``net``; with ``return_sigma`` ``(occ, sigma)``.

    A network the fused kernels take (D=8, W=256, skips=[4], this package's position encoder) in f16x3 mode: one
    ``inerf_occupancy_grid`` launch per ``chunk_points`` lattice points (default: the whole lattice), with one f16 range word per
    2^20 points; the spans of flagged words are evaluated again in exact fp32 (``inerf_grid_points`` + ``inerf_encode_mlp``), announced
    like every such fallback.  ``INERF_PRECISION=f32``, other depths or widths and foreign callables: ``inerf_grid_points``, then the
    existing path 2^20 points at a time, channel 3, the same activation (``embeddirs_fn``: the direction encoder a foreign callable
    expects, fed zeros as the reference feeds it; this package's networks need none).  Never reads anything back but the range words."""
    with torch.no_grad():
        dim = int(grid_dim)
        if not 2 <= dim <= _capi.MAX_GRID_DIM:
            raise ValueError(f"grid_dim = {dim}: expected 2 .. {_capi.MAX_GRID_DIM}")
        params = list(net.parameters()) if isinstance(net, torch.nn.Module) else []
        device = params[0].device if params else torch.device("cuda", torch.cuda.current_device())
        if device.type != "cuda":
            raise RuntimeError(f"occupancy_grid: the network lives on {device}: intrinsicnerf_amd runs only on a HIP device")
        t = _axis(occ_range, dim, device)
        sc, m = _scene_scale(occ_range, extents).tolist(), _rows34(transform)
        total, dist = dim ** 3, float(distances)
        occ = torch.empty(total, dtype=torch.float32, device=device)
        sigma = torch.empty(total, dtype=torch.float32, device=device) if return_sigma else None
        desc = _fused_desc(net, embed_fn)

        def exact(first, count):
            s = _sigma_exact(net, embed_fn, embeddirs_fn, desc, kernels.grid_points(t, sc, m, first, count)).float()
            if sigma is not None:
                sigma[first:first + count] = s
            occ[first:first + count] = occupancy_activation(s, dist)

        if desc is not None and desc.precision == _capi.PREC_F16X3:
            packed = packing.packed_for_module(net, desc, device)
            status = torch.zeros(-(-total // STATUS_POINTS), dtype=torch.int32, device=device)
            step = total if not chunk_points else max(1, int(chunk_points))
            for first in range(0, total, step):
                count = min(step, total - first)
                kernels.occupancy_grid(desc, packed, t, sc, m, dist, first, count, occ[first:first + count], None if sigma is None else sigma[first:first + count],
                                       status, STATUS_POINTS)
            flagged = [w for w, f in enumerate(status.cpu().tolist()) if int(f) & _capi.STATUS_F16_RANGE]      # the one host sync
            if flagged:
                kernels.warn_f32_fallback(f"occupancy_grid: {len(flagged)} of {status.numel()} chunks left the f16 range of the "
                                          "split-precision MLP kernel.")
                for w in flagged:
                    exact(w * STATUS_POINTS, min(STATUS_POINTS, total - w * STATUS_POINTS))
        else:
            step = STATUS_POINTS if not chunk_points else max(1, int(chunk_points))
            for first in range(0, total, step):
                exact(first, min(step, total - first))
        occ = occ.reshape(dim, dim, dim)
        return (occ, sigma.reshape(dim, dim, dim)) if return_sigma else occ


def _vertex_pair(vertices, normals):
    """``vertices`` and ``normals`` (numpy or torch, float32 or float64) as two [V, 3] tensors of one dtype, where they are, uncopied
    unless their dtypes differ (float64 then: its rounding to fp32 is the reference's)."""
    out = []
    for name, a in (("vertices", vertices), ("normals", normals)):
        t = a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
        if t.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{name} must be float32 or float64, got {t.dtype}")
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected [V, 3]")
        out.append(t)
    v, m = out
    if v.shape != m.shape:
        raise ValueError(f"vertices {tuple(v.shape)} and normals {tuple(m.shape)} do not match: one normal per vertex")
    if v.dtype != m.dtype:
        v, m = v.double(), m.double()
    return v, m


def vertex_rays(vertices, normals, near=0.1, far=10.0, near_t=2.0, device=None):
    """``[V, 11]`` ray batch of extract_colour_mesh.py:232-238 - ``rays_d = -normals``, ``rays_o = vertices - rays_d * near * near_t``,
    ``viewdirs = rays_d / |rays_d|``, ``cat([rays_o, rays_d, near, far, viewdirs])`` - with the reference's CPU bits.  ``vertices`` /
    ``normals``: [V, 3], numpy or torch, float32 or float64 (``np.asarray(mesh.vertices)`` goes in as it is; float64 is rounded to fp32
    inside, as ``torch.FloatTensor`` does).  ``device`` None: where the inputs live - ``inerf_vertex_rays_host`` on the CPU; a device:
    the arrays are uploaded as they are and ``inerf_vertex_rays`` runs there, one launch."""
    v, m = _vertex_pair(vertices, normals)
    if device is not None:
        v, m = v.to(device), m.to(device)
    elif v.device != m.device:
        raise ValueError(f"vertices are on {v.device} and normals on {m.device}")
    return kernels.vertex_rays(v, m, near, far, near_t)


def _colour_map(colour_map):
    """the caller's valid_colour_map as a uint8 [C, 3] CPU tensor (extract_colour_mesh.py:250, 257: indexed, then .astype(np.uint8))"""
    t = colour_map.detach().cpu() if isinstance(colour_map, torch.Tensor) else torch.as_tensor(np.asarray(colour_map))
    if t.dim() != 2 or t.shape[1] != 3 or not 1 <= t.shape[0] <= _capi.MAX_CLASSES:
        raise ValueError(f"colour_map has shape {tuple(t.shape)}, expected [C, 3] with 1 <= C <= {_capi.MAX_CLASSES}")
    return t.to(torch.uint8).contiguous()


def vertex_colours(render_rays, vertices, normals, *, near=0.1, far=10.0, near_t=2.0, sem=False, colour_map=None, chunk=None,
                   return_labels=False):
    """``uint8 [V, 3]`` vertex colours of extract_colour_mesh.py:232-257 as a numpy array (with ``return_labels``: ``(colours, int32 [V]
    labels)``): ``to8b(rgb_fine)`` of the ray cast against every vertex normal or, with ``sem``, ``colour_map[label]`` of
    ``sem_logits_fine`` (``colour_map``: the caller's ``valid_colour_map`` [C, 3], numpy or tensor; the label is ``kernels.sem_maps``').

    ``render_rays``: ``rays [n, 11] -> dict`` (``SSRTrainer.render_rays`` with ``return_raw = False``: SSRRenderMixin.vertex_colours sets
    that).  ``chunk`` vertices (default 65 536) at a time: their rays are built on the device (``inerf_vertex_rays``), rendered, and the one
    key that is needed - ``rgb_fine`` / ``sem_logits_fine``, the ``_coarse`` keys of a render without a fine pass - goes through
    ``inerf_vertex_colours`` into a device ``uint8 [V, 3]``.  Nothing is read back per chunk and no [V, ...] float tensor exists; one copy
    to the host at the end.  Rays are independent, so the bytes do not depend on ``chunk``."""
    v, m = _vertex_pair(vertices, normals)
    if sem and colour_map is None:
        raise ValueError("sem=True needs colour_map (the [C, 3] valid_colour_map of the scene)")
    if return_labels and not sem:
        raise ValueError("return_labels needs sem=True")
    cmap = _colour_map(colour_map) if sem else None
    chunk = VERTEX_CHUNK if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk = {chunk}: expected a positive number of vertices")
    total = v.shape[0]
    with torch.no_grad():
        device = v.device if v.is_cuda else (m.device if m.is_cuda else torch.device("cuda", torch.cuda.current_device()))
        colours = torch.empty(total, 3, dtype=torch.uint8, device=device)
        labels = torch.empty(total, dtype=torch.int32, device=device) if return_labels else None
        cmap = None if cmap is None else cmap.to(device)
        what = "sem_logits" if sem else "rgb"
        for first in range(0, total, chunk):
            count = min(chunk, total - first)
            rays = kernels.vertex_rays(v[first:first + count].to(device), m[first:first + count].to(device), near, far, near_t)
            ret = render_rays(rays)
            x = ret.get(what + "_fine", ret.get(what + "_coarse"))
            if x is None:
                raise KeyError(f"render_rays returned neither {what}_fine nor {what}_coarse")
            x = x.reshape(count, -1)
            kernels.vertex_colours(rgb=None if sem else x, logits=x if sem else None, colour_map=cmap, out=colours[first:first + count],
                                   labels=None if labels is None else labels[first:first + count])
        colours = colours.cpu().numpy()
        return (colours, labels.cpu().numpy()) if return_labels else colours


def lattice_to_scene(dims, extents, transform):
    """The fp64 3 x 4 map (numpy) from lattice coordinates to scene coordinates of extract_colour_mesh.py:190-201 composed into one:
    ``/ (dim - 1)``, ``- 0.5``, ``x 2``, ``x extents / 2``, then ``transform`` (box to scene, [4, 4] or its first three rows).
    ``dims``: the lattice's points per axis, one number or three."""
    d = np.broadcast_to(np.asarray(dims, np.float64).reshape(-1), (3,))
    if (d < 2).any():
        raise ValueError(f"dims = {dims}: at least two lattice points per axis")
    e = np.broadcast_to(np.asarray(extents, np.float64).reshape(-1), (3,))
    t = np.asarray(transform.detach().cpu() if isinstance(transform, torch.Tensor) else transform, np.float64)
    if t.ndim != 2 or t.shape[0] < 3 or t.shape[1] != 4:
        raise ValueError(f"transform has shape {t.shape}, expected [4, 4] (or its first three rows)")
    scale = 2.0 / (d - 1.0) * (e / 2.0)                  # x -> (x / (dim - 1) - 0.5) * 2 * extents / 2 = x * scale - extents / 2
    out = np.empty((3, 4), np.float64)
    out[:, :3] = t[:3, :3] * scale[None, :]
    out[:, 3] = t[:3, :3] @ (-e / 2.0) + t[:3, 3]
    return out


def marching_cubes(occ, level, affine=None):
    """``(vertices_lattice float32 [V, 3], vertices_scene float64 [V, 3] | None, faces int32 [F, 3])`` of the isosurface ``occ == level``
    of a device lattice [nx, ny, nz], on the device.  Vertices lie on the lattice edges whose ends differ in ``occ > level``, in the
    order owner lattice point, then axis (``index + (level - v0) / (v1 - v0)`` in fp32); faces wind so that their normals point
    towards lower values.  ``affine``: a 3 x 4 fp64 map (``lattice_to_scene``) for the scene coordinates.  One host read of three
    counters sizes the outputs; a lattice with a NaN or an infinity raises."""
    with torch.no_grad():
        workspace, totals = kernels.mc_count(occ, level)
        nv, nt, bad = (int(x) for x in totals.cpu().tolist())                                        # the one host sync
        if bad:
            raise ValueError(f"marching_cubes: the lattice holds {bad} non-finite values")
        a = None if affine is None else np.asarray(affine, np.float64)[:3].reshape(-1).tolist()
        return kernels.mc_emit(occ, level, workspace, nv, nt, a)


def vertex_normals(vertices, faces):
    """float64 [V, 3] area-weighted vertex normals (open3d's compute_vertex_normals as far as it is known without it: DESIGN.md section 3)
    of a device mesh: the fp64 sum of the incident triangles' cross products in ascending triangle index, normalised; a zero sum stays
    zero.  ``vertices``: float32 or float64 [V, 3]; ``faces``: int32 [F, 3]."""
    with torch.no_grad():
        return kernels.mesh_normals(vertices.double() if isinstance(vertices, torch.Tensor) else vertices, faces)


def clean_mesh(vertices, faces, normals=None, vertices_lattice=None, min_num_cluster=400, keep_single_cluster=False, return_counts=False):
    """open3d_utils.clean_mesh on the device: ``(vertices, faces, normals, vertices_lattice)`` without the connected components of fewer
    than ``min_num_cluster`` triangles (``keep_single_cluster``: without all but the largest) and without the vertices nothing
    references any more, order kept, faces re-indexed.  ``vertices`` / ``normals``: float64 [V, 3] (normals may be None),
    ``vertices_lattice``: float32 [V, 3] or None.  One host read of four counters; ``return_counts`` appends them as a dict."""
    with torch.no_grad():
        v = vertices.double()
        f_out, l_out, v_out, n_out, totals = kernels.mesh_clean(faces, v.shape[0], min_num_cluster, keep_single_cluster, rows_f32=vertices_lattice,
                                                                rows_f64_a=v, rows_f64_b=None if normals is None else normals.double())
        nv, nt, comps, kept = (int(x) for x in totals.cpu().tolist())                                  # the one host sync
        out = (v_out[:nv], f_out[:nt], None if n_out is None else n_out[:nv], None if l_out is None else l_out[:nv])
        return out + ({"vertices": nv, "triangles": nt, "components": comps, "kept_components": kept},) if return_counts else out


def extract_mesh(net, embed_fn, extents, transform, grid_dim, distances, level, occ_range=(-1., 1.), min_num_cluster=400,
                 keep_single_cluster=False, embeddirs_fn=None):
    """extract_colour_mesh.py:149-219 on the device: ``occupancy_grid``, ``marching_cubes`` with ``lattice_to_scene``, ``vertex_normals``
    and ``clean_mesh``.  Returns ``(vertices float64 [V, 3] in scene coordinates, faces int32 [F, 3], normals float64 [V, 3])``, device
    tensors.  Two host reads of a few counters (marching cubes' totals, the cleaning's), plus the grid's range words."""
    occ = occupancy_grid(net, embed_fn, occ_range, extents, transform, grid_dim, distances, embeddirs_fn=embeddirs_fn)
    _, scene, faces = marching_cubes(occ, level, lattice_to_scene(grid_dim, extents, transform))
    normals = vertex_normals(scene, faces)
    vertices, faces, normals, _ = clean_mesh(scene, faces, normals, min_num_cluster=min_num_cluster, keep_single_cluster=keep_single_cluster)
    return vertices, faces, normals


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def write_ply(path, vertices, faces, colours=None, normals=None):
    """Binary little-endian PLY: float64 x y z (as open3d writes them), optional float64 nx ny nz, optional uchar red green blue, then
    ``uchar 3, int32 x 3`` per face.  Arrays may be numpy or tensors (device tensors are copied to the host here)."""
    v = np.ascontiguousarray(_host(vertices), np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(_host(faces), np.int32).reshape(-1, 3)
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    header = ["ply", "format binary_little_endian 1.0", "comment intrinsicnerf_amd", f"element vertex {v.shape[0]}",
              "property double x", "property double y", "property double z"]
    if normals is not None:
        n = np.ascontiguousarray(_host(normals), np.float64).reshape(-1, 3)
        if n.shape != v.shape:
            raise ValueError(f"normals {n.shape} do not match vertices {v.shape}")
        fields += [("nx", "<f8"), ("ny", "<f8"), ("nz", "<f8")]
        header += ["property double nx", "property double ny", "property double nz"]
    if colours is not None:
        c = np.ascontiguousarray(_host(colours)).reshape(-1, 3)
        if c.dtype != np.uint8 or c.shape != v.shape:
            raise ValueError(f"colours must be uint8 {v.shape}, got {c.dtype} {c.shape}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rows = np.empty(v.shape[0], dtype=np.dtype(fields))
    rows["x"], rows["y"], rows["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        rows["nx"], rows["ny"], rows["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if colours is not None:
        rows["red"], rows["green"], rows["blue"] = c[:, 0], c[:, 1], c[:, 2]
    tris = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    tris["n"], tris["v"] = 3, f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(rows.tobytes())
        fh.write(tris.tobytes())
