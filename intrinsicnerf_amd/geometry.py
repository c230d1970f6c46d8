"""Geometry out of a trained scene: the query lattice of mesh extraction and the occupancy of a network on it.

Mirrors, with the reference's names, arguments and returned tensors (citations relative to ``/root/reference/SSR``):
  grid_within_bound, make_3D_grid      geometry/occupancy.py:5-48
  occupancy_grid                       extract_colour_mesh.py:149-185 (lattice, chunk loop over run_network, raw[..., 3],
                                       occupancy_activation) - one launch of ``inerf_occupancy_grid`` on the fused networks
Marching cubes stays with the caller (``skimage.measure.marching_cubes`` on the returned array); the vertex-colour rays are
``SSRTrainer.render_rays``.  See INTEGRATION.md.
"""
import numpy as np
import torch

from . import _capi, kernels, layered, packing
from .object_level import Embedder

__all__ = ["grid_within_bound", "make_3D_grid", "occupancy_grid", "occupancy_activation"]

STATUS_POINTS = 1 << 20        # lattice points per f16 range word of the fused launch - and per launch of the other paths


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
