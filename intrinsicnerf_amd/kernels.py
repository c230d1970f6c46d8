"""Tensor-level launchers for the C ABI (``include/inerf.h``): validate, allocate, pass raw pointers.

torch is plumbing here - it owns device memory and the HIP stream; all arithmetic happens in
``libinerf.so``.  Every function requires fp32 tensors on a HIP device and raises otherwise: there is
no CPU or eager fallback.
"""
import ctypes as C
import os

import torch

from . import _capi
from ._capi import (BASE_CHANNELS, ENDPOINT_DIM, FLAG_ENDPOINT, FLAG_GATE_COLOUR, FLAG_GATE_PROBE, FLAG_LINDISP, FLAG_U_PER_RAY, FLAG_WHITE_BKGD,
                    RAY_FLOATS, CompositeOut, RenderArgs)

MAX_POINTS_PER_LAUNCH = (1 << 31) - 1


def _dev(t, name, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} lives on {t.device}: intrinsicnerf_amd runs only on a HIP device "
                           "(no CPU / eager fallback exists)")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if shape is not None:
        if t.dim() != len(shape) or any(s is not None and int(t.shape[i]) != s for i, s in enumerate(shape)):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple('*' if s is None else s for s in shape)}")
    return t if t.is_contiguous() else t.contiguous()


def _opt(t, name, shape, like):
    if t is None:
        return None
    t = _dev(t, name, shape)
    if t.device != like.device:
        raise ValueError(f"{name} is on {t.device}, expected {like.device}")
    return t


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _new(like, *shape):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


# ---------------------------------------------------------------------------------------------------------------------
# training draws (include/inerf.h, "Training draws"): a launcher's ``draw`` argument is an inerf_draw_args (_capi.DrawArgs, from
# draws.DrawState.args) - the random tensor of the classic form is then drawn inside the kernel and must not be given
# ---------------------------------------------------------------------------------------------------------------------
def _draw_arg(draw, classic, name):
    if draw is None:
        return None
    if not isinstance(draw, _capi.DrawArgs):
        raise TypeError(f"draw must be an inerf_draw_args (DrawState.args()), got {type(draw).__name__}")
    if classic is not None:
        raise ValueError(f"{name} is drawn inside the kernel when draw is given: pass one or the other")
    return C.byref(draw)


def copy_draw(draw, **fields):
    """A copy of an inerf_draw_args with ``fields`` replaced (the step tensor it reads stays referenced)."""
    d = _capi.DrawArgs.from_buffer_copy(draw)
    d.step_tensor = getattr(draw, "step_tensor", None)
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def freeze_draw(draw):
    """``draw`` reading an 8-byte device copy of its step counter (DrawState.snapshot): what a backward node keeps, so that it
    regenerates the forward's draws even after the counter has advanced.  Capturable."""
    t = getattr(draw, "step_tensor", None)
    if t is None or not draw.step_dev:
        return copy_draw(draw)
    snap = t.clone()
    d = copy_draw(draw, step_dev=snap.data_ptr())
    d.step_tensor = snap
    return d


def draw_fill(draw, stream, n_rays, n_per_ray, device):
    """One stream of the draws as the [n_rays, n_per_ray] tensor the classic entry points take (inerf_draw_fill)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"draw_fill on {device}: intrinsicnerf_amd runs only on a HIP device (no CPU / eager fallback exists)")
    out = torch.empty((int(n_rays), int(n_per_ray)), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        rc = _capi.lib().inerf_draw_fill(_draw_arg(draw, None, ""), int(stream), int(n_rays), int(n_per_ray), _ptr(out), _stream(out))
    _capi.check(rc, "inerf_draw_fill")
    return out


def draw_advance(step_dev):
    """step_dev[0] += 1 on the device, as a launch of its own on the current stream (inerf_draw_advance)."""
    if not (isinstance(step_dev, torch.Tensor) and step_dev.is_cuda and step_dev.dtype == torch.int64 and step_dev.numel() == 1):
        raise ValueError("step_dev must be one int64 on a HIP device")
    with torch.cuda.device(step_dev.device):
        rc = _capi.lib().inerf_draw_advance(_ptr(step_dev), _stream(step_dev))
    _capi.check(rc, "inerf_draw_advance")


def sample_coarse(rays, t_vals, t_rand=None, lindisp=False, draw=None):
    """z_vals[N,S] (run_nerf.py:464-486 / trainer.py:730-746).  ``draw``: the jitter is drawn in the kernel."""
    rays = _dev(rays, "rays", (None, RAY_FLOATS))
    t_vals = _dev(t_vals, "t_vals", (None,))
    n, s = rays.shape[0], t_vals.shape[0]
    d = _draw_arg(draw, t_rand, "t_rand")
    t_rand = _opt(t_rand, "t_rand", (n, s), rays)
    z = _new(rays, n, s)
    with torch.cuda.device(rays.device):
        if d is not None:
            rc = _capi.lib().inerf_sample_coarse_drawn(_ptr(rays), _ptr(t_vals), None, n, s, FLAG_LINDISP if lindisp else 0, _ptr(z), d,
                                                       _stream(rays))
        else:
            rc = _capi.lib().inerf_sample_coarse(_ptr(rays), _ptr(t_vals), _ptr(t_rand), n, s,
                                                 FLAG_LINDISP if lindisp else 0, _ptr(z), _stream(rays))
    _capi.check(rc, "inerf_sample_coarse")
    return z


def _ndc_arg(ndc):
    """``ndc`` = (sx, sy, near_plane) as an inerf_ndc (each rounded to fp32 once, as ATen rounds a Python scalar), or None."""
    if ndc is None:
        return None
    sx, sy, near_plane = ndc
    return _capi.Ndc(float(sx), float(sy), float(near_plane))


def _rows3(t, name):
    """``t`` [..., 3] float32 on a HIP device as ([n, 3] view, row stride in floats) without a copy; ValueError when its flattening is
    no view with inner stride 1 and a row stride of at least 3."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} lives on {t.device}: intrinsicnerf_amd runs only on a HIP device "
                           "(no CPU / eager fallback exists)")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if t.dim() < 1 or t.shape[-1] != 3:
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected [..., 3]")
    try:
        flat = t.view(-1, 3)
    except RuntimeError:
        flat = None
    if flat is None or flat.stride(1) != 1 or (flat.shape[0] > 1 and flat.stride(0) < 3):
        raise ValueError(f"{name} (shape {tuple(t.shape)}, strides {tuple(t.stride())}) does not flatten to [n, 3] rows with inner "
                         "stride 1 and a row stride >= 3 without a copy: pass it .contiguous()")
    return flat, max(int(flat.stride(0)), 3)


def rows3_viewable(t):
    """Whether ``t`` [..., 3] goes into assemble_rays / ndc_rays as it is (see _rows3)."""
    try:
        _rows3(t, "t")
    except (TypeError, RuntimeError, ValueError):
        return False
    return True


def gen_rays(poses, height, width, fx, fy, cx, cy, near, far, opengl, static_poses=None, ndc=None):
    """[B * H * W, 11] ray batch ``[o3, d3, near, far, viewdir3]`` of B pinhole cameras through ``inerf_gen_rays``
    (get_rays + render()'s assembly, run_nerf_helpers.py:359-368 + run_nerf.py:99-128 | create_rays, rays.py:223-256).
    ``poses``: [B, 3, 4] / [B, 4, 4] / [3, 4] / [4, 4] float32 device tensor; bit-identical to the reference's CPU rays.
    ``ndc`` = (sx, sy, near_plane): origin and direction go through ndc_rays (run_nerf_helpers.py:381-399, run_nerf.py:117-119) in
    the same launch (``inerf_gen_rays_ndc``); view directions stay world-space."""
    def prep(t, name):
        t = _dev(t, name)
        if t.dim() == 2:
            t = t[None]
        if t.dim() != 3 or t.shape[1] not in (3, 4) or t.shape[2] != 4:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected [B, 3|4, 4]")
        return t.contiguous()
    poses = prep(poses, "poses")
    b = poses.shape[0]
    if static_poses is not None:
        static_poses = prep(static_poses, "static_poses")
        if static_poses.shape != poses.shape:
            raise ValueError("static_poses must have the shape of poses")
    out = _new(poses, b * int(height) * int(width), RAY_FLOATS)
    coeff = _ndc_arg(ndc)
    with torch.cuda.device(poses.device):
        if coeff is None:
            rc = _capi.lib().inerf_gen_rays(_ptr(poses), poses.shape[1] * 4, _ptr(static_poses), b, int(height), int(width),
                                            float(fx), float(fy), float(cx), float(cy), float(near), float(far),
                                            _capi.CAM_OPENGL if opengl else 0, _ptr(out), _stream(poses))
        else:
            rc = _capi.lib().inerf_gen_rays_ndc(_ptr(poses), poses.shape[1] * 4, _ptr(static_poses), b, int(height), int(width),
                                                float(fx), float(fy), float(cx), float(cy), float(near), float(far),
                                                _capi.CAM_OPENGL if opengl else 0, C.byref(coeff), _ptr(out), _stream(poses))
    _capi.check(rc, "inerf_gen_rays")
    return out


def _given_rays(rays_o, rays_d):
    o, o_stride = _rows3(rays_o, "rays_o")
    d, d_stride = _rows3(rays_d, "rays_d")
    if o.shape[0] != d.shape[0] or o.device != d.device:
        raise ValueError(f"rays_o {tuple(rays_o.shape)} on {rays_o.device} and rays_d {tuple(rays_d.shape)} on {rays_d.device} do not match")
    return o, o_stride, d, d_stride


def assemble_rays(rays_o, rays_d, near, far, ndc=None):
    """[n, 11] ray batch ``[o3, d3, near, far, viewdir3]`` from GIVEN rays through ``inerf_assemble_rays`` (render(rays=...)'s
    assembly, run_nerf.py:106-128): view direction = d / |d| with the reference's CPU bits; ``ndc`` = (sx, sy, near_plane) applies
    ndc_rays to origin and direction.  ``rays_o`` / ``rays_d``: [..., 3] float32 device tensors whose flattening to [n, 3] is a view
    with inner stride 1 (columns of an [n, 11] batch go in without a copy)."""
    o, o_stride, d, d_stride = _given_rays(rays_o, rays_d)
    n = o.shape[0]
    out = _new(o, n, RAY_FLOATS)
    coeff = _ndc_arg(ndc)
    with torch.cuda.device(o.device):
        rc = _capi.lib().inerf_assemble_rays(_ptr(o), o_stride, _ptr(d), d_stride, n, float(near), float(far),
                                             None if coeff is None else C.byref(coeff), _ptr(out), _stream(o))
    _capi.check(rc, "inerf_assemble_rays")
    return out


def ndc_rays(rays_o, rays_d, ndc):
    """``(o, d)`` of ndc_rays (run_nerf_helpers.py:381-399) in one launch (``inerf_ndc_rays``), each with the leading shape of
    ``rays_d``; ``ndc`` = (sx, sy, near_plane).  Inputs as in assemble_rays."""
    if ndc is None:
        raise ValueError("ndc_rays needs ndc = (sx, sy, near_plane)")
    o, o_stride, d, d_stride = _given_rays(rays_o, rays_d)
    n = o.shape[0]
    o_out, d_out = _new(o, n, 3), _new(o, n, 3)
    coeff = _ndc_arg(ndc)
    with torch.cuda.device(o.device):
        rc = _capi.lib().inerf_ndc_rays(_ptr(o), o_stride, _ptr(d), d_stride, n, C.byref(coeff), _ptr(o_out), _ptr(d_out), _stream(o))
    _capi.check(rc, "inerf_ndc_rays")
    shape = tuple(rays_d.shape)
    return o_out.reshape(shape), d_out.reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------
# mesh extraction (include/inerf.h, "Mesh extraction"): the query lattice and the occupancy of a network on it
# ---------------------------------------------------------------------------------------------------------------------
def _grid_arg(t, scale, transform):
    """(t as a contiguous fp32 vector, dim, float[3], float[12]) of the lattice entry points; ``scale`` (3 numbers) and ``transform`` (the
    3 x 4 rows of the box-to-scene matrix, 12 numbers) are rounded to fp32 here, once, like ``Tensor.float()``."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1:
        raise ValueError("t must be a float32 vector (torch.linspace(occ_range[0], occ_range[1], dim))")
    scale, transform = [float(v) for v in scale], [float(v) for v in transform]
    if len(scale) != 3 or len(transform) != 12:
        raise ValueError(f"scale holds {len(scale)} numbers and transform {len(transform)}, expected 3 and 12 (rows 0..2 of the 3 x 4 matrix)")
    return t.contiguous(), int(t.shape[0]), (C.c_float * 3)(*scale), (C.c_float * 12)(*transform)


def grid_points(t, scale, transform, first=0, count=None):
    """Lattice points ``[first, first + count)`` of make_3D_grid (SSR/geometry/occupancy.py:24-48) as a ``[count, 3]`` tensor where ``t``
    lives: ``inerf_grid_points`` for a device table, ``inerf_grid_points_host`` for a CPU one - the same bits either way."""
    t, dim, sc, m = _grid_arg(t, scale, transform)
    count = dim ** 3 - int(first) if count is None else int(count)
    out = torch.empty(max(count, 0), 3, dtype=torch.float32, device=t.device)
    if t.is_cuda:
        with torch.cuda.device(t.device):
            rc = _capi.lib().inerf_grid_points(_ptr(t), dim, sc, m, int(first), count, _ptr(out), _stream(t))
        _capi.check(rc, "inerf_grid_points")
    else:
        _capi.check(_capi.lib().inerf_grid_points_host(_ptr(t), dim, sc, m, int(first), count, _ptr(out)), "inerf_grid_points_host")
    return out


def occupancy_grid(desc, packed, t, scale, transform, dist, first=0, count=None, occ=None, sigma=None, status=None, status_points=0):
    """``occ[count] = 1 - exp(-relu(sigma) * dist)`` of lattice points ``[first, first + count)`` in one ``inerf_occupancy_grid`` launch
    (position encoding, trunk and density head only).  ``occ`` / ``sigma``: optional float32 device vectors of ``count`` elements to write
    into (``sigma=True``: allocate one; None: sigma is not stored).  ``status``: int32 device words, one per ``status_points`` LATTICE points
    (word = lattice index // status_points; 0: one word).  Returns ``(occ, sigma or None)``."""
    t, dim, sc, m = _grid_arg(_dev(t, "t"), scale, transform)
    packed = _dev(packed, "packed weights", (None,))
    count = dim ** 3 - int(first) if count is None else int(count)
    occ = _new(t, max(count, 0)) if occ is None else occ
    sigma = _new(t, max(count, 0)) if sigma is True else sigma
    for name, o in (("occ", occ), ("sigma", sigma)):
        if o is not None and (not o.is_cuda or o.dtype != torch.float32 or not o.is_contiguous() or o.numel() != max(count, 0) or o.device != t.device):
            raise ValueError(f"{name} must be a contiguous float32 vector of {count} elements on {t.device}")
    with torch.cuda.device(t.device):
        rc = _capi.lib().inerf_occupancy_grid(desc, _ptr(packed), _ptr(t), dim, sc, m, float(dist), int(first), count, _ptr(occ), _ptr(sigma),
                                              None if status is None else C.c_void_p(status.data_ptr()), int(status_points), _stream(t))
    _capi.check(rc, "inerf_occupancy_grid")
    return occ, sigma


def _vertex_rows(t, name):
    """``t`` [n, 3] float32 or float64, on any device, as (tensor, row stride in elements) without a copy."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name} must be float32 or float64, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected [n, 3]")
    if t.shape[0] > 0 and (t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < 3)):
        raise ValueError(f"{name} (strides {tuple(t.stride())}) must have unit stride along its rows and a row stride >= 3: pass it .contiguous()")
    return t, max(int(t.stride(0)), 3)


def vertex_rays(vertices, normals, near=0.1, far=10.0, near_t=2.0):
    """[n, 11] ray batch ``[o3, d3, near, far, viewdir3]`` of the vertex-colour pass (SSR/extract_colour_mesh.py:232-238): ``d = -normal``,
    ``o = vertex - d * near * near_t``, view direction ``d / |d|``, with the reference's CPU bits, where the inputs live:
    ``inerf_vertex_rays`` (one launch) for device tensors, ``inerf_vertex_rays_host`` for CPU ones.  ``vertices`` / ``normals``: [n, 3]
    of one dtype, float32 or float64 (rounded to fp32 inside, as ``torch.FloatTensor(...)`` does), rows any stride >= 3 apart."""
    v, v_stride = _vertex_rows(vertices, "vertices")
    m, m_stride = _vertex_rows(normals, "normals")
    if v.shape != m.shape or v.dtype != m.dtype or v.device != m.device:
        raise ValueError(f"vertices {tuple(v.shape)} {v.dtype} on {v.device} and normals {tuple(m.shape)} {m.dtype} on {m.device} do not match")
    n = v.shape[0]
    dtype = _capi.DTYPE_F64 if v.dtype == torch.float64 else _capi.DTYPE_F32
    out = torch.empty(n, RAY_FLOATS, dtype=torch.float32, device=v.device)
    if v.is_cuda:
        with torch.cuda.device(v.device):
            rc = _capi.lib().inerf_vertex_rays(_ptr(v), v_stride, _ptr(m), m_stride, n, dtype, float(near), float(far), float(near_t),
                                               _ptr(out), _stream(v))
        _capi.check(rc, "inerf_vertex_rays")
    else:
        _capi.check(_capi.lib().inerf_vertex_rays_host(_ptr(v), v_stride, _ptr(m), m_stride, n, dtype, float(near), float(far),
                                                       float(near_t), _ptr(out)), "inerf_vertex_rays_host")
    return out


def vertex_colours(rgb=None, logits=None, colour_map=None, out=None, labels=None):
    """8-bit vertex colours in one launch of ``inerf_vertex_colours`` (extract_colour_mesh.py:248-257).  Exactly one of ``rgb`` [n, 3]
    and ``logits`` [n, C] (float32 device views: unit stride along a row, any row stride - a column range of a wider tensor goes in as
    it is): ``to8b(rgb)`` as ``frame_to_u8`` gives it, or ``colour_map[label]`` with the label of ``sem_maps`` and ``colour_map`` a
    contiguous uint8 [C, 3] device tensor.  ``out``: contiguous uint8 [n, 3] to write into (rows of a larger buffer), allocated when
    None.  ``labels``: contiguous int32 [n] to receive the labels, ``True`` to allocate it, None for none (semantic mode only).
    Returns ``(out, labels)``."""
    if (rgb is None) == (logits is None):
        raise ValueError("vertex_colours takes exactly one of rgb and logits")
    if rgb is not None:
        if labels is not None:
            raise ValueError("labels exist only in semantic mode (logits)")
        src, stride = _eval_view(rgb, "rgb", 3)
        c, named = 0, [("rgb", src)]
    else:
        if (not isinstance(colour_map, torch.Tensor) or colour_map.dtype != torch.uint8 or colour_map.dim() != 2 or colour_map.shape[1] != 3
                or not colour_map.is_contiguous()):
            raise ValueError("colour_map must be a contiguous uint8 [C, 3] tensor")
        c = _eval_classes(colour_map.shape[0])
        if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[1] != c:
            raise ValueError(f"logits must be a [n, {c}] tensor, one column per row of colour_map")
        src, stride = _eval_view(logits, "logits", c)
        named = [("logits", src), ("colour_map", colour_map)]
    n = src.shape[0]
    if out is None:
        out = torch.empty(n, 3, dtype=torch.uint8, device=src.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (n, 3) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 [{n}, 3] tensor")
    named.append(("out", out))
    if labels is True:
        labels = torch.empty(n, dtype=torch.int32, device=src.device)
    if labels is not None:
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or tuple(labels.shape) != (n,) or not labels.is_contiguous():
            raise ValueError(f"labels must be a contiguous int32 [{n}] tensor")
        named.append(("labels", labels))
    device = _eval_devices(named)
    u8 = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    with torch.cuda.device(device):
        rc = _capi.lib().inerf_vertex_colours(_ptr(src) if rgb is not None else None, stride if rgb is not None else 0,
                                              _ptr(src) if rgb is None else None, stride if rgb is None else 0, n, c,
                                              u8(colour_map) if rgb is None else None, u8(out), u8(labels), _stream(src))
    _capi.check(rc, "inerf_vertex_colours")
    return out, labels


# ---------------------------------------------------------------------------------------------------------------------
# marching cubes and mesh cleaning (include/inerf.h, "Marching cubes and mesh cleaning"; csrc/mcubes.hip)
# ---------------------------------------------------------------------------------------------------------------------
def _mesh_tensor(t, name, dtype, cols=3):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a tensor on a HIP device (no CPU / eager fallback exists)")
    if t.dtype != dtype or t.dim() != 2 or t.shape[1] != cols:
        raise ValueError(f"{name} must be {dtype} [n, {cols}], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def _workspace(nbytes, what, device):
    if nbytes < 0:
        _capi.check(int(nbytes), what)
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def mc_count(occ, level):
    """``inerf_mc_count`` on a float32 device lattice [nx, ny, nz]: ``(workspace, totals)`` - the workspace ``mc_emit`` reads and the
    int64 [3] device tensor {vertices, triangles, non-finite values}.  Nothing is read back here."""
    if not isinstance(occ, torch.Tensor) or occ.dim() != 3:
        raise ValueError("occ must be a [nx, ny, nz] tensor")
    occ = _dev(occ, "occ")
    nx, ny, nz = (int(s) for s in occ.shape)
    workspace = _workspace(_capi.lib().inerf_mc_workspace_bytes(nx, ny, nz), "inerf_mc_workspace_bytes", occ.device)
    totals = torch.empty(3, dtype=torch.int64, device=occ.device)
    with torch.cuda.device(occ.device):
        rc = _capi.lib().inerf_mc_count(_ptr(occ), nx, ny, nz, float(level), _ptr(workspace), workspace.numel(), _ptr(totals), _stream(occ))
    _capi.check(rc, "inerf_mc_count")
    return workspace, totals


def mc_emit(occ, level, workspace, n_vertices, n_triangles, affine=None):
    """``inerf_mc_emit`` after ``mc_count`` on the same lattice and level: ``(vertices_lattice float32 [V, 3], vertices_scene float64
    [V, 3] or None, faces int32 [F, 3])`` on the device.  ``affine``: twelve numbers, the row-major 3 x 4 fp64 map to scene coordinates."""
    occ = _dev(occ, "occ")
    nx, ny, nz = (int(s) for s in occ.shape)
    nv, nt = int(n_vertices), int(n_triangles)
    lattice = torch.empty(nv, 3, dtype=torch.float32, device=occ.device)
    scene = torch.empty(nv, 3, dtype=torch.float64, device=occ.device) if affine is not None else None
    faces = torch.empty(nt, 3, dtype=torch.int32, device=occ.device)
    a = None
    if affine is not None:
        flat = [float(x) for x in affine]
        if len(flat) != 12:
            raise ValueError(f"affine holds {len(flat)} numbers, expected the 12 of a 3 x 4 map")
        a = (C.c_double * 12)(*flat)
    with torch.cuda.device(occ.device):
        rc = _capi.lib().inerf_mc_emit(_ptr(occ), nx, ny, nz, float(level), _ptr(workspace), workspace.numel(), a, nv, nt, _ptr(lattice),
                                       _ptr(scene), _ptr(faces), _stream(occ))
    _capi.check(rc, "inerf_mc_emit")
    return lattice, scene, faces


def mesh_normals(vertices, faces):
    """float64 [V, 3] vertex normals of ``inerf_mesh_normals`` (vertices float64 [V, 3], faces int32 [F, 3], both on the device)."""
    v = _mesh_tensor(vertices, "vertices", torch.float64)
    f = _mesh_tensor(faces, "faces", torch.int32)
    nv, nt = int(v.shape[0]), int(f.shape[0])
    out = torch.empty(nv, 3, dtype=torch.float64, device=v.device)
    workspace = _workspace(_capi.lib().inerf_mesh_workspace_bytes(nv, nt), "inerf_mesh_workspace_bytes", v.device)
    with torch.cuda.device(v.device):
        rc = _capi.lib().inerf_mesh_normals(_ptr(v), nv, _ptr(f), nt, _ptr(workspace), workspace.numel(), _ptr(out), _stream(v))
    _capi.check(rc, "inerf_mesh_normals")
    return out


def mesh_clean(faces, n_vertices, min_triangles, keep_single_cluster=False, rows_f32=None, rows_f64_a=None, rows_f64_b=None):
    """``inerf_mesh_clean``: ``(faces_out, out_f32, out_f64_a, out_f64_b, totals)`` - outputs sized for the input counts (the caller slices
    them by ``totals``, the int64 [4] device tensor {vertices kept, triangles kept, components, components kept})."""
    f = _mesh_tensor(faces, "faces", torch.int32)
    nv, nt = int(n_vertices), int(f.shape[0])
    rows = []
    for name, t, dtype in (("rows_f32", rows_f32, torch.float32), ("rows_f64_a", rows_f64_a, torch.float64), ("rows_f64_b", rows_f64_b, torch.float64)):
        t = None if t is None else _mesh_tensor(t, name, dtype)
        if t is not None and (t.shape[0] != nv or t.device != f.device):
            raise ValueError(f"{name} has {t.shape[0]} rows on {t.device}, expected {nv} on {f.device}")
        rows.append(t)
    outs = [None if t is None else torch.empty_like(t) for t in rows]
    faces_out = torch.empty_like(f)
    totals = torch.empty(4, dtype=torch.int64, device=f.device)
    workspace = _workspace(_capi.lib().inerf_mesh_workspace_bytes(nv, nt), "inerf_mesh_workspace_bytes", f.device)
    with torch.cuda.device(f.device):
        rc = _capi.lib().inerf_mesh_clean(_ptr(f), nv, nt, int(min_triangles), int(bool(keep_single_cluster)), _ptr(rows[0]), _ptr(rows[1]),
                                          _ptr(rows[2]), _ptr(workspace), workspace.numel(), _ptr(faces_out), _ptr(outs[0]), _ptr(outs[1]),
                                          _ptr(outs[2]), _ptr(totals), _stream(f))
    _capi.check(rc, "inerf_mesh_clean")
    return faces_out, outs[0], outs[1], outs[2], totals


def frame_to_u8(values):
    """``(255 * clip(x, 0, 1)).astype(uint8)`` (to8b, run_nerf_helpers.py:13) on the device; same shape, dtype uint8."""
    values = _dev(values, "values")
    out = torch.empty(values.shape, dtype=torch.uint8, device=values.device)
    with torch.cuda.device(values.device):
        rc = _capi.lib().inerf_frame_to_u8(_ptr(values), values.numel(), C.c_void_p(out.data_ptr()), _stream(values))
    _capi.check(rc, "inerf_frame_to_u8")
    return out


def frame_subsample(frame, height, width, albedo_col, out_pixels, offset=0, label_col=-1, out_labels=None, class_counts=None, step=2):
    """Every ``step``-th pixel of a packed frame (``frames.pack_maps``: [height * width, row_stride] fp32) into the cluster fit's
    sample table (``inerf_frame_subsample``): rows ``offset ..`` of ``out_pixels`` [N, 3] receive
    ``albedo[::step, ::step].reshape(-1, 3)`` and, with a label column, the same rows of ``out_labels`` [N] (int64) the
    truncated labels, while ``class_counts`` [K] (int32) gains the bincount of those inside [0, K).  Returns the rows written."""
    frame = _dev(frame, "frame", (int(height) * int(width), None))
    out_pixels = _dev(out_pixels, "out_pixels", (None, 3))
    rows = -(-int(height) // int(step)) * -(-int(width) // int(step)) if step >= 1 else 0
    offset = int(offset)
    if offset < 0 or offset + rows > out_pixels.shape[0] or out_pixels.device != frame.device:
        raise ValueError(f"out_pixels holds {out_pixels.shape[0]} rows on {out_pixels.device}: rows {offset} .. {offset + rows} of a frame on {frame.device}")
    labelled = label_col is not None and int(label_col) >= 0
    lab_ptr = cnt_ptr = None
    k = 0
    if labelled:
        if not (isinstance(out_labels, torch.Tensor) and out_labels.dtype == torch.int64 and out_labels.dim() == 1 and out_labels.is_contiguous()
                and out_labels.device == frame.device and out_labels.shape[0] >= offset + rows):
            raise ValueError("out_labels must be a contiguous int64 vector on the frame's device, as long as out_pixels")
        lab_ptr = C.c_void_p(out_labels.data_ptr() + 8 * offset)
        if class_counts is not None:
            if not (isinstance(class_counts, torch.Tensor) and class_counts.dtype == torch.int32 and class_counts.dim() == 1
                    and class_counts.is_contiguous() and class_counts.device == frame.device):
                raise ValueError("class_counts must be a contiguous int32 vector on the frame's device")
            cnt_ptr, k = _ptr(class_counts), class_counts.shape[0]
    with torch.cuda.device(frame.device):
        rc = _capi.lib().inerf_frame_subsample(_ptr(frame), frame.shape[1], int(albedo_col), int(label_col) if labelled else -1, int(height),
                                               int(width), int(step), C.c_void_p(out_pixels.data_ptr() + 12 * offset), lab_ptr, cnt_ptr, k,
                                               _stream(frame))
    _capi.check(rc, "inerf_frame_subsample")
    return rows


def snap_row_bytes(n):
    """Bytes per image of ``cluster_snap_compose``'s output buffer: 3 * n rounded up to the kernel's dword stores."""
    return (3 * int(n) + 3) & ~3


def snap_images(out, n):
    """The two [n, 3] uint8 images inside ``cluster_snap_compose``'s buffer (a tensor, or its host copy as a numpy array)."""
    return out[0, :3 * n].reshape(n, 3), out[1, :3 * n].reshape(n, 3)


def cluster_snap_compose(tables, pack, albedo_col, shading_col, residual_col, label_col=-1, out=None, want_color=False):
    """A frame's albedo snapped to its cluster centres and the image re-composed from it, as 8-bit images, in one launch of
    ``inerf_cluster_snap_compose``: ``pack`` is [n, row_stride] fp32 holding the albedo (3), shading (1) and residual (3) columns
    and - ``label_col >= 0`` - a float label column; without one every pixel belongs to class 0 (``dest_color``'s ``class_num == 1``
    shortcut).  ``tables``: ``cluster.ClusterTables``.  Returns ``(out, colour)``: ``out`` [2, snap_row_bytes(n)] uint8, one buffer for
    one device->host copy - ``out[0, :3 * n]`` = to8b(clustered) and ``out[1, :3 * n]`` = to8b(clustered * shading + residual) as
    [n, 3] images (``snap_images``); ``colour`` [n, 3] fp32 = ``cluster.lookup``'s, only with ``want_color``."""
    pack = _dev(pack, "pack", (None, None))
    n, stride = pack.shape
    if pack.device != tables.device:
        raise ValueError(f"pack is on {pack.device}, the cluster tables on {tables.device}")
    labelled = label_col is not None and int(label_col) >= 0
    for name, col, w in (("albedo", albedo_col, 3), ("shading", shading_col, 1), ("residual", residual_col, 3)) + ((("label", label_col, 1),) if labelled else ()):
        if not 0 <= int(col) <= stride - w:
            raise ValueError(f"{name}_col={col} lies outside a row of {stride} floats")
    row = snap_row_bytes(n)
    if out is None:
        out = torch.empty(2, row, dtype=torch.uint8, device=pack.device)
    elif not (out.dtype == torch.uint8 and tuple(out.shape) == (2, row) and out.is_contiguous() and out.device == pack.device):
        raise ValueError(f"out must be a contiguous [2, {row}] uint8 tensor on {pack.device}")
    color = torch.empty(n, 3, dtype=torch.float32, device=pack.device) if want_color else None
    base = pack.data_ptr()
    at = lambda col: C.c_void_p(base + 4 * int(col))
    with torch.cuda.device(pack.device):
        rc = _capi.lib().inerf_cluster_snap_compose(
            at(albedo_col), at(label_col) if labelled else None, at(shading_col), at(residual_col), stride, n, _ptr(tables.anchors),
            _ptr(tables.links), _ptr(tables.anchor_begin), _ptr(tables.factor), _ptr(tables.centers), _ptr(tables.center_begin),
            tables.n_classes, 0 if labelled else _capi.CLUSTER_IGNORE_LABEL, C.c_void_p(out.data_ptr()),
            C.c_void_p(out.data_ptr() + row), _ptr(color), _stream(pack))
    _capi.check(rc, "inerf_cluster_snap_compose")
    return out, color


# ---------------------------------------------------------------------------------------------------------------------
# scene editing (csrc/edit.hip): the edit engine of gui.py.  ``out`` follows cluster_snap_compose's convention - with
# ``want_c`` a [2, snap_row_bytes(n)] uint8 buffer whose rows are to8b(colour) and to8b(result) (``snap_images``), one
# buffer for one device->host copy; without it a [1, snap_row_bytes(n)] buffer holding the result alone (``out[-1]``)
# ---------------------------------------------------------------------------------------------------------------------
def _edit_params(tables, edit_centers, shading_mode, residual_mode, shading_scale, residual_scale):
    if not (isinstance(edit_centers, torch.Tensor) and edit_centers.dtype == torch.float32 and edit_centers.is_contiguous()
            and edit_centers.device == tables.device and tuple(edit_centers.shape) == tuple(tables.centers.shape)):
        raise ValueError(f"edit_centers must be a contiguous float32 {tuple(tables.centers.shape)} tensor on {tables.device}, like the tables' centers")
    for name, mode in (("shading_mode", shading_mode), ("residual_mode", residual_mode)):
        if mode not in (0, 1, False, True):
            raise ValueError(f"{name} must be 0 or 1, got {mode!r}")
    return _capi.EditParams(edit_centers.data_ptr(), int(shading_mode), int(residual_mode), float(shading_scale), float(residual_scale))


def _edit_outputs(n, device, out, want_c, want_f32):
    rows, row = (2 if want_c else 1), snap_row_bytes(n)
    if out is None:
        out = torch.empty(rows, row, dtype=torch.uint8, device=device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and tuple(out.shape) == (rows, row) and out.is_contiguous()
              and out.device == device):
        raise ValueError(f"out must be a contiguous [{rows}, {row}] uint8 tensor on {device}")
    base = out.data_ptr()
    result_f32 = torch.empty(n, 3, dtype=torch.float32, device=device) if want_f32 else None
    return out, (C.c_void_p(base) if want_c else None), C.c_void_p(base + (row if want_c else 0)), result_f32


def _edit_slots(slot, n, device):
    if not (isinstance(slot, torch.Tensor) and slot.dtype == torch.int32 and slot.dim() == 1 and slot.shape[0] == n and slot.is_contiguous()
            and slot.device == device):
        raise ValueError(f"slot must be a contiguous int32 vector of {n} entries on {device}")
    return slot


def edit_frame(tables, edit_centers, pack, albedo_col, shading_col, residual_col, label_col=-1, shading_mode=0, residual_mode=0,
               shading_scale=1.0, residual_scale=1.0, out=None, want_c=True, want_f32=False, want_slot=False):
    """Search form of the edit (``inerf_edit_frame``): ``cluster_snap_compose``'s inputs, the colour read from ``edit_centers``
    (the editable copy of ``tables.centers``), gui.py:163's transfers and scales.  Returns ``(out, result, slot)``: ``result``
    [n, 3] fp32 only with ``want_f32``; ``slot`` [n] int32 only with ``want_slot`` - the global row of every pixel's centre in
    ``edit_centers``, -1 where the pixel keeps its albedo: what ``edit_recompose`` takes instead of a search."""
    pack = _dev(pack, "pack", (None, None))
    n, stride = pack.shape
    if pack.device != tables.device:
        raise ValueError(f"pack is on {pack.device}, the cluster tables on {tables.device}")
    labelled = label_col is not None and int(label_col) >= 0
    for name, col, w in (("albedo", albedo_col, 3), ("shading", shading_col, 1), ("residual", residual_col, 3)) + ((("label", label_col, 1),) if labelled else ()):
        if not 0 <= int(col) <= stride - w:
            raise ValueError(f"{name}_col={col} lies outside a row of {stride} floats")
    params = _edit_params(tables, edit_centers, shading_mode, residual_mode, shading_scale, residual_scale)
    out, c_ptr, result_ptr, result = _edit_outputs(n, pack.device, out, want_c, want_f32)
    slot = torch.empty(n, dtype=torch.int32, device=pack.device) if want_slot else None
    base = pack.data_ptr()
    at = lambda col: C.c_void_p(base + 4 * int(col))
    with torch.cuda.device(pack.device):
        rc = _capi.lib().inerf_edit_frame(
            at(albedo_col), at(label_col) if labelled else None, at(shading_col), at(residual_col), stride, n, _ptr(tables.anchors),
            _ptr(tables.links), _ptr(tables.anchor_begin), _ptr(tables.factor), _ptr(tables.center_begin), tables.n_classes,
            0 if labelled else _capi.CLUSTER_IGNORE_LABEL, C.byref(params), result_ptr, c_ptr, _ptr(result), _ptr(slot), _stream(pack))
    _capi.check(rc, "inerf_edit_frame")
    return out, result, slot


def edit_recompose(tables, edit_centers, pack, albedo_col, shading_col, residual_col, slot, shading_mode=0, residual_mode=0,
                   shading_scale=1.0, residual_scale=1.0, out=None, want_c=True, want_f32=False):
    """Cached form of the edit over fp32 pack columns (``inerf_edit_recompose``): no search - ``slot`` (``edit_frame``'s) selects
    each pixel's centre.  Returns ``(out, result)`` as ``edit_frame``."""
    pack = _dev(pack, "pack", (None, None))
    n, stride = pack.shape
    if pack.device != tables.device:
        raise ValueError(f"pack is on {pack.device}, the cluster tables on {tables.device}")
    for name, col, w in (("albedo", albedo_col, 3), ("shading", shading_col, 1), ("residual", residual_col, 3)):
        if not 0 <= int(col) <= stride - w:
            raise ValueError(f"{name}_col={col} lies outside a row of {stride} floats")
    slot = _edit_slots(slot, n, pack.device)
    params = _edit_params(tables, edit_centers, shading_mode, residual_mode, shading_scale, residual_scale)
    out, c_ptr, result_ptr, result = _edit_outputs(n, pack.device, out, want_c, want_f32)
    base = pack.data_ptr()
    at = lambda col: C.c_void_p(base + 4 * int(col))
    with torch.cuda.device(pack.device):
        rc = _capi.lib().inerf_edit_recompose(at(albedo_col), at(shading_col), at(residual_col), stride, _ptr(slot), n, C.byref(params),
                                              result_ptr, c_ptr, _ptr(result), _stream(pack))
    _capi.check(rc, "inerf_edit_recompose")
    return out, result


def edit_recompose_u8(tables, edit_centers, albedo, shading, residual, slot, shading_mode=0, residual_mode=0, shading_scale=1.0,
                      residual_scale=1.0, out=None, want_c=True, want_f32=False):
    """Cached form of the edit over the 8-bit planes ``load_all_image`` reads (``inerf_edit_recompose_u8``): ``albedo`` [n, 3],
    ``shading`` [n], ``residual`` [n, 3] uint8, each ``v / 255`` as numpy rounds it; views into a longer sequence are taken at any
    byte offset.  Returns ``(out, result)`` as ``edit_frame``."""
    for name, t in (("albedo", albedo), ("shading", shading), ("residual", residual)):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous uint8 tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{name} lives on {t.device}: intrinsicnerf_amd runs only on a HIP device (no CPU / eager fallback exists)")
        if t.device != tables.device:
            raise ValueError(f"{name} is on {t.device}, the cluster tables on {tables.device}")
    n = shading.numel()
    if shading.dim() != 1 or tuple(albedo.shape) != (n, 3) or tuple(residual.shape) != (n, 3):
        raise ValueError(f"expected albedo [n, 3], shading [n], residual [n, 3]; got {tuple(albedo.shape)}, {tuple(shading.shape)}, {tuple(residual.shape)}")
    slot = _edit_slots(slot, n, shading.device)
    params = _edit_params(tables, edit_centers, shading_mode, residual_mode, shading_scale, residual_scale)
    out, c_ptr, result_ptr, result = _edit_outputs(n, shading.device, out, want_c, want_f32)
    u8 = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(shading.device):
        rc = _capi.lib().inerf_edit_recompose_u8(u8(albedo), u8(shading), u8(residual), _ptr(slot), n, C.byref(params), result_ptr, c_ptr,
                                                 _ptr(result), _stream(shading))
    _capi.check(rc, "inerf_edit_recompose_u8")
    return out, result


def _new_status(like):
    return torch.zeros(1, dtype=torch.int32, device=like.device)


_deferred = None          # the innermost open deferred_range_checks() block, else None
_status_rays = 0          # rays per f16 range word of the launches inside a chunked_status() block (0: one word per launch)


class chunked_status:
    """Launches of ``render_rays_fused`` inside this block keep ONE f16 range word per ``rays_per_word`` rays
    (inerf_encode_mlp_chunked): the chunk loops of the front-ends render an eval-mode frame as one launch sequence and still learn
    which of the CALLER's chunks left the range.  In a ``deferred_range_checks`` block such a launch's words are tagged
    ``(block.tag, word index)``."""

    def __init__(self, rays_per_word):
        self.rays = int(rays_per_word)

    def __enter__(self):
        global _status_rays
        self.outer, _status_rays = _status_rays, self.rays
        return self

    def __exit__(self, *exc):
        global _status_rays
        _status_rays = self.outer
        return False
captured_status = None    # list collecting the status words of launches recorded into a HIP graph (graphs.GraphedTrainStep)


def _capturing():
    """True while the current stream records a HIP graph: nothing may be read back to the host then."""
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _defer_to_graph_owner(words):
    """Status words of launches that are being CAPTURED cannot be read here; they are handed to whoever owns the graph
    (graphs.GraphedTrainStep reads them after every replay).  Capturing without an owner would silently drop the f16 range
    guard, so that is an error."""
    if captured_status is None:
        raise RuntimeError("split-precision MLP launches are being captured into a HIP graph outside graphs.GraphedTrainStep: "
                           "their f16 range words would never be checked")
    captured_status.extend(words)


class deferred_range_checks:
    """Context manager for launches whose f16 range words can be read later: ``check_f16_range(..., deferrable=True)`` calls
    inside only remember their status word (together with the block's current ``tag``), and ONE device->host read at the
    end of the block checks them all - a multi-chunk frame costs one host synchronisation instead of one per chunk.

    At exit ``tripped`` holds the tags (in order, without repeats) whose launches left f16's range.  With
    ``raise_on_trip`` (default) a non-empty set raises FloatingPointError; the chunk loops of the front-ends pass False,
    tag every chunk with its index and re-render ONLY the tripped chunks in exact fp32.

    Blocks do not delegate: a block opened inside another one (a training step inside a frame loop) reads its OWN words at
    its own exit, so its handler - which restores the RNG and re-evaluates the same draws - is the one that runs."""

    def __init__(self, what, raise_on_trip=True):
        self.what, self.raise_on_trip = what, raise_on_trip
        self.tag, self.tripped = None, []
        self.words, self.tags = [], []

    def __len__(self):
        return len(self.words)

    def __enter__(self):
        global _deferred
        self.outer, _deferred = _deferred, self
        return self

    def __exit__(self, exc_type, exc, tb):
        global _deferred
        _deferred = self.outer
        if exc_type is not None or not self.words:
            return False
        if _capturing():
            _defer_to_graph_owner(self.words)
            return False
        flags = (self.words[0] if len(self.words) == 1 else torch.cat(self.words)).cpu().tolist()      # the block's one sync
        assert len(flags) == len(self.tags)
        for flag, tag in zip(flags, self.tags):
            if int(flag) & _capi.STATUS_F16_RANGE and tag not in self.tripped:
                self.tripped.append(tag)
        if self.tripped and self.raise_on_trip:
            raise FloatingPointError(_RANGE_MESSAGE.format(what=self.what))
        return False


_RANGE_MESSAGE = ("{what}: an activation exceeded the f16 range (|v| > 6e4) in the split-precision MLP kernel; "
                  "results are invalid - re-run with precision f32 (INERF_PRECISION=f32)")


def check_f16_range(status, what, deferrable=False):
    """Raise if a PREC_F16X3 launch met an activation outside f16's range (one device sync) - or, inside a
    ``deferred_range_checks`` block and with ``deferrable``, leave the word for the block's single check."""
    if status is None:
        return
    status = status.reshape(-1)                # (one word per launch, or one per chunk of its rays: chunked_status)
    if _capturing():
        _defer_to_graph_owner([status[i:i + 1] for i in range(status.numel())])
        return
    if deferrable and _deferred is not None:
        _deferred.words.append(status)
        _deferred.tags.extend([_deferred.tag] if status.numel() == 1 else [(_deferred.tag, i) for i in range(status.numel())])
        return
    if int(status.max().item()) & _capi.STATUS_F16_RANGE:
        raise FloatingPointError(_RANGE_MESSAGE.format(what=what))


def coalesced_chunk(n_rays, chunk, n_samples, n_importance, channels, device):
    """How many rays ONE launch sequence of an eval-mode frame may take instead of the caller's ``chunk``.

    The reference's ``chunk`` (run_nerf.py:59-71, training_utils.py:5-17: 32 768 rays) exists for 11 GB cards and "does not affect
    final results"; here results are bit-identical for any chunking (tests/test_full_size_properties.py, test_gpu_parity.py), a
    launch of 32 768 rays runs 7 % below a launch of 65 536+ (it ends on a partly filled wave of tiles per CU:
    profiles/r05_gemm_priority_ab.txt) and a frame's tail chunk is worse.  So when nothing depends on the chunk boundaries - no random
    draw per chunk, no ``raw`` returned, no autograd - the front-ends merge chunks up to a workspace cap: ``INERF_COALESCE_BYTES``
    (default 16 GiB, at most half the device's free memory; 0 = keep the caller's chunks).  Returns a multiple of ``chunk``."""
    import os
    cap = int(float(os.environ.get("INERF_COALESCE_BYTES", 16 * 2 ** 30)))
    if cap <= 0 or n_rays <= chunk or chunk <= 0:
        return chunk
    if device.type == "cuda":
        cap = min(cap, torch.cuda.mem_get_info(device)[0] // 2)
    # the density gate's record buffer (include/inerf.h INERF_FLAG_GATE_COLOUR: at most INERF_GATE_BYTES, default 2 GiB) is a fixed part
    # of a large launch's workspace, whatever the ray count; a cap below twice that budget is taken as it is (the buffer comes on top).
    # The probe path keeps no records (INERF_FLAG_GATE_PROBE unless INERF_GATE_FUSED=0): its candidate list and (s, S), 12 B per point of
    # the larger pass, grow with the rays instead
    gated = os.environ.get("INERF_GATE", "1")[:1] != "0"
    records = os.environ.get("INERF_PROBE", "1")[:1] == "0" or os.environ.get("INERF_GATE_FUSED", "1")[:1] == "0"
    gate = int(float(os.environ.get("INERF_GATE_BYTES", 2 * 2 ** 30)))
    if gated and records and cap >= 2 * gate:
        cap -= gate
    s, f = int(n_samples), int(n_samples) + int(n_importance)
    # per ray: z coarse / new / merged, coarse weights, raw of both levels, maps (include/inerf.h: inerf_render_workspace_bytes), + 10 %
    per_ray = int(1.1 * 4 * (s + n_importance + f + s + (s + f) * channels + 2 * (16 + channels)))
    if gated and not records:
        per_ray += 12 * f
    rays = min(n_rays, cap // max(per_ray, 1))
    return max(chunk, rays // chunk * chunk if rays < n_rays else -(-n_rays // chunk) * chunk)


_warned_fallback = False


def warn_f32_fallback(e):
    global _warned_fallback
    if not _warned_fallback:
        import warnings
        warnings.warn(f"{e}  Re-running this batch with the exact fp32 MFMA kernel (set INERF_PRECISION=f32 to "
                      "skip the attempt).")
        _warned_fallback = True


def with_f32_fallback(desc, run):
    """``run(desc)`` and, if the split-precision kernel reports an out-of-range activation, once more in exact fp32.

    ``run`` must call ``check_f16_range`` on its status word (that is the one host sync of the f16x3 mode)."""
    global _warned_fallback
    try:
        return run(desc)
    except FloatingPointError as e:
        if desc.precision != _capi.PREC_F16X3:
            raise
        warn_f32_fallback(e)
        d32 = _capi.NetDesc(desc.variant, desc.n_classes, desc.l_xyz, desc.l_dir, desc.xyz_div, _capi.PREC_F32)
        return run(d32)


def gate_margin(state):
    """{r_max, observed, kappa_in_use, launches} of a gate-probe margin state (``packing.gate_state_of``; include/inerf.h
    INERF_FLAG_GATE_PROBE).  Synchronises: for logs and tests."""
    w = state.detach().cpu()
    f = w.view(torch.float32)
    return dict(r_max=float(f[0]), kappa_in_use=float(f[1]), observed=int(w.view(torch.int64)[1]), launches=int(w[4]) & 0xFFFFFFFF)


def _gate_state_ptr(state, like):
    if state is None:
        return None
    if not (isinstance(state, torch.Tensor) and state.is_cuda and state.device == like.device and state.dtype == torch.int32
            and state.numel() == 8 and state.is_contiguous()):
        raise ValueError("gate_state must be a contiguous int32[8] tensor on the rays' device (packing.gate_state_of)")
    return C.c_void_p(state.data_ptr())


def encode_mlp(desc, packed, rays, z_vals, endpoint=False, status=None, gate_colour=False, status_rays=0, gate_probe=False, probe_out=None,
               gate_state=None):
    """raw[N,S,CH]: fused encoding + MLP (run_network + NeRF.forward).

    ``status``: optional int32[1] device tensor that collects INERF_STATUS_* bits (PREC_F16X3 range check); with ``status_rays`` > 0
    one word per that many rays.  ``gate_colour``: INERF_FLAG_GATE_COLOUR (include/inerf.h) - rows with sigma <= 0 carry zero colours.
    ``gate_probe``: INERF_FLAG_GATE_PROBE on top of it; ``probe_out`` (tests): a float32 [N * S, 2] device tensor for the probe's (s, S);
    ``gate_state``: the probe's margin state of ``packed`` (``packing.gate_state_of``) - None: the constant margin."""
    rays = _dev(rays, "rays", (None, RAY_FLOATS))
    z_vals = _dev(z_vals, "z_vals", (rays.shape[0], None))
    packed = _dev(packed, "packed weights", (None,))
    n, s = z_vals.shape
    flags = (FLAG_ENDPOINT if endpoint else 0) | (FLAG_GATE_COLOUR if gate_colour else 0) | (FLAG_GATE_PROBE if gate_probe else 0)
    if probe_out is not None:
        probe_out = _dev(probe_out, "probe_out", (z_vals.shape[0] * z_vals.shape[1], 2))
    ch = _capi.lib().inerf_raw_channels(desc, flags, 1)
    raw = _new(rays, n, s, ch)
    with torch.cuda.device(rays.device):
        ws_bytes = int(_capi.lib().inerf_encode_mlp_workspace_bytes(desc, n, s, flags))      # > 0: the SSR network's semantic-head scratch
        if ws_bytes < 0:
            _capi.check(ws_bytes, "inerf_encode_mlp_workspace_bytes")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=rays.device) if ws_bytes > 0 else None
        rc = _capi.lib().inerf_encode_mlp_margin(desc, _ptr(packed), _ptr(rays), _ptr(z_vals), n, s, flags, _ptr(raw),
                                                 None if status is None else C.c_void_p(status.data_ptr()), int(status_rays),
                                                 None if ws is None else C.c_void_p(ws.data_ptr()), ws_bytes,
                                                 None if probe_out is None else C.c_void_p(probe_out.data_ptr()),
                                                 _gate_state_ptr(gate_state, rays), _stream(rays))
    _capi.check(rc, "inerf_encode_mlp_margin")
    return raw


_COMPOSITE_KEYS = ("rgb", "disp", "acc", "depth", "albedo", "shading", "residual", "sem", "feat", "weights")


def composite(raw, z_vals, rays_d, noise=None, white_bkgd=False, n_classes=0, feat_dim=0, want_weights=True, draw=None):
    """raw2outputs (run_nerf.py:359-412 / model_utils.py:39-116) -> dict of maps.

    When ``raw`` requires grad (a training step through the staged path) the maps carry a grad_fn whose backward
    is the HIP kernel behind ``inerf_composite_backward``; ``z_vals`` / ``rays_d`` / ``noise`` get no gradient,
    as in the reference (resampled depths are detached, run_nerf.py:501).  ``draw``: the noise is drawn in the kernel (scaled
    by its noise_std; the fine pass's stream with its FINE flag) and the backward regenerates it from a snapshot of the step."""
    _draw_arg(draw, noise, "noise")
    if torch.is_grad_enabled() and isinstance(raw, torch.Tensor) and raw.requires_grad:
        keys, maps = _CompositeFn.run(raw, z_vals, rays_d, noise, white_bkgd, n_classes, feat_dim, want_weights, draw)
        return dict(zip(keys, maps))
    return _composite_forward(raw, z_vals, rays_d, noise, white_bkgd, n_classes, feat_dim, want_weights, draw)


def composite_backward(raw, z_vals, rays_d, grads, noise=None, white_bkgd=False, n_classes=0, feat_dim=0, draw=None):
    """d_raw[N,S,CH] for the output gradients in ``grads`` (dict: subset of rgb, disp, acc, depth, albedo, shading,
    residual, sem, feat, weights) - what autograd computes for raw2outputs in the reference's training step."""
    raw = _dev(raw, "raw", (None, None, None))
    n, s, ch = raw.shape
    z_vals = _dev(z_vals, "z_vals", (n, s))
    rays_d = _dev(rays_d, "rays_d", (n, 3))
    d = _draw_arg(draw, noise, "noise")
    noise = _opt(noise, "noise", (n, s), raw)
    shapes = {"rgb": (n, 3), "albedo": (n, 3), "residual": (n, 3), "disp": (n,), "acc": (n,), "depth": (n,), "shading": (n,),
              "sem": (n, n_classes), "feat": (n, feat_dim), "weights": (n, s)}
    held = {}
    for k, t in grads.items():
        if k not in shapes:
            raise KeyError(f"unknown output {k!r}")
        if t is not None:
            held[k] = _dev(t, "grad of " + k, shapes[k])
    d_raw = _new(raw, n, s, ch)
    co = CompositeOut(**{k: t.data_ptr() for k, t in held.items()})
    with torch.cuda.device(raw.device):
        if d is not None:
            rc = _capi.lib().inerf_composite_backward_drawn(_ptr(raw), _ptr(z_vals), _ptr(rays_d), 3, None, n, s, ch, n_classes,
                                                            feat_dim, FLAG_WHITE_BKGD if white_bkgd else 0, C.byref(co), _ptr(d_raw),
                                                            d, _stream(raw))
        else:
            rc = _capi.lib().inerf_composite_backward(_ptr(raw), _ptr(z_vals), _ptr(rays_d), 3, _ptr(noise), n, s, ch, n_classes,
                                                      feat_dim, FLAG_WHITE_BKGD if white_bkgd else 0, C.byref(co), _ptr(d_raw),
                                                      _stream(raw))
    _capi.check(rc, "inerf_composite_backward")
    return d_raw


class _CompositeFn(torch.autograd.Function):
    """Differentiable raw2outputs: HIP forward, HIP backward (the forward is recomputed there: only inputs are saved)."""

    @staticmethod
    def run(raw, z_vals, rays_d, noise, white_bkgd, n_classes, feat_dim, want_weights, draw=None):
        keys = [k for k in _COMPOSITE_KEYS if not (k == "sem" and n_classes == 0) and not (k == "feat" and feat_dim == 0)
                and not (k == "weights" and not want_weights)]
        maps = _CompositeFn.apply(raw, z_vals, rays_d, noise, white_bkgd, n_classes, feat_dim, tuple(keys), draw)
        return keys, maps

    @staticmethod
    def forward(ctx, raw, z_vals, rays_d, noise, white_bkgd, n_classes, feat_dim, keys, draw=None):
        raw_c, z_c, d_c = raw.detach().float().contiguous(), z_vals.detach().float().contiguous(), rays_d.detach().float().contiguous()
        noise_c = None if noise is None else noise.detach().float().contiguous()
        # drawn noise is not kept: the node holds the draw arguments with an 8-byte copy of the step they were drawn at
        ctx.draw = None if draw is None else freeze_draw(draw)
        out = _composite_forward(raw_c, z_c, d_c, noise_c, white_bkgd, n_classes, feat_dim, "weights" in keys, ctx.draw)
        # Outputs the loss does not use must arrive as None, not as zero tensors: the reference's autograd never visits the
        # branch of an unused output, while a ZERO cotangent on disp = 1 / (depth / acc) turns into NaN on every ray with
        # acc == 0 (0 x d(1/(0/0))) - and a trained network has such rays (sigma <= 0 along a ray through empty space) in every
        # batch.  Found by scripts/fit_synthetic.py: with materialised zeros the fit went NaN after a few hundred steps.
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(raw_c, z_c, d_c, *([] if noise_c is None else [noise_c]))
        ctx.cfg = (white_bkgd, n_classes, feat_dim, keys, noise_c is not None)
        return tuple(out[k] for k in keys)

    @staticmethod
    def backward(ctx, *gouts):
        white_bkgd, n_classes, feat_dim, keys, has_noise = ctx.cfg
        saved = ctx.saved_tensors
        raw, z_vals, rays_d = saved[:3]
        noise = saved[3] if has_noise else None
        grads = {k: g for k, g in zip(keys, gouts) if g is not None}
        d_raw = composite_backward(raw, z_vals, rays_d, grads, noise, white_bkgd, n_classes, feat_dim, ctx.draw)
        return d_raw, None, None, None, None, None, None, None, None


def _composite_forward(raw, z_vals, rays_d, noise=None, white_bkgd=False, n_classes=0, feat_dim=0, want_weights=True, draw=None):
    raw = _dev(raw, "raw", (None, None, None))
    n, s, ch = raw.shape
    z_vals = _dev(z_vals, "z_vals", (n, s))
    rays_d = _dev(rays_d, "rays_d", (n, 3))
    d = _draw_arg(draw, noise, "noise")
    noise = _opt(noise, "noise", (n, s), raw)
    out = {k: _new(raw, n, 3) for k in ("rgb", "albedo", "residual")}
    out.update({k: _new(raw, n) for k in ("disp", "acc", "depth", "shading")})
    if n_classes > 0:
        out["sem"] = _new(raw, n, n_classes)
    if feat_dim > 0:
        out["feat"] = _new(raw, n, feat_dim)
    if want_weights:
        out["weights"] = _new(raw, n, s)
    co = CompositeOut(**{k: t.data_ptr() for k, t in out.items()})
    with torch.cuda.device(raw.device):
        if d is not None:
            rc = _capi.lib().inerf_composite_drawn(_ptr(raw), _ptr(z_vals), _ptr(rays_d), 3, None, n, s, ch, n_classes,
                                                   feat_dim, FLAG_WHITE_BKGD if white_bkgd else 0, C.byref(co), d, _stream(raw))
        else:
            rc = _capi.lib().inerf_composite(_ptr(raw), _ptr(z_vals), _ptr(rays_d), 3, _ptr(noise), n, s, ch, n_classes,
                                             feat_dim, FLAG_WHITE_BKGD if white_bkgd else 0, C.byref(co), _stream(raw))
    _capi.check(rc, "inerf_composite")
    return out


def _u_arg(u, n, n_imp, like):
    u = _dev(u, "u")
    if u.dim() == 1 and u.shape[0] == n_imp:
        return u, 0
    if u.dim() == 2 and tuple(u.shape) == (n, n_imp):
        return u, FLAG_U_PER_RAY
    raise ValueError(f"u has shape {tuple(u.shape)}, expected ({n_imp},) or ({n}, {n_imp})")


def sample_fine(z_coarse, weights, u, n_importance, draw=None):
    """z_mid + sample_pdf + sort(cat) + std (run_nerf.py:499-503,519) -> (z_samples, z_merged, z_std).  ``draw``: per-ray u drawn in
    the kernel (``u`` None)."""
    z_coarse = _dev(z_coarse, "z_coarse", (None, None))
    n, sc = z_coarse.shape
    weights = _dev(weights, "weights", (n, sc))
    d = _draw_arg(draw, u, "u")
    if d is None:
        u, flags = _u_arg(u, n, n_importance, z_coarse)
    z_s, z_m, z_std = _new(z_coarse, n, n_importance), _new(z_coarse, n, sc + n_importance), _new(z_coarse, n)
    with torch.cuda.device(z_coarse.device):
        if d is not None:
            rc = _capi.lib().inerf_sample_fine_drawn(_ptr(z_coarse), _ptr(weights), None, n, sc, n_importance, 0,
                                                     _ptr(z_s), _ptr(z_m), _ptr(z_std), d, _stream(z_coarse))
        else:
            rc = _capi.lib().inerf_sample_fine(_ptr(z_coarse), _ptr(weights), _ptr(u), n, sc, n_importance, flags,
                                               _ptr(z_s), _ptr(z_m), _ptr(z_std), _stream(z_coarse))
    _capi.check(rc, "inerf_sample_fine")
    return z_s, z_m, z_std


def sample_pdf(bins, weights, u, n_samples, draw=None):
    """Stand-alone sample_pdf(bins, weights, N) (run_nerf_helpers.py:402-445).  ``draw``: per-ray u drawn in the kernel (``u`` None)."""
    bins = _dev(bins, "bins", (None, None))
    n, nb = bins.shape
    weights = _dev(weights, "weights", (n, nb - 1))
    d = _draw_arg(draw, u, "u")
    if d is None:
        u, flags = _u_arg(u, n, n_samples, bins)
    out = _new(bins, n, n_samples)
    with torch.cuda.device(bins.device):
        if d is not None:
            rc = _capi.lib().inerf_sample_pdf_drawn(_ptr(bins), _ptr(weights), None, n, nb, n_samples, 0, _ptr(out), d, _stream(bins))
        else:
            rc = _capi.lib().inerf_sample_pdf(_ptr(bins), _ptr(weights), _ptr(u), n, nb, n_samples, flags, _ptr(out),
                                              _stream(bins))
    _capi.check(rc, "inerf_sample_pdf")
    return out


_MAP_KEYS = ("rgb", "disp", "acc", "depth", "albedo", "shading", "residual")


def render_rays_fused(desc, packed_coarse, packed_fine, rays, n_samples, n_importance, t_vals, u=None, t_rand=None,
                      noise_coarse=None, noise_fine=None, white_bkgd=False, lindisp=False, endpoint=False,
                      want_raw_coarse=False, want_raw_fine=False, want_stages=False, want_sem=True, draw=None):
    """Whole render_rays path for one ray batch through ``inerf_render_rays`` - or, with ``draw`` (an inerf_draw_args whose PERTURB
    flag and noise_std say what the reference would draw), through ``inerf_render_rays_drawn``: t_rand and the noise tensors must
    then be None, and u too when PERTURB is set.

    Returns a dict with ``{rgb,disp,acc,depth,albedo,shading,residual[,sem]}_{coarse,fine}``, ``z_std``
    and, on request, ``raw_*`` / stage tensors (``z_coarse, weights_coarse, z_samples, z_fine,
    weights_fine``).  Everything is enqueued on the current stream; nothing synchronises.

    The gate probe's cull margin adapts to each network (include/inerf.h INERF_FLAG_GATE_PROBE): the margin state of a blob is
    ``packing.gate_state_of(blob)``, so it is remembered for as long as the same blob tensor is passed.  INERF_PROBE_ADAPT=0: no state,
    the constant margin.
    """
    L = _capi.lib()
    rays = _dev(rays, "rays", (None, RAY_FLOATS))
    n = rays.shape[0]
    if n * (n_samples + n_importance) > MAX_POINTS_PER_LAUNCH:
        raise ValueError("ray batch too large for one launch; chunk it (the render() front-ends do)")
    packed_coarse = _dev(packed_coarse, "packed_coarse", (None,))
    packed_fine = _opt(packed_fine, "packed_fine", (None,), rays)
    t_vals = _dev(t_vals, "t_vals", (n_samples,))
    d = _draw_arg(draw, next((t for t in (t_rand, noise_coarse, noise_fine) if t is not None), None), "t_rand / noise")
    drawn_u = d is not None and bool(draw.flags & _capi.DRAW_PERTURB)
    if drawn_u and u is not None:
        raise ValueError("u is drawn inside the kernel when draw has the PERTURB flag: pass one or the other")
    t_rand = _opt(t_rand, "t_rand", (n, n_samples), rays)
    noise_coarse = _opt(noise_coarse, "noise_coarse", (n, n_samples), rays)
    s_f = n_samples + n_importance
    noise_fine = _opt(noise_fine, "noise_fine", (n, s_f), rays) if n_importance > 0 else None
    flags = (FLAG_WHITE_BKGD if white_bkgd else 0) | (FLAG_LINDISP if lindisp else 0) | (FLAG_ENDPOINT if endpoint else 0)
    if n_importance > 0 and not drawn_u:
        if u is None:
            raise ValueError("u is required when n_importance > 0")
        u, uf = _u_arg(u, n, n_importance, rays)
        flags |= uf
    n_cls = desc.n_classes if (desc.variant == _capi.VARIANT_SSR and want_sem) else 0
    ch_c, ch_f = L.inerf_raw_channels(desc, flags, 0), L.inerf_raw_channels(desc, flags, 1)

    out = {}

    def maps(level, s_count, with_feat):
        d = {k: _new(rays, n, 3) for k in ("rgb", "albedo", "residual")}
        d.update({k: _new(rays, n) for k in ("disp", "acc", "depth", "shading")})
        if n_cls > 0:
            d["sem"] = _new(rays, n, n_cls)
        if with_feat:
            d["feat"] = _new(rays, n, ENDPOINT_DIM)
        if want_stages:
            d["weights"] = _new(rays, n, s_count)
        for k, t in d.items():
            out[f"{k}_{level}"] = t
        return CompositeOut(**{k: t.data_ptr() for k, t in d.items()})

    args = RenderArgs()
    args.net = desc
    args.packed_coarse, args.packed_fine = packed_coarse.data_ptr(), (packed_fine.data_ptr() if packed_fine is not None else None)
    args.rays, args.n_rays, args.n_samples, args.n_importance, args.flags = rays.data_ptr(), n, n_samples, n_importance, flags
    args.t_vals = t_vals.data_ptr()
    args.t_rand = t_rand.data_ptr() if t_rand is not None else None
    args.u = u.data_ptr() if (n_importance > 0 and not drawn_u) else None
    args.noise_coarse = noise_coarse.data_ptr() if noise_coarse is not None else None
    args.noise_fine = noise_fine.data_ptr() if noise_fine is not None else None
    args.coarse = maps("coarse", n_samples, False)
    if n_importance > 0:
        args.fine = maps("fine", s_f, bool(endpoint and desc.variant == _capi.VARIANT_SSR))
        out["z_std"] = _new(rays, n)
        args.z_std = out["z_std"].data_ptr()
    if want_raw_coarse:
        out["raw_coarse"] = _new(rays, n, n_samples, ch_c)
        args.raw_coarse = out["raw_coarse"].data_ptr()
    if want_raw_fine and n_importance > 0:
        out["raw_fine"] = _new(rays, n, s_f, ch_f)
        args.raw_fine = out["raw_fine"].data_ptr()
    if want_stages:
        out["z_coarse"] = _new(rays, n, n_samples)
        args.z_coarse = out["z_coarse"].data_ptr()
        if n_importance > 0:
            out["z_samples"], out["z_fine"] = _new(rays, n, n_importance), _new(rays, n, s_f)
            args.z_samples, args.z_fine = out["z_samples"].data_ptr(), out["z_fine"].data_ptr()
    ws_bytes = L.inerf_render_workspace_bytes(C.byref(args))       # nothing is reserved for stage tensors requested as outputs
    if ws_bytes < 0:
        _capi.check(int(ws_bytes), "inerf_render_workspace_bytes")
    ws = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device=rays.device)
    args.workspace, args.workspace_bytes = ws.data_ptr(), int(ws_bytes)
    if os.environ.get("INERF_PROBE_ADAPT", "1")[:1] != "0":
        from . import packing
        st_c = packing.gate_state_of(packed_coarse)
        st_f = st_c if packed_fine is None else packing.gate_state_of(packed_fine)
        args.gate_state_coarse, args.gate_state_fine = _gate_state_ptr(st_c, rays), _gate_state_ptr(st_f, rays)
    if desc.precision == _capi.PREC_F16X3:
        # caller checks it (check_f16_range) when it next synchronises; inside a chunked_status() block: one word per chunk of rays
        words = -(-n // _status_rays) if (_status_rays > 0 and n > _status_rays) else 1
        out["status"] = torch.zeros(words, dtype=torch.int32, device=rays.device)
        args.status = out["status"].data_ptr()
        args.status_rays = _status_rays if words > 1 else 0
    with torch.cuda.device(rays.device):
        rc = L.inerf_render_rays(C.byref(args), _stream(rays)) if d is None else L.inerf_render_rays_drawn(C.byref(args), d, _stream(rays))
    _capi.check(rc, "inerf_render_rays")
    # `ws` and the input tensors are kept alive by the caching allocator's stream semantics: they are
    # released on the same stream the kernels were enqueued on.
    return out


# ---------------------------------------------------------------------------------------------------------------------
# training: fused forward that keeps the activations, MFMA input-gradient chain, split-K MFMA weight gradients
# ---------------------------------------------------------------------------------------------------------------------
(SAVE_ENC, SAVE_DIR, SAVE_H0, SAVE_AS1H, SAVE_FEAT, SAVE_VH, SAVE_SEMH, SAVE_DPRE, SAVE_H7R, SAVE_SLOTS) = (0, 1, 2, 10, 11, 12, 13, 14, 15, 16)
ACT_SCALE = 8.0                 # activations travel as f16 hi/lo of 8 * value (csrc/layout.h kActScale)
SAVE_SCALARS = 64               # floats behind the slots and the mask area (reserved; include/inerf.h)


def frag_decode(frag, n_points, scale=ACT_SCALE, width=256):
    """A FRAGMENT slot of an ACTIVATION buffer (include/inerf.h: f16 hi/lo operand fragments of the weight-gradient products;
    ``frag``: its elements as a float32 or float16 tensor; ``width``: 256, or 64 for the encoding's slot) -> the fp32
    [n_points, width] matrix it encodes: (hi + lo) / scale."""
    h = frag.view(torch.float16) if frag.dtype != torch.float16 else frag
    cbs = width // 32
    tiles = h.numel() // (64 * width * 2)
    # [tile, pb, q, cb, plane, h, c, i_hi, i_lo]: point = 32 pb + 16 q + 8 i_hi + 4 h + i_lo, channel = 32 cb + c
    v = h.view(tiles, 2, 2, cbs, 2, 2, 32, 2, 4).float()
    v = v[:, :, :, :, 0] + v[:, :, :, :, 1]                                  # hi + lo: [tile, pb, q, cb, h, c, i_hi, i_lo]
    v = v.permute(0, 1, 2, 6, 4, 7, 3, 5).reshape(tiles * 64, width)        # -> [tile, pb, q, i_hi, h, i_lo, cb, c]
    return v[:n_points] / scale


def frag_encode(rows, scale=ACT_SCALE):
    """fp32 [n_points, W] (W = 256 or 64) -> the FRAGMENT slot of ``frag_decode`` (float16 tensor of 64 * ceil(n / 64) * 2 W
    halfs): hi = f16 of scale * value rounded towards zero, lo = f16(scale * value - hi); padding points are zero.  What the
    training forward's epilogue emits, restated with torch for the tests of the weight-gradient kernel."""
    n, width = rows.shape
    tiles = (n + 63) // 64
    v = torch.zeros(tiles * 64, width, dtype=torch.float32, device=rows.device)
    v[:n] = rows.float() * scale
    hi = (v.view(torch.int32) & ~0x1FFF).view(torch.float32)                 # 13 low mantissa bits cleared: exact in f16's normal range
    hi16 = hi.clamp(-65504.0, 65504.0).half()
    sub = hi16.float().abs() < 2.0 ** -14                                   # subnormal results were rounded, not truncated: fix up
    hi16 = torch.where(sub & (hi16.float().abs() > v.abs()), torch.nextafter(hi16.float(), torch.zeros_like(v)).half(), hi16)
    lo16 = (v - hi16.float()).half()
    both = torch.stack([hi16, lo16], 0)                                      # [plane, point, channel]
    both = both.view(2, tiles, 2, 2, 2, 2, 4, width // 32, 32)               # [plane, tile, pb, q, i_hi, h, i_lo, cb, c]
    return both.permute(1, 2, 3, 7, 0, 5, 8, 4, 6).contiguous().view(-1)     # [tile, pb, q, cb, plane, h, c, i_hi, i_lo]


def grad_frag_encode(rows):
    """fp32 [n_points, W] gradients (W = 256, or 128) -> (FRAGMENT slot, normalisers) as the input-gradient chain writes them into a gradient
    buffer: every point p is normalised by s_p = the power of two above its largest |value| (the chain uses its largest HEAD
    gradient; any power of two keeps the encoding exact) and stored as the split f16 halves of 8 * value / s_p;
    normalisers: float32[64 * ceil(n / 64) + 64] (1 for padding points; 64 readable floats behind the end)."""
    n = rows.shape[0]
    tiles = (n + 63) // 64
    m = rows.float().abs().amax(1)
    _, e = torch.frexp(m)
    s = torch.where(m > 0, torch.ldexp(torch.ones_like(m), e), torch.ones_like(m))
    scales = torch.ones(tiles * 64 + 64, dtype=torch.float32, device=rows.device)
    scales[:n] = s
    return frag_encode(rows.float() / s[:, None], ACT_SCALE), scales


def grad_frag_decode(frag, scales, n_points, width=256):
    """The inverse: (FRAGMENT slot of a gradient buffer, the points' normalisers) -> fp32 [n_points, width]."""
    return frag_decode(frag, n_points, ACT_SCALE, width) * scales[:n_points, None]


def save_slot_views(desc, buf, n_points, gradient=False):
    """The [n_points, width] matrices of an activation buffer (``gradient``: of a buffer of pre-activation gradients;
    include/inerf.h: slot list).  Row-format slots are views; FRAGMENT slots are decoded into new fp32 tensors."""
    views = []
    lib = _capi.lib()
    off, width = C.c_int64(), C.c_int()
    padded = (n_points + 63) // 64 * 64
    for slot in range(SAVE_SLOTS):
        _capi.check(lib.inerf_mlp_save_slot(desc, slot, n_points, C.byref(off), C.byref(width)), "inerf_mlp_save_slot")
        if width.value == 0:                        # (a slot this network does not have)
            views.append(buf[0:0].view(n_points, 0))
        elif lib.inerf_mlp_save_slot_is_fragment(slot, 1 if gradient else 0) == 1:
            frag = buf[off.value: off.value + padded * width.value]
            views.append(grad_frag_decode(frag, views[SAVE_ENC], n_points, width.value) if gradient else frag_decode(frag, n_points, width=width.value))
        elif gradient and slot == SAVE_ENC:         # the points' normalisers (include/inerf.h), not an [n, 64] matrix
            views.append(buf[off.value: off.value + padded])
        else:
            views.append(buf[off.value: off.value + n_points * width.value].view(n_points, width.value))
    return views


def encode_mlp_train(desc, packed, rays, z_vals, endpoint=False, status=None, act_max=None):
    """``encode_mlp`` that also returns the activation buffer the backward pass needs (PREC_F16X3 only).  ``act_max``:
    optional zeroed float32[1] device tensor that receives max |activation|."""
    rays = _dev(rays, "rays", (None, RAY_FLOATS))
    z_vals = _dev(z_vals, "z_vals", (rays.shape[0], None))
    packed = _dev(packed, "packed weights", (None,))
    n, s = z_vals.shape
    flags = FLAG_ENDPOINT if endpoint else 0
    ch = _capi.lib().inerf_raw_channels(desc, flags, 1)
    raw = _new(rays, n, s, ch)
    save = _new(rays, _capi.lib().inerf_mlp_save_floats(desc, n * s))
    with torch.cuda.device(rays.device):
        rc = _capi.lib().inerf_encode_mlp_train(desc, _ptr(packed), _ptr(rays), _ptr(z_vals), n, s, flags, _ptr(raw), _ptr(save),
                                                _ptr(act_max), None if status is None else C.c_void_p(status.data_ptr()),
                                                _stream(rays))
    _capi.check(rc, "inerf_encode_mlp_train")
    return raw, save


def mlp_backward_inputs(desc, packed_bwd, raw, d_raw, save, endpoint=False, status=None, dz_max=None, want_heads=False):
    """Pre-activation gradients of every layer (same slot layout as ``save``) from d loss / d raw.  ``dz_max``: optional
    zeroed float32[1] device tensor that receives max |dz| (the weight-gradient kernel's operand range).  ``want_heads``:
    also return the summed weight / bias gradients of the 1-4-row heads (see include/inerf.h) as a second value."""
    raw = _dev(raw, "raw", (None, None))
    p, ch = raw.shape
    d_raw = _dev(d_raw, "d_raw", (p, ch))
    save = _dev(save, "save", (None,))
    packed_bwd = _dev(packed_bwd, "packed transposed weights", (None,))
    dz = _new(raw, save.shape[0])
    heads = _new(raw, _capi.lib().inerf_mlp_backward_grid(p), _capi.lib().inerf_mlp_head_partial_floats()) if want_heads else None
    with torch.cuda.device(raw.device):
        rc = _capi.lib().inerf_mlp_backward_inputs(desc, _ptr(packed_bwd), _ptr(raw), _ptr(d_raw), _ptr(save), p,
                                                   FLAG_ENDPOINT if endpoint else 0, _ptr(dz), _ptr(dz_max), _ptr(heads),
                                                   None if status is None else C.c_void_p(status.data_ptr()), _stream(raw))
    _capi.check(rc, "inerf_mlp_backward_inputs")
    return (dz, heads.sum(0)) if want_heads else dz


def mlp_backward(desc, packed_bwd, raw, d_raw, save, act_max, endpoint=False, status=None):
    """The network's whole backward pass through ``inerf_mlp_backward`` (ONE call: chain, every weight-gradient product,
    reduction, scatter into the reference's parameter layout).  Returns the flat gradient blob - the parameter tensors of
    ``packing.tensor_table(desc)`` in order; ``param_views`` cuts it into named views."""
    L = _capi.lib()
    raw = _dev(raw, "raw", (None, None))
    p, ch = raw.shape
    d_raw = _dev(d_raw, "d_raw", (p, ch))
    save = _dev(save, "save", (None,))
    packed_bwd = _dev(packed_bwd, "packed transposed weights", (None,))
    act_max = _dev(act_max, "act_max", (1,))
    grads = _new(raw, L.inerf_param_floats(desc))
    ws_bytes = L.inerf_mlp_backward_workspace_bytes(desc, p)
    if ws_bytes < 0:
        _capi.check(int(ws_bytes), "inerf_mlp_backward_workspace_bytes")
    ws = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device=raw.device)
    with torch.cuda.device(raw.device):
        rc = L.inerf_mlp_backward(desc, _ptr(packed_bwd), _ptr(raw), _ptr(d_raw), _ptr(save), _ptr(act_max), p,
                                  FLAG_ENDPOINT if endpoint else 0, _ptr(grads), C.c_void_p(ws.data_ptr()), int(ws_bytes),
                                  None if status is None else C.c_void_p(status.data_ptr()), _stream(raw))
    _capi.check(rc, "inerf_mlp_backward")
    return grads


def param_views(desc, flat):
    """name -> view of the flat gradient / parameter blob with the reference's shapes (packing.tensor_table order)."""
    from . import packing
    out, off = {}, 0
    for name, (rows, cols) in packing.tensor_table(desc):
        n = rows * (cols if cols else 1)
        out[name] = flat[off:off + n].view((rows, cols) if cols else (rows,))
        off += n
    return out


def _head_names(desc):
    if desc.variant == _capi.VARIANT_OBJECT:      # run_nerf_helpers.py:259-279: 'shading_linear' is the residual head
        return "test_linear1", "test_linear2", "shading_linear"
    return "shading_linear1", "shading_linear2", "residual_linear"


def _split_k(n_points, target=64):
    """Largest divisor of n_points not above ``target``: dW = dZ^T X has a tiny output (<= 256 x 320) and K = n_points in
    the hundreds of thousands, which a GEMM library runs on a handful of workgroups; as a batched GEMM over K-chunks plus
    a sum it fills the chip (measured on 393 216 points: 11.0 ms with 8 chunks, 5.8 ms with 64, no gain beyond)."""
    for nc in range(min(target, n_points), 0, -1):
        if n_points % nc == 0:
            return nc
    return 1


def _tn(g, x, nc):
    """g^T @ x for g[P, M], x[P, N], split over P into nc chunks."""
    if nc == 1:
        return g.t() @ x
    p = g.shape[0]
    return torch.bmm(g.view(nc, p // nc, g.shape[1]).transpose(1, 2), x.view(nc, p // nc, x.shape[1])).sum(0)


def _pow2_scale(t):
    """Device scalar 2^k with max|t| * 2^k in [2^13, 2^14) (1 for an all-zero tensor) - no host sync."""
    m = t.abs().amax()
    _, e = torch.frexp(m)
    return torch.where((m > 0) & torch.isfinite(m), torch.ldexp(torch.ones_like(m), 14 - e), torch.ones_like(m))


ACTIVATION_RANGE = 6.0e4 / 8.0          # what the forward's f16 range check admits


class _WgradBatch:
    """Several ``G^T X`` products (and the column sums of their G) through inerf_mlp_weight_gradient, every workgroup's
    partial tiles side by side in ONE [grid, total] buffer: one launch per product, one sum at the end."""

    def __init__(self, n_points, ranges, like):
        self.p, self.ranges, self.like = n_points, ranges, like
        self.jobs, self.total = [], 0

    def add(self, g, x, m, n, want_bias=False, ranges=None):
        """Schedules g[:, :m]^T @ x[:, :n]; returns a key for ``result`` (and ``bias`` if want_bias).  ``ranges``: this
        product's own operand bounds (default: the batch's)."""
        job = dict(g=g, x=x, m=m, n=n, off=self.total, boff=None, ranges=ranges)
        self.total += m * n
        if want_bias:
            job["boff"] = self.total
            self.total += m
        self.jobs.append(job)
        return len(self.jobs) - 1

    def run(self):
        lib = _capi.lib()
        if self.p == 0:                        # no sample points: every gradient is zero
            self.sums = torch.zeros(self.total, dtype=torch.float32, device=self.like.device)
            return
        grid = lib.inerf_wgrad_grid(self.p)
        buf = _new(self.like, grid, self.total)
        with torch.cuda.device(self.like.device):
            for j in self.jobs:
                g, x = j["g"], j["x"]
                base = buf.data_ptr()
                rc = lib.inerf_mlp_weight_gradient(C.c_void_p(g.data_ptr()), g.stride(0), C.c_void_p(x.data_ptr()), x.stride(0), self.p,
                                                   j["m"], j["n"], _ptr(self.ranges if j["ranges"] is None else j["ranges"]),
                                                   C.c_void_p(base + 4 * j["off"]),
                                                   None if j["boff"] is None else C.c_void_p(base + 4 * j["boff"]), self.total,
                                                   _stream(self.like))
                _capi.check(rc, "inerf_mlp_weight_gradient")
        self.sums = buf.sum(0)

    def result(self, key):
        j = self.jobs[key]
        return self.sums[j["off"]: j["off"] + j["m"] * j["n"]].view(j["m"], j["n"])

    def bias(self, key):
        j = self.jobs[key]
        return self.sums[j["boff"]: j["boff"] + j["m"]]


def weight_gradient(g, x, m, n, ranges=None, want_bias=False):
    """g[:, :m]^T @ x[:, :n] (and optionally the column sums of g[:, :m]) through the HIP split-K kernel.  g / x: row-major
    fp32 matrices (or 32-column-aligned views of one); m in {128, 256}, n in {32, 64, 128, 256}; ``ranges``: float32[2] device
    tensor with upper bounds of |g| and |x| (computed here when absent - two extra passes over the data)."""
    if ranges is None:
        ranges = torch.stack([g[:, :m].abs().amax(), x[:, :n].abs().amax()]).float()
    b = _WgradBatch(g.shape[0], ranges, g)
    k = b.add(g, x, m, n, want_bias)
    b.run()
    return (b.result(k), b.bias(k)) if want_bias else b.result(k)


def weight_gradient_frag(g_frag, g_scale, x_frag, ranges, n_points, want_bias=False, x_rows=None, n=256):
    """G^T X with G a FRAGMENT slot of a gradient buffer (256 channels; ``g_scale``: the points' normalisers, see
    ``grad_frag_encode``) through the HIP split-K kernels: against ``x_frag``, a FRAGMENT slot of activations (the LDS-DMA
    kernel, 256 x 256), or, with ``x_rows`` ([n_points, >= n] fp32 rows), against row-format activations.  ``ranges``:
    float32[2] device tensor, upper bounds of the true |G| and of |X|."""
    lib = _capi.lib()
    grid = lib.inerf_wgrad_grid(n_points)
    total = 256 * n + (256 if want_bias else 0)
    buf = _new(ranges, grid, total)
    base = buf.data_ptr()
    bias = C.c_void_p(base + 4 * 256 * n) if want_bias else None
    with torch.cuda.device(ranges.device):
        if x_rows is None:
            rc = lib.inerf_mlp_weight_gradient_frag(_ptr(g_frag), _ptr(g_scale), _ptr(x_frag), _ptr(ranges), n_points, C.c_void_p(base), bias,
                                                    total, _stream(ranges))
        else:
            rc = lib.inerf_mlp_weight_gradient_gfrag(_ptr(g_frag), _ptr(g_scale), C.c_void_p(x_rows.data_ptr()), x_rows.stride(0), n_points, n,
                                                     _ptr(ranges), C.c_void_p(base), bias, total, _stream(ranges))
    _capi.check(rc, "inerf_mlp_weight_gradient_frag")
    sums = buf.sum(0)
    w = sums[:256 * n].view(256, n)
    return (w, sums[256 * n:]) if want_bias else w


def weight_gradient_frag_batch(g_frags, g_scale, x_frags, ranges, n_points, x_cols=None, g_rows=None):
    """Several products G_j^T X_j over the same points (fragment slots, shared normalisers; shapes ``g_rows[j]`` x ``x_cols[j]`` =
    256 x 256 (default), 256 x 64, 128 x 256, 128 x 32) in ONE launch of the LDS-DMA kernel, each split over its share of the
    grid (include/inerf.h inerf_mlp_weight_gradient_frag_batch).  Returns [(dW_j [rows, cols], db_j [rows])]."""
    lib = _capi.lib()
    n = len(g_frags)
    cols = [256] * n if x_cols is None else [int(c) for c in x_cols]
    grows = [256] * n if g_rows is None else [int(r) for r in g_rows]
    ccols, crows = (C.c_int * n)(*cols), (C.c_int * n)(*grows)
    rows = [lib.inerf_wgrad_frag_rows(n_points, n, crows, ccols, j) for j in range(n)]
    per = 256 * 256 + 256
    total = n * per
    buf = _new(ranges, max(rows), total)
    base = buf.data_ptr()
    arr = lambda vals: (C.c_void_p * n)(*vals)
    with torch.cuda.device(ranges.device):
        rc = lib.inerf_mlp_weight_gradient_frag_batch(n, arr([g.data_ptr() for g in g_frags]), _ptr(g_scale), arr([x.data_ptr() for x in x_frags]),
                                                      crows, ccols, _ptr(ranges), n_points, arr([base + 4 * j * per for j in range(n)]),
                                                      arr([base + 4 * (j * per + 65536) for j in range(n)]), total, _stream(ranges))
    _capi.check(rc, "inerf_mlp_weight_gradient_frag_batch")
    out = []
    for j in range(n):
        sums = buf[:rows[j], j * per:(j + 1) * per].sum(0)
        out.append((sums[:grows[j] * cols[j]].view(grows[j], cols[j]), sums[65536:65536 + grows[j]]))
    return out


def weight_gradient_xfrag(g_rows, x_frag, ranges, n_points, want_bias=False):
    """G^T X with G row-format ([n_points, >= 128] fp32: a 128-channel gradient slot) and X a FRAGMENT slot of activations
    (256 channels): the products of views_linears.0's feature columns and of the semantic hidden layer.  ``ranges[0]``: an
    upper bound of |G|."""
    lib = _capi.lib()
    grid = lib.inerf_wgrad_grid(n_points)
    m = 128
    total = m * 256 + (m if want_bias else 0)
    buf = _new(ranges, grid, total)
    base = buf.data_ptr()
    bias = C.c_void_p(base + 4 * m * 256) if want_bias else None
    with torch.cuda.device(ranges.device):
        rc = lib.inerf_mlp_weight_gradient_xfrag(C.c_void_p(g_rows.data_ptr()), g_rows.stride(0), _ptr(x_frag), n_points, m, _ptr(ranges),
                                                 C.c_void_p(base), bias, total, _stream(ranges))
    _capi.check(rc, "inerf_mlp_weight_gradient_xfrag")
    sums = buf.sum(0)
    w = sums[:m * 256].view(m, 256)
    return (w, sums[m * 256:]) if want_bias else w


def _colsum(g, nc):
    return g.sum(0) if nc == 1 else g.view(nc, g.shape[0] // nc, g.shape[1]).sum(1).sum(0)


def mlp_weight_gradients(desc, names, save, dz, d_raw, n_points, endpoint=False, heads=None):
    """dW = dZ^T X and db = column sums of dZ for every layer, from the buffers of ``encode_mlp_train`` / ``mlp_backward_inputs``
    through LIBRARY GEMMs split over K (fragment slots are decoded first): the independent restatement that the tests and
    scripts/bench_train_kernels.py hold ``mlp_backward`` - the product path: one C call, HIP kernels only - against.  The 1-4-row
    heads' gradients are taken from ``heads`` (as accumulated by the chain kernel) when given.  Returns a dict name -> gradient
    with the reference's parameter names and shapes."""
    X = save_slot_views(desc, save, n_points)
    G = save_slot_views(desc, dz, n_points, gradient=True)
    e, dv = 3 + 6 * desc.l_xyz, 3 + 6 * desc.l_dir
    sh1, sh2, res = _head_names(desc)
    sem = desc.variant == _capi.VARIANT_SSR and desc.n_classes > 0
    nc = _split_k(n_points)
    h = [X[SAVE_H0 + i] for i in range(8)]        # enc / dir: zero-padded columns, cut from the products
    # (G slot, X slot): the products with 128 / 256 rows
    big = {"t0": (SAVE_H0, SAVE_ENC), "t5e": (SAVE_H0 + 5, SAVE_ENC), "as1": (SAVE_AS1H, SAVE_H0 + 7), "feat": (SAVE_FEAT, SAVE_H0 + 7),
           "vf": (SAVE_VH, SAVE_FEAT), "vd": (SAVE_VH, SAVE_DIR)}
    for i in range(1, 8):
        big[f"t{i}"] = (SAVE_H0 + i, SAVE_H0 + i - 1)
    if sem:
        big["sem1"] = (SAVE_SEMH, SAVE_H0 + 7)
    W, B = {}, {}
    for k, (gs, xs) in big.items():
        W[k] = _tn(G[gs], X[xs], nc)
        if gs not in B:
            B[gs] = _colsum(G[gs], nc)
    out = {}

    def lin(name, g, x):
        out[name + ".weight"] = _tn(g, x, nc)
        out[name + ".bias"] = _colsum(g, nc)

    out["pts_linears.0.weight"] = W["t0"][:, :e]
    for i in range(1, 8):
        out[f"pts_linears.{i}.weight"] = torch.cat([W["t5e"][:, :e], W["t5"]], 1) if i == 5 else W[f"t{i}"]   # cat([pts, h]), helpers:290-291
    for i in range(8):
        out[f"pts_linears.{i}.bias"] = B[SAVE_H0 + i]
    out["albedo_linear1.weight"], out["albedo_linear1.bias"] = W["as1"][0:128], B[SAVE_AS1H][0:128]
    out[sh1 + ".weight"], out[sh1 + ".bias"] = W["as1"][128:256], B[SAVE_AS1H][128:256]
    out["feature_linear.weight"], out["feature_linear.bias"] = W["feat"], B[SAVE_FEAT]
    out["views_linears.0.weight"], out["views_linears.0.bias"] = torch.cat([W["vf"], W["vd"][:, :dv]], 1), B[SAVE_VH]
    dpre = G[SAVE_DPRE]
    if heads is None:
        lin("alpha_linear", dpre[:, 7:8], h[7])
    if sem:
        out["semantic_linear.0.0.weight"], out["semantic_linear.0.0.bias"] = W["sem1"], B[SAVE_SEMH]
        c = desc.n_classes
        lin("semantic_linear.1", d_raw[:, BASE_CHANNELS:BASE_CHANNELS + c], X[SAVE_SEMH])
    if heads is None:
        as1h = X[SAVE_AS1H]
        lin("albedo_linear2", dpre[:, 0:3], as1h[:, :128])
        lin(sh2, dpre[:, 3:4], as1h[:, 128:])
        lin(res, dpre[:, 4:7], X[SAVE_VH])
    else:                      # accumulated by the chain kernel itself (layout: include/inerf.h)
        as2 = heads[384:1408].view(4, 256)
        out[res + ".weight"], out[res + ".bias"] = heads[0:384].view(3, 128), heads[1668:1671]
        out["albedo_linear2.weight"], out["albedo_linear2.bias"] = as2[0:3, 0:128], heads[1664:1667]
        out[sh2 + ".weight"], out[sh2 + ".bias"] = as2[3:4, 128:256], heads[1667:1668]
        out["alpha_linear.weight"], out["alpha_linear.bias"] = heads[1408:1664].view(1, 256), heads[1671:1672]
    return {k: out[k] for k in names}


class _FusedMlpFn(torch.autograd.Function):
    """raw = MLP(encode(o + d z), encode(viewdir)) with a HIP forward AND backward: fused split-f16 forward that keeps the
    activations, MFMA input-gradient chain, split-K MFMA weight gradients.  Parameters are re-packed on the device
    (packing.DevicePacker).  rays / z get no gradient (as in the reference: rays are data, resampled depths are detached)."""

    @staticmethod
    def forward(ctx, rays, z_vals, desc, endpoint, names, exact, *params):
        from . import packing
        named = dict(zip(names, params))
        status = _new_status(rays)
        act_max = torch.zeros(1, dtype=torch.float32, device=rays.device)
        packed = packing.device_packer(desc, False, rays.device)(named)
        raw, save = encode_mlp_train(desc, packed, rays.detach(), z_vals.detach(), endpoint, status, act_max)
        if exact:
            # INERF_PRECISION=f32: the values that leave the node come from the exact-fp32 MFMA kernel (bit for bit what a
            # no_grad render returns); the split-precision forward above is kept for what it SAVES - activations, ReLU masks,
            # operand ranges - which is what the backward kernels consume (22-bit operands, fp32 accumulation: within 1e-5 of
            # fp64 autograd).  The chain takes its sigmoid' from the exact outputs.
            d32 = _capi.NetDesc(desc.variant, desc.n_classes, desc.l_xyz, desc.l_dir, desc.xyz_div, _capi.PREC_F32)
            raw = encode_mlp(d32, packing.device_packer_f32(desc, rays.device)(named), rays.detach(), z_vals.detach(), endpoint)
        # the transposed blob of the backward pass is packed NOW, behind the forward kernel in the queue: at the start of the
        # backward the queue is empty, and its ~25 small launches would each cost a host round trip of GPU idle time
        packed_bwd = packing.device_packer(desc, True, rays.device)(named)
        check_f16_range(status, "training forward", deferrable=True)      # the front-ends read both networks' words once per batch
        ctx.packed_bwd = packed_bwd
        ctx.save_for_backward(raw, save, act_max, *params)
        ctx.cfg = (desc, endpoint, names)
        return raw

    @staticmethod
    def backward(ctx, d_raw):
        desc, endpoint, names = ctx.cfg
        raw, save, act_max = ctx.saved_tensors[:3]
        n, s, ch = raw.shape
        status = _new_status(raw)
        d2 = d_raw.contiguous().view(n * s, ch).float()
        # one C call: chain + weight gradients + reduction + scatter (inerf_mlp_backward)
        flat = mlp_backward(desc, ctx.packed_bwd, raw.view(n * s, ch), d2, save, act_max, endpoint, status)
        grads = param_views(desc, flat)
        check_f16_range(status, "training backward")      # read AFTER everything is enqueued: the GPU works through it meanwhile
        return (None, None, None, None, None, None) + tuple(grads[k] for k in names)


TRAIN_POINTS_PER_NODE = 2 * 1024 * 1024


def mlp_train(desc, module, rays, z_vals, endpoint=False):
    """Differentiable fused network evaluation for a training step: ``module``'s parameters receive gradients.
    ``desc.precision`` = INERF_PREC_F32: the forward values come from the exact-fp32 kernel (see _FusedMlpFn.forward)."""
    from . import packing
    exact = desc.precision == _capi.PREC_F32
    d = _capi.NetDesc(desc.variant, desc.n_classes, desc.l_xyz, desc.l_dir, desc.xyz_div, _capi.PREC_F16X3)
    names = tuple(name for name, _ in packing.tensor_table(d))
    named = dict(module.named_parameters())
    params = [named[k] for k in names]
    n, s = z_vals.shape
    per = max(1, TRAIN_POINTS_PER_NODE // s)        # the library keeps 11 KB per point; one node stays below its 4 M-point limit
    if n <= per:
        return _FusedMlpFn.apply(rays, z_vals, d, bool(endpoint), names, exact, *params)
    return torch.cat([_FusedMlpFn.apply(rays[i:i + per], z_vals[i:i + per], d, bool(endpoint), names, exact, *params)
                      for i in range(0, n, per)], 0)


# ---------------------------------------------------------------- training batch assembly (csrc/batch.hip)
_INDEX_NAMES = ("image", "pixels", "off_row", "off_col")


def _table(t, name, dtypes, shape, like=None):
    """A device-resident table of one of ``dtypes`` with ``shape`` (None: any extent), contiguous."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} lives on {t.device}: intrinsicnerf_amd runs only on a HIP device "
                           "(no CPU / eager fallback exists)")
    if t.dtype not in dtypes:
        raise ValueError(f"{name} must be one of {[str(d) for d in dtypes]}, got {t.dtype}")
    if t.dim() != len(shape) or any(s is not None and int(t.shape[i]) != s for i, s in enumerate(shape)):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple('*' if s is None else s for s in shape)}")
    if like is not None and t.device != like.device:
        raise ValueError(f"{name} is on {t.device}, expected {like.device}")
    return t if t.is_contiguous() else t.contiguous()


def _batch_indices(a, n, indices, draw, like):
    """Fill the index half of a BatchArgs: form (a) from ``indices`` = (image, pixels, off_row, off_col), form (b) from
    ``draw`` = dict(seed, step | step_dev, advance, image_ids).  Returns the tensors whose pointers it stored: a ``.contiguous()``
    copy among them must stay referenced until the launch is issued (its block could otherwise be handed to an output)."""
    keep = []
    if (indices is None) == (draw is None):
        raise ValueError("give either indices=(image, pixels, off_row, off_col) or draw=dict(seed=..., step=...)")
    if indices is not None:
        image, pixels, off_row, off_col = indices
        if isinstance(image, torch.Tensor):
            image = _table(image.reshape(-1), "indices[0] (image)", (torch.int64,), (1,), like)
            a.image_index = _ptr(image)
            keep.append(image)
        else:
            a.image_host = int(image)
        for name, t in (("pixels", pixels), ("off_row", off_row), ("off_col", off_col)):
            t = _table(t, f"indices ({name})", (torch.int64,), (n,), like)
            setattr(a, name, _ptr(t))
            keep.append(t)
        return keep
    a.flags |= _capi.BATCH_DRAW
    a.seed = int(draw["seed"]) & 0xFFFFFFFFFFFFFFFF
    step_dev = draw.get("step_dev")
    if step_dev is not None:
        step_dev = _table(step_dev, "step_dev", (torch.int64,), (1,), like)
        a.step_dev = _ptr(step_dev)
        keep.append(step_dev)
        if draw.get("advance", False):
            a.flags |= _capi.BATCH_ADVANCE
    else:
        a.step = int(draw.get("step", 0))
    ids = draw.get("image_ids")
    if ids is not None:
        ids = _table(ids, "image_ids", (torch.int64,), (None,), like)
        a.image_ids, a.n_image_ids = _ptr(ids), ids.shape[0]
        keep.append(ids)
    return keep


def _batch_index_outputs(a, n, like, want):
    if not want:
        return None
    out = {"image": torch.empty(1, dtype=torch.int64, device=like.device)}
    out.update({k: torch.empty(n, dtype=torch.int64, device=like.device) for k in _INDEX_NAMES[1:]})
    a.out_image, a.out_pixels, a.out_off_row, a.out_off_col = (_ptr(out[k]) for k in _INDEX_NAMES)
    return out


def _batch_poses(poses, like=None):
    poses = _dev(poses, "poses")
    if poses.dim() != 3 or poses.shape[1] not in (3, 4) or poses.shape[2] != 4:
        raise ValueError(f"poses has shape {tuple(poses.shape)}, expected [n_images, 3|4, 4]")
    if like is not None and poses.device != like.device:
        raise ValueError(f"poses is on {poses.device}, expected {like.device}")
    return poses


def check_batch_status(status, what="inerf_batch_assemble"):
    """Raise if a batch launch clamped a supplied index or ran into the bound of its cycle walk (reads the word: synchronises)."""
    word = int(status.item())
    if word & _capi.BATCH_STATUS_INDEX:
        raise IndexError(f"{what}: an index lies outside its table (it was clamped into it)")
    if word & _capi.BATCH_STATUS_WALK:
        raise RuntimeError(f"{what}: the cycle walk of the pixel permutation reached its bound of {_capi.BATCH_MAX_WALK} (duplicate pixel)")


def batch_object(images, masks, poses, intrinsics, window, n, indices=None, draw=None, status=None, return_indices=False):
    """Object-level training batch (run_nerf.py:886-938) through ``inerf_batch_assemble``: ``(batch_rays [2, 2n, 3],
    target_s [2n, 3], target_m [2n, 1] | None)`` - the n selected pixels, then their n neighbours - plus the dict of the indices
    used with ``return_indices``.  ``images`` [n_img, H, W, 3] / ``masks`` [n_img, H, W, 1] | None / ``poses`` [n_img, 3|4, 4]:
    fp32, device-resident.  ``intrinsics`` = (fx, fy, cx, cy); ``window`` = (row0, col0, rows, cols).  ``indices`` =
    (image, pixels, off_row, off_col) (form a) or ``draw`` = dict(seed, step | step_dev [, advance, image_ids]) (form b)."""
    images = _dev(images, "images", (None, None, None, 3))
    n_img, h, w = (int(s) for s in images.shape[:3])
    masks = _opt(masks, "masks", (n_img, h, w, 1), images)
    poses = _batch_poses(poses, images)
    if poses.shape[0] != n_img:
        raise ValueError(f"{poses.shape[0]} poses for {n_img} images")
    n = int(n)
    a = _capi.BatchArgs()
    a.form, a.flags, a.n = _capi.BATCH_OBJECT, _capi.BATCH_OPENGL, n
    a.n_images, a.height, a.width = n_img, h, w
    a.row0, a.col0, a.win_h, a.win_w = (int(v) for v in window)
    a.poses, a.pose_stride = _ptr(poses), poses.shape[1] * 4
    a.fx, a.fy, a.cx, a.cy = (float(v) for v in intrinsics)
    a.images, a.image_bytes = _ptr(images), 4
    held = _batch_indices(a, n, indices, draw, images) if n >= 0 else None
    rays, target_s = _new(images, 2, 2 * max(n, 0), 3), _new(images, 2 * max(n, 0), 3)
    target_m = _new(images, 2 * max(n, 0), 1) if masks is not None else None
    a.out_rays, a.out_rgb = _ptr(rays), _ptr(target_s)
    if masks is not None:
        a.aux, a.aux_bytes, a.out_aux = _ptr(masks), 4, _ptr(target_m)
    a.status = _ptr(status)
    idx = _batch_index_outputs(a, max(n, 0), images, return_indices)
    with torch.cuda.device(images.device):
        rc = _capi.lib().inerf_batch_assemble(C.byref(a), _stream(images))
    del held                                  # (referenced until the launch was issued; the stream orders the rest)
    _capi.check(rc, "inerf_batch_assemble")
    return (rays, target_s, target_m, idx) if return_indices else (rays, target_s, target_m)


_SEMANTIC_DTYPES = (torch.uint8, torch.int16, torch.int32, torch.int64)


def batch_ssr(image, depth, semantic, n, rays=None, camera=None, avail=None, indices=None, draw=None, status=None,
              return_indices=False):
    """SSR training batch (trainer.py:627-691 with no_batching=True; sampling_index, rays.py:153-172) through
    ``inerf_batch_assemble``: ``(sampled_rays [2n, 11], gt_rgb [2n, 3], gt_depth [2n] | None, gt_semantic [2n] int64 | None,
    avail [1] fp64 | None)`` (+ the indices dict).  ``image`` [n_img, H, W, 3] fp32 | fp64, ``depth`` [n_img, H, W] fp32 | fp64,
    ``semantic`` [n_img, H, W] uint8 | int16 | int32 | int64, ``avail`` [n_img] fp64 (mask_ids): device-resident.  Rays: rows of
    ``rays`` [n_img, H*W, 11], or computed from ``camera`` = dict(poses, fx, fy, cx, cy, near, far, opengl) as inerf_gen_rays
    writes them.  ``indices`` / ``draw`` as in ``batch_object`` (pixels are flat h * W + w; drawn ones come with replacement)."""
    image = _table(image, "image", (torch.float32, torch.float64), (None, None, None, 3))
    n_img, h, w = (int(s) for s in image.shape[:3])
    n = int(n)
    a = _capi.BatchArgs()
    a.form, a.n = _capi.BATCH_SSR, n
    a.n_images, a.height, a.width = n_img, h, w
    a.images, a.image_bytes = _ptr(image), image.element_size()
    if (rays is None) == (camera is None):
        raise ValueError("give either the ray table `rays` or `camera`")
    if rays is not None:
        rays = _table(rays, "rays", (torch.float32,), (n_img, h * w, RAY_FLOATS), image)
        a.ray_table = _ptr(rays)
    else:
        poses = _batch_poses(camera["poses"], image)
        if poses.shape[0] != n_img:
            raise ValueError(f"{poses.shape[0]} poses for {n_img} images")
        a.poses, a.pose_stride = _ptr(poses), poses.shape[1] * 4
        a.fx, a.fy, a.cx, a.cy, a.near, a.far = (float(camera[k]) for k in ("fx", "fy", "cx", "cy", "near", "far"))
        if camera.get("opengl", False):
            a.flags |= _capi.BATCH_OPENGL
    rows = 2 * max(n, 0)
    out_rays = _new(image, rows, RAY_FLOATS)
    out_rgb = torch.empty((rows, 3), dtype=image.dtype, device=image.device)
    a.out_rays, a.out_rgb = _ptr(out_rays), _ptr(out_rgb)
    out_depth = out_sem = out_avail = None
    if depth is not None:
        depth = _table(depth, "depth", (torch.float32, torch.float64), (n_img, h, w), image)
        out_depth = torch.empty(rows, dtype=depth.dtype, device=image.device)
        a.aux, a.aux_bytes, a.out_aux = _ptr(depth), depth.element_size(), _ptr(out_depth)
    if semantic is not None:
        semantic = _table(semantic, "semantic", _SEMANTIC_DTYPES, (n_img, h, w), image)
        out_sem = torch.empty(rows, dtype=torch.int64, device=image.device)
        a.semantic, a.semantic_bytes, a.out_semantic = _ptr(semantic), semantic.element_size(), _ptr(out_sem)
    if avail is not None:
        avail = _table(avail, "avail", (torch.float64,), (n_img,), image)
        out_avail = torch.zeros(1, dtype=torch.float64, device=image.device) if n <= 0 else torch.empty(1, dtype=torch.float64, device=image.device)
        a.avail, a.out_avail = _ptr(avail), _ptr(out_avail)
    held = _batch_indices(a, n, indices, draw, image) if n >= 0 else None
    a.status = _ptr(status)
    idx = _batch_index_outputs(a, max(n, 0), image, return_indices)
    with torch.cuda.device(image.device):
        rc = _capi.lib().inerf_batch_assemble(C.byref(a), _stream(image))
    del held
    _capi.check(rc, "inerf_batch_assemble")
    out = (out_rays, out_rgb, out_depth, out_sem, out_avail)
    return out + (idx,) if return_indices else out


# ---------------------------------------------------------------------------------------------------------------------
# validation metrics (csrc/eval.hip).  Every float argument is a VIEW, never copied: [n] with any element stride or [n, width]
# with unit stride along the row and any row stride >= width - a column (range) of a frames.pack_maps pack, or a tensor of its own
# ---------------------------------------------------------------------------------------------------------------------
def _eval_view(t, name, width, n=None):
    """(tensor, stride in floats) of one float argument of the evaluation kernels; validates everything but the device."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if t.dim() == 2 and width == 1 and t.shape[1] == 1:
        t = t[:, 0]
    if (t.dim() != 1 if width == 1 else (t.dim() != 2 or t.shape[1] != width)):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {('*',) if width == 1 else ('*', width)}")
    if n is not None and t.shape[0] != n:
        raise ValueError(f"{name} holds {t.shape[0]} rows, expected {n}")
    if width > 1 and t.shape[0] > 0 and t.stride(1) != 1:
        raise ValueError(f"{name} must have unit stride along its rows, got stride {t.stride(1)}")
    stride = int(t.stride(0))
    if t.shape[0] <= 1:
        stride = max(stride, width)
    if stride < width:
        raise ValueError(f"{name} has a row stride of {stride} floats, smaller than its width {width}")
    return t, stride


def _eval_classes(n_classes):
    c = int(n_classes)
    if not 1 <= c <= _capi.MAX_CLASSES:
        raise ValueError(f"n_classes={c}: the evaluation kernels take 1 .. {_capi.MAX_CLASSES} classes")
    return c


def _eval_devices(named):
    """All tensors on one device, and that device a HIP one."""
    like_name, like = named[0]
    for name, t in named[1:]:
        if t.device != like.device:
            raise ValueError(f"{name} is on {t.device}, expected {like.device} ({like_name}'s device)")
    if not like.is_cuda:
        raise RuntimeError(f"{like_name} lives on {like.device}: intrinsicnerf_amd runs only on a HIP device (no CPU / eager fallback exists)")
    return like.device


def sem_maps(logits, label=None, entropy=None, want_label=True, want_entropy=True):
    """Label map and entropy map of semantic logits [n, C] in one launch of ``inerf_sem_maps`` (trainer.py:1244-1245): the lowest
    index of each row's maximum as a float, and the entropy of its softmax.  ``label`` / ``entropy``: [n] fp32 views to write into
    (any element stride: a column of a pack), allocated when not given and wanted.  Returns ``(label, entropy)``."""
    if isinstance(logits, torch.Tensor) and logits.dim() == 2:
        width = int(logits.shape[1])
    else:
        raise ValueError("logits must be a [n, C] tensor" if isinstance(logits, torch.Tensor) else "logits must be a torch.Tensor")
    c = _eval_classes(width)
    logits, ld = _eval_view(logits, "logits", c)
    n = logits.shape[0]
    named = [("logits", logits)]
    outs = []
    for name, t, want in (("label", label, want_label), ("entropy", entropy, want_entropy)):
        if t is not None:
            t, st = _eval_view(t, name, 1, n)
            named.append((name, t))
        elif want:
            t, st = torch.empty(n, dtype=torch.float32, device=logits.device), 1
        else:
            st = 1
        outs.append((t, st))
    device = _eval_devices(named)
    (label, lst), (entropy, est) = outs
    with torch.cuda.device(device):
        rc = _capi.lib().inerf_sem_maps(_ptr(logits), ld, n, c, _ptr(label), lst, _ptr(entropy), est, _stream(logits))
    _capi.check(rc, "inerf_sem_maps")
    return label, entropy


def eval_workspace_bytes(n):
    return int(_capi.lib().inerf_eval_workspace_bytes(int(n)))


def eval_tables(n_classes, device):
    """Zeroed accumulators of ``eval_accumulate``: ``counts`` [C * C + 8] int64 and ``sums`` [6] float64 on ``device``."""
    c = _eval_classes(n_classes)
    return (torch.zeros(c * c + _capi.EVAL_COUNTS, dtype=torch.int64, device=device),
            torch.zeros(_capi.EVAL_SUMS, dtype=torch.float64, device=device))


def eval_accumulate(counts, sums, n_classes, ignore_label=-1, logits=None, pred_label=None, true_label=None, depth_pred=None,
                    depth_trgt=None, rgb_pred=None, rgb_trgt=None, out_label=None, out_entropy=None, want_maps=True, workspace=None):
    """One pass of ``inerf_eval_accumulate`` over n pixels, ADDING into ``counts`` / ``sums`` (``eval_tables``; the caller zeroes
    them): the confusion table of (``true_label``, predicted label) - the prediction a float column ``pred_label`` or derived
    from ``logits`` [n, C] in the same launch -, the depth counts and error sums of (``depth_trgt``, ``depth_pred``) and the squared
    error of (``rgb_pred``, ``rgb_trgt``) [n, 3].  Each group is optional.  With ``logits`` the label and entropy maps are written
    as ``sem_maps`` writes them (``out_label`` / ``out_entropy``, allocated when not given unless ``want_maps`` is false) and
    returned; otherwise ``(None, None)``."""
    c = _eval_classes(n_classes)
    for name, t, size, dtype in (("counts", counts, c * c + _capi.EVAL_COUNTS, torch.int64), ("sums", sums, _capi.EVAL_SUMS, torch.float64)):
        if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.dim() == 1 and t.shape[0] == size and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {dtype} vector of {size} entries ({c} classes)")
    named = [("counts", counts), ("sums", sums)]
    a = _capi.EvalArgs()
    a.n_classes, a.ignore_label = c, int(ignore_label)
    n = None
    held = []

    def take(name, t, width):
        nonlocal n
        t, st = _eval_view(t, name, width, n)
        n = t.shape[0]
        named.append((name, t))
        held.append(t)
        setattr(a, name, t.data_ptr())
        setattr(a, name + "_stride", st)
        return t

    if logits is not None:
        if pred_label is not None:
            raise ValueError("pred_label and logits are alternatives: give one")
        if not (isinstance(logits, torch.Tensor) and logits.dim() == 2 and logits.shape[1] == c):
            raise ValueError(f"logits must be a [n, {c}] tensor, got {tuple(logits.shape) if isinstance(logits, torch.Tensor) else type(logits).__name__}")
        logits = take("logits", logits, c)
    if true_label is not None:
        if logits is None and pred_label is None:
            raise ValueError("true_label needs a prediction: pred_label or logits")
        take("true_label", true_label, 1)
        if pred_label is not None:
            take("pred_label", pred_label, 1)
    elif pred_label is not None:
        raise ValueError("pred_label given without true_label")
    for (pn, p), (tn, t), width in ((("depth_pred", depth_pred), ("depth_trgt", depth_trgt), 1), (("rgb_pred", rgb_pred), ("rgb_trgt", rgb_trgt), 3)):
        if (p is None) != (t is None):
            raise ValueError(f"{pn} and {tn} go together")
        if p is not None:
            take(pn, p, width)
            take(tn, t, width)
    if n is None:
        raise ValueError("eval_accumulate: no group given (logits, true_label, depth_pred or rgb_pred)")
    label = entropy = None
    if logits is not None:
        for name, t in (("out_label", out_label), ("out_entropy", out_entropy)):
            if t is not None:
                take(name, t, 1)
            elif want_maps:
                t = torch.empty(n, dtype=torch.float32, device=logits.device)
                setattr(a, name, t.data_ptr())
                setattr(a, name + "_stride", 1)
            if name == "out_label":
                label = t
            else:
                entropy = t
    elif out_label is not None or out_entropy is not None:
        raise ValueError("out_label / out_entropy are written only with logits")
    if workspace is not None:
        if not (isinstance(workspace, torch.Tensor) and workspace.dtype == torch.float64 and workspace.is_contiguous()):
            raise ValueError("workspace must be a contiguous float64 tensor")
        named.append(("workspace", workspace))
    device = _eval_devices(named)
    a.n = n
    need = eval_workspace_bytes(n)
    if workspace is None:
        workspace = torch.empty(max(need // 8, 1), dtype=torch.float64, device=device)
    a.counts, a.sums = counts.data_ptr(), sums.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * 8
    with torch.cuda.device(device):
        rc = _capi.lib().inerf_eval_accumulate(C.byref(a), _stream(counts))
    del held
    _capi.check(rc, "inerf_eval_accumulate")
    return label, entropy


# ---------------------------------------------------------------------------------------------------------------------
# intrinsic-image quality metrics (csrc/imq.hip).  Inputs are VIEWS, never copied: an image is [H, W, C] or, with ``shape=(H, W)``,
# its flat form [H * W, C] - either with a leading stack axis - with unit stride along the channels, one pixel stride and one image
# stride: a column range of a frames.pack_maps pack, or a tensor of its own
# ---------------------------------------------------------------------------------------------------------------------
def _imq_view(t, name, shape, channels, n=None):
    """``(tensor, n_images, height, width, pixel stride, image stride)`` of one input of ``image_quality``; ``channels`` None: the
    mask (one float per pixel, no channel axis)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    dims, strides = list(t.shape), list(t.stride())
    width = 1 if channels is None else channels
    if channels is not None:
        if not dims or dims[-1] != width:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected a last axis of {width}")
        if width > 1 and strides[-1] != 1:
            raise ValueError(f"{name} must have unit stride along its channels, got stride {strides[-1]}")
        dims, strides = dims[:-1], strides[:-1]
    if shape is not None:
        h, w = int(shape[0]), int(shape[1])
    elif len(dims) in (2, 3):
        h, w = dims[-2], dims[-1]
    else:
        raise ValueError(f"{name} has shape {tuple(t.shape)}: expected [H, W{', C' if channels else ''}] with an optional leading stack "
                         "axis (or a flat form with shape=(H, W))")
    if dims[-2:] == [h, w] and len(dims) in (2, 3):
        if h > 1 and w > 1 and strides[-2] != w * strides[-1]:
            raise ValueError(f"{name}: its rows are {strides[-2]} floats apart, expected width * pixel stride = {w * strides[-1]}")
        pixel = strides[-1] if w > 1 else strides[-2]
        lead = len(dims) - 2
    elif dims[-1:] == [h * w] and len(dims) in (1, 2):
        pixel = strides[-1]
        lead = len(dims) - 1
    else:
        raise ValueError(f"{name} has shape {tuple(t.shape)}, which is not {h} x {w} pixels{f' of {channels}' if channels else ''}")
    if h * w <= 1:
        pixel = width
    if pixel < width:
        raise ValueError(f"{name} has a pixel stride of {pixel} floats, smaller than its width {width}")
    count = dims[0] if lead else 1
    image = strides[0] if lead and count > 1 else 0
    if n is not None and count != n:
        raise ValueError(f"{name} holds {count} images, expected {n}")
    if image < 0:
        raise ValueError(f"{name} has a negative image stride")
    return t, count, h, w, int(pixel), int(image)


def image_quality_workspace_bytes(n_images, height, width, channels, window_size=20, window_shift=10):
    need = int(_capi.lib().inerf_image_quality_workspace_bytes(int(n_images), int(height), int(width), int(channels), int(window_size),
                                                               int(window_shift)))
    _capi.check(min(need, 0), "inerf_image_quality_workspace_bytes")
    return need


def image_quality(pred, target, mask=None, shape=None, window_size=20, window_shift=10, workspace=None):
    """One ``inerf_image_quality`` call: ``(sums [N, 7] float64, counts [N, 3] int64)`` on the device for N pairs of fp32 images
    (``_capi.IMQ_SUM_NAMES`` / ``IMQ_COUNT_NAMES``; finished on the host by ``evaluation.finish_image_quality``).  ``pred`` and
    ``target``: [H, W, C] or [N, H, W, C], C = 1 or 3; with ``shape=(H, W)`` also [H * W, C] or [N, H * W, C] - e.g. columns of a
    frame's pack.  ``mask`` (optional): the same without the channel axis; a pixel is valid iff its mask value > 0."""
    if not isinstance(pred, torch.Tensor) or pred.dim() < 2 or pred.shape[-1] not in (1, 3):
        raise ValueError("pred must be a tensor whose last axis holds 1 or 3 channels")
    c = int(pred.shape[-1])
    pred, n, h, w, pp, pi = _imq_view(pred, "pred", shape, c)
    target, _, _, _, tp, ti = _imq_view(target, "target", (h, w), c, n)
    named = [("pred", pred), ("target", target)]
    a = _capi.ImqArgs()
    a.n_images, a.height, a.width, a.channels = n, h, w, c
    a.pred, a.pred_pixel_stride, a.pred_image_stride = pred.data_ptr(), pp, pi
    a.trgt, a.trgt_pixel_stride, a.trgt_image_stride = target.data_ptr(), tp, ti
    a.mask_pixel_stride = 1
    if mask is not None:
        mask, _, _, _, mp, mi = _imq_view(mask, "mask", (h, w), None, n)
        named.append(("mask", mask))
        a.mask, a.mask_pixel_stride, a.mask_image_stride = mask.data_ptr(), mp, mi
    if workspace is not None:
        if not (isinstance(workspace, torch.Tensor) and workspace.dtype == torch.float64 and workspace.is_contiguous()):
            raise ValueError("workspace must be a contiguous float64 tensor")
        named.append(("workspace", workspace))
    device = _eval_devices(named)
    a.window_size, a.window_shift = int(window_size), int(window_shift)
    from .evaluation import ssim_taps
    a.taps = (C.c_double * 11)(*ssim_taps())
    a.c1, a.c2 = 1e-4, 9e-4
    need = image_quality_workspace_bytes(n, h, w, c, window_size, window_shift)
    if workspace is None:
        workspace = torch.empty(max(need // 8, 1), dtype=torch.float64, device=device)
    sums = torch.empty(n, _capi.IMQ_SUMS, dtype=torch.float64, device=device)
    counts = torch.empty(n, _capi.IMQ_COUNTS, dtype=torch.int64, device=device)
    if n == 0 or h * w == 0:
        sums.zero_()
        counts.zero_()
    a.sums, a.counts = sums.data_ptr(), counts.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * 8
    with torch.cuda.device(device):
        rc = _capi.lib().inerf_image_quality(C.byref(a), _stream(sums))
    _capi.check(rc, "inerf_image_quality")
    return sums, counts


# ---------------------------------------------------------------------------------------------------------------------
# frame images (csrc/frame_vis.hip): the 8- and 16-bit planes of one packed frame in one launch.  A product is
# ``(kind, column, width, a, b, range)``: kind one of _capi.FRAME_*, ``range`` None or a device float32[2] tensor (JET: the
# (lo, hi) the kernel reads instead of (a, b) - ``frame_range`` writes one)
# ---------------------------------------------------------------------------------------------------------------------
def frame_products_plan(n, products, n_colours=0):
    """Host only (``inerf_frame_products_layout``; no device is touched): ``(args, planes, total)`` - an inerf_frame_products_args
    with ``n``, the products and their offsets filled in, ``planes`` = [(offset, bytes)] per product (every offset a multiple of 16)
    and the byte count the output needs."""
    products = list(products)
    if len(products) > _capi.FRAME_MAX_PRODUCTS:
        raise ValueError(f"{len(products)} products: one launch takes at most {_capi.FRAME_MAX_PRODUCTS}")
    a = _capi.FrameProductsArgs()
    a.n, a.n_products, a.n_colours = int(n), len(products), int(n_colours)
    held = []
    for k, (kind, column, width, pa, pb, rng) in enumerate(products):
        p = a.products[k]
        p.kind, p.column, p.width, p.a, p.b = int(kind), int(column), int(width), float(pa), float(pb)
        if rng is not None:
            if not (isinstance(rng, torch.Tensor) and rng.dtype == torch.float32 and rng.numel() == 2 and rng.is_contiguous()):
                raise ValueError(f"product {k}: range must be a contiguous float32 tensor of 2 values (lo, hi)")
            p.range = rng.data_ptr()
            held.append(rng)
    total = int(_capi.lib().inerf_frame_products_layout(C.byref(a)))
    if total < 0:
        _capi.check(total, "inerf_frame_products_layout")
    a.held = held                                          # the range tensors stay referenced as long as the args do
    planes = []
    for k in range(len(products)):
        p = a.products[k]
        bpp = p.width if p.kind == _capi.FRAME_TO8B else _capi.FRAME_BYTES_PER_PIXEL[p.kind]
        planes.append((int(p.offset), int(n) * bpp))
    return a, planes, total


def frame_products(frame, products, palette=None, out=None, plan=None):
    """All image planes of one packed frame in one launch of ``inerf_frame_products``.  ``frame``: [n, stride] fp32 on the device -
    a view is taken as it is (unit stride along a row, any row stride); ``palette``: uint8 [C, 3] on the device, for PALETTE
    products; ``out``: a contiguous uint8 tensor of at least the plan's total (allocated when not given); ``plan``: what
    ``frame_products_plan(n, products, C)`` returned, to skip planning per frame.  Returns ``(out, planes)``, ``planes`` =
    [(offset, bytes)] per product."""
    if not (isinstance(frame, torch.Tensor) and frame.dim() == 2):
        raise ValueError("frame must be a [n, stride] tensor" if isinstance(frame, torch.Tensor) else "frame must be a torch.Tensor")
    if frame.dtype != torch.float32:
        raise ValueError(f"frame must be float32, got {frame.dtype}")
    n = int(frame.shape[0])
    if n > 0 and frame.shape[1] > 0 and frame.stride(1) != 1:
        raise ValueError(f"frame must have unit stride along its rows, got stride {frame.stride(1)}")
    if n > 1 and frame.stride(0) < frame.shape[1]:
        raise ValueError(f"frame has a row stride of {frame.stride(0)} floats, smaller than its width {frame.shape[1]}")
    stride = int(frame.stride(0)) if n > 1 else max(int(frame.shape[1]), 1)
    named = [("frame", frame)]
    n_colours = 0
    if palette is not None:
        if not (isinstance(palette, torch.Tensor) and palette.dtype == torch.uint8 and palette.dim() == 2 and palette.shape[1] == 3
                and palette.is_contiguous()):
            raise ValueError("palette must be a contiguous uint8 [C, 3] tensor")
        n_colours = int(palette.shape[0])
        named.append(("palette", palette))
    a, planes, total = plan if plan is not None else frame_products_plan(n, products, n_colours)
    if a.n != n or a.n_colours != n_colours:
        raise ValueError(f"the plan was made for {a.n} pixels and {a.n_colours} colours, the frame holds {n} and the palette {n_colours}")
    for k in range(a.n_products):
        p = a.products[k]
        if p.column < 0 or p.column + p.width > frame.shape[1]:
            raise ValueError(f"product {k} reads columns {p.column} .. {p.column + p.width - 1} of a frame with {frame.shape[1]}")
        if p.kind == _capi.FRAME_PALETTE and palette is None:
            raise ValueError(f"product {k} is a palette gather: pass palette")
    named += [(f"range of product {k}", t) for k, t in enumerate(a.held)]
    if out is None:
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=frame.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= total):
        raise ValueError(f"out must be a contiguous uint8 tensor of at least {total} bytes")
    named.append(("out", out))
    device = _eval_devices(named)
    a.frame, a.stride = frame.data_ptr(), stride
    a.palette = palette.data_ptr() if palette is not None else None
    a.out, a.out_bytes = out.data_ptr(), out.numel()
    with torch.cuda.device(device):
        rc = _capi.lib().inerf_frame_products(C.byref(a), _stream(frame))
    _capi.check(rc, "inerf_frame_products")
    return out, planes


def frame_range_workspace_bytes(n):
    return int(_capi.lib().inerf_frame_range_workspace_bytes(int(n)))


def frame_range(values, minmax=None, accumulate=False, workspace=None):
    """``(nanmin, nanmax)`` of ``values`` ([n] fp32 on the device, any element stride: a column of a pack) into ``minmax`` (float32
    [2] on the device, allocated when not given) - two launches of ``inerf_frame_range``, no host synchronisation.  ``accumulate``:
    the pair ``minmax`` holds takes part (the range over several frames).  ``workspace``: a contiguous float32 tensor of at least
    ``frame_range_workspace_bytes(n)`` bytes (allocated when not given).  Returns ``minmax``."""
    values, stride = _eval_view(values, "values", 1)
    n = int(values.shape[0])
    named = [("values", values)]
    if minmax is None:
        if accumulate:
            raise ValueError("accumulate needs the minmax to accumulate into")
        minmax = torch.full((2,), float("nan"), dtype=torch.float32, device=values.device)
    elif not (isinstance(minmax, torch.Tensor) and minmax.dtype == torch.float32 and minmax.numel() == 2 and minmax.is_contiguous()):
        raise ValueError("minmax must be a contiguous float32 tensor of 2 values")
    named.append(("minmax", minmax))
    need = frame_range_workspace_bytes(n)
    if workspace is None:
        workspace = torch.empty(max(need // 4, 1), dtype=torch.float32, device=values.device)
    elif not (isinstance(workspace, torch.Tensor) and workspace.dtype == torch.float32 and workspace.is_contiguous()):
        raise ValueError("workspace must be a contiguous float32 tensor")
    named.append(("workspace", workspace))
    device = _eval_devices(named)
    with torch.cuda.device(device):
        rc = _capi.lib().inerf_frame_range(_ptr(values), stride, n, _ptr(minmax), _ptr(workspace), workspace.numel() * 4,
                                           int(bool(accumulate)), _stream(values))
    _capi.check(rc, "inerf_frame_range")
    return minmax


def jet_table():
    """JET[256, 3] uint8 (numpy) - the colour table of the JET products, from the library (csrc/jet_table.h)."""
    import numpy as np
    return np.frombuffer(bytes(_capi.lib().inerf_jet_table().contents), dtype=np.uint8).reshape(256, 3).copy()


# ---------------------------------------------------------------------------------------------------------------------
# PNG files on the device (csrc/png.hip): up to 16 planes - what ``frame_products`` wrote - become 16 complete PNG files in three
# launches.  An image is ``(height, width, channels, bit_depth, src_offset[, filter])``: channels 1 | 3, bit_depth 8 | 16 (16 only
# grey, little-endian in the plane), ``src_offset`` the plane's byte offset in ``src`` (a product's offset), ``filter``
# _capi.PNG_FILTER_ADAPTIVE (default) or 0 .. 4
# ---------------------------------------------------------------------------------------------------------------------
def png_plan(images):
    """Host only (``inerf_png_layout`` / ``inerf_png_workspace_bytes``; no device is touched): ``(args, files, total, workspace)`` -
    an inerf_png_args with the images and their offsets filled in, ``files`` = [(offset, capacity)] per image (every offset a multiple
    of 16; capacity: the worst-case file length), the byte count the output needs and the workspace's."""
    images = list(images)
    if len(images) > _capi.PNG_MAX_IMAGES:
        raise ValueError(f"{len(images)} images: one call takes at most {_capi.PNG_MAX_IMAGES}")
    a = _capi.PngArgs()
    a.n_images = len(images)
    for k, spec in enumerate(images):
        im = a.images[k]
        im.height, im.width, im.channels, im.bit_depth, im.src_offset = (int(v) for v in spec[:5])
        im.filter = int(spec[5]) if len(spec) > 5 else _capi.PNG_FILTER_ADAPTIVE
    total = int(_capi.lib().inerf_png_layout(C.byref(a)))
    if total < 0:
        _capi.check(total, "inerf_png_layout")
    workspace = int(_capi.lib().inerf_png_workspace_bytes(C.byref(a)))
    if workspace < 0:
        _capi.check(workspace, "inerf_png_workspace_bytes")
    files = [(int(a.images[k].dst_offset), int(a.images[k].dst_capacity)) for k in range(len(images))]
    return a, files, total, workspace


def png_encode(src, plan, out=None, sizes=None, workspace=None):
    """The planes in ``src`` (a contiguous uint8 tensor on the device: ``frame_products``' output) as PNG files, in the three launches
    of ``inerf_png_encode``.  ``plan``: what ``png_plan(images)`` returned; ``out``: a contiguous uint8 tensor of at least the plan's
    total, ``sizes``: int64 [n_images], ``workspace``: a contiguous uint8 tensor of at least the plan's workspace (each allocated when
    not given).  Returns ``(out, sizes)``: file k is ``out[offset_k : offset_k + sizes[k]]`` with ``offset_k`` = ``plan[1][k][0]``;
    ``sizes`` lives on the device - nothing waits for it here."""
    a, files, total, need = plan
    if not (isinstance(src, torch.Tensor) and src.dtype == torch.uint8 and src.dim() == 1 and src.is_contiguous()):
        raise ValueError("src must be a contiguous 1-d uint8 tensor")
    named = [("src", src)]
    if out is None:
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=src.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= total):
        raise ValueError(f"out must be a contiguous uint8 tensor of at least {total} bytes")
    named.append(("out", out))
    if sizes is None:
        sizes = torch.zeros(max(a.n_images, 1), dtype=torch.int64, device=src.device)
    elif not (isinstance(sizes, torch.Tensor) and sizes.dtype == torch.int64 and sizes.is_contiguous() and sizes.numel() >= a.n_images):
        raise ValueError(f"sizes must be a contiguous int64 tensor of at least {a.n_images} values")
    named.append(("sizes", sizes))
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=src.device)
    elif not (isinstance(workspace, torch.Tensor) and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise ValueError("workspace must be a contiguous uint8 tensor")
    named.append(("workspace", workspace))
    device = _eval_devices(named)
    a.src, a.src_bytes = src.data_ptr(), src.numel()
    a.dst, a.dst_bytes = out.data_ptr(), out.numel()
    a.sizes = sizes.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    with torch.cuda.device(device):
        rc = _capi.lib().inerf_png_encode(C.byref(a), _stream(src))
    _capi.check(rc, "inerf_png_encode")
    return out, sizes


# ---------------------------------------------------------------------------------------------------------------------
# Frame movies on the device (csrc/jpeg.hip): up to 16 planes - what ``frame_products`` wrote - become 16 baseline JPEG files, each
# appended as an AVI chunk to a device-resident stream.  An image is ``(height, width, channels, quality, src_offset)``: channels
# 1 (grey) | 3 (RGB), quality 1 .. 100
# ---------------------------------------------------------------------------------------------------------------------
def jpeg_tables(quality):
    """Host only (``inerf_jpeg_tables``): ``(luma, chroma)``, uint8 numpy [64] in natural order, of libjpeg's quality rule."""
    import numpy as np
    luma, chroma = (C.c_ubyte * 64)(), (C.c_ubyte * 64)()
    _capi.check(_capi.lib().inerf_jpeg_tables(int(quality), luma, chroma), "inerf_jpeg_tables")
    return np.frombuffer(bytes(luma), np.uint8), np.frombuffer(bytes(chroma), np.uint8)


def jpeg_header(height, width, channels, quality):
    """Host only (``inerf_jpeg_header``): the bytes in front of every frame's entropy-coded data, SOI to SOS."""
    buf = (C.c_ubyte * 1024)()
    n = int(_capi.lib().inerf_jpeg_header(int(height), int(width), int(channels), int(quality), buf, 1024))
    if n < 0:
        _capi.check(n, "inerf_jpeg_header")
    return bytes(buf[:n])


def jpeg_frame_bound(height, width, channels):
    """Host only (``inerf_jpeg_frame_bound``): the worst-case length of one frame's chunk."""
    n = int(_capi.lib().inerf_jpeg_frame_bound(int(height), int(width), int(channels)))
    if n < 0:
        _capi.check(n, "inerf_jpeg_frame_bound")
    return n


class JpegStream:
    """The device side of one movie: the header every frame starts with, the arena its chunks are appended to, the cursor (bytes
    used, frames written), the index (chunk offset and file length per frame) and the status word.  ``tail`` bytes behind the
    arena's capacity and entries behind the index are allocated but never named to the encoder (tests put sentinels there)."""

    def __init__(self, height, width, channels, quality, capacity, frames, device, tail=0):
        import numpy as np
        self.shape = (int(height), int(width), int(channels))
        self.quality, self.capacity, self.frames = int(quality), int(capacity), int(frames)
        host = jpeg_header(height, width, channels, quality)
        self.header_bytes = len(host)
        self.header = torch.from_numpy(np.frombuffer(host, np.uint8).copy()).to(device)
        self.arena = torch.zeros(self.capacity + int(tail), dtype=torch.uint8, device=device)
        self.state = torch.zeros(3 + 2 * (self.frames + int(tail)), dtype=torch.int64, device=device)      # cursor, status, index
        self.cursor, self.status, self.index = self.state[:2], self.state[2:3], self.state[3:].view(-1, 2)


def jpeg_plan(images):
    """Host only (``inerf_jpeg_workspace_bytes``; no device is touched): ``(args, workspace)`` - an inerf_jpeg_args with the images
    filled in and the workspace's byte count."""
    images = list(images)
    if len(images) > _capi.JPEG_MAX_IMAGES:
        raise ValueError(f"{len(images)} images: one call takes at most {_capi.JPEG_MAX_IMAGES}")
    a = _capi.JpegArgs()
    a.n_images = len(images)
    for k, spec in enumerate(images):
        im = a.images[k]
        im.height, im.width, im.channels, im.quality, im.src_offset = (int(v) for v in spec[:5])
    workspace = int(_capi.lib().inerf_jpeg_workspace_bytes(C.byref(a)))
    if workspace < 0:
        _capi.check(workspace, "inerf_jpeg_workspace_bytes")
    return a, workspace


def jpeg_encode(src, plan, streams, workspace=None):
    """The planes in ``src`` (a contiguous uint8 tensor on the device) as JPEG files appended to ``streams`` (one ``JpegStream`` per
    image of ``plan``; several images may name one stream and land in order), in the three launches of ``inerf_jpeg_encode``.
    Nothing waits; the cursors, indices and status words live on the device.  Returns the workspace."""
    a, need = plan
    if not (isinstance(src, torch.Tensor) and src.dtype == torch.uint8 and src.dim() == 1 and src.is_contiguous()):
        raise ValueError("src must be a contiguous 1-d uint8 tensor")
    streams = list(streams)
    if len(streams) != a.n_images:
        raise ValueError(f"{len(streams)} streams for {a.n_images} images")
    named = [("src", src)]
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=src.device)
    elif not (isinstance(workspace, torch.Tensor) and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise ValueError("workspace must be a contiguous uint8 tensor")
    named.append(("workspace", workspace))
    for k, s in enumerate(streams):
        im = a.images[k]
        if (im.height, im.width, im.channels) != s.shape or im.quality != s.quality:
            raise ValueError(f"image {k} is {(im.height, im.width, im.channels)} at quality {im.quality}, its stream was made for "
                             f"{s.shape} at {s.quality}")
        named += [(f"streams[{k}].arena", s.arena), (f"streams[{k}].state", s.state), (f"streams[{k}].header", s.header)]
        im.header, im.header_bytes = s.header.data_ptr(), s.header_bytes
        im.arena, im.arena_bytes = s.arena.data_ptr(), s.capacity
        im.cursor, im.status, im.index, im.index_frames = s.cursor.data_ptr(), s.status.data_ptr(), s.index.data_ptr(), s.frames
    device = _eval_devices(named)
    a.src, a.src_bytes = src.data_ptr(), src.numel()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    with torch.cuda.device(device):
        rc = _capi.lib().inerf_jpeg_encode(C.byref(a), _stream(src))
    _capi.check(rc, "inerf_jpeg_encode")
    return workspace
