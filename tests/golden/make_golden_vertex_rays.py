"""Writes tests/golden/vertex_rays.npz: the [n, 11] ray batch of mesh extraction's vertex-colour pass (one ray per mesh vertex, cast
against its normal), evaluated by torch on the CPU.  Not needed at test time: the tests read the .npz.

    python tests/golden/make_golden_vertex_rays.py

Inputs (100 rows, kept as float64 and as their float32 roundings): unit normals, unnormalised normals, normals with a zero component
and with -0.0, tiny (1e-20) and large (1e18) normals; the all-zero normal is left out (0 / 0).  Expected, per near_t in (2.0, 0.0, 0.3)
and per input dtype, with near = 0.1 and far = 10.0:
    d = -float32(normals);  o = float32(vertices) - d * near * near_t  (near a float32 column of 0.1, near_t a Python float)
    viewdirs = d / norm(d, dim=-1, keepdim=True);  rays = cat([o, d, near, far, viewdirs], -1)
"""
import os

import numpy as np
import torch

NEAR, FAR, NEAR_TS = 0.1, 10.0, (2.0, 0.0, 0.3)


def inputs():
    rng = np.random.default_rng(20261020)
    unit = rng.standard_normal((30, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    free = rng.standard_normal((30, 3)) * rng.uniform(0.05, 40.0, (30, 1))
    zero = rng.standard_normal((12, 3))
    for r in range(12):                                   # one or two zero components, never three
        zero[r, r % 3] = 0.0
        if r >= 6:
            zero[r, (r + 1) % 3] = 0.0
    negzero = rng.standard_normal((8, 3))
    for r in range(8):
        negzero[r, r % 3] = -0.0
    negzero[6] = [-0.0, -0.0, 1.0]
    negzero[7] = [0.0, -2.5, -0.0]
    tiny = rng.standard_normal((10, 3)) * 1e-20
    large = rng.standard_normal((10, 3)) * 1e18
    normals = np.concatenate([unit, free, zero, negzero, tiny, large], 0)
    vertices = rng.uniform(-3.0, 3.0, normals.shape)
    vertices[:4] = [[0.0, 0.0, 0.0], [-0.0, 1.0, -1.0], [1e-30, -1e-30, 2.0], [123.456, -789.0, 0.001]]
    assert normals.shape == (100, 3) and (np.abs(normals).sum(1) > 0).all()
    return vertices, normals


def expected(vertices, normals, near_t):
    rays_d = -torch.FloatTensor(normals)
    near = NEAR * torch.ones_like(rays_d[:, :1])
    far = FAR * torch.ones_like(rays_d[:, :1])
    rays_o = torch.FloatTensor(vertices) - rays_d * near * near_t
    viewdirs = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
    return torch.cat([rays_o, rays_d, near, far, viewdirs], -1).numpy()


if __name__ == "__main__":
    torch.set_num_threads(1)
    v64, n64 = inputs()
    v32, n32 = v64.astype(np.float32), n64.astype(np.float32)
    out = {"vertices_f64": v64, "normals_f64": n64, "vertices_f32": v32, "normals_f32": n32,
           "near": np.float32(NEAR), "far": np.float32(FAR), "near_t": np.asarray(NEAR_TS, np.float64)}
    for i, near_t in enumerate(NEAR_TS):
        out[f"rays_f64_{i}"] = expected(v64, n64, near_t)
        out[f"rays_f32_{i}"] = expected(v32, n32, near_t)
        assert np.isfinite(out[f"rays_f64_{i}"]).all() and np.isfinite(out[f"rays_f32_{i}"]).all()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vertex_rays.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
