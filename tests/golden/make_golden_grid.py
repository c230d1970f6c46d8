#!/usr/bin/env python3
"""Golden vectors of mesh extraction's grid query, produced by the real reference on the CPU (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grid.py

``grid_query.npz`` holds, for oriented random boxes with non-cubic extents:

  points_d2 / _d5 / _d16 / _d13   what SSR/geometry/occupancy.py's grid_within_bound returns (its file is loaded by path), with the
                                  box (extents_*, transform_*) it was called on; occ_range is [-1, 1] throughout
  ssr/* and object/* (dim 13)     a Semantic_NeRF (5 classes, the trainer's scalar_factor = 10) and an object-level NeRF, weights from a
                                  seed (oracle.make_state_dict) with the density head rescaled so that sigma straddles zero on the lattice
                                  (alpha_weight / alpha_bias stored); the reference's run_network in 1 024-point chunks with zero view
                                  directions as extract_colour_mesh.py:156-164 calls it, raw[..., 3] and occupancy_activation (:172-179):
                                  sigma32 / occ32, and the same modules and expressions in fp64: sigma64 / occ64; dist = the voxel size

Before it writes, the script asserts per network that between 10 % and 90 % of the points have sigma > 0, that everything is finite
and that the reference's fp32 values lie within a QUARTER of the tests' tolerance (rtol 1e-4, atol 1e-5) of the fp64 ones; it tries
the next seed otherwise.  The calibrated density has std 1/8 over the lattice: at std 1 the reference's own fp32 error reaches
the whole tolerance where sigma crosses zero.  The fixture's entry for the table of this directory's README.md, with this
calibration, is grid_query.md.  Only inputs and the reference's outputs are stored, nothing of its text.
"""
import copy
import importlib.util
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402
import oracle  # noqa: E402

RTOL, ATOL = 1e-4, 1e-5
OCC_RANGE = [-1.0, 1.0]
SIGMA_STD = 0.125          # of the calibrated density over the lattice (see network_case)


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def random_box(rng, centre_scale, size):
    """an oriented box: a random rotation (QR of a Gaussian matrix, determinant +1), a centre, non-cubic extents - float64, as
    trimesh.bounds.oriented_bounds hands them over"""
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4)
    T[:3, :3] = q
    T[:3, 3] = rng.uniform(-1.0, 1.0, 3) * centre_scale
    extents = size * np.array([1.0, 0.61, 1.37]) * rng.uniform(0.8, 1.2, 3)
    return T, extents


def activation(alpha, distances):
    return 1.0 - torch.exp(-torch.relu(alpha) * distances)          # extract_colour_mesh.py:172-175


def network_case(tag, variant, make_net, run_network, embed, embed_d, pts, dist, n_classes, first_seed):
    """(seed, arrays) of the first seed that passes the three assertions"""
    pts32 = pts.reshape(-1, 1, 3)
    for seed in range(first_seed, first_seed + 20):
        sd = oracle.make_state_dict(variant, n_classes, seed=seed)
        net = make_net()
        net.load_state_dict(sd)
        net64 = copy.deepcopy(net).double()
        with torch.no_grad():
            def query(n, p):
                return torch.cat([run_network(p[i:i + 1024], torch.zeros_like(p[i:i + 1024]).squeeze(1), n, embed, embed_d, 2048 * 128)
                                  for i in range(0, p.shape[0], 1024)], 0)[..., 3].reshape(-1)

            # density head: sigma = g (s - q), g a power of two, the bias a multiple of 2^-10 (as oracle/calibration.py does on rays).
            # A default-init network's density is almost constant in space (std(s) ~ 2^-7 against layer outputs of order 1), so the gain
            # multiplies the reference's own fp32 rounding error as well: at std(sigma) = 1 that error alone reaches the tests' whole
            # tolerance where sigma crosses zero (measured: 0.4 .. 1.0 of it over twenty seeds); std(sigma) = 1/8 leaves it near a tenth
            s = query(net64, pts32.double())
            q = float(torch.quantile(s, 0.6))
            g = 2.0 ** round(float(np.log2(SIGMA_STD / max(float(s.std()), 1e-12))))
            w = net.alpha_linear.weight.detach() * g
            b = torch.round((net.alpha_linear.bias.detach() - q) * g * 1024.0) / 1024.0
            for n in (net, net64):
                n.alpha_linear.weight.copy_(w)
                n.alpha_linear.bias.copy_(b)
            s32, s64 = query(net, pts32), query(net64, pts32.double())
            o32, o64 = activation(s32, dist), activation(s64, dist)
        positive = float((s64 > 0).double().mean())
        finite = bool(torch.isfinite(s32).all() and torch.isfinite(s64).all() and torch.isfinite(o32).all() and torch.isfinite(o64).all())
        dev_s = float(((s32.double() - s64).abs() / (ATOL + RTOL * s64.abs())).max())
        dev_o = float(((o32.double() - o64).abs() / (ATOL + RTOL * o64.abs())).max())
        print(f"{tag}: seed {seed}: gain 2^{int(np.log2(g))}, sigma in [{float(s64.min()):.3f}, {float(s64.max()):.3f}], {100 * positive:.1f} % positive, "
              f"fp32 against fp64: sigma {dev_s:.3f}, occ {dev_o:.3f} of the tolerance")
        if 0.1 <= positive <= 0.9 and finite and dev_s < 0.25 and dev_o < 0.25:
            return {f"{tag}/seed": seed, f"{tag}/alpha_weight": w, f"{tag}/alpha_bias": b, f"{tag}/sigma32": s32, f"{tag}/occ32": o32,
                    f"{tag}/sigma64": s64, f"{tag}/occ64": o64}
    raise AssertionError(f"{tag}: no seed gives a usable network")


def main():
    run_nerf, H_ref, SSRTrainer, ssr_rays, ssr_mu = mg.import_reference()
    from SSR.models import semantic_nerf as ssr_models
    occupancy = load_by_path("ref_occupancy", os.path.join(mg.REF, "SSR", "geometry", "occupancy.py"))
    rng = np.random.default_rng(20260)
    out = {"occ_range": np.array(OCC_RANGE)}

    for dim, centre, size in ((2, 3.0, 4.0), (5, 0.5, 2.5), (16, 2.0, 5.0)):
        T, extents = random_box(rng, centre, size)
        pts, scale = occupancy.grid_within_bound(OCC_RANGE, extents, T, grid_dim=dim)
        out.update({f"points_d{dim}": pts.reshape(-1, 3), f"transform_d{dim}": T, f"extents_d{dim}": extents, f"scale_d{dim}": scale})

    # dim 13: a room-sized box for the SSR network (positions / 10 inside the encoder), an object-sized one for the object-level network
    dim = 13
    near, far, n_importance = 0.1, 10.0, 128
    T, extents = random_box(rng, 1.5, 6.0)
    pts, scale = occupancy.grid_within_bound(OCC_RANGE, extents, T, grid_dim=dim)
    out.update({"points_d13": pts.reshape(-1, 3), "transform_d13": T, "extents_d13": extents, "scale_d13": scale,
                "ssr/dist": np.float64((far - near) / n_importance), "ssr/near": near, "ssr/far": far, "ssr/n_importance": n_importance,
                "ssr/n_classes": 5, "ssr/xyz_div": 10.0})
    embed, ch = ssr_models.get_embedder(10, 0, scalar_factor=10)
    embed_d, ch_d = ssr_models.get_embedder(4, 0, scalar_factor=1)
    out.update(network_case("ssr", "ssr", lambda: ssr_models.Semantic_NeRF(enable_semantic=True, num_semantic_classes=5, D=8, W=256,
                                                                             input_ch=ch, output_ch=5, skips=[4], input_ch_views=ch_d,
                                                                             use_viewdirs=True),
                            ssr_mu.run_network, embed, embed_d, pts, (far - near) / n_importance, 5, 100))

    T, extents = random_box(rng, 0.3, 2.2)
    pts, scale = occupancy.grid_within_bound(OCC_RANGE, extents, T, grid_dim=dim)
    out.update({"object/points": pts.reshape(-1, 3), "object/transform": T, "object/extents": extents, "object/scale": scale,
                "object/dist": np.float64((6.0 - 2.0) / 128)})
    embed, ch = H_ref.get_embedder(10, 0)
    embed_d, ch_d = H_ref.get_embedder(4, 0)
    out.update(network_case("object", "object", lambda: H_ref.NeRF(D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=ch_d,
                                                                    use_viewdirs=True),
                            run_nerf.run_network, embed, embed_d, pts, (6.0 - 2.0) / 128, 0, 200))
    mg.save("grid_query", **out)
    assert os.path.getsize(os.path.join(HERE, "grid_query.npz")) < (1 << 20)


if __name__ == "__main__":
    main()
