#!/usr/bin/env python3
"""Ray batches of the object-level front-end: the torch expressions render() used for NDC frames and for given rays (restated below:
get_rays kernel -> norm / divide -> ndc_rays' ~20 small launches -> ones_like -> cat) against the one launch of csrc/frame_ops.hip
(inerf_gen_rays_ndc / inerf_assemble_rays) - on the same GPU, in the same process, in alternating rounds.

    python scripts/bench_ray_forms.py [--rounds 20] [--iters 200] [--out profiles/ray_forms_bench.txt]
Legs: pose -> NDC batch at 378 x 504 (fern at factor 8) and 756 x 1008; given rays at N = 2 048 and 4 096 with and without NDC; a
whole 378 x 504 LLFF frame (64 + 64 samples, default-init networks, render(c2w=..., ndc=True)); an object-level training step fed by
(o, d) (N_rand = 1 024, LLFF config: NDC, perturb, raw noise; forward, loss, backward, Adam).  Prints the median of the rounds and
their range per leg, whether the two ways give the same bits, and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time
import types
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402

__graft_entry__.build()
from intrinsicnerf_amd import kernels, object_level as ol, optim  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--iters", type=int, default=200, help="calls per round of the batch-only legs")
ap.add_argument("--out", default=None, help="also write the report to this file")
a = ap.parse_args()
if a.rounds < 20:
    raise SystemExit("bench_ray_forms.py reports the median of at least 20 rounds")
if not torch.cuda.is_available():
    raise SystemExit("bench_ray_forms.py measures on the GPU: no HIP device visible")
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def torch_ndc_rays(H, W, focal, near, rays_o, rays_d):
    """ndc_rays as torch expressions on whatever device the rays live on (run_nerf_helpers.py:381-399)."""
    t = -(near + rays_o[..., 2]) / rays_d[..., 2]
    rays_o = rays_o + t[..., None] * rays_d
    sx, sy = -1. / (W / (2. * focal)), -1. / (H / (2. * focal))
    o = torch.stack([sx * rays_o[..., 0] / rays_o[..., 2], sy * rays_o[..., 1] / rays_o[..., 2], 1. + 2. * near / rays_o[..., 2]], -1)
    d = torch.stack([sx * (rays_d[..., 0] / rays_d[..., 2] - rays_o[..., 0] / rays_o[..., 2]),
                     sy * (rays_d[..., 1] / rays_d[..., 2] - rays_o[..., 1] / rays_o[..., 2]), -2. * near / rays_o[..., 2]], -1)
    return o, d


def torch_batch(H, W, K, rays_o, rays_d, near, far, ndc):
    """render()'s batch assembly as torch expressions (run_nerf.py:106-128, use_viewdirs, no static camera)."""
    viewdirs = rays_d
    viewdirs = viewdirs / torch.norm(viewdirs, dim=-1, keepdim=True)
    viewdirs = torch.reshape(viewdirs, [-1, 3]).float()
    if ndc:
        rays_o, rays_d = torch_ndc_rays(H, W, K[0][0], 1., rays_o, rays_d)
    rays_o = torch.reshape(rays_o, [-1, 3]).float()
    rays_d = torch.reshape(rays_d, [-1, 3]).float()
    near, far = near * torch.ones_like(rays_d[..., :1]), far * torch.ones_like(rays_d[..., :1])
    return torch.cat([rays_o, rays_d, near, far, viewdirs], -1)


def torch_pose_batch(H, W, K, c2w, near, far, ndc):
    rays = kernels.gen_rays(c2w, H, W, K[0][0], K[1][1], K[0][2], K[1][2], 0., 1., True).reshape(H, W, -1)     # get_rays on a device pose
    return torch_batch(H, W, K, rays[..., 0:3], rays[..., 3:6], near, far, ndc)


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def compare(name, runners, iters, same=None, warm=10):
    """Alternating rounds of every runner; median and range in milliseconds per call."""
    for fn in runners.values():
        for _ in range(warm):
            fn()
    times = {k: [] for k in runners}
    for _ in range(a.rounds):
        for k, fn in runners.items():
            times[k].append(timed(fn, iters))
    res = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}
    for k, v in res.items():
        say(f"{name:38s} {k:18s} {v['median_ms'] * 1e3:10.1f} us per call (rounds {v['min_ms'] * 1e3:.1f} .. {v['max_ms'] * 1e3:.1f})")
    if same is not None:
        say(f"{name:38s} {'same bits':18s} {same}")
        res["same_bits"] = same
    return res


def llff_camera(H, W):
    """A forward-facing camera like fern's: focal 407.57 at 378 x 504, looking down -z from a little off the origin."""
    focal = 407.5653 * W / 504.0
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    c2w = torch.tensor([[0.998, 0.017, -0.061, 0.31], [-0.019, 0.999, -0.033, -0.12], [0.060, 0.034, 0.998, 0.08]])
    return K, c2w.to(dev)


def llff_args():
    return types.SimpleNamespace(multires=10, multires_views=4, i_embed=0, use_viewdirs=True, N_importance=64, N_samples=64, netdepth=8,
                                 netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=1024 * 64, perturb=1., white_bkgd=False,
                                 raw_noise_std=1e0, lindisp=False, dataset_type="llff", no_ndc=False)


result = {}
say(f"device: {torch.cuda.get_device_name(0)}; {a.rounds} alternating rounds per leg; batch-only legs {a.iters} calls per round")

# ---- pose -> NDC batch
for H, W in ((378, 504), (756, 1008)):
    K, c2w = llff_camera(H, W)
    coeff = ol._ndc_coefficients(H, W, K[0][0], 1.)
    old = lambda: torch_pose_batch(H, W, K, c2w, 0., 1., True)
    new = lambda: kernels.gen_rays(c2w, H, W, K[0][0], K[1][1], K[0][2], K[1][2], 0., 1., True, ndc=coeff)
    same = bool(torch.equal(old(), new()))
    result[f"pose_ndc_{H}x{W}"] = compare(f"pose -> NDC batch {H}x{W}", {"torch expressions": old, "hip, one launch": new}, a.iters, same)

# ---- given rays
for n in (2048, 4096):
    K, c2w = llff_camera(378, 504)
    frame = kernels.gen_rays(c2w, 378, 504, K[0][0], K[1][1], K[0][2], K[1][2], 0., 1., True)
    sel = torch.randperm(frame.shape[0], generator=torch.Generator().manual_seed(n))[:n].to(dev)
    batch_rays = torch.stack([frame[sel, 0:3], frame[sel, 3:6]], 0)                      # what ObjectBatcher.next() returns: [2, n, 3]
    for ndc in (False, True):
        coeff = ol._ndc_coefficients(378, 504, K[0][0], 1.) if ndc else None
        old = lambda: torch_batch(378, 504, K, batch_rays[0], batch_rays[1], 0., 1., ndc)
        new = lambda: kernels.assemble_rays(batch_rays[0], batch_rays[1], 0., 1., ndc=coeff)
        same = bool(torch.equal(old(), new()))
        tag = "NDC" if ndc else "no NDC"
        result[f"given_{n}_{'ndc' if ndc else 'plain'}"] = compare(f"given rays N={n}, {tag}", {"torch expressions": old, "hip, one launch": new},
                                                                  a.iters, same)

# ---- a whole LLFF frame and a training step, default-init networks
torch.manual_seed(0)
train_kw, test_kw, grad_vars = ol.create_nerf(llff_args(), device=dev)
H, W = 378, 504
K, c2w = llff_camera(H, W)
chunk = 1024 * 32
maps = ("rgb_map", "disp_map", "acc_map", "albedo_map", "shading_map", "residual_map")
frame_kw = {k: v for k, v in test_kw.items() if k != "use_viewdirs"}


def frame_old():
    with torch.no_grad():
        return ol.batchify_rays(torch_pose_batch(H, W, K, c2w, 0., 1., True), chunk, **frame_kw)["rgb_map"]


def frame_new():
    with torch.no_grad():
        return ol.render(H, W, K, chunk=chunk, c2w=c2w, ndc=True, near=0., far=1., **test_kw)[0].reshape(-1, 3)


result["llff_frame_378x504"] = compare("LLFF frame 378x504, 64+64", {"torch expressions": frame_old, "hip, one launch": frame_new}, 2, warm=2)

frame = kernels.gen_rays(c2w, H, W, K[0][0], K[1][1], K[0][2], K[1][2], 0., 1., True)
sel = torch.randperm(frame.shape[0], generator=torch.Generator().manual_seed(1))[:1024].to(dev)
batch_rays = torch.stack([frame[sel, 0:3], frame[sel, 3:6]], 0)
target = torch.rand(1024, 3, generator=torch.Generator().manual_seed(2)).to(dev)
optimizer = optim.Adam(grad_vars, lr=5e-4, betas=(0.9, 0.999))
step_kw = {k: v for k, v in train_kw.items() if k != "use_viewdirs"}


def step(way):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if way == "old":
            ret = ol.batchify_rays(torch_batch(H, W, K, batch_rays[0], batch_rays[1], 0., 1., True), chunk, retraw=True, **step_kw)
            rgb, rgb0 = ret["rgb_map"], ret["rgb0"]
        else:
            out = ol.render(H, W, K, chunk=chunk, rays=batch_rays, verbose=False, retraw=True, near=0., far=1., **train_kw)
            rgb, rgb0 = out[0], out[6]["rgb0"]
    optimizer.zero_grad()
    loss = ((rgb - target) ** 2).mean() + ((rgb0 - target) ** 2).mean()          # run_nerf.py:976, 1006
    loss.backward()
    optimizer.step()


result["train_step_1024"] = compare("training step N_rand=1024, LLFF", {"torch expressions": lambda: step("old"), "hip, one launch": lambda: step("new")},
                                    5, warm=3)
say(json.dumps(result))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
