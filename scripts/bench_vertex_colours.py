"""Vertex colours of an extracted mesh: the reference-shaped loop against geometry.vertex_colours.

    python scripts/bench_vertex_colours.py [--vertices 65536] [--rounds 5] [--paths abc] [--out profiles/vertex_colours_bench.txt]

One SSR network pair as the 320x240 Replica configuration has it (C = 28, 64 + 128 samples, default initialisation with the density
heads' bias raised to 0.5 so that every sample carries density and no colour head is skipped - the dearest render there is), V
synthetic vertices on a sphere with outward normals, float64 as open3d hands them out.  Three paths on one GPU, on identical inputs:
  a  the reference's loop (SSR/extract_colour_mesh.py:27-41, 232-257): the [V, 11] batch built by torch on the host and uploaded,
     4 096 vertices per render_rays call with raw_coarse / raw_fine returned, `.cpu()` of EVERY returned key, torch.cat, to8b on the host
  b  the same loop with return_raw = False
  c  SSRRenderMixin.vertex_colours: rays, render and the 8-bit colours on the device, one copy of 3 V bytes at the end
The three results are compared byte for byte before anything is timed.  Then wall time, synchronised, the paths alternating round by
round after that first (warm-up) run; median round with min / max / spread, the bytes each path copies to the host and its peak device
memory above what the networks occupy.  `--paths bc` leaves the first path out (at 10^6 vertices it keeps ~80 GB of host memory).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from intrinsicnerf_amd import ssr                                                   # noqa: E402

NEAR, FAR, NEAR_T, REF_CHUNK = 0.1, 10.0, 2.0, 4096


def sphere(n):
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    normals = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
    return 0.4 * normals, normals


def reference_loop(trainer, vertices, normals, return_raw, copied):
    """extract_colour_mesh.py:232-257 with the colour branch; `copied[0]` receives the bytes the loop moves to the host"""
    rays_d = -torch.FloatTensor(normals)
    near = NEAR * torch.ones_like(rays_d[:, :1])
    far = FAR * torch.ones_like(rays_d[:, :1])
    rays_o = torch.FloatTensor(vertices) - rays_d * near * NEAR_T
    viewdirs = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
    rays = torch.cat([rays_o, rays_d, near, far, viewdirs], -1).cuda()
    trainer.return_raw = return_raw
    results, moved = {}, 0
    with torch.no_grad():
        for i in range(0, rays.shape[0], REF_CHUNK):
            for k, v in trainer.render_rays(rays[i:i + REF_CHUNK]).items():
                results.setdefault(k, []).append(v.cpu())
                moved += v.numel() * v.element_size()
    results = {k: torch.cat(v, 0) for k, v in results.items()}
    copied[0] = moved
    return (255 * np.clip(results["rgb_fine"].numpy(), 0, 1)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--paths", default="abc")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    trainer = ssr.SSRRenderer(28, N_samples=64, N_importance=128, perturb=0., raw_noise_std=0., device=dev)
    with torch.no_grad():
        for net in (trainer.ssr_net_coarse, trainer.ssr_net_fine):
            net.alpha_linear.bias.fill_(0.5)
    vertices, normals = sphere(args.vertices)
    copied = {k: [0] for k in "abc"}
    names = {"a": f"a  reference loop, {REF_CHUNK} per chunk, .cpu() of every key, return_raw=True",
             "b": f"b  reference loop, {REF_CHUNK} per chunk, .cpu() of every key, return_raw=False",
             "c": "c  vertex_colours (rays, render, 8-bit colours on the device; one copy)"}

    def path_c():
        out = trainer.vertex_colours(vertices, normals, near_t=NEAR_T)
        copied["c"][0] = out.nbytes
        return out

    sides = {"a": lambda: reference_loop(trainer, vertices, normals, True, copied["a"]),
             "b": lambda: reference_loop(trainer, vertices, normals, False, copied["b"]),
             "c": path_c}
    sides = {k: fn for k, fn in sides.items() if k in args.paths}

    # first run of every path: the results byte for byte, and the peak of device memory
    with torch.no_grad():                                                           # (packs the weights)
        trainer.render_rays(torch.tensor([[0., 0., 0., 0., 0., 1., NEAR, FAR, 0., 0., 1.]], device=dev).repeat(8, 1))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    first, peak = {}, {}
    for k, fn in sides.items():
        torch.cuda.reset_peak_memory_stats(dev)
        first[k] = fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated(dev) - base
    ref = first[min(first)]
    for k, v in first.items():
        assert v.dtype == np.uint8 and v.shape == (args.vertices, 3) and np.array_equal(v, ref), f"path {k} differs from path {min(first)}"
    assert np.unique(ref).size > 8, "the render is flat: nothing would be compared"

    times = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)

    lines = [f"# python scripts/bench_vertex_colours.py --vertices {args.vertices} --rounds {args.rounds} --paths {args.paths}   "
             f"({torch.cuda.get_device_name(dev)}; C = 28, 64 + 128 samples; wall time, synchronised; the paths alternate round by round "
             f"after a first run of each; median round, min, max, spread = (max - min) / median)",
             f"V = {args.vertices} vertices; the {len(sides)} paths give identical bytes: True ({np.unique(ref).size} distinct byte values)"]
    for k in sides:
        ts = times[k]
        med = statistics.median(ts)
        lines.append(f"  {names[k]:<84s} {med * 1e3:10.1f} ms (min {min(ts) * 1e3:.1f}, max {max(ts) * 1e3:.1f}; spread {(max(ts) - min(ts)) / med * 100:.1f} %)"
                     f";  {copied[k][0] / 1e6:12.3f} MB to the host;  peak device memory {peak[k] / 1e6:9.1f} MB")
    med = {k: statistics.median(v) for k, v in times.items()}
    if "c" in med:
        for k in med:
            if k != "c":
                lo, hi = min(times[k]) / max(times["c"]), max(times[k]) / min(times["c"])
                lines.append(f"  {k} / c = {med[k] / med['c']:.2f} (between {lo:.2f} and {hi:.2f} over the rounds)")
    lines.append(json.dumps({"vertices": args.vertices, "times_s": times, "bytes_to_host": {k: copied[k][0] for k in sides}, "peak_device_bytes": peak}))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
