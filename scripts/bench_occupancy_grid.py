#!/usr/bin/env python3
"""Occupancy grid of an SSR network (28 classes) for mesh extraction, three ways on the same lattice, same GPU, same process, in
alternating rounds:

  (a) geometry.occupancy_grid: one inerf_occupancy_grid launch (position encoding, trunk, density head; 4 bytes per point out)
  (b) one ssr.run_network call over every lattice point with zero view directions (the whole network, [N, 11] rays in, [N, 11 + C] raw
      out), channel 3, the activation in torch - the best path the package had before
  (c) the reference's call pattern on the same run_network (SSR/extract_colour_mesh.py:156-164): 1 024 points per call, `.cpu()` after
      every call, torch.cat on the host, then channel 3 and the activation

    python scripts/bench_occupancy_grid.py [--dims 128 256] [--rounds 7] [--out profiles/occupancy_grid_bench.txt]
Prints per grid size the median of the rounds and their range per way (host clock around work that ends in a device synchronise), the peak
device memory of (a) and (b) above what was allocated before the call, the trunk's matrix rate of (a), whether (a) has the bits of (b)'s
density, and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402

__graft_entry__.build()
from intrinsicnerf_amd import geometry, ssr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dims", type=int, nargs="+", default=[128, 256])
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--chunk-rounds", type=int, default=3, help="rounds of (c), whose 256^3 round is 16 384 calls and host copies")
ap.add_argument("--out", default=None, help="also write the report to this file")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_occupancy_grid.py measures on the GPU: no HIP device visible")
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


N_CLASSES, NEAR, FAR, N_IMPORTANCE = 28, 0.1, 10.0, 128
DIST = (FAR - NEAR) / N_IMPORTANCE
torch.manual_seed(0)
embed, ch = ssr.get_embedder(10, 0, scalar_factor=10)
embed_d, ch_d = ssr.get_embedder(4, 0, scalar_factor=1)
net = ssr.Semantic_NeRF(True, N_CLASSES, D=8, W=256, input_ch=ch, input_ch_views=ch_d, output_ch=5, skips=[4], use_viewdirs=True)
net = net.to(dev).requires_grad_(False)
# a room-sized oriented box (extents and box-to-scene transform as trimesh.bounds.oriented_bounds gives them)
rng = np.random.default_rng(3)
q, r = np.linalg.qr(rng.standard_normal((3, 3)))
T = np.eye(4)
T[:3, :3] = q * np.sign(np.diag(r))
T[:3, 3] = [0.4, -1.1, 0.7]
EXTENTS = np.array([6.2, 3.1, 7.9])
OCC_RANGE = [-1.0, 1.0]
TRUNK_FLOP = 2 * (63 * 256 + 6 * 256 * 256 + (256 + 63) * 256 + 256)          # per point: eight trunk layers and the density head


def new_call(dim):
    return geometry.occupancy_grid(net, embed, OCC_RANGE, EXTENTS, T, dim, DIST)


def one_run_network(dim, pts):
    raw = ssr.run_network(pts, torch.zeros_like(pts).squeeze(1), net, embed, embed_d)
    return geometry.occupancy_activation(raw[..., 3], DIST).reshape(dim, dim, dim)


def chunked_run_network(dim, pts, chunk=1024):
    raw = torch.cat([ssr.run_network(pts[i:i + chunk], torch.zeros_like(pts[i:i + chunk]).squeeze(1), net, embed, embed_d).cpu()
                     for i in range(0, pts.shape[0], chunk)], dim=0)
    occ = geometry.occupancy_activation(raw[..., 3], DIST)
    return occ.reshape(dim, dim, dim) if occ.numel() == dim ** 3 else occ          # (the warm-up takes a part of the lattice)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (time.perf_counter() - t0) * 1e3


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


result = {}
say(f"device: {torch.cuda.get_device_name(0)}; SSR network, {N_CLASSES} classes, f16x3; {a.rounds} alternating rounds of (a) and (b), "
    f"{a.chunk_rounds} of (c); times are per whole grid, host clock around a device synchronise")
with torch.no_grad():
    for dim in a.dims:
        n = dim ** 3
        pts = geometry.grid_within_bound(OCC_RANGE, EXTENTS, T, dim, device=dev)[0]          # (b) and (c) are handed the lattice: not timed
        ways = {"(a) inerf_occupancy_grid": lambda: new_call(dim), "(b) one run_network": lambda: one_run_network(dim, pts),
                "(c) 1024-point chunks + .cpu()": lambda: chunked_run_network(dim, pts)}
        occ_a, sig_a = geometry.occupancy_grid(net, embed, OCC_RANGE, EXTENTS, T, dim, DIST, return_sigma=True)
        raw_b = ssr.run_network(pts, torch.zeros_like(pts).squeeze(1), net, embed, embed_d)
        same = bool(torch.equal(sig_a.reshape(-1).view(torch.int32), raw_b[..., 3].reshape(-1).view(torch.int32)))
        occ_diff = float((occ_a.reshape(-1) - geometry.occupancy_activation(raw_b[..., 3], DIST).reshape(-1)).abs().max())
        positive = float((sig_a > 0).float().mean())
        del occ_a, sig_a, raw_b
        for k in list(ways)[:2]:
            for _ in range(2):
                timed(ways[k])
        timed(lambda: chunked_run_network(dim, pts[:64 * 1024]))
        times = {k: [] for k in ways}
        for rnd in range(a.rounds):
            for k, fn in ways.items():
                if k.startswith("(c)") and rnd >= a.chunk_rounds:
                    continue
                times[k].append(timed(fn))
        peaks = {k: peak_bytes(ways[k]) for k in list(ways)[:2]}
        res = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds": len(v)} for k, v in times.items()}
        say(f"grid {dim}^3 = {n} points ({100 * positive:.1f} % with sigma > 0)")
        for k, v in res.items():
            extra = f"; peak device memory {peaks[k] / 2 ** 20:9.1f} MiB" if k in peaks else ""
            say(f"  {k:32s} {v['median_ms']:10.2f} ms (rounds {v['min_ms']:.2f} .. {v['max_ms']:.2f}, {v['rounds']}){extra}")
        ta = res["(a) inerf_occupancy_grid"]["median_ms"]
        say(f"  (a) against (b): {res['(b) one run_network']['median_ms'] / ta:.2f} x; against (c): {res['(c) 1024-point chunks + .cpu()']['median_ms'] / ta:.1f} x; "
            f"(a) as a whole call: {n * TRUNK_FLOP / (ta * 1e-3) / 1e12:.1f} TFLOP/s of trunk work (3 f16 products per MAC not counted)")
        say(f"  sigma of (a) has the bits of (b)'s channel 3: {same}; largest |occ(a) - occ(b)|: {occ_diff:.3g}")
        res["peak_bytes"] = {k: int(v) for k, v in peaks.items()}
        res.update(same_sigma_bits=same, occ_diff=occ_diff, points=n)
        result[f"grid_{dim}"] = res
        del pts
say(json.dumps(result))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
