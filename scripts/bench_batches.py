#!/usr/bin/env python3
"""Batch assembly alone: the trainers' host + torch expressions (scripts/torch_batches.py, host draws and uploads included) against
the one launch of csrc/batch.hip - with caller-supplied indices (form a: the host draws and three small uploads stay), with
indices drawn in the kernel (form b), and form b replayed from a captured graph - on the same GPU in the same process, alternating.

    python scripts/bench_batches.py [--iters 200] [--rounds 5]
Shapes: object level 400 x 400 and 800 x 800 with N_rand = 1 024 (100 images on the host / on the device), SSR 320 x 240 with
n = 512 (20 images).  Prints milliseconds per batch: median of the rounds and their range; one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__  # noqa: E402

__graft_entry__.build()
import torch_batches  # noqa: E402
from intrinsicnerf_amd import batches  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_batches.py measures on the GPU: no HIP device visible")
dev = torch.device("cuda:0")


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def object_runners(size, n_img=100, n_rand=1024):
    rng = np.random.RandomState(0)
    images = rng.rand(n_img, size, size, 3).astype(np.float32)
    masks = (rng.rand(n_img, size, size, 1) > 0.3).astype(np.float32)
    poses = np.tile(np.eye(4, dtype=np.float32), (n_img, 1, 1))
    poses[:, :3, 3] = rng.randn(n_img, 3)
    focal = 0.5 * size / np.tan(0.5 * 0.6911112070083618)
    K = np.array([[focal, 0, 0.5 * size], [0, focal, 0.5 * size], [0, 0, 1]])
    i_train = np.arange(n_img)
    b = batches.ObjectBatcher(images, masks, poses, K, i_train, n_rand, device=dev)
    it = [0]

    def reference():
        it[0] += 1
        return torch_batches.object_batch(it[0], images, masks, poses, K, i_train, n_rand, 0, 0.5, dev)

    def supplied():                     # the reference's host draws (the full permutation included), three uploads, one launch
        img = np.random.choice(i_train)
        sel = np.random.choice(size * size, size=[n_rand], replace=False)
        return b.next(0, indices=(img, sel, np.random.choice([-1, 0, 1], n_rand), np.random.choice([-1, 0, 1], n_rand)))
    return {"reference expressions": reference, "hip, indices supplied": supplied, "hip, drawn in the kernel": b.next,
            "hip, drawn, graph replay": graphed(b.next)}


def ssr_runners(h=240, w=320, n_img=20, n=512):
    g = torch.Generator().manual_seed(0)
    image, depth = torch.rand(n_img, h, w, 3, generator=g, dtype=torch.float64).to(dev), torch.rand(n_img, h, w, generator=g, dtype=torch.float64).to(dev)
    semantic = torch.randint(0, 29, (n_img, h, w), generator=g, dtype=torch.uint8).to(dev)
    rays = torch.randn(n_img, h * w, 11, generator=g).to(dev)
    mask_ids = np.ones(n_img)
    b = batches.SSRBatcher(image, depth, semantic, n, rays=rays, mask_ids=mask_ids, device=dev)

    def supplied():
        return b.next(0, indices=(np.random.choice(np.arange(n_img)), torch.randint(0, h * w, (n,)), np.random.choice([-1, 0, 1], n),
                                  np.random.choice([-1, 0, 1], n)))
    return {"reference expressions": lambda: torch_batches.ssr_batch(rays, image, depth, semantic, mask_ids, n),
            "hip, indices supplied": supplied, "hip, drawn in the kernel": b.next, "hip, drawn, graph replay": graphed(b.next)}


result = {}
for name, make in (("object 400x400 N_rand=1024", lambda: object_runners(400)), ("object 800x800 N_rand=1024", lambda: object_runners(800)),
                   ("ssr 320x240 n=512", ssr_runners)):
    runners = make()
    for fn in runners.values():
        for _ in range(10):
            fn()
    times = {k: [] for k in runners}
    for _ in range(a.rounds):                   # alternating: other work shares the machine
        for k, fn in runners.items():
            times[k].append(timed(fn, a.iters))
    result[name] = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}
    for k, v in result[name].items():
        print(f"{name:28s} {k:26s} {v['median_ms']:8.3f} ms per batch (rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f})", flush=True)
    del runners
    torch.cuda.empty_cache()
print(json.dumps(result))
