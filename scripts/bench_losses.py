#!/usr/bin/env python3
"""The training losses: torch expressions (scripts/torch_losses.py) against the two HIP launches (csrc/losses.hip), forward +
backward, issued eagerly and replayed from a captured graph, on the same GPU in the same process, alternating.

    python scripts/bench_losses.py [--iters 300] [--rounds 5]
Shapes: object level N = 2 048 (a [N,1] mask, cluster target), SSR N = 1 024 with C = 28 (cluster target, cross-entropy);
coarse and fine level each.  Prints milliseconds per forward+backward (median of the rounds) and kernel launches per call."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__  # noqa: E402

__graft_entry__.build()
import torch_losses  # noqa: E402
from intrinsicnerf_amd import losses  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=300)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_losses.py measures on the GPU: no HIP device visible")
dev = torch.device("cuda:0")
WEIGHTS = {"image": 1.0, "chroma": 1.0, "sparsity": 0.01, "far": 0.01, "shading": 1.0, "residual": 1.0, "intensity": 0.1, "cluster": 1.0,
           "semantic": 0.04}


def make(kind):
    g = torch.Generator().manual_seed(0)
    n, c = (2048, 0) if kind == "object" else (1024, 28)
    gt = torch.rand(n, 3, generator=g) * 0.8 + 0.1
    gt[n // 2:] = (gt[:n // 2] + 0.02 * torch.randn(n // 2, 3, generator=g)).clamp(0.02, 1)
    key = (torch.rand(n, 1, generator=g) > 0.2).float() if kind == "object" else torch.randint(0, c + 1, (n,), generator=g)
    levels = []
    for _ in range(2):
        lv = {"albedo": torch.rand(n, 3, generator=g) * 0.6 + 0.05, "shading": torch.rand(n, generator=g) + 0.1,
              "residual": 0.1 * torch.randn(n, 3, generator=g), "rgb": torch.rand(n, 3, generator=g)}
        if c:
            lv["logits"] = 2 * torch.randn(n, c, generator=g)
        levels.append({k: v.to(dev).requires_grad_(True) for k, v in lv.items()})
    return levels, gt.to(dev), key.to(dev), torch.rand(n, 3, generator=g).to(dev)


def runners(kind):
    levels, gt, key, target = make(kind)
    leaves = [v for lv in levels for v in lv.values()]
    if kind == "object":
        ret = {"rgb0": levels[0]["rgb"], "albedo0": levels[0]["albedo"], "shading0": levels[0]["shading"], "residual0": levels[0]["residual"],
               "rgb_map": levels[1]["rgb"], "albedo_map": levels[1]["albedo"], "shading_map": levels[1]["shading"], "residual_map": levels[1]["residual"]}
        hip = lambda: losses.object_step_loss(ret, gt, key, WEIGHTS, target)[0]
    else:
        ret = {k + t: lv[n] for t, lv in zip(("_coarse", "_fine"), levels) for k, n in
               (("rgb", "rgb"), ("albedo", "albedo"), ("shading", "shading"), ("residual", "residual"), ("sem_logits", "logits"))}
        hip = lambda: losses.ssr_step_loss(ret, gt, key, WEIGHTS, target)[0]
    tor = lambda: torch_losses.step_loss(levels, gt, key, WEIGHTS, target, semantic=kind == "ssr")

    def fb(fn):
        def run():
            for v in leaves:
                v.grad = None
            fn().backward()
        return run
    return fb(tor), fb(hip), leaves


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


def launches(fn):
    """GPU kernels one call launches (torch.profiler's device events); None where the profiler gives none."""
    from torch.profiler import ProfilerActivity, profile
    fn(); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    return n or None


result = {}
for kind in ("object", "ssr"):
    tor, hip, leaves = runners(kind)
    for fn in (tor, hip):
        for _ in range(20):
            fn()
    tor(); want = [v.grad.clone() for v in leaves]
    hip(); worst = max(float((v.grad - w).abs().max() / w.abs().max().clamp_min(1e-30)) for v, w in zip(leaves, want))
    row = {"max_gradient_difference_over_scale": worst}
    try:
        row["launches_torch"], row["launches_hip"] = launches(tor), launches(hip)
    except Exception as e:            # a profiler problem must not cost the timings
        row["launches_torch"] = row["launches_hip"] = None
        row["launch_count_error"] = repr(e)[:200]
    modes = {"eager": (tor, hip), "graph": (graphed(tor), graphed(hip))}
    for mode, (f_t, f_h) in modes.items():
        ts, hs = [], []
        for _ in range(a.rounds):                # alternating: other work shares the machine
            ts.append(timed(f_t, a.iters)); hs.append(timed(f_h, a.iters))
        row[f"{mode}_torch_ms"], row[f"{mode}_hip_ms"] = statistics.median(ts), statistics.median(hs)
        row[f"{mode}_torch_ms_rounds"], row[f"{mode}_hip_ms_rounds"] = ts, hs
    result[kind] = row
    print(f"{kind:6s} forward+backward, 2 levels: eager torch {row['eager_torch_ms']:.3f} ms / hip {row['eager_hip_ms']:.3f} ms; "
          f"graph torch {row['graph_torch_ms']:.3f} ms / hip {row['graph_hip_ms']:.3f} ms; launches torch {row['launches_torch']} / hip {row['launches_hip']}; "
          f"gradients agree to {worst:.1e} of scale")
print(json.dumps(result))
