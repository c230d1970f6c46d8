#!/usr/bin/env python3
"""``optimizer.step()`` alone: ``optim.Adam`` (csrc/adam.hip) against ``torch.optim.Adam`` three ways - default (foreach),
``fused=True``, and ``capturable=True`` replayed from a graph - on the same GPU in the same process, alternating.

    python scripts/bench_adam.py [--iters 300] [--rounds 5]
Shapes: the object pair of networks (2 x 662 152 parameters, 64 tensors) and the SSR pair at C = 28 (2 x 698 660, 72 tensors).
Prints, per variant, milliseconds per step() including the host's part (median of the rounds), GPU time per step and kernel
launches per step (torch.profiler's device events; None where the profiler gives none), and for the HIP launch the bytes per
second its GPU time means against the 28 B per parameter it must move."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402

__graft_entry__.build()
from intrinsicnerf_amd import object_level as ol, optim, ssr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=300)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_adam.py measures on the GPU: no HIP device visible")
dev = torch.device("cuda:0")


def shapes(kind):
    e, ch = ol.get_embedder(10, 0)
    ed, chd = ol.get_embedder(4, 0)
    if kind == "object":
        net = ol.NeRF(D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=chd, use_viewdirs=True)
    else:
        net = ssr.Semantic_NeRF(True, 28, D=8, W=256, input_ch=ch, output_ch=5, skips=[4], input_ch_views=chd, use_viewdirs=True)
    return [tuple(p.shape) for p in net.parameters()] * 2


def make(kind, factory):
    gen = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.06).to(dev)) for s in shapes(kind)]
    for p in params:
        p.grad = (torch.randn(p.shape, generator=gen) * 1e-3).to(dev)
    return params, factory(params)


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


def device_events(fn, reps=20):
    """(kernel launches per call, GPU microseconds per call) from torch.profiler's device events; (None, None) without any."""
    from torch.profiler import ProfilerActivity, profile
    fn(); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    if not ev:
        return None, None
    return len(ev) / reps, sum(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total for e in ev) / reps


VARIANTS = {
    "inerf": (lambda ps: optim.Adam(ps, lr=5e-4, betas=(0.9, 0.999)), False),
    "inerf_graph": (lambda ps: optim.Adam(ps, lr=torch.tensor(5e-4, device=dev), betas=(0.9, 0.999)), True),
    "torch_foreach": (lambda ps: torch.optim.Adam(ps, lr=5e-4, betas=(0.9, 0.999)), False),
    "torch_fused": (lambda ps: torch.optim.Adam(ps, lr=5e-4, betas=(0.9, 0.999), fused=True), False),
    "torch_fused_graph": (lambda ps: torch.optim.Adam(ps, lr=torch.tensor(5e-4, device=dev), betas=(0.9, 0.999), fused=True, capturable=True), True),
    "torch_capturable_graph": (lambda ps: torch.optim.Adam(ps, lr=torch.tensor(5e-4, device=dev), betas=(0.9, 0.999), capturable=True), True),
}

result = {}
for kind in ("object", "ssr"):
    fns, row = {}, {}
    n_params = None
    for name, (factory, graph) in VARIANTS.items():
        params, opt = make(kind, factory)
        n_params = sum(p.numel() for p in params)
        for _ in range(5):
            opt.step()
        fns[name] = graphed(opt.step) if graph else opt.step
    for name, fn in fns.items():
        try:
            row[name + "_launches"], row[name + "_gpu_us"] = device_events(fn)
        except Exception as e:            # a profiler problem must not cost the timings
            row[name + "_launches"] = row[name + "_gpu_us"] = None
            row["profiler_error"] = repr(e)[:200]
    times = {name: [] for name in fns}
    for _ in range(a.rounds):                # alternating: other work shares the machine
        for name, fn in fns.items():
            times[name].append(timed(fn, a.iters))
    for name, ts in times.items():
        row[name + "_ms"], row[name + "_ms_rounds"] = statistics.median(ts), ts
    row["parameters"], row["bytes_moved"] = n_params, 28 * n_params
    for name in ("inerf", "inerf_graph"):
        us = row.get(name + "_gpu_us")
        row[name + "_gpu_bytes_per_s"] = 28 * n_params / (us * 1e-6) if us else None
        row[name + "_wall_bytes_per_s"] = 28 * n_params / (row[name + "_ms"] * 1e-3)
    result[kind] = row
    print(f"{kind}: {n_params} parameters in {len(params)} tensors, {28 * n_params / 1e6:.1f} MB per step")
    for name in fns:
        us, ln = row[name + "_gpu_us"], row[name + "_launches"]
        extra = ""
        if name.startswith("inerf"):
            rate = row[name + "_gpu_bytes_per_s"]
            extra = f"; {rate / 1e12:.2f} TB/s over its GPU time" if rate else ""
            extra += f"; {row[name + '_wall_bytes_per_s'] / 1e12:.2f} TB/s over its wall time"
        print(f"  {name:24s} {row[name + '_ms'] * 1e3:8.1f} us per step() (wall, back to back); GPU {'%.1f us' % us if us else 'n/a'}; launches {ln}{extra}")
print(json.dumps(result))
