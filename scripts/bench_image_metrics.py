"""Intrinsic-image metrics on the device (csrc/imq.hip) against eager torch on the same GPU (scripts/torch_image_metrics.py:
float64 conv2d SSIM, unfold LMSE).

    python scripts/bench_image_metrics.py [--rounds 7] [--out profiles/image_metrics_bench.txt]

Two shapes: one 800x800x3 frame (a Blender test view) and a 200-frame 320x240x3 stack, both with a 70 % mask.  The sides get
identical device-resident inputs and alternate round by round after a warm-up; a round is `--calls` back-to-back calls timed by
device events; the median round is reported with min, max and spread; the two sides' metrics are compared in the same run.  The
kernel side is also replayed from a HIP graph (its four launches without the host's share).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch_image_metrics as TM                                                    # noqa: E402
from intrinsicnerf_amd import evaluation, kernels                                   # noqa: E402


def device_time(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / iters


def graph_time(fn, iters=10, replays=10):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            fn()
    graph.replay()
    return device_time(graph.replay, replays) / iters


def alternate(sides, rounds, measure):
    for fn in sides.values():
        measure(fn)
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            times[k].append(measure(fn))
    return times


def line(name, ts, extra=""):
    med = statistics.median(ts)
    return f"  {name:<44s} {med * 1e3:10.4f} ms (min {min(ts) * 1e3:.4f}, max {max(ts) * 1e3:.4f}; spread {(max(ts) - min(ts)) / med * 100:.1f} %){extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(0)
    lines = [f"# python scripts/bench_image_metrics.py --rounds {args.rounds} --calls {args.calls}   ({torch.cuda.get_device_name(dev)}; the two sides "
             f"alternate round by round after a warm-up, {args.calls} calls per round by device events; median round, min, max, spread = (max - min) / median)"]
    record = {}
    for n, h, w in ((1, 800, 800), (200, 240, 320)):
        target = torch.rand(n, h, w, 3, generator=g).to(dev)
        pred = (0.25 + 0.75 * (0.7 * target + 0.3 * torch.rand(n, h, w, 3, generator=g).to(dev))).contiguous()
        mask = (torch.rand(n, h, w, generator=g) < 0.7).float().to(dev)
        ws = torch.empty(kernels.image_quality_workspace_bytes(n, h, w, 3) // 8, dtype=torch.float64, device=dev)
        sums, counts = kernels.image_quality(pred, target, mask, workspace=ws)
        ours = evaluation.finish_image_quality_stack(sums.cpu().numpy(), counts.cpu().numpy(), 3)
        theirs = {k: v.cpu().numpy() for k, v in TM.image_metrics(pred, target, mask).items()}
        diffs = {k: float(np.max(np.abs(np.array([f[k] for f in ours["frames"]]) - theirs[k]))) for k in theirs}
        key = f"{n} x {w}x{h}x3"
        byts = n * h * w * (3 * 4 * 2 + 4)
        lines.append(f" {key}, 70 % mask; {byts / 1e6:.1f} MB of inputs.  max |inerf - torch| over the frames: "
                     + ", ".join(f"{k} {v:.1e}" for k, v in diffs.items()))
        sides = {"torch (fp64 conv2d + unfold)": lambda: TM.image_metrics(pred, target, mask),
                 "inerf image_quality": lambda: kernels.image_quality(pred, target, mask, workspace=ws)}
        times = alternate(sides, args.rounds, lambda fn: device_time(fn, args.calls))
        for k, v in times.items():
            lines.append(line(k, v, f";  {byts / statistics.median(v) / 1e9:8.1f} GB/s of inputs"))
        graphed = alternate({"inerf image_quality, replayed from a graph": sides["inerf image_quality"]}, args.rounds, graph_time)
        for k, v in graphed.items():
            lines.append(line(k, v, f";  {byts / statistics.median(v) / 1e9:8.1f} GB/s of inputs"))
        names = list(times)
        ratio = statistics.median(times[names[0]]) / statistics.median(times[names[1]])
        lines.append(f"  torch / inerf = {ratio:.1f} launch by launch")
        record[key] = {"diffs": diffs, "ratio": ratio, **times, **graphed}
        del sides, pred, target, mask, ws
        torch.cuda.empty_cache()
    lines.append(json.dumps(record))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
