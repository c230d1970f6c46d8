"""Validation metrics on the device against what the validation step does without them (scripts/torch_evaluation.py).

    python scripts/bench_evaluation.py [--rounds 7] [--frames 180] [--out profiles/evaluation_bench.txt]

Three measurements, each with both sides on identical inputs, the sides alternating round by round after a warm-up, the median
round reported with min / max / spread, and the results of the sides compared in the same run:
  1. label + entropy maps of one frame (320x240 C=28, 640x480 C=101): ssr.render_path's torch expressions against inerf_sem_maps,
     device time per frame and the achieved bytes per second over the algorithmic bytes (4 C + 8 per pixel);
  2. the metric calls over `frames` frames of 320x240, C=28: the restated reference (sklearn + numpy) on host arrays,
     evaluation.calculate_* on the same host arrays (upload included), and FrameEvaluator on device-resident maps (the time
     add_frame adds to a frame over sem_maps alone, and results());
  3. device time of inerf_eval_accumulate on one 320x240 frame, C=28: random labels against all pixels in one class (the
     LDS-atomic contention case), label column only and with every group, next to eager torch counting the same tables.
Device times are given launch by launch (events around 200 calls: the host's launch rate bounds them) and replayed from a HIP
graph of 20 calls (the kernels alone).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch_evaluation as TE                                                       # noqa: E402
from intrinsicnerf_amd import evaluation, kernels                                   # noqa: E402


def device_time(fn, iters):
    """Seconds per call of `iters` back-to-back calls, by device events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3 / iters


def graph_time(fn, iters=20, replays=10):
    """Seconds per call with `iters` calls captured into one HIP graph and the graph replayed: the launches' device time without
    the host's share (the Python launchers here cost about as much as these kernels run)."""
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


def wall_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(sides, rounds, measure):
    """{name: [seconds per round]}: one warm-up of every side, then `rounds` rounds in which the sides take turns."""
    for fn in sides.values():
        measure(fn)
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            times[k].append(measure(fn))
    return times


def line(name, ts, extra=""):
    med = statistics.median(ts)
    return f"  {name:<62s} {med * 1e3:10.4f} ms (min {min(ts) * 1e3:.4f}, max {max(ts) * 1e3:.4f}; spread {(max(ts) - min(ts)) / med * 100:.1f} %){extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=180)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(0)
    lines = [f"# python scripts/bench_evaluation.py --rounds {args.rounds} --frames {args.frames}   ({torch.cuda.get_device_name(dev)}; the sides of every "
             f"measurement alternate round by round after a warm-up; median round, min, max, spread = (max - min) / median)"]
    record = {}

    # ---- 1. label + entropy per frame -------------------------------------------------------------------------------------------
    lines.append("1. label + entropy maps of one frame, device time per frame (200 launches per round)")
    for (h, w, c) in ((240, 320, 28), (480, 640, 101)):
        n = h * w
        x = (torch.randn(n, c, generator=g) * 3).to(dev)
        label, entropy = torch.empty(n, device=dev), torch.empty(n, device=dev)
        t_label, t_entropy = TE.torch_sem_maps(x)
        kernels.sem_maps(x, label=label, entropy=entropy)
        same = bool(torch.equal(label, t_label))
        err = float((entropy - t_entropy).abs().max())
        times = alternate({"torch": lambda: TE.torch_sem_maps(x), "inerf": lambda: kernels.sem_maps(x, label=label, entropy=entropy)},
                          args.rounds, lambda fn: device_time(fn, 200))
        graphed = alternate({"torch": lambda: TE.torch_sem_maps(x), "inerf": lambda: kernels.sem_maps(x, label=label, entropy=entropy)},
                            args.rounds, graph_time)
        byts = n * (4 * c + 8)
        key = f"{w}x{h}, C={c}"
        lines.append(f" {key}: labels of the two sides identical: {same}; max |entropy difference| {err:.2e}; {byts / 1e6:.2f} MB algorithmic")
        for k in ("torch", "inerf"):
            lines.append(line(k + " maps", times[k], f";  {byts / statistics.median(times[k]) / 1e9:8.1f} GB/s"))
        for k in ("torch", "inerf"):
            lines.append(line(k + " maps, replayed from a graph", graphed[k], f";  {byts / statistics.median(graphed[k]) / 1e9:8.1f} GB/s"))
        ratio = statistics.median(times["torch"]) / statistics.median(times["inerf"])
        lines.append(f"  torch / inerf = {ratio:.2f} launch by launch, {statistics.median(graphed['torch']) / statistics.median(graphed['inerf']):.2f} replayed")
        record[key + " graphed"] = graphed
        record[key] = {"same_labels": same, "entropy_diff": err, "bytes": byts, "ratio": ratio, **{k + "_s": v for k, v in times.items()}}

    # ---- 3. the accumulate kernel on one frame (before 2: it is short) ------------------------------------------------------------
    h, w, c = 240, 320, 28
    n = h * w
    lines.append(f"3. inerf_eval_accumulate (+ its finishing launch) on one {w}x{h} frame, C={c}, device time (200 launches per round)")
    dt = (torch.rand(n, generator=g) * 12 + 1e-3).to(dev)
    dp = dt * (0.5 + 1.2 * torch.rand(n, generator=g).to(dev))
    rp, rt = torch.rand(n, 3, generator=g).to(dev), torch.rand(n, 3, generator=g).to(dev)
    x = (torch.randn(n, c, generator=g) * 3).to(dev)
    x_one = x.clone(); x_one[:, 5] = 40.0
    regimes = {"random labels": (torch.randint(-1, c, (n,), generator=g).float().to(dev), torch.randint(0, c, (n,), generator=g).float().to(dev), x),
               "one class": (torch.full((n,), 5.0, device=dev), torch.full((n,), 5.0, device=dev), x_one)}
    counts, sums = kernels.eval_tables(c, dev)
    ws = torch.empty(kernels.eval_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
    label, entropy = torch.empty(n, device=dev), torch.empty(n, device=dev)
    sides = {}
    for name, (t, p, logits) in regimes.items():
        # the eager partner and the kernel count the same table
        counts.zero_(); sums.zero_()
        kernels.eval_accumulate(counts, sums, c, -1, true_label=t, pred_label=p, depth_pred=dp, depth_trgt=dt, workspace=ws)
        table, tc, ts = TE.torch_accumulate(c, -1, t, p, dt, dp)
        same = bool(torch.equal(counts[:c * c].reshape(c, c), table)) and bool(torch.equal(counts[c * c + 1:c * c + 7], tc))
        lines.append(f" {name}: table and depth counts of kernel and eager torch identical: {same}; "
                     f"max relative difference of the five depth sums {float(((sums[:5] - ts) / ts).abs().max()):.2e}")
        record["accumulate " + name + " same"] = same
        sides[name + ", label column only"] = (lambda t=t, p=p: kernels.eval_accumulate(counts, sums, c, -1, true_label=t, pred_label=p, workspace=ws))
        sides[name + ", labels + depth + rgb"] = (lambda t=t, p=p: kernels.eval_accumulate(counts, sums, c, -1, true_label=t, pred_label=p, depth_pred=dp,
                                                                                      depth_trgt=dt, rgb_pred=rp, rgb_trgt=rt, workspace=ws))
        sides[name + ", logits + all groups"] = (lambda t=t, lg=logits: kernels.eval_accumulate(counts, sums, c, -1, logits=lg, true_label=t, depth_pred=dp,
                                                                                               depth_trgt=dt, rgb_pred=rp, rgb_trgt=rt, out_label=label,
                                                                                               out_entropy=entropy, workspace=ws))
        sides[name + ", eager torch (labels + depth)"] = (lambda t=t, p=p: TE.torch_accumulate(c, -1, t, p, dt, dp))
    sides["sem_maps alone (for scale)"] = lambda: kernels.sem_maps(x, label=label, entropy=entropy)
    times = alternate(sides, args.rounds, lambda fn: device_time(fn, 200))
    for k, v in times.items():
        lines.append(line(k, v))
    record["accumulate"] = times
    graphed = alternate({k: fn for k, fn in sides.items() if "eager" not in k}, args.rounds, graph_time)      # (the eager partner's masked gathers synchronise)
    for k, v in graphed.items():
        lines.append(line(k + ", replayed from a graph", v))
    record["accumulate graphed"] = graphed

    # ---- 2. the metric calls over a frame set -----------------------------------------------------------------------------------
    f = args.frames
    lines.append(f"2. the metric calls over {f} frames of {w}x{h}, C={c} (wall time, synchronised)")
    true = np.random.default_rng(0).integers(-1, c, size=(f, h, w)).astype(np.int64)
    sems = np.random.default_rng(1).integers(0, c, size=(f, h, w)).astype(np.uint8)
    depth_t = (np.random.default_rng(2).random((f, h, w)) * 12 + 1e-3).astype(np.float32)
    deps = (depth_t * (0.5 + 1.2 * np.random.default_rng(3).random((f, h, w)))).astype(np.float32)
    results = {}

    def host_side():
        results["host"] = (TE.host_segmentation(true, sems, c, -1), TE.host_depth(depth_t, deps))

    def inerf_side():
        results["inerf"] = (evaluation.calculate_segmentation_metrics(true, sems, c, -1), evaluation.calculate_depth_metrics(depth_t, deps))

    times = alternate({"restated reference (sklearn + numpy), host arrays": host_side, "evaluation.calculate_*, same host arrays, upload included": inerf_side},
                      args.host_rounds, wall_time)
    seg_same = all(np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)
                   for a, b in zip(results["host"][0], results["inerf"][0]))
    depth_diff = max(abs(float(results["host"][1][k]) - float(results["inerf"][1][k])) / max(abs(float(results["inerf"][1][k])), 1e-30) for k in results["host"][1])
    lines.append(f" segmentation metrics of the two sides identical: {seg_same}; largest relative difference of a depth metric (numpy means in fp32, "
                 f"here fp64 sums): {depth_diff:.2e}")
    for k, v in times.items():
        lines.append(line(k, v))
    names = list(times)
    lines.append(f"  host / inerf = {statistics.median(times[names[0]]) / statistics.median(times[names[1]]):.2f}")
    record["metric calls"] = {"seg_same": seg_same, "depth_rel_diff": depth_diff, **times}

    rays = torch.zeros(f, 1, 11, device=dev)
    ev = evaluation.FrameEvaluator(c)
    ev.register(rays, depth=depth_t.reshape(f, -1), semantic=true.reshape(f, -1))
    deps_dev = torch.from_numpy(deps).reshape(f, -1).to(dev)

    def evaluator_frames():
        ev.begin(rays)
        for i in range(f):
            ev.add_frame(i, logits=x, depth=deps_dev[i])

    def maps_only():
        for i in range(f):
            kernels.sem_maps(x)

    times = alternate({f"FrameEvaluator.add_frame x {f} (maps + accumulation)": evaluator_frames, f"sem_maps x {f} (maps alone)": maps_only,
                       "FrameEvaluator.results()": lambda: ev.results()}, args.rounds, wall_time)
    for k, v in times.items():
        lines.append(line(k, v))
    names = list(times)
    added = (statistics.median(times[names[0]]) - statistics.median(times[names[1]])) / f
    lines.append(f"  added per frame by the accumulation: {added * 1e6:.2f} us")
    record["frame evaluator"] = {"added_per_frame_s": added, **times}

    lines.append(json.dumps(record))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
