#!/usr/bin/env python3
"""One slider tick of the edit engine - a centre recoloured, shading squared, both scales moved, the shown 8-bit frame back on
the host - through ``editing.EditSession`` (csrc/edit.hip: the cached, streaming form over 8-bit sources and slots) against the
reference's expressions (scripts/torch_editing.py: ``update_img``'s per-class gather / scatter loop on fp32 tensors, a blocking
``.cpu()``, numpy ``to8b``), on the same GPU in the same process, in separate rounds that alternate.

    python scripts/bench_editing.py [--rounds 7]
Cases: one 320x240 frame with K = 28 semantic classes; one 800x800 frame with K = 1; a 200-frame 320x240 sequence with K = 28,
every frame re-edited per tick (``sequence()``: one launch; the reference: ``update_img`` frame by frame, as its play mode does).
Per case and path: seconds per tick with the frames fetched to the host (median, min, max of the rounds after a warm-up; spread
= (max - min) / median), and the device work alone between two events - the launches without the copy to the host - with, for
this package's path (at least 200 launches per round: three of them are too short a window), the bytes the kernel moves (7 source
bytes, a 4-byte slot, 3 output bytes per pixel) over that time - the 200-frame case's 276 MB do not fit the 256 MiB last-level
cache, the single frames' do.  Whether
the two paths show the same bytes is reported from the warm-up ticks (no sine transfer: that mode is not bit-reproducible)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402

__graft_entry__.build()
from intrinsicnerf_amd import editing  # noqa: E402
from torch_editing import TorchEditor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_editing.py measures on the GPU: no HIP device visible")
dev = torch.device("cuda:0")


class Manager:
    def __init__(self, clusters):
        self.class_num, self.clusters = len(clusters), clusters


def manager(K, seed):
    """K classes, each with 6 centres and 400 anchors in the mapped colour space (intensity / 3 * factor, g / I, b / I)."""
    g = torch.Generator().manual_seed(seed)
    clusters = []
    for _ in range(K):
        anchors = torch.cat([torch.rand(400, 1, generator=g) * 0.5, torch.rand(400, 2, generator=g) * 0.6], 1)
        clusters.append({"anchors": anchors.to(dev), "links": torch.randint(0, 6, (400, 1), generator=g).to(dev),
                         "rgb_centers": torch.rand(6, 3, generator=g).to(dev), "intensity_factor": 0.5, "batch_size": 10240})
    return Manager(clusters)


def scene(F, H, W, K, seed):
    g = np.random.RandomState(seed)
    rows = np.arange(H)[:, None] * 6 // H
    label = np.stack([(rows * 8 + (np.arange(W)[None, :] * 8 // W + f) % 8) % K for f in range(F)], 0).astype(np.int64)
    return (g.randint(1, 256, size=(F, H, W, 3)).astype(np.uint8), g.randint(0, 256, size=(F, H, W)).astype(np.uint8),
            g.randint(0, 64, size=(F, H, W, 3)).astype(np.uint8), label)


def timed(fn, ticks):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ticks):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / ticks


def device_ms(fn, ticks):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(ticks):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / ticks * 1e-3


CASES = [("1 x 320x240, K=28", 1, 240, 320, 28, 200), ("1 x 800x800, K=1", 1, 800, 800, 1, 100), ("200 x 320x240, K=28", 200, 240, 320, 28, 3)]
print(f"# python scripts/bench_editing.py --rounds {a.rounds}   ({torch.cuda.get_device_name(0)}; seconds per slider tick - every frame of the case "
      f"re-edited and, for 'tick', fetched to the host as 8-bit images; {a.rounds} rounds per path, the two paths alternating, after a warm-up)")
result = {}
for name, F, H, W, K, ticks in CASES:
    mgr = manager(K, 100 + K)
    albedo, shading, residual, label = scene(F, H, W, K, F + H)
    session = editing.EditSession(mgr, dev)
    session.add_frames_u8(albedo, shading, residual, label)
    ref = TorchEditor(mgr, albedo, shading, residual, label, dev)
    # the edit of the tick: one centre recoloured, shading squared, both scales off 1
    session.set_color(K - 1, 2, 250, 40, 10)
    ref.update_color(K - 1, 2, 250, 40, 10)
    session.change_shading, session.shading_scale, session.residual_scale = True, 0.8, 1.3
    ref.global_change_shading, ref.global_shading_scale, ref.global_residual_scale = True, 0.8, 1.3
    block = session._blocks[0]
    paths = {
        "inerf": dict(tick=lambda: list(session.sequence()) if F > 1 else session.frame(0),
                      device=lambda: session._launch(block, 0, F, False)),
        "torch": dict(tick=lambda: [ref.update_img(i) for i in range(F)], device=lambda: [ref.compose(i) for i in range(F)]),
    }
    ours, theirs = paths["inerf"]["tick"](), paths["torch"]["tick"]()                        # warm-up, and the comparison
    ours = ours if F > 1 else [ours]
    same = all(np.array_equal(x, y) for x, y in zip(ours, theirs))
    for p in paths.values():
        p["device"]()
    times = {p: {"tick": [], "device": []} for p in paths}
    for _ in range(a.rounds):
        for p, fns in paths.items():
            times[p]["tick"].append(timed(fns["tick"], ticks))
            times[p]["device"].append(device_ms(fns["device"], max(ticks, 200) if p == "inerf" else ticks))
    pixels = F * H * W
    row = {"frames": F, "pixels": pixels, "ticks_per_round": ticks, "inerf_device_launches_per_round": max(ticks, 200), "same_images": bool(same)}
    print(f"{name}: the 8-bit frames of the two paths identical: {same}; resident bytes per pixel: 11 + 4 (slot) against 52")
    for p in paths:
        for kind in ("tick", "device"):
            ts = times[p][kind]
            med = statistics.median(ts)
            row[f"{p}_{kind}_s"], row[f"{p}_{kind}_rounds"], row[f"{p}_{kind}_spread"] = med, ts, (max(ts) - min(ts)) / med
            extra = f"; {18 * pixels / med / 1e9:8.1f} GB/s of 18 B per pixel" if (p, kind) == ("inerf", "device") else ""
            print(f"  {p:5s} {kind:6s} {med * 1e3:10.4f} ms (min {min(ts) * 1e3:.4f}, max {max(ts) * 1e3:.4f}; spread {row[f'{p}_{kind}_spread'] * 100:.1f} %)"
                  f"{extra}")
    for kind in ("tick", "device"):
        row[f"{kind}_ratio"] = row[f"torch_{kind}_s"] / row[f"inerf_{kind}_s"]
        print(f"  {kind}: torch / inerf = {row[f'{kind}_ratio']:.2f}")
    result[name] = row
    del session, ref
    torch.cuda.empty_cache()
print(json.dumps(result))
