#!/usr/bin/env python
"""Frame movies: Motion-JPEG AVI files made on the device (``FrameProducts(movies=...)``, csrc/jpeg.hip) against the same frames copied
to the host and encoded there by Pillow at the same quality (4:4:4, fixed Huffman tables) into the same container, one MI355X.

Two image sets, as in bench_frame_png.py: the SSR frame (320x240, 28 classes) with five movies and the object-level frame (800x800)
with two.  No real render is at hand here, so the planes are SYNTHETIC ('smooth': waves + 1 % noise + a flat background; 'noise':
``torch.rand``), and the renderer is a stub: every frame of a loop is the same pack.  Per set and content:

  the three launches of ``inerf_jpeg_encode`` alone (events around back-to-back calls into a worst-case arena that is rewound), and
  the bytes per frame of both encoders;
  a 40-frame loop - ``add_frame`` per frame, the files finished at the end - in alternating rounds:
    device  ``FrameProducts(movies=...)``: one more call per frame, ``close_movies()`` copies each arena once and writes the file
    host    ``FrameProducts()``: every frame's planes travel to the host (the streamer both paths share), Pillow encodes the named
            planes, ``frames.avi_bytes`` assembles the files
No time here is a threshold.  Prints the report; ``--out FILE`` also writes it.

  python scripts/bench_frame_movies.py --out profiles/frame_movies_bench.txt
"""
import argparse
import io
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench_frame_png as P  # noqa: E402
import bench_frame_products as B  # noqa: E402
from intrinsicnerf_amd import frames, kernels  # noqa: E402

QUALITY = 90
WANTED = {"ssr": ("rgb", "vis_depth", "albedo", "vis_label", "vis_entropy"), "object": ("", "a")}


def movie_names(case, kind):
    have = [p[0] for p in case["products"] if p[1] != "u16"]
    names = [n for n in WANTED[kind] if n in have]
    names += [n for n in have if n not in names][:len(WANTED[kind]) - len(names)]
    return names


def pillow_jpeg(plane):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(plane).save(buf, "JPEG", quality=QUALITY, subsampling=0)
    return buf.getvalue()


def begin(case, movies=None):
    fp = frames.FrameProducts(movies=movies, fps=30, quality=QUALITY)
    fp.begin(case["products"], case["keys"], case["widths"], case["shape"], case["pack"].device, palette=case["palette"])
    return fp


def launches_alone(case, names, say, reps=50):
    with tempfile.TemporaryDirectory() as tmp:
        fp = begin(case, {n: os.path.join(tmp, f"{k}.avi") for k, n in enumerate(names)})
        for column, rng in fp.ranged:
            kernels.frame_range(case["pack"][:, column], minmax=rng, workspace=fp.workspace)
        planes, _ = kernels.frame_products(case["pack"], None, palette=fp.palette, plan=fp.plan)
        streams = [kernels.JpegStream(*w.stream.shape, QUALITY, w.bound, 1, planes.device) for w in fp.writers]

        def call():
            for s in streams:
                s.state.zero_()
            kernels.jpeg_encode(planes[:fp.plan[2]], fp.jpeg_plan, streams, workspace=fp.jpeg_workspace)

        for _ in range(5):
            call()
        times = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                call()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e-3 / reps)
        t = statistics.median(times)
        device_bytes = sum(int(s.state[4]) for s in streams)
        plane_bytes = sum(s.shape[0] * s.shape[1] * s.shape[2] for s in streams)
        fp.add_frame(0, case["pack"])
        images = fp.images(0)
        host_bytes = sum(len(pillow_jpeg(np.ascontiguousarray(images[n]))) for n in names)
        fp.writers = []                                  # (nothing to finish: the writers only lent their shapes)
    say(f"the three launches + rewinding {len(streams)} cursors, device time (events around {reps} back-to-back calls, median of 5; min "
        f"{min(times) * 1e6:.1f}, max {max(times) * 1e6:.1f}): {t * 1e6:.1f} us for {len(streams)} images, {plane_bytes} plane bytes = "
        f"{plane_bytes / t / 1e9:.2f} GB/s")
    say(f"JPEG bytes per frame at quality {QUALITY}: Pillow (4:4:4, fixed tables) {host_bytes}, device {device_bytes} "
        f"({device_bytes / host_bytes * 100:.1f} % of Pillow's; {device_bytes / plane_bytes * 100:.1f} % of the planes)")


def loop(case, names, n_frames, device_path, tmp):
    paths = {n: os.path.join(tmp, f"{k}.avi") for k, n in enumerate(names)}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fp = begin(case, paths if device_path else None)
    files = {n: [] for n in names}
    for i in range(n_frames):
        fp.add_frame(i, case["pack"])
        if i >= 2:
            images = fp.images(i - 2)
            if not device_path:
                for n in names:
                    files[n].append(pillow_jpeg(np.ascontiguousarray(images[n])))
    for i in range(max(n_frames - 2, 0), n_frames):
        images = fp.images(i)
        if not device_path:
            for n in names:
                files[n].append(pillow_jpeg(np.ascontiguousarray(images[n])))
    if device_path:
        fp.close_movies()
    else:
        h, w = case["shape"]
        for n in names:
            with open(paths[n], "wb") as fh:
                fh.write(frames.avi_bytes(files[n], w, h, 30))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, sum(os.path.getsize(p) for p in paths.values()) // n_frames


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop-frames", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_movies.py measures on a HIP device; none is visible (no CPU fallback)")
    import PIL
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"frame movies: Pillow {PIL.__version__} on the host vs inerf_jpeg_encode - {torch.cuda.get_device_name(0)}, torch {torch.__version__}, "
        f"numpy {np.__version__}")
    say("Planes are synthetic (no render at hand): 'smooth' = waves + 1 % noise + flat background, 'noise' = torch.rand; the renderer is a "
        "stub (every frame the same pack); both paths make the frame's planes with FrameProducts and stream them to the host")
    noise = {"ssr": B.ssr_case(dev), "object": B.object_case(dev)}
    smooth = {k: P.smooth_case(v, dev, seed=i) for i, (k, v) in enumerate(noise.items())}
    for label, cases in (("smooth", smooth), ("noise", noise)):
        for kind, case in cases.items():
            names = movie_names(case, kind)
            say(f"\n== {case['name']}, {label} planes, {len(names)} movies: {names} ==")
            launches_alone(case, names, say)
            res, size = {"device": [], "host": []}, {}
            for rnd in range(args.rounds + 1):             # the first round warms up; the paths alternate
                for path in ("host", "device"):
                    with tempfile.TemporaryDirectory() as tmp:
                        dt, size[path] = loop(case, names, args.loop_frames, path == "device", tmp)
                    if rnd > 0:
                        res[path].append(dt)
            for path, ts in res.items():
                n = args.loop_frames
                say(f"{path:7s} {size[path]:8d} file bytes per frame: {statistics.median(ts) / n * 1e3:7.2f} ms per frame (min {min(ts) / n * 1e3:.2f}, "
                    f"max {max(ts) / n * 1e3:.2f}, {len(ts)} rounds of {n} frames)")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
