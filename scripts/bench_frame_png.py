#!/usr/bin/env python
"""Frame images as PNG files: the host encoder of ``frames.write_png`` against ``inerf_png_encode`` (csrc/png.hip), one MI355X.

Two image sets: the SSR frame (320x240, 28 classes, eleven images) and the object-level frame (800x800, five images).  No real
render is at hand here, so the planes are SYNTHETIC, in two contents:

  smooth   every map a sum of low-frequency waves with 1 % noise over a flat background (a third of the frame) - the generator of the
           size table in DESIGN.md, the nearer of the two to a rendered frame
  noise    ``torch.rand`` maps, what profiles/frame_products_bench.txt was measured on: the worst case of any encoder

Per set and content: the device time of the three launches alone (events around back-to-back calls), the bytes per frame both paths
write, and a 40-frame ``render_path`` of each front-end around a stub renderer that writes its files - the parent's path
(``FrameProducts()``: planes to the host, ``write_png`` per file) against ``FrameProducts(encode=True)``, the two alternating in rounds.
Prints the report; ``--out FILE`` also writes it.

  python scripts/bench_frame_png.py --out profiles/frame_png_bench.txt
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench_frame_products as B  # noqa: E402
from intrinsicnerf_amd import frames, kernels, object_level  # noqa: E402


def smooth_map(h, w, width, g, lo=0.0, hi=1.0):
    """[h * w, width] fp32: waves, 1 % noise, a flat background outside an ellipse that covers two thirds of the frame."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    cols = []
    for c in range(width):
        f = g.uniform(0.5, 3.0, 4)
        wave = 0.5 + 0.2 * np.sin(2 * np.pi * f[0] * x / w + c) * np.cos(2 * np.pi * f[1] * y / h) + 0.15 * np.sin(2 * np.pi * (f[2] * x / w + f[3] * y / h))
        cols.append(wave + g.normal(0, 0.01, (h, w)))
    m = np.stack(cols, -1)
    inside = ((x - w / 2) / (0.46 * w)) ** 2 + ((y - h / 2) / (0.46 * h)) ** 2 < 1.0
    m[~inside] = 1.0
    return torch.from_numpy((lo + (hi - lo) * np.clip(m, 0, 1)).reshape(h * w, width).astype(np.float32))


def smooth_case(case, dev, classes=28, seed=0):
    """``case`` (bench_frame_products) with its pack replaced by smooth maps."""
    g = np.random.default_rng(seed)
    h, w = case["shape"]
    ranges = {"disp_fine": (0, 9), "depth_fine": (0.1, 9.6), "sem_entropy": (0, 3.3), "acc_map": (0, 20)}
    cols = []
    for k, width in zip(case["keys"], case["widths"]):
        if k == "sem_label":
            yy, xx = np.mgrid[0:h, 0:w]
            cols.append(torch.from_numpy(((xx // 40 + 3 * (yy // 40)) % classes).reshape(h * w, 1).astype(np.float32)))      # blocks of one label
        else:
            cols.append(smooth_map(h, w, width, g, *ranges.get(k, (0.0, 1.0))))
    out = dict(case)
    out["pack"] = torch.cat(cols, 1).to(dev)
    out["smooth"] = True
    return out


def launches_alone(case, say, reps=50):
    dev = case["pack"].device
    fp = frames.FrameProducts(encode=True)
    fp.begin(case["products"], case["keys"], case["widths"], case["shape"], dev, palette=case["palette"])
    for column, rng in fp.ranged:
        kernels.frame_range(case["pack"][:, column], minmax=rng, workspace=fp.workspace)
    planes, _ = kernels.frame_products(case["pack"], None, palette=fp.palette, plan=fp.plan)
    plan = fp.png_plan
    out = torch.empty(plan[2], dtype=torch.uint8, device=dev)
    sizes = torch.zeros(len(fp.names), dtype=torch.int64, device=dev)
    call = lambda: kernels.png_encode(planes[:fp.plan[2]], plan, out=out, sizes=sizes, workspace=fp.png_workspace)
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
    plane_bytes = sum(size for _, size in fp.plan[1])
    file_bytes = int(sizes.sum())
    segments = plan[3] // (32 + 32768 + 16)
    # what the host encoder writes for the same planes
    fp.add_frame(0, case["pack"])
    images = fp.images(0)
    with tempfile.TemporaryDirectory() as tmp:
        for name, img in images.items():
            frames.write_png(os.path.join(tmp, f"{name}_.png"), img)
        host_bytes = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp))
    say(f"the three launches, device time (events around {reps} back-to-back calls, median of 5; min {min(times) * 1e6:.1f}, max {max(times) * 1e6:.1f}): "
        f"{t * 1e6:.1f} us for {len(fp.names)} images, {segments} segments, {plane_bytes} plane bytes = {plane_bytes / t / 1e9:.1f} GB/s")
    say(f"bytes written per frame: host write_png {host_bytes}, device files {file_bytes} ({file_bytes / host_bytes * 100:.1f} % of the host's; "
        f"{file_bytes / plane_bytes * 100:.1f} % of the planes); travelling to the host per frame: {plan[2] + 8 * len(fp.names)} (worst-case buffers)")


def loops(ssr_c, obj_c, n_frames, rounds, say):
    stub = B.StubSSR(ssr_c, 28)
    if ssr_c.get("smooth") and "sem_label" in ssr_c["keys"]:
        # the stub draws its logits at random; here they follow the case's label blocks, with a confidence that varies smoothly
        at = sum(w for k, w in zip(ssr_c["keys"], ssr_c["widths"]) if ssr_c["keys"].index(k) < ssr_c["keys"].index("sem_label"))
        label = ssr_c["pack"][:, at].long()
        conf = 2.0 + 4.0 * ssr_c["pack"][:, 0:1]
        stub.out["sem_logits_fine"] = torch.nn.functional.one_hot(label, 28).float() * conf
    rays = [None] * n_frames
    orig_render = object_level.render
    o = obj_c
    n = o["shape"][0] * o["shape"][1]
    cols, c = [], 0
    for w in o["widths"]:
        cols.append(o["pack"][:, c:c + w].reshape(*o["shape"], w) if w > 1 else o["pack"][:, c].reshape(o["shape"]))
        c += w
    object_level.render = lambda H, W, K, **kw: cols + [{}]
    poses = torch.eye(4, device=o["pack"].device)[None].repeat(n_frames, 1, 1)
    res, files, nbytes = {}, {}, {}
    try:
        for rnd in range(rounds + 1):                  # the first round warms up; the variants alternate
            for name in ("ssr products", "ssr png", "object products", "object png"):
                encode = name.endswith("png")
                with tempfile.TemporaryDirectory() as tmp:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if name.startswith("ssr"):
                        stub.frame_products = frames.FrameProducts(encode=encode)
                        stub.render_path(rays, save_dir=tmp)
                    else:
                        object_level.render_path(poses, (o["shape"][0], o["shape"][1], 1.0), None, n, {}, savedir=tmp,
                                                 products=frames.FrameProducts(encode=encode))
                    torch.cuda.synchronize()
                    if rnd > 0:
                        res.setdefault(name, []).append(time.perf_counter() - t0)
                    files[name] = len(os.listdir(tmp)) // n_frames
                    nbytes[name] = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp)) // n_frames
    finally:
        object_level.render = orig_render
    for name, ts in res.items():
        say(f"{name:16s} {files[name]:2d} files, {nbytes[name]:8d} bytes per frame: {statistics.median(ts) / n_frames * 1e3:7.2f} ms per frame "
            f"(min {min(ts) / n_frames * 1e3:.2f}, max {max(ts) / n_frames * 1e3:.2f}, {len(ts)} rounds of {n_frames} frames)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop-frames", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_png.py measures on a HIP device; none is visible (no CPU fallback)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        import imageio  # noqa: F401
        host = "imageio.imwrite for 8-bit images (frames.write_png prefers it), zlib level 6 over filter-0 rows for 16-bit"
    except ImportError:
        host = "frames.write_png's own encoder: zlib level 6 over filter-0 rows"
    say(f"frame PNG files: host encoder vs inerf_png_encode - {torch.cuda.get_device_name(0)}, torch {torch.__version__}, numpy {np.__version__}")
    say(f"host encoder: {host}.  Planes are synthetic (no render at hand): 'smooth' = waves + 1 % noise + flat background, 'noise' = torch.rand")
    noise = {"ssr": B.ssr_case(dev), "object": B.object_case(dev)}
    smooth = {k: smooth_case(v, dev, seed=i) for i, (k, v) in enumerate(noise.items())}
    for label, cases in (("smooth", smooth), ("noise", noise)):
        for case in cases.values():
            say(f"\n== {case['name']}, {label} planes ==")
            launches_alone(case, say)
        say(f"\n== {args.loop_frames}-frame render_path around a stub renderer, files written, {label} planes ==")
        loops(cases["ssr"], cases["object"], args.loop_frames, args.rounds, say)
    say("\n('products': the parent's path - planes to the host, write_png per file; 'png': FrameProducts(encode=True) - files encoded on the device, "
        "the host writes bytes.  The parent's record for 'noise': 68.00 / 159.16 ms per frame, profiles/frame_products_bench.txt)")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
