#!/usr/bin/env python
"""Frame images: the host expressions of render_path's ``finish`` against ``frames.FrameProducts`` (csrc/frame_vis.hip), one MI355X.

Two shapes: the SSR frame (320x240, 28 classes, all eleven products) and the object-level frame (800x800, five products).  Per
shape, after the bytes of both paths were asserted identical and both were warmed up, the two paths alternate in rounds:

  host     the numpy statements of the loops as they stand - to8b, astype(np.uint16), the label cast, valid_colour_map[label],
           (acc > 10) - starting from the frame's float maps on the host; the two jet maps (imgviz.depth2rgb in the reference, which this
           package does not require) are timed separately through ``frames.depth2rgb``'s numpy statement of the same rule
  device   ``FrameProducts.add_frame`` (range + product launches, the bytes' copy to the host) and ``images`` (the wait for it)

Then the device time of the product launch alone (events around back-to-back launches), its achieved bytes/s over the algorithmic
bytes (distinct columns read + planes written) beside the HBM peak, and a 40-frame ``render_path`` of each front-end around a stub
renderer, with and without the products.  Prints the report; ``--out FILE`` also writes it.

  python scripts/bench_frame_products.py --out profiles/frame_products_bench.txt
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from intrinsicnerf_amd import frames, kernels, object_level, ssr  # noqa: E402

HBM_PEAK_SPEC, HBM_PEAK_MEASURED = 8.0e12, 6.29e12          # bytes/s, MI355X: spec | float4 copy


def ssr_case(dev, H=240, W=320, C=28, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = H * W
    maps = {"rgb_fine": torch.rand(n, 3, generator=g), "disp_fine": torch.rand(n, generator=g) * 9, "depth_fine": torch.rand(n, generator=g) * 9.5 + 0.1,
            "albedo_fine": torch.rand(n, 3, generator=g), "shading_fine": torch.rand(n, generator=g), "residual_fine": torch.rand(n, 3, generator=g),
            "sem_label": torch.randint(0, C, (n,), generator=g).float(), "sem_entropy": torch.rand(n, generator=g) * 3.3}
    keys = list(maps)
    pack, widths = frames.pack_maps({k: v.to(dev) for k, v in maps.items()}, keys)
    colours = torch.randint(0, 256, (C, 3), generator=g).to(torch.uint8)
    plist = [(k, "to8b", f"{k}_fine") for k in ("rgb", "albedo", "shading", "residual")]
    plist += [("disp", "u16", "disp_fine", 1.0), ("depth", "u16", "depth_fine", 1000.0), ("vis_depth", "jet", "depth_fine", (0.1, 10.0)),
              ("label", "u8_cast", "sem_label"), ("entropy", "to8b", "sem_entropy"), ("vis_entropy", "jet", "sem_entropy", None),
              ("vis_label", "palette", "sem_label")]

    def host(m, jet):
        cmap = colours.numpy()
        label = m["sem_label"].astype(np.uint8)
        out = {k: frames.to8b(m[f"{k}_fine"]) for k in ("rgb", "albedo", "shading", "residual")}
        out.update(disp=m["disp_fine"].astype(np.uint16), depth=(m["depth_fine"] * 1000).astype(np.uint16), label=label,
                   entropy=frames.to8b(m["sem_entropy"]), vis_label=cmap[label.astype(np.int64)].astype(np.uint8))
        if jet:
            out.update(vis_depth=frames.depth2rgb(m["depth_fine"], min_value=0.1, max_value=10.0), vis_entropy=frames.depth2rgb(m["sem_entropy"]))
        return out

    return dict(name=f"SSR {W}x{H}, C = {C}, 11 products", shape=(H, W), pack=pack, keys=keys, widths=widths, products=plist, palette=colours, host=host,
                jet=("vis_depth", "vis_entropy"))


def object_case(dev, side=800, seed=1):
    g = torch.Generator().manual_seed(seed)
    n = side * side
    maps = {"rgb_map": torch.rand(n, 3, generator=g), "disp_map": torch.rand(n, generator=g), "acc_map": torch.rand(n, generator=g) * 20,
            "albedo_map": torch.rand(n, 3, generator=g), "shading_map": torch.rand(n, generator=g), "residual_map": torch.rand(n, 3, generator=g)}
    keys = list(maps)
    pack, widths = frames.pack_maps({k: v.to(dev) for k, v in maps.items()}, keys)
    plist = [("", "to8b", "rgb_map"), ("a", "to8b", "albedo_map"), ("s", "to8b", "shading_map"), ("res", "to8b", "residual_map"),
             ("acc", "thresh", "acc_map", 10.0)]

    def host(m, jet):
        acc = (m["acc_map"] > 10).astype(int).astype(np.float32)                   # run_nerf.py:173
        return {"": frames.to8b(m["rgb_map"]), "a": frames.to8b(m["albedo_map"]), "s": frames.to8b(m["shading_map"]),
                "res": frames.to8b(m["residual_map"]), "acc": frames.to8b(acc)}

    return dict(name=f"object level {side}x{side}, 5 products", shape=(side, side), pack=pack, keys=keys, widths=widths, products=plist, palette=None,
                host=host, jet=())


def algorithmic_bytes(case, fp):
    n = case["shape"][0] * case["shape"][1]
    start, c = {}, 0
    for k, w in zip(case["keys"], case["widths"]):
        start[k] = (c, w)
        c += w
    columns = set()
    for spec in case["products"]:
        c0, w = start[spec[2]]
        columns.update(range(c0, c0 + w))
    return 4 * n * len(columns) + sum(size for _, size in fp.plan[1])


def spread(xs):
    return f"{statistics.median(xs) * 1e3:8.3f} ms  (min {min(xs) * 1e3:.3f}, max {max(xs) * 1e3:.3f}, {len(xs)} rounds)"


def bench_case(case, rounds, frames_per_round, say):
    dev = case["pack"].device
    host_frame = case["pack"].cpu().numpy()
    fp = frames.FrameProducts()
    fp.begin(case["products"], case["keys"], case["widths"], case["shape"], dev, palette=case["palette"])
    # identical bytes first
    fp.add_frame(0, case["pack"])
    got = fp.images(0)
    want = case["host"](frames.unpack_frame(host_frame, case["widths"], case["keys"], case["shape"]), True)
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    say(f"\n== {case['name']} ==")
    say(f"bytes of both paths identical: {', '.join(repr(k) for k in want)}")

    def host_path(jet):
        for _ in range(frames_per_round):
            case["host"](frames.unpack_frame(host_frame, case["widths"], case["keys"], case["shape"]), jet)

    def device_path():
        for i in range(frames_per_round):
            fp.add_frame(i, case["pack"])
            if i > 0:
                fp.images(i - 1)                       # as the loops do: a frame is looked at after the next one is enqueued
        fp.images(frames_per_round - 1)

    for _ in range(2):                                 # warm-up of every shape and path
        host_path(True); host_path(False); device_path()
    torch.cuda.synchronize()
    t_host, t_host_jet, t_dev = [], [], []
    for _ in range(rounds):                            # the paths alternate
        for path, acc in ((lambda: host_path(False), t_host), (lambda: host_path(True), t_host_jet), (device_path, t_dev)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            path()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) / frames_per_round)
    say(f"per frame, host expressions{' without the jet maps' if case['jet'] else ''}: {spread(t_host)}")
    if case["jet"]:
        say(f"per frame, host expressions with the jet maps in numpy:     {spread(t_host_jet)}")
    say(f"per frame, FrameProducts.add_frame + images:                {spread(t_dev)}")
    # the product launch alone: device events around back-to-back launches
    reps = 200
    out = torch.empty(fp.plan[2], dtype=torch.uint8, device=dev)
    launch = lambda: kernels.frame_products(case["pack"], None, palette=fp.palette, out=out, plan=fp.plan)
    for _ in range(20):
        launch()
    times = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / reps)
    t = statistics.median(times)
    nbytes = algorithmic_bytes(case, fp)
    say(f"product launch, device time (events around {reps} back-to-back launches, median of 5): {t * 1e6:.2f} us")
    say(f"algorithmic bytes (distinct columns read + planes written): {nbytes} -> {nbytes / t / 1e12:.3f} TB/s achieved; "
        f"HBM peak {HBM_PEAK_SPEC / 1e12:.1f} TB/s spec, {HBM_PEAK_MEASURED / 1e12:.2f} TB/s measured copy "
        f"({nbytes / t / HBM_PEAK_MEASURED * 100:.1f} % of the measured peak; between back-to-back launches the frame stays in L2 / Infinity Cache)")


class StubSSR(ssr.SSRRenderMixin):
    """render_path around a renderer that returns ready maps: what remains is the loop itself."""

    def __init__(self, case, C):
        self.case, self.H_scaled, self.W_scaled, self.near, self.far = case, case["shape"][0], case["shape"][1], 0.1, 10.0
        self.N_importance, self.enable_semantic, self.valid_colour_map = 1, True, case["palette"]
        n = self.H_scaled * self.W_scaled
        c = 0
        self.out = {}
        for k, w in zip(case["keys"], case["widths"]):
            if not k.startswith("sem_"):
                self.out[k] = case["pack"][:, c:c + w].reshape(n, w) if w > 1 else case["pack"][:, c]
            c += w
        self.out["sem_logits_fine"] = torch.randn(n, C, device=case["pack"].device)

    def render_rays(self, rays):
        return self.out


def bench_loops(ssr_c, obj_c, n_frames, say):
    say(f"\n== {n_frames}-frame render_path around a stub renderer (no render; what remains is the loop) ==")
    stub = StubSSR(ssr_c, 28)
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
    try:
        for save in (False, True):
            res, files = {}, {}
            for rnd in range(3):                       # the first round warms up; the variants alternate
                for name in ("ssr host", "ssr products", "object host", "object products"):
                    with tempfile.TemporaryDirectory() as tmp:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        if name.startswith("ssr"):
                            stub.frame_products = frames.FrameProducts() if name.endswith("products") else None
                            stub.render_path(rays, save_dir=tmp if save else None)
                        else:
                            object_level.render_path(poses, (o["shape"][0], o["shape"][1], 1.0), None, n, {}, savedir=tmp if save else None,
                                                     products=frames.FrameProducts() if name.endswith("products") else None)
                        torch.cuda.synchronize()
                        if rnd > 0:
                            res.setdefault(name, []).append(time.perf_counter() - t0)
                        files[name] = len(os.listdir(tmp)) // n_frames
            for name, ts in res.items():
                say(f"{name:16s} {'%2d files per frame' % files[name] if save else 'no files          '}: {min(ts):7.3f} s / {max(ts):7.3f} s (2 rounds) = "
                    f"{min(ts) / n_frames * 1e3:7.2f} ms per frame")
        say("(without imgviz the SSR host path makes no vis_depth / vis_entropy: with the products it returns both and writes two more files per frame)")
    finally:
        object_level.render = orig_render


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=10, help="frames per round")
    ap.add_argument("--loop-frames", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_products.py measures on a HIP device; none is visible (no CPU fallback)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"frame products: host expressions vs frames.FrameProducts - {torch.cuda.get_device_name(0)}, torch {torch.__version__}, numpy {np.__version__}")
    say(f"rounds {args.rounds}, {args.frames} frames per round, the paths alternating after a warm-up of every shape")
    ssr_c, obj_c = ssr_case(dev), object_case(dev)
    for case in (ssr_c, obj_c):
        bench_case(case, args.rounds, args.frames, say)
    bench_loops(ssr_c, obj_c, args.loop_frames, say)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
