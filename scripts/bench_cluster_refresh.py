#!/usr/bin/env python3
"""The part of ``render_path(update_cluster=True)`` that is not rendering - sample collection, mean-shift fit, the ``c`` / ``edit``
post-pass - on the host path (``cluster_manager_factory=cluster.Cluster_Manager``: numpy slicing, labels through the host,
per frame an upload, ``dest_color``, a float download and numpy ``to8b`` / compose) against the device path
(``refresh.ClusterRefresh``, csrc/refresh.hip), on the same GPU in the same process, alternating.

    python scripts/bench_cluster_refresh.py [--rounds 5] [--png]
The renderer is a stub that hands back fixed device maps, so that the render does not hide the difference; everything else is
the front-ends' own code: the frame streamer, the host's unpacking and the 8-bit conversion of the other images (common to both
paths).  PNG encoding (zlib on the host, the same bytes for both paths) is replaced by a no-op unless ``--png`` is given.
Shapes: object level, 20 frames of 400x400 and of 800x800 (one class); SSR, 40 frames of 320x240 with C = 28.
Per shape: whether the two paths fit the same clusters and write the same images (checksums taken in the warm-up passes); per path: seconds per pass (median, min, max of the rounds after one warm-up pass of each path) and the spread
(max - min) / median; then the difference of the medians."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402

__graft_entry__.build()
from intrinsicnerf_amd import cluster, frames, object_level as ol, refresh, ssr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--png", action="store_true", help="encode the PNG files for real (zlib on the host, equal work for both paths)")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_cluster_refresh.py measures on the GPU: no HIP device visible")
dev = torch.device("cuda:0")
written = None                    # {file name: checksum of the image} while a warm-up pass records what it writes
_write_png = frames.write_png


def write_png(path, image):
    if written is not None:
        written[os.path.basename(path)] = (image.shape, str(image.dtype), zlib.adler32(np.ascontiguousarray(image).tobytes()))
    if a.png:
        _write_png(path, image)


frames.write_png = write_png

PALETTE = torch.tensor([[0.80, 0.25, 0.20], [0.20, 0.55, 0.30], [0.25, 0.30, 0.75], [0.85, 0.80, 0.30], [0.55, 0.55, 0.55],
                        [0.70, 0.40, 0.65], [0.30, 0.70, 0.75]])


def scene(n_frames, H, W, n_classes, seed):
    """Per frame: a label map of rectangular regions and an albedo of one palette colour per region, lit and noisy."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for f in range(n_frames):
        rows = torch.arange(H)[:, None] * 6 // H
        cols = (torch.arange(W)[None, :] * 8 // W + f) % 8
        region = rows * 8 + cols                                                  # 48 regions, shifting from frame to frame
        label = region % max(n_classes, 1)
        albedo = (PALETTE[region % len(PALETTE)] * (0.6 + 0.4 * torch.rand(H, W, 1, generator=g))
                  + 0.02 * torch.randn(H, W, 3, generator=g)).clamp(0.02, 1.0)
        shading = 0.3 + 0.9 * torch.rand(H, W, generator=g)
        residual = 0.1 * torch.randn(H, W, 3, generator=g)
        rgb = (albedo * shading[..., None] + residual).clamp(0, 1)
        depth = 2.0 + 3.0 * torch.rand(H, W, generator=g)
        out.append({"rgb": rgb, "disp": 1.0 / depth, "depth": depth, "acc": torch.ones(H, W), "albedo": albedo, "shading": shading,
                    "residual": residual, "label": label})
    return out


def object_case(n_frames, side):
    maps = [{k: v.to(dev) for k, v in m.items()} for m in scene(n_frames, side, side, 1, side)]
    poses = [torch.cat([torch.eye(4)[:, :3], torch.full((4, 1), float(i))], 1).to(dev) for i in range(n_frames)]

    def fake_render(H, W, K, chunk=0, c2w=None, **kw):             # the frames in order, whatever the pose
        m = maps[fake_render.next % n_frames]
        fake_render.next += 1
        return [m["rgb"], m["disp"], m["acc"], m["albedo"], m["shading"], m["residual"], {}]
    fake_render.next = 0
    ol.render = fake_render

    def run(savedir, **extra):
        fake_render.next = 0
        return ol.render_path(poses, (side, side, float(side)), np.eye(3), side * side, {}, savedir=savedir, update_cluster=True,
                              b_f=0.5, **extra)
    return run, dict(host=dict(cluster_manager_factory=cluster.Cluster_Manager), device=dict(refresh=refresh.ClusterRefresh()))


class StubTrainer(ssr.SSRRenderMixin):
    N_importance, enable_semantic, near, far = 128, True, 0.1, 10.0


def ssr_case(n_frames, H, W, C):
    maps = []
    for m in scene(n_frames, H, W, C, 7):
        d = {f"{k}_fine": m[k].reshape(H * W, -1).squeeze(-1).to(dev) for k in ("rgb", "disp", "depth", "albedo", "shading", "residual")}
        d["sem_logits_fine"] = (torch.nn.functional.one_hot(m["label"].reshape(-1), C).float() * 8.0).to(dev)
        maps.append(d)
    t = StubTrainer()
    t.H_scaled, t.W_scaled, t.num_valid_semantic_class = H, W, C
    count = [0]

    def fake_render_rays(rays):                                   # the frames in order, whatever the rays
        count[0] += 1
        return maps[(count[0] - 1) % n_frames]
    t.render_rays = fake_render_rays
    rays = [torch.zeros(1, 11, device=dev) for _ in range(n_frames)]

    def run(savedir, **extra):
        count[0] = 0
        t.cluster_manager_factory, t.cluster_refresh = extra.get("factory"), extra.get("refresh")
        return t.render_path(rays, save_dir=savedir, update_cluster=True, b_f=0.5)
    return run, dict(host=dict(factory=cluster.Cluster_Manager), device=dict(refresh=refresh.ClusterRefresh()))


def same_manager(x, y):
    for p, q in zip(x.clusters, y.clusters):
        if (p is None) != (q is None) or (p is not None and not (torch.equal(p.rgb_centers, q.rgb_centers) and torch.equal(p.anchors, q.anchors))):
            return False
    return len(x.clusters) == len(y.clusters)


CASES = [("object 20 x 400x400", lambda: object_case(20, 400), 20), ("object 20 x 800x800", lambda: object_case(20, 800), 20),
         ("ssr 40 x 320x240, C=28", lambda: ssr_case(40, 240, 320, 28), 40)]
result = {}
print(f"# python scripts/bench_cluster_refresh.py{' --png' if a.png else ''}   ({torch.cuda.get_device_name(0)}; seconds per pass of "
      f"render_path(update_cluster=True) around a stub renderer; {a.rounds} rounds, the two paths alternating, after one warm-up pass each; "
      f"PNG encoding {'on' if a.png else 'replaced by a no-op'})")
for name, make, n_frames in CASES:
    run, paths = make()
    times, managers, files = {p: [] for p in paths}, {}, {}
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        for p, extra in paths.items():                       # warm-up: code objects, pinned buffers, the allocator's pools
            written = files[p] = {}
            managers[p] = run(tmp, **extra)[-1]
            written = None
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for p, extra in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(tmp, **extra)
                torch.cuda.synchronize()
                times[p].append(time.perf_counter() - t0)
    row = {"frames": n_frames, "same_clusters": same_manager(managers["host"], managers["device"]), "files": len(files["host"]),
           "same_files": files["host"] == files["device"] and any(k.startswith("edit") for k in files["host"])}
    print(f"{name}: clusters of the two paths identical: {row['same_clusters']}; the {row['files']} images each path writes identical: {row['same_files']}")
    for p, ts in times.items():
        med = statistics.median(ts)
        row[p + "_s"], row[p + "_s_rounds"], row[p + "_spread"] = med, ts, (max(ts) - min(ts)) / med
        print(f"  {p:7s} {med:8.4f} s per pass (min {min(ts):.4f}, max {max(ts):.4f}; spread {row[p + '_spread'] * 100:.1f} %); "
              f"{med / n_frames * 1e3:7.2f} ms per frame")
    saved = row["host_s"] - row["device_s"]
    row["saved_s"], row["saved_fraction"] = saved, saved / row["host_s"]
    print(f"  device path saves {saved:.4f} s per pass = {saved / n_frames * 1e3:.2f} ms per frame = {row['saved_fraction'] * 100:.1f} % of the host path")
    result[name] = row
    torch.cuda.empty_cache()
print(json.dumps(result))
