#!/usr/bin/env python3
"""Wall-clock time of the mean-shift cluster fit (intrinsicnerf_amd.cluster.fit, csrc/cluster_fit.hip) at the two
training shapes of the reference, on synthetic albedo; prints one JSON line.

    python scripts/bench_cluster_fit.py [--repeats 3] [--sklearn]

  ssr_room0    180 views x 160 x 120 = 3 456 000 pixels over 28 classes (SSR/training/trainer.py:1065)
  object_chair 25 views x 200 x 200 = 1 000 000 pixels, one class (object_level/run_nerf.py:1061-1071)

``permutation_ms`` is the host draw of estimate_bandwidth's subsample (numpy's legacy RandomState stream), ``fit_ms``
everything else up to the tables on the device (median of the repeats, after one warm-up).  With ``--sklearn`` and
sklearn importable, the reference's CPU fit (estimate_bandwidth + MeanShift(bin_seeding=True)) is timed on the same
points of the object shape.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic(n, K, seed):
    g = torch.Generator().manual_seed(seed)
    modes = torch.rand(K, 6, 3, generator=g) * 0.8 + 0.1
    lab = torch.randint(0, K, (n,), generator=g)
    pick = torch.randint(0, 6, (n,), generator=g)
    shade = torch.rand(n, 1, generator=g) * 0.6 + 0.6
    px = (modes[lab, pick] * shade + 0.02 * torch.randn(n, 3, generator=g)).clamp(0.01, 1.0)
    return px.numpy(), lab.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sklearn", action="store_true")
    args = ap.parse_args()
    from intrinsicnerf_amd import cluster as ic
    out = {"metric": "cluster_fit"}
    for name, n, K in (("ssr_room0", 3_456_000, 28), ("object_chair", 1_000_000, 1)):
        px, lab = synthetic(n, K, 1)
        labels = lab if K > 1 else None
        counts = np.bincount(lab, minlength=K) if K > 1 else np.array([n])
        t0 = time.perf_counter()
        sample = ic.sample_indices(counts, 5000)
        perm_ms = (time.perf_counter() - t0) * 1e3
        pxd = torch.from_numpy(px).cuda()
        times = []
        for r in range(args.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ic.fit(pxd, labels, K, [0.5] * K, sample=sample)
            torch.cuda.synchronize()
            if r:
                times.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"pixels": n, "classes": K, "permutation_ms": round(perm_ms, 2), "fit_ms": round(float(np.median(times)), 2),
                     "total_ms": round(perm_ms + float(np.median(times)), 2),
                     "centres": int(sum(0 if c is None else c.shape[0] for c in res.centers)),
                     "anchors": int(sum(0 if a is None else a.shape[0] for a in res.anchors))}
        if args.sklearn and K == 1:
            try:
                from sklearn.cluster import MeanShift, estimate_bandwidth
            except ImportError:
                continue
            I = px.sum(-1)
            d = np.stack([I / 3.0 * 0.5, px[:, 1] / I, px[:, 2] / I], -1).astype(np.float32)
            t0 = time.perf_counter()
            bw = max(estimate_bandwidth(d, quantile=0.3, n_samples=5000) * 0.5, 0.01)
            MeanShift(bandwidth=bw, bin_seeding=True).fit(d)
            out[name]["sklearn_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
