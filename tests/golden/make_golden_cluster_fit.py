#!/usr/bin/env python3
"""Golden vectors for the mean-shift fit of the albedo clusters, from the reference's own classes and the real sklearn
(build container only; GPU tests read the .npz alone).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cluster_fit.py

Runs the reference's ``Cluster_Manager.update_center`` / ``Cluster.update_center`` (SSR/training/cluster.py:52-70,
138-182) on synthetic albedo samples and records, per fitted class, what sklearn computed on the way: the bandwidth
after band_factor and the floor, the number of bin seeds, ``cluster_centers_``, ``labels_`` and the number of points
behind every centre (the count ``_mean_shift_single_seed`` returned for it), then the anchors, links and rgb_centers
the reference keeps.  Cases (tests/golden/README.md):

  ssr_multi    SSR manager, 6 classes: a regular class, an empty one, a 1-pixel one, a 9-pixel class whose bins are all
               distinct (seeds = the points), a tight class where the 0.01 bandwidth floor binds, a larger regular one;
               band_factor 0.5
  ssr_single   class_num == 1 manager (labels ignored, :55-59); band_factor 0.25
  cluster_f08  a single Cluster with intensity_factor 0.8; band_factor 1.0
"""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
from make_golden_cluster import albedo_samples  # noqa: E402


class Recorder:
    """Wraps sklearn's MeanShift.fit and _mean_shift_single_seed to record what each fit computed."""

    def __init__(self, ref):
        import sklearn.cluster._mean_shift as skms
        self.fits = []
        rec = self
        orig_seed, orig_fit = skms._mean_shift_single_seed, skms.MeanShift.fit

        def seed(*a, **k):
            out = orig_seed(*a, **k)
            rec.cur["seeds"].append(out)
            return out

        def fit(ms, X, y=None):
            rec.cur = {"seeds": [], "bw": float(ms.bandwidth)}
            out = orig_fit(ms, X, y)
            counts = {}
            for centre, n, _ in rec.cur["seeds"]:
                if n:
                    counts[centre] = n                      # the dict of MeanShift.fit: the last seed wins
            rec.cur["n_seeds"] = len(rec.cur["seeds"])
            rec.cur["centers"] = ms.cluster_centers_.astype(np.float32)
            rec.cur["labels"] = ms.labels_.astype(np.int32)
            rec.cur["counts"] = np.array([counts[tuple(c)] for c in ms.cluster_centers_], np.int32)
            rec.fits.append(rec.cur)
            return out

        skms._mean_shift_single_seed = seed
        skms.MeanShift.fit = fit


def class_sets(rng):
    a = albedo_samples(rng, 10000, 4)
    one = albedo_samples(rng, 1, 1)
    # 9 pixels far apart in the mapped space: every bin holds one pixel, so sklearn seeds with the points themselves
    spread = np.array([[0.9, 0.1, 0.1], [0.1, 0.9, 0.1], [0.1, 0.1, 0.9], [0.5, 0.5, 0.1], [0.1, 0.5, 0.5],
                       [0.5, 0.1, 0.5], [0.3, 0.3, 0.3], [0.8, 0.8, 0.2], [0.2, 0.3, 0.85]], np.float32)
    tight = np.clip(np.array([0.4, 0.5, 0.3]) + rng.normal(0, 0.012, size=(3000, 3)), 0.01, 1).astype(np.float32)
    big = albedo_samples(rng, 12000, 7)
    return [a, None, one, spread, tight, big]


def main():
    mg.import_reference()
    from SSR.training import cluster as ref
    # choose_anchors' `voxel[id] = pixels` after the descending sort: with one thread the CPU index_put writes in order, so
    # the last (minimum-dist) pixel of every voxel wins; several threads write chunks concurrently and any may win
    torch.set_num_threads(1)
    cpu = torch.device("cpu")
    ref.Cluster.__init__.__defaults__ = (cpu, 0.5, None)            # Cluster() inside update_center: on the CPU here
    rec = Recorder(ref)
    rng = np.random.default_rng(20221016)
    out = {}

    def record(case, clusters, fits, extra):
        it = iter(fits)
        for c, cl in enumerate(clusters):
            if cl is None:
                out[f"{case}_c{c}_none"] = np.array(1)
                continue
            f = next(it)
            out[f"{case}_c{c}_bw"] = np.float64(f["bw"])
            out[f"{case}_c{c}_n_seeds"] = np.int64(f["n_seeds"])
            out[f"{case}_c{c}_centers_mapped"] = f["centers"]
            out[f"{case}_c{c}_labels"] = f["labels"]
            out[f"{case}_c{c}_counts"] = f["counts"]
            out[f"{case}_c{c}_anchors"] = cl.anchors.numpy().astype(np.float32)
            out[f"{case}_c{c}_links"] = cl.links.numpy().astype(np.int64)
            out[f"{case}_c{c}_rgb_centers"] = cl.rgb_centers.float().numpy()
        out.update({f"{case}_{k}": v for k, v in extra.items()})

    # ssr_multi: labels in an interleaved order, so that every class's pixels keep a non-trivial original order
    sets = class_sets(rng)
    pixels, labels = [], []
    for c, s in enumerate(sets):
        if s is not None:
            pixels.append(s)
            labels.append(np.full(len(s), c, np.int64))
    pixels, labels = np.concatenate(pixels), np.concatenate(labels)
    order = rng.permutation(len(pixels))
    pixels, labels = pixels[order], labels[order][:, None]
    mgr = ref.Cluster_Manager(class_num=len(sets))
    rec.fits = []
    with contextlib.redirect_stdout(io.StringIO()):
        mgr.update_center(labels, pixels, band_factor=0.5)
    record("ssr_multi", mgr.clusters, rec.fits, {"pixels": pixels, "labels": labels, "class_num": len(sets), "band_factor": 0.5})
    assert out["ssr_multi_c3_n_seeds"] == 9, "the spread class must fall back to the points as seeds"
    assert out["ssr_multi_c4_bw"] == 0.01, "the tight class must hit the bandwidth floor"

    # ssr_single: class_num == 1 ignores the labels
    px = albedo_samples(rng, 20000, 5)
    lab = rng.integers(0, 3, size=(len(px), 1))
    one = ref.Cluster_Manager(class_num=1)
    rec.fits = []
    with contextlib.redirect_stdout(io.StringIO()):
        one.update_center(lab, px, band_factor=0.25)
    record("ssr_single", one.clusters, rec.fits, {"pixels": px, "labels": lab, "class_num": 1, "band_factor": 0.25})

    # cluster_f08: Cluster.update_center with a non-default intensity_factor
    px = albedo_samples(rng, 10000, 3)
    cl = ref.Cluster(device=cpu, intensity_factor=0.8)
    rec.fits = []
    with contextlib.redirect_stdout(io.StringIO()):
        cl.update_center(px, band_factor=1.0)
    record("cluster_f08", [cl], rec.fits, {"pixels": px, "factor": 0.8, "band_factor": 1.0})

    path = os.path.join(HERE, "cluster_fit.npz")
    np.savez_compressed(path, **out)
    for k in sorted(out):
        if k.endswith("_bw") or k.endswith("_n_seeds"):
            print(k, out[k], end="; ")
    print()
    print({k: out[k].shape[0] for k in out if k.endswith("centers_mapped")})
    print("wrote cluster_fit.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
