"""CPU oracle of the albedo-cluster mean-shift fit.  TEST INFRASTRUCTURE ONLY.

A plain fp64 statement, one class at a time and with brute-force neighbours, of what ``intrinsicnerf_amd.cluster.fit``
(csrc/cluster_fit.hip) computes for every class of a manager:

* ``Cluster.update_center`` / ``choose_anchors`` (SSR/training/cluster.py:138-182) and ``mapping_color_np`` /
  ``inv_mapping_color`` (:316-322, 335-341);
* sklearn's ``estimate_bandwidth`` (k-th neighbour distance of the ``RandomState(0).permutation`` subsample, its mean),
  ``get_bin_seeds`` (first-occurrence dict order, the points themselves when every bin holds one point),
  ``_mean_shift_single_seed`` (flat kernel, stop at ``1e-3 * bandwidth`` or 300 iterations, a seed without a point in
  reach is dropped) and the merge of ``MeanShift.fit`` (sorted by (count, centre tuple) descending, greedy suppression
  within the bandwidth, labels = nearest surviving centre).

No sklearn import: the neighbour queries are dense distance matrices.  The arithmetic rules are the ones written down in
cluster_fit.hip: the mapping in fp32 without contraction; every distance as ``(dx*dx + dy*dy) + dz*dz`` in fp64;
``np.round(point / bin_size)`` and ``bin_seeds * bin_size`` in fp32 when the bandwidth is the Python float ``0.01`` (the
floor bound) and in fp64 when it is an ``np.float64``; the subsample from ``cluster.sample_indices``.  Means are taken in
fp64 and rounded to fp32 (sklearn's ``np.mean`` accumulates in fp32: that difference is what the centre tolerance of the
tests pays for).  Where choose_anchors' voxel distances tie, the pixel of the lowest rank wins, as in the kernel.

Pinned by ``tests/golden/cluster_fit.npz`` and ``tests/golden/cluster_fit_edges.npz`` (the reference's classes on the real
sklearn), replayed by ``tests/test_cluster_fit_oracle_cpu.py``.
"""
import numpy as np
import torch

MAX_ITER = 300          # MeanShift(max_iter=300)
FLOOR = 0.01            # max(bandwidth * band_factor, 0.01), cluster.py:141
LEAF = 0.01             # choose_anchors' leaf_size


def mapping_color_np(rgb, intensity_factor):
    """cluster.py:316-322 on float32 pixels."""
    rgb = np.asarray(rgb, np.float32)
    intensity = np.sum(rgb, axis=-1)
    d_rgb = np.zeros_like(rgb)
    d_rgb[..., 0] = intensity / 3.0 * np.float32(intensity_factor)
    d_rgb[..., 1] = rgb[..., 1] / intensity
    d_rgb[..., 2] = rgb[..., 2] / intensity
    return d_rgb


def inv_mapping_color(d_rgb, intensity_factor):
    """cluster.py:335-341 and the clamp of :152, torch float32 on the CPU."""
    d_rgb = torch.as_tensor(d_rgb)
    intensity = d_rgb[..., 0] * 3.0 / intensity_factor
    rgb = torch.zeros_like(d_rgb)
    rgb[..., 1] = d_rgb[..., 1] * intensity
    rgb[..., 2] = d_rgb[..., 2] * intensity
    rgb[..., 0] = intensity - rgb[..., 1] - rgb[..., 2]
    return rgb.clamp(0, 1)


def sq_dists(a, b):
    """[len(a), len(b)] squared distances of fp64 rows, summed in the kernel's order."""
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def estimate_bandwidth(X, sample_idx, quantile):
    """sklearn's estimate_bandwidth on the rows ``sample_idx`` of X: mean distance to the k-th nearest subsample row (the
    row itself is the first), k = max(1, int(S * quantile))."""
    Xs = np.asarray(X, np.float64)[np.asarray(sample_idx, np.int64)]
    S = Xs.shape[0]
    k = min(S, max(1, int(S * quantile)))
    total = 0.0
    for b in range(0, S, 512):
        r2 = sq_dists(Xs[b:b + 512], Xs)
        total += float(np.sqrt(np.partition(r2, k - 1, axis=1)[:, k - 1]).sum())
    return total / S


def bin_seeds(X, bw, floor_bound):
    """get_bin_seeds(X, bw, min_bin_freq=1): (seed positions [T,3] fp64 in sklearn's dict order, seeds_are_points)."""
    if floor_bound:                     # bin_size is the Python float 0.01: numpy stays in fp32
        binned = np.round(X / np.float32(bw))
    else:                               # bin_size is an np.float64
        binned = np.round(X.astype(np.float64) / np.float64(bw))
    _, first = np.unique(binned, axis=0, return_index=True)
    first = np.sort(first)              # a dict keeps the order in which its keys first appeared
    if first.shape[0] == X.shape[0]:
        return X.astype(np.float64), True
    seeds = binned[first].astype(np.float32)
    if floor_bound:
        return (seeds * np.float32(bw)).astype(np.float64), False
    return seeds.astype(np.float64) * np.float64(bw), False


def mean_shift_seeds(X, seeds, bw, block=64):
    """_mean_shift_single_seed for every seed: (centre [T,3] fp32, count [T] - 0 for a seed that was dropped)."""
    X64 = X.astype(np.float64)
    T = seeds.shape[0]
    centre = np.zeros((T, 3), np.float32)
    count = np.zeros(T, np.int64)
    r2max, stop = bw * bw, 1e-3 * bw
    for b in range(0, T, block):
        idx = np.arange(b, min(T, b + block))
        m = seeds[idx].copy()
        for it in range(MAX_ITER + 1):
            within = sq_dists(m, X64) <= r2max
            n_in = within.sum(1)
            count[idx] = n_in
            live = n_in > 0
            if not live.all():          # no point within bw: the seed is dropped
                idx, m, within, n_in = idx[live], m[live], within[live], n_in[live]
                if idx.size == 0:
                    break
            new = ((within.astype(np.float64) @ X64) / n_in[:, None]).astype(np.float32)
            shift = np.sqrt(((new.astype(np.float64) - m) ** 2).sum(1))
            centre[idx] = new
            m = new.astype(np.float64)
            go = ~((shift <= stop) | (it == MAX_ITER))
            idx, m = idx[go], m[go]
            if idx.size == 0:
                break
    return centre, count


def merge(centre, count, bw):
    """The post-processing of MeanShift.fit: indices into the seeds of the surviving centres, in merge order."""
    table = {}
    for i in range(centre.shape[0]):
        if count[i]:
            table[tuple(centre[i].tolist())] = (int(count[i]), i)          # the dict of MeanShift.fit: the last seed wins
    order = sorted(table.items(), key=lambda kv: (kv[1][0], kv[0]), reverse=True)
    cand = np.array([kv[1][1] for kv in order], np.int64)
    pts = centre[cand].astype(np.float64)
    unique = np.ones(len(cand), bool)
    for i in range(len(cand)):
        if unique[i]:
            unique[sq_dists(pts[i:i + 1], pts)[0] <= bw * bw] = False
            unique[i] = True
    return cand[unique], cand


def choose_anchors(X, labels):
    """cluster.py:156-182: per occupied voxel of edge 0.01 the pixel nearest the voxel centre (lowest rank on ties), the
    voxels in C order: (anchors [A,3] fp32, links [A,1] int64, rank of every anchor's pixel)."""
    p = torch.from_numpy(np.ascontiguousarray(X))
    vid = torch.clamp((p / LEAF).long(), 0, int(1 / LEAF) - 1)
    dist = torch.sum((vid * LEAF + LEAF / 2 - p) ** 2, dim=1).numpy()
    flat = ((vid[:, 0] * 100 + vid[:, 1]) * 100 + vid[:, 2]).numpy()
    order = np.lexsort((np.arange(len(flat)), dist, flat))      # by voxel, then distance, then rank
    keep = np.ones(len(flat), bool)
    keep[1:] = flat[order][1:] != flat[order][:-1]
    rank = order[keep]
    return X[rank].astype(np.float32), np.asarray(labels, np.int64)[rank].reshape(-1, 1), rank


def fit_class(pixels_c, factor, quantile=0.3, n_samples=5000, band_factor=0.5):
    """Everything the fit decides for the pixels [n_c,3] of one class, as a dict."""
    from intrinsicnerf_amd.cluster import sample_indices
    X = mapping_color_np(np.asarray(pixels_c, np.float32).reshape(-1, 3), factor)
    idx, _ = sample_indices([X.shape[0]], n_samples)
    bw_raw = estimate_bandwidth(X, idx, quantile)
    bw = bw_raw * band_factor
    floor_bound = bool(bw < FLOOR)
    bw = FLOOR if floor_bound else float(bw)
    seeds, are_points = bin_seeds(X, bw, floor_bound)
    seed_centers, seed_counts = mean_shift_seeds(X, seeds, bw)
    surv, cand = merge(seed_centers, seed_counts, bw)
    centers = seed_centers[surv]
    labels = np.argmin(sq_dists(X.astype(np.float64), centers.astype(np.float64)), axis=1).astype(np.int64)
    anchors, links, anchor_rank = choose_anchors(X, labels)
    return {"mapped": X, "bandwidth_raw": bw_raw, "bandwidth": bw, "floor_bound": floor_bound, "seeds": seeds,
            "seeds_are_points": are_points, "seed_centers": seed_centers, "seed_counts": seed_counts, "candidates": cand,
            "centers": centers, "center_counts": seed_counts[surv], "labels": labels, "anchors": anchors, "links": links,
            "anchor_rank": anchor_rank, "rgb_centers": inv_mapping_color(centers, factor).numpy()}


def fit(pixels, labels, class_num, factors, quantile=0.3, n_samples=5000, band_factor=0.5):
    """Like ``intrinsicnerf_amd.cluster.fit``: a list with ``fit_class``'s dict per class, None for a class without pixels.
    ``labels`` None = every pixel in class 0; labels outside [0, class_num) belong to no class."""
    pixels = np.asarray(pixels, np.float32).reshape(-1, 3)
    lab = np.zeros(pixels.shape[0], np.int64) if labels is None else np.asarray(labels).reshape(-1).astype(np.int64)
    out = []
    for c in range(int(class_num)):
        px = pixels[lab == c]
        out.append(fit_class(px, factors[c], quantile, n_samples, band_factor) if len(px) else None)
    return out
