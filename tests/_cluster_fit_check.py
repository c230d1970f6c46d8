"""Shared checker of the mean-shift fit tests: one fitted class against one class of a reference fixture
(tests/golden/cluster_fit.npz, cluster_fit_edges.npz), plus the adaptors that let the fp64 oracle (oracle/cluster_fit.py)
stand on either side of it - as the result under test, or as the fixture a GPU fit is held to."""
import os
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "cluster_fit.npz")
GOLD_EDGES = os.path.join(HERE, "golden", "cluster_fit_edges.npz")


def load(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _voxel_dist(p):
    """choose_anchors' torch expressions (cluster.py:168-170) on the CPU: (voxel id [n,3], dist [n])."""
    p = torch.from_numpy(p)
    vid = torch.clamp((p / 0.01).long(), 0, 99)
    return vid, torch.sum((vid * 0.01 + 0.005 - p) ** 2, dim=1)


def _match(ours, ref, tol):
    """index of our centre for every reference centre (one-to-one, each within tol)."""
    d = torch.cdist(torch.from_numpy(ref).double(), torch.from_numpy(ours).double())
    m = d.argmin(1).numpy()
    assert len(set(m.tolist())) == len(m), f"two reference centres share one fitted centre: {d}"
    worst = float(d[np.arange(len(m)), m].max())
    assert worst <= tol, f"centre off by {worst:.3e} > {tol:.3e}"
    return m


def _check_class(gold, key, pixels_c, factor, res, c, bw_rel=1e-9):
    import intrinsicnerf_amd.cluster as ic  # noqa: F401
    n_c = pixels_c.shape[0]
    bw = float(gold[f"{key}_bw"])
    # classes of <= 11 pixels: sklearn's NearestNeighbors(n_neighbors=5) switches to the float32 brute-force path, whose
    # distances (|x|^2 + |y|^2 - 2xy) differ from the exact fp64 ones by rounding: points at the radius may fall on the
    # other side, so only the bandwidth (kd-tree up to 3 pixels, floor below) and the centre count are compared exactly
    tiny = n_c <= 11
    assert abs(res.bandwidth[c] - bw) <= bw_rel * bw, (key, res.bandwidth[c], bw)
    ref_c = gold[f"{key}_centers_mapped"]
    ours_c = res.mapped_centers[c].cpu().numpy()
    assert ours_c.shape == ref_c.shape, (key, ours_c.shape, ref_c.shape)
    assert int(res.stats[c, 1]) == int(gold[f"{key}_n_seeds"]), (key, res.stats[c], int(gold[f"{key}_n_seeds"]))
    tol = 5 * 1e-3 * bw
    m = _match(ours_c, ref_c, tol)
    rgb = res.centers[c].cpu().numpy()
    assert np.abs(rgb[m] - gold[f"{key}_rgb_centers"]).max() <= 1e-5
    # labels_: ours mapped to the reference's centre order
    inv = np.empty(len(m), np.int64)
    inv[m] = np.arange(len(m))
    ours_l = inv[res.labels_c[c]]
    ref_l = gold[f"{key}_labels"]
    bad = np.nonzero(ours_l != ref_l)[0]
    mapped = torch.from_numpy(res.mapped_points[c]).double()
    if len(bad):
        assert tiny or len(bad) <= 1e-3 * n_c, (key, len(bad), n_c)
        rc = torch.from_numpy(ref_c).double()
        d_ours = (mapped[bad] - rc[ours_l[bad]]).norm(dim=1)
        d_ref = (mapped[bad] - rc[ref_l[bad]]).norm(dim=1)
        assert float((d_ours - d_ref).abs().max()) <= tol, f"{key}: a label mismatch that is not a near-tie"
    # anchors: bit-equal, links equal - except voxels whose winning dist ties or whose pixel is a tolerated mismatch
    a_ours, l_ours = res.anchors[c].cpu().numpy(), res.links[c].cpu().numpy().reshape(-1)
    a_ref, l_ref = gold[f"{key}_anchors"], gold[f"{key}_links"].reshape(-1)
    assert a_ours.shape == a_ref.shape and a_ours.dtype == np.float32
    assert res.links[c].dtype == torch.int64 and tuple(res.links[c].shape) == (a_ref.shape[0], 1)
    vid, dist = _voxel_dist(res.mapped_points[c])
    flat = (vid[:, 0] * 100 + vid[:, 1]) * 100 + vid[:, 2]
    best = torch.full((10 ** 6,), float("inf")).scatter_reduce(0, flat, dist, "amin")
    ties = torch.zeros(10 ** 6, dtype=torch.long).index_add_(0, flat, (dist == best[flat]).long())
    diff = np.nonzero(np.any(a_ours != a_ref, axis=1) | (inv[l_ours] != l_ref))[0]
    bad_set = set(bad.tolist())
    row_of = {tuple(r): i for i, r in enumerate(res.mapped_points[c].tolist())}
    for a in diff:
        v = int(flat[row_of[tuple(a_ref[a].tolist())]])
        pixel = row_of[tuple(a_ours[a].tolist())]
        assert ties[v] > 1 or pixel in bad_set, f"{key}: anchor {a} differs without a tie"
    return m


def mapping_np(s, factor):
    """the reference's mapping_color_np (cluster.py:316-322) in numpy fp32."""
    I = np.sum(s, axis=-1)
    d = np.zeros_like(s)
    d[..., 0] = I / 3.0 * np.float32(factor)
    d[..., 1] = s[..., 1] / I
    d[..., 2] = s[..., 2] / I
    return d


def _attach(res, sets, factors):
    """per-class labels_ and mapped points (the reference's mapping_color_np in numpy fp32) for the comparisons."""
    pl = res.pixel_label.cpu().numpy()
    res.labels_c, res.mapped_points = [], []
    K = len(sets)
    lab = None if K == 1 else res._labels
    for c, s in enumerate(sets):
        res.mapped_points.append(mapping_np(s, factors[c]))
        res.labels_c.append(pl if lab is None else pl[lab == c])


# ---------------------------------------------------------------- the oracle on either side of _check_class
def oracle_result(fits):
    """oracle.cluster_fit.fit's list as the object _check_class reads (what ``ic.fit`` + ``_attach`` give on the GPU)."""
    res = types.SimpleNamespace(bandwidth=[], mapped_centers=[], centers=[], anchors=[], links=[], labels_c=[], mapped_points=[],
                                center_counts=[])
    res.stats = np.zeros((len(fits), 4), np.int64)
    for c, f in enumerate(fits):
        if f is None:
            res.bandwidth.append(0.0)
            for lst in (res.mapped_centers, res.centers, res.anchors, res.links, res.labels_c, res.mapped_points, res.center_counts):
                lst.append(None)
            continue
        res.bandwidth.append(f["bandwidth"])
        res.mapped_centers.append(torch.from_numpy(f["centers"]))
        res.centers.append(torch.from_numpy(f["rgb_centers"]))
        res.anchors.append(torch.from_numpy(f["anchors"]))
        res.links.append(torch.from_numpy(f["links"]))
        res.labels_c.append(f["labels"])
        res.mapped_points.append(f["mapped"])
        res.center_counts.append(torch.from_numpy(f["center_counts"]))
        res.stats[c] = (f["mapped"].shape[0], f["seeds"].shape[0], int((f["seed_counts"] > 0).sum()), f["centers"].shape[0])
    return res


def oracle_gold(fits, case):
    """oracle.cluster_fit.fit's list under the key names of a fixture, so that a fit can be held to it by _check_class."""
    g = {}
    for c, f in enumerate(fits):
        if f is None:
            continue
        k = f"{case}_c{c}"
        g[f"{k}_bw"] = np.float64(f["bandwidth"])
        g[f"{k}_n_seeds"] = np.int64(f["seeds"].shape[0])
        g[f"{k}_centers_mapped"] = f["centers"]
        g[f"{k}_labels"] = f["labels"].astype(np.int32)
        g[f"{k}_counts"] = f["center_counts"].astype(np.int32)
        g[f"{k}_anchors"] = f["anchors"]
        g[f"{k}_links"] = f["links"]
        g[f"{k}_rgb_centers"] = f["rgb_centers"]
    return g


# ---------------------------------------------------------------- cases of cluster_fit_edges.npz
def edge_cases(gold):
    return [str(c) for c in gold["cases"]]


def edge_inputs(gold, case):
    """(pixels [n,3] fp32, labels [n] int64 or None, K, factor, band_factor) of a case of cluster_fit_edges.npz; the
    class-size sweep stores one pool and every case's slice of it."""
    if f"{case}_pool_off" in gold:
        off, n = int(gold[f"{case}_pool_off"]), int(gold[f"{case}_n"])
        px = gold["sweep_pool"][off:off + n]
    else:
        px = gold[f"{case}_pixels"]
    K = int(gold[f"{case}_class_num"])
    lab = gold[f"{case}_labels"].reshape(-1).astype(np.int64) if K > 1 else None
    return np.ascontiguousarray(px), lab, K, float(gold[f"{case}_factor"]), float(gold[f"{case}_band_factor"])


def class_sets(px, lab, K):
    return [px] if lab is None else [px[lab == c] for c in range(K)]
