"""Albedo-cluster lookup behind the reference's ``Cluster`` / ``Cluster_Manager`` interface.

``Cluster_Manager.dest_color(rgb, label)`` / ``dest_class(rgb, label)`` (SSR/training/cluster.py:73-98) run once per
training step (trainer.py:913-920) and once per rendered frame (:1427-1430).  The reference loops over the semantic
classes on the host - per class a boolean-mask gather (a host sync), the ``[anchors, 10240]`` distance matrix, an argmin
and a masked scatter.  Here every class goes through ONE launch of ``inerf_cluster_lookup`` (csrc/cluster.hip): the
anchors of all classes live in one device table and the distance matrix is never materialised.

Two ways in:

* ``dest_color(manager, rgb, label)`` / ``dest_class(manager, rgb, label)`` take ANY object with the reference's
  attributes (``class_num``, ``clusters[i].anchors / .links / .rgb_centers / .intensity_factor``), so the reference's own
  ``Cluster_Manager`` - including one that just ran its mean-shift ``update_center`` - can be handed over as it is;
* ``Cluster`` / ``Cluster_Manager`` below read and write the reference's ``clusters.json`` / ``c<i>/config.json`` files
  (cluster.py:20-50,112-129) and expose the same two lookups.

Building clusters - the reference's mean-shift ``update_center`` (cluster.py:52-70,138-182: sklearn's estimate_bandwidth,
``MeanShift(bin_seeding=True)`` on one CPU thread, the voxel filter of the anchors) - is ``fit``: ONE call of
``inerf_cluster_fit`` (csrc/cluster_fit.hip) for every class of a manager.  Only estimate_bandwidth's subsample
(``RandomState(0).permutation``, numpy's legacy stream) is drawn on the host and handed over as indices.
``update_center(manager, labels, pixels)`` fills any object with the reference's attributes (the reference's own
``Cluster_Manager`` included); ``Cluster.update_center`` / ``Cluster_Manager.update_center`` below are the same call.

There is no CPU path: pixels that are not on a HIP device raise.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

from . import _capi
from .kernels import _dev, _ptr, _stream


class ClusterTables:
    """The device tables ``inerf_cluster_lookup`` reads, built from a manager's clusters."""

    def __init__(self, clusters, device):
        anchors, links, centers, factors = [], [], [], []
        a_begin, c_begin = [0], [0]
        for c in clusters:
            if _has(c):
                a = torch.as_tensor(_field(c, "anchors")).to(device=device, dtype=torch.float32).reshape(-1, 3)
                # |a|^2 with the reference's own expression (cluster.py:300-301), so that it rounds like the reference's
                sq = torch.sum(a ** 2, dim=1)
                lk = torch.as_tensor(_field(c, "links")).to(device=device).reshape(-1).to(torch.int32)
                ctr = torch.as_tensor(_field(c, "rgb_centers")).to(device=device, dtype=torch.float32).reshape(-1, 3)
                if lk.shape[0] != a.shape[0]:
                    raise ValueError("a cluster's links and anchors differ in length")
                if int(lk.max()) >= ctr.shape[0] or int(lk.min()) < 0:
                    raise ValueError("a cluster's links point outside its rgb_centers")
                anchors.append(torch.cat([a, sq[:, None]], 1))
                links.append(lk)
                centers.append(ctr)
                factors.append(float(_field(c, "intensity_factor")))
                a_begin.append(a_begin[-1] + a.shape[0])
                c_begin.append(c_begin[-1] + ctr.shape[0])
            else:                                   # `clusters[i] is None`: an empty anchor range
                factors.append(0.0)
                a_begin.append(a_begin[-1])
                c_begin.append(c_begin[-1])
        self.n_classes = len(clusters)
        self.device = torch.device(device)
        i32 = dict(dtype=torch.int32, device=device)
        self.anchors = torch.cat(anchors, 0).contiguous() if anchors else torch.zeros(1, 4, device=device)
        self.links = torch.cat(links, 0).contiguous() if links else torch.zeros(1, **i32)
        self.centers = torch.cat(centers, 0).contiguous() if centers else torch.zeros(1, 3, device=device)
        self.anchor_begin = torch.tensor(a_begin, **i32)
        self.center_begin = torch.tensor(c_begin, **i32)
        self.factor = torch.tensor(factors, dtype=torch.float32, device=device)


def _field(c, name):
    return c[name] if isinstance(c, dict) else getattr(c, name, None)


def _has(c):
    return c is not None and _field(c, "anchors") is not None and _field(c, "anchors").shape[0] > 0


def _signature(clusters, device):
    sig = [str(device)]
    for c in clusters:
        if not _has(c):
            sig.append(None)
            continue
        parts = []
        for name in ("anchors", "links", "rgb_centers"):
            t = _field(c, name)
            parts.append((t.data_ptr(), t._version, tuple(t.shape)) if isinstance(t, torch.Tensor) else id(t))
        sig.append((id(c), tuple(parts), float(_field(c, "intensity_factor"))))
    return tuple(sig)


_tables = {}        # id(owner) -> (signature, ClusterTables); rebuilt when the owner's clusters change


def tables_for(owner, clusters, device):
    """Device tables for ``clusters`` (a list with None for classes without a cluster), cached per owning manager."""
    device = torch.device(device)
    sig = _signature(clusters, device)
    hit = _tables.get(id(owner))
    if hit is None or hit[0] != sig:
        if len(_tables) > 64:
            _tables.clear()
        hit = (sig, ClusterTables(clusters, device))
        _tables[id(owner)] = hit
    return hit[1]


def lookup(tables, rgb, label=None, want_color=True, want_class=False, ignore_label=False):
    """One launch of ``inerf_cluster_lookup``: (colour [n,3] float32 or None, class [n] int64 or None)."""
    rgb = _dev(rgb, "rgb", (None, 3))
    n = rgb.shape[0]
    if rgb.device != tables.device:
        raise ValueError(f"rgb is on {rgb.device}, the cluster tables on {tables.device}")
    if not ignore_label:
        if label is None:
            raise ValueError("label is required unless ignore_label is set")
        label = label.reshape(-1)
        if label.shape[0] != n or not label.is_cuda:
            raise ValueError(f"label must hold {n} entries on {rgb.device}")
        label = label.to(torch.int64).contiguous()
    color = torch.empty(n, 3, dtype=torch.float32, device=rgb.device) if want_color else None
    cls = torch.empty(n, dtype=torch.int64, device=rgb.device) if want_class else None
    with torch.cuda.device(rgb.device):
        rc = _capi.lib().inerf_cluster_lookup(
            _ptr(rgb), None if ignore_label else _ptr(label), n, _ptr(tables.anchors), _ptr(tables.links),
            _ptr(tables.anchor_begin), _ptr(tables.factor), _ptr(tables.centers), _ptr(tables.center_begin),
            tables.n_classes, _capi.CLUSTER_IGNORE_LABEL if ignore_label else 0, _ptr(color), _ptr(cls), _stream(rgb))
    _capi.check(rc, "inerf_cluster_lookup")
    return color, cls


def dest_color(manager, rgb, label):
    """``Cluster_Manager.dest_color`` (cluster.py:73-86): every pixel replaced by the centre colour of the cluster its
    mapped colour falls into, per semantic class; pixels of classes without a cluster come back unchanged."""
    single = manager.class_num == 1
    clusters = list(manager.clusters)[:1] if single else list(manager.clusters)[:manager.class_num]
    color, _ = lookup(tables_for(manager, clusters, rgb.device), rgb, label, ignore_label=single)
    # the single-class shortcut returns Cluster.dest_color's squeezed tensor (cluster.py:75-77,285)
    return torch.squeeze(color) if single else color


def dest_class(manager, rgb, label):
    """``Cluster_Manager.dest_class`` (cluster.py:88-98): [n,1] int64 cluster index inside the pixel's class."""
    clusters = list(manager.clusters)[:manager.class_num]
    _, cls = lookup(tables_for(manager, clusters, rgb.device), rgb, label, want_color=False, want_class=True)
    return cls[:, None]


MAX_CLASS_SAMPLES = 8192          # subsample rows the k-th neighbour kernel holds per class


def sample_indices(counts, n_samples=5000, random_state=0):
    """estimate_bandwidth's subsample of every class (sklearn/cluster/_mean_shift.py: ``check_random_state(0)`` and
    ``permutation(n)[:n_samples]``): (int32 indices into each class's pixels in their original order, back to back;
    int32 begin offsets [K+1])."""
    parts, begin = [], [0]
    for n_c in counts:
        n_c = int(n_c)
        if n_c <= 0:
            idx = np.zeros(0, np.int64)
        elif n_samples is None:
            idx = np.arange(n_c)
        else:
            idx = np.random.RandomState(random_state).permutation(n_c)[:n_samples]
        parts.append(idx.astype(np.int32))
        begin.append(begin[-1] + idx.shape[0])
    return (np.concatenate(parts) if parts else np.zeros(0, np.int32)), np.asarray(begin, np.int32)


class FitResult:
    """What ``inerf_cluster_fit`` returns for the K classes of one manager.  Per class c (``None`` for a class without
    pixels): ``centers[c]`` rgb [C,3] float32, ``anchors[c]`` [A,3] float32, ``links[c]`` [A,1] int64 - device tensors;
    ``bandwidth[c]`` (float).  Intermediate results for tests: ``mapped_centers`` (sklearn's cluster_centers_),
    ``center_counts``, ``pixel_label`` ([n] labels_ of every pixel inside its class, -1 outside), ``stats`` [K,4] (pixels,
    seeds, non-empty seeds, centres)."""


def _device_of(device):
    device = torch.device("cuda") if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"cluster fitting runs on a HIP device, not {device} (no CPU fallback exists)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def fit(pixels, labels, class_num, factors, device=None, quantile=0.3, n_samples=5000, band_factor=0.5, sample=None, counts=None):
    """Mean-shift clusters of every class: ``labels`` None = every pixel in class 0 (the SSR ``class_num == 1`` path);
    ``factors`` = intensity_factor per class; ``sample`` = (indices, begin) to override ``sample_indices``.  ``counts`` = the
    pixels of each class, ``np.bincount(labels[(labels >= 0) & (labels < K)], minlength=K)``, for ``labels`` that are an integer
    tensor on the device (``kernels.frame_subsample`` counts while it writes them): the labels then stay where they are - only
    those K numbers are read on the host."""
    device = _device_of(device)
    K = int(class_num)
    if isinstance(pixels, torch.Tensor):
        px = pixels.detach().reshape(-1, 3).to(device=device, dtype=torch.float32).contiguous()
    else:
        px = torch.from_numpy(np.ascontiguousarray(np.asarray(pixels, dtype=np.float32).reshape(-1, 3))).to(device)
    n = px.shape[0]
    if labels is None:
        lab_host, lab_dev = None, None
        counts = np.array([n] + [0] * (K - 1), np.int64)
    elif counts is not None:
        if not (isinstance(labels, torch.Tensor) and labels.is_cuda and not labels.is_floating_point()):
            raise ValueError("counts goes with labels that are an integer tensor on the device")
        lab_dev = labels.detach().reshape(-1).to(device=device, dtype=torch.int64).contiguous()
        if lab_dev.shape[0] != n:
            raise ValueError(f"{lab_dev.shape[0]} labels for {n} pixels")
        counts = (counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)).reshape(-1).astype(np.int64)
        if counts.shape[0] != K or (counts < 0).any() or int(counts.sum()) > n:
            raise ValueError(f"counts must hold the pixels of each of the {K} classes ({n} pixels in all)")
    else:
        lab_host = (labels.detach().reshape(-1).cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels).reshape(-1))
        lab_host = lab_host.astype(np.int64)
        if lab_host.shape[0] != n:
            raise ValueError(f"{lab_host.shape[0]} labels for {n} pixels")
        inside = lab_host[(lab_host >= 0) & (lab_host < K)]
        counts = np.bincount(inside, minlength=K)[:K]
        lab_dev = torch.from_numpy(lab_host).to(device)
    res = FitResult()
    res.counts = counts
    idx, begin = sample_indices(counts, n_samples) if sample is None else sample
    res.sample_idx, res.sample_begin = idx, begin
    empty = [None] * K
    if n == 0 or int(counts.sum()) == 0:
        res.bandwidth, res.centers, res.anchors, res.links, res.mapped_centers, res.center_counts = [0.0] * K, empty, empty, empty, empty, empty
        res.pixel_label = torch.full((n,), -1, dtype=torch.int32, device=device)
        res.stats = np.zeros((K, 4), np.int64)
        return res
    max_s = int(np.diff(begin).max()) if K else 0
    if max_s > MAX_CLASS_SAMPLES:
        raise ValueError(f"n_samples={n_samples}: the bandwidth subsample of a class is at most {MAX_CLASS_SAMPLES} pixels here")
    factor = torch.tensor([float(f) for f in factors], dtype=torch.float32, device=device)
    idx_d = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(device)
    begin_d = torch.from_numpy(np.ascontiguousarray(begin, dtype=np.int32)).to(device)
    lib = _capi.lib()
    ws_bytes = lib.inerf_cluster_fit_workspace_bytes(n, K, int(idx.shape[0]))
    if ws_bytes < 0:
        _capi.check(int(ws_bytes) if ws_bytes >= -4 else _capi.E_INVALID, "inerf_cluster_fit_workspace_bytes")
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=device)
    f32 = dict(dtype=torch.float32, device=device)
    centers, anchors, mapped = torch.empty(n, 3, **f32), torch.empty(n, 3, **f32), torch.empty(n, 3, **f32)
    links = torch.empty(n, dtype=torch.int64, device=device)
    center_counts = torch.empty(n, dtype=torch.int32, device=device)
    pixel_label = torch.empty(n, dtype=torch.int32, device=device)
    # bandwidth [K] doubles, then int32: status[4], center_begin[K+1], anchor_begin[K+1], stats[K,4] - read back at once
    n_int = 4 + 2 * (K + 1) + 4 * K
    meta = torch.zeros(K + (n_int + 1) // 2, dtype=torch.float64, device=device)
    ints = meta[K:].view(torch.int32)
    a = _capi.ClusterFitArgs(
        pixels=px.data_ptr(), labels=None if lab_dev is None else lab_dev.data_ptr(), n_pixels=n, n_classes=K,
        max_class_samples=max_s, sample_idx=idx_d.data_ptr(), sample_begin=begin_d.data_ptr(), n_sample_idx=int(idx.shape[0]),
        factor=factor.data_ptr(), quantile=float(quantile), band_factor=float(band_factor), workspace=ws.data_ptr(),
        workspace_bytes=int(ws_bytes), out_bandwidth=meta.data_ptr(), out_centers=centers.data_ptr(),
        out_center_begin=ints[4:].data_ptr(), out_anchors=anchors.data_ptr(), out_links=links.data_ptr(),
        out_anchor_begin=ints[4 + K + 1:].data_ptr(), out_mapped_centers=mapped.data_ptr(),
        out_center_counts=center_counts.data_ptr(), out_pixel_label=pixel_label.data_ptr(),
        out_class_stats=ints[4 + 2 * (K + 1):].data_ptr(), status=ints.data_ptr())
    with torch.cuda.device(device):
        rc = lib.inerf_cluster_fit(C.byref(a), C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    _capi.check(rc, "inerf_cluster_fit")
    host = meta.cpu()                                  # the one read: bandwidths, status, table offsets
    hi = host[K:].view(torch.int32).numpy()
    status = int(hi[0])
    if status & _capi.CLUSTER_FIT_NONFINITE:
        raise ValueError("cluster fit: a mapped colour is NaN or infinite (zero-intensity pixel?) - sklearn rejects such input too")
    if status & _capi.CLUSTER_FIT_RANGE:
        raise RuntimeError("cluster fit: a mapped colour has magnitude >= 256, outside what the kernels support")
    if status & _capi.CLUSTER_FIT_SAMPLE:
        raise ValueError("cluster fit: a subsample index lies outside its class")
    cb, ab = hi[4:4 + K + 1], hi[4 + K + 1:4 + 2 * (K + 1)]
    res.stats = hi[4 + 2 * (K + 1):4 + 2 * (K + 1) + 4 * K].reshape(K, 4).astype(np.int64)
    res.bandwidth = [float(v) for v in host[:K].numpy()]
    res.centers, res.anchors, res.links, res.mapped_centers, res.center_counts = [], [], [], [], []
    for c in range(K):
        if counts[c] == 0:
            for lst in (res.centers, res.anchors, res.links, res.mapped_centers, res.center_counts):
                lst.append(None)
            continue
        res.centers.append(centers[cb[c]:cb[c + 1]].clone())
        res.mapped_centers.append(mapped[cb[c]:cb[c + 1]].clone())
        res.center_counts.append(center_counts[cb[c]:cb[c + 1]].clone())
        res.anchors.append(anchors[ab[c]:ab[c + 1]].clone())
        res.links.append(links[ab[c]:ab[c + 1]].clone().reshape(-1, 1))
    res.pixel_label = pixel_label
    return res


def _fill(cluster, res, c):
    cluster.anchors, cluster.links, cluster.rgb_centers = res.anchors[c], res.links[c], res.centers[c]
    return cluster


def _cluster_factory(manager, device):
    """Cluster objects of the manager's own kind: the class named ``Cluster`` in the manager's module (the reference's
    for the reference's manager), this module's otherwise."""
    cls = getattr(sys.modules.get(type(manager).__module__), "Cluster", None)
    if cls is None or cls is Cluster:
        return lambda: Cluster(device=device)
    return cls


def update_center(manager, labels, pixels, quantile=0.3, n_samples=5000, band_factor=0.5, cluster_factory=None, counts=None):
    """``Cluster_Manager.update_center`` (SSR/training/cluster.py:52-70) on the GPU for any object with the reference's
    attributes: ``manager.clusters`` becomes one fitted cluster per class (``None`` for a class without pixels).  With
    ``class_num == 1`` every pixel is fitted and the labels are ignored (:55-59).  ``counts``: see ``fit``."""
    K = int(manager.class_num)
    device = _device_of(getattr(manager, "device", None))
    make = cluster_factory or _cluster_factory(manager, device)
    first = make()
    factor = float(getattr(first, "intensity_factor", 0.5))          # Cluster() defaults: the reference fits with 0.5
    res = fit(pixels, None if K == 1 else labels, K, [factor] * K, device=getattr(first, "device", device), quantile=quantile,
              n_samples=n_samples, band_factor=band_factor, counts=None if K == 1 else counts)
    clusters = []
    for c in range(K):
        if res.centers[c] is None:
            clusters.append(None)
        else:
            clusters.append(_fill(first, res, c))
            first = make()
    manager.clusters = clusters
    return res


def fit_cluster(cluster, pixels, quantile=0.3, n_samples=5000, band_factor=0.5):
    """``Cluster.update_center`` (cluster.py:138-152) on the GPU: fills ``cluster.anchors / links / rgb_centers``."""
    res = fit(pixels, None, 1, [float(cluster.intensity_factor)], device=getattr(cluster, "device", None), quantile=quantile,
              n_samples=n_samples, band_factor=band_factor)
    if res.centers[0] is None:
        raise ValueError("cluster fit: no pixels")
    _fill(cluster, res, 0)
    return res


class Cluster:
    """Data holder with the reference's ``Cluster`` fields and file format (cluster.py:101-129)."""

    def __init__(self, device=None, intensity_factor=0.5, cluster_dir=None):
        self.batch_size = 10240          # kept for the file format; the HIP lookup has no batches
        self.anchors = None
        self.links = None
        self.rgb_centers = None
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self.intensity_factor = intensity_factor
        if cluster_dir is not None:
            self.load(cluster_dir)

    def load(self, cluster_dir):
        with open(os.path.join(cluster_dir, "config.json"), "r") as f:
            data = json.load(f)
        self.batch_size = data["batch_size"]
        self.intensity_factor = data["intensity_factor"]
        self.anchors = torch.tensor(data["anchors"], dtype=torch.float32).reshape(-1, 3).to(self.device)
        self.rgb_centers = torch.tensor(data["rgb_centers"], dtype=torch.float32).reshape(-1, 3).to(self.device)
        self.links = torch.tensor(data["links"]).long().reshape(-1, 1).to(self.device)

    def save(self, cluster_dir):
        """Writes config.json like cluster.py:122-129 (the reference also drops a 50x50 PNG swatch per centre next to it)."""
        os.makedirs(cluster_dir, exist_ok=True)
        data = {"batch_size": self.batch_size, "intensity_factor": self.intensity_factor,
                "rgb_centers": self.rgb_centers.cpu().numpy().tolist(), "anchors": self.anchors.cpu().numpy().tolist(),
                "links": self.links.cpu().numpy().tolist()}
        with open(os.path.join(cluster_dir, "config.json"), "w") as f:
            json.dump(data, f)

    def dest_color(self, rgb):
        return torch.squeeze(lookup(tables_for(self, [self], rgb.device), rgb, ignore_label=True)[0])

    def dest_class(self, rgb):
        return lookup(tables_for(self, [self], rgb.device), rgb, want_color=False, want_class=True, ignore_label=True)[1][:, None]

    def update_center(self, pixels, quantile=0.3, n_samples=5000, band_factor=0.5):
        fit_cluster(self, pixels, quantile=quantile, n_samples=n_samples, band_factor=band_factor)


class Cluster_Manager:
    """The reference's ``Cluster_Manager`` (cluster.py:12-98); ``update_center`` fits on the GPU (``fit``)."""

    def __init__(self, class_num=0, cluster_config_file=None, device=None):
        self.class_num = class_num
        self.clusters = []
        self.device = device
        if cluster_config_file is not None:
            self.load(cluster_config_file)

    def load(self, cluster_config_file):
        with open(os.path.join(cluster_config_file, "clusters.json"), "r") as f:
            data = json.load(f)
        self.class_num = data["class_num"]
        configs = data["cluster_dirs"]
        assert self.class_num == len(configs)
        self.clusters = [None if cfg is None else Cluster(device=self.device, cluster_dir=os.path.join(cluster_config_file, "c" + str(i)))
                         for i, cfg in enumerate(configs)]

    def save(self, cluster_manager_dir):
        os.makedirs(cluster_manager_dir, exist_ok=True)
        dirs = []
        for i, cluster in enumerate(self.clusters):
            if cluster is None:
                dirs.append(None)
                continue
            d = os.path.join(cluster_manager_dir, "c" + str(i))
            cluster.save(d)
            dirs.append(d)
        with open(os.path.join(cluster_manager_dir, "clusters.json"), "w") as f:
            json.dump({"class_num": self.class_num, "cluster_dirs": dirs}, f)

    def update_center(self, labels, pixels, quantile=0.3, n_samples=5000, band_factor=0.5):
        update_center(self, labels, pixels, quantile=quantile, n_samples=n_samples, band_factor=band_factor)

    def dest_color(self, rgb, label):
        return dest_color(self, rgb, label)

    def dest_class(self, rgb, label):
        return dest_class(self, rgb, label)
